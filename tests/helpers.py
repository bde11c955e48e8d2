"""Shared input builders for the parity tests (numpy only; seeds are explicit)."""
import numpy as np

from oracle import sputnik_oracle as O


def make_csr(m, n, sparsity, seed, round_to=4, empty_rows=(), order="descending"):
    """Random CSR pattern with the reference's input distribution
    (tests/connectors.py:34-59), optional forced-empty rows, and a choice of
    row_indices order (callers pass both)."""
    rng = np.random.default_rng(seed)
    mask = O.random_mask(m, n, sparsity, round_to=round_to, rng=rng)
    for r in empty_rows:
        mask[r, :] = 0
    values = (rng.uniform(0.0, 1.0, size=(m, n)).astype(np.float32) + np.float32(1e-3)) * mask
    vals, row_indices, row_offsets, column_indices = O.dense_to_csr(values)
    if order == "ascending":
        row_indices = O.diffsort(row_offsets)
    elif order == "random":
        row_indices = rng.permutation(m).astype(np.int32)
    elif order == "identity":
        row_indices = np.arange(m, dtype=np.int32)
    return values.astype(np.float32), vals, row_indices, row_offsets, column_indices


# ---------------------------------------------------------------------------
# structured masks for the single-mask SpMM / SDDMM routes: what a uniform mask cannot put in
# front of a kernel -- a chunk of 256 entries next to empty ones, a wave of empty rows next to
# a wave of full ones, a tile without an entry
# ---------------------------------------------------------------------------
STRUCTURED_KINDS = (
    "causal", "band", "global_columns_one_chunk", "global_columns_per_chunk",
    "heavy_rows_start", "heavy_rows_end", "heavy_rows_wave", "heavy_rows_block",
    "last_chunk", "block_diagonal", "stride", "alternating", "corner", "uniform")


def _heavy_first_row(kind, m, h):
    """First of the h full rows: at the start, at the end, or with h // 2 rows in front of a
    multiple of 8 (a wave's rows in the flat SpMM kernel) / of 128 (a workgroup's rows)."""
    if kind == "heavy_rows_start":
        return 0
    if kind == "heavy_rows_end":
        return m - h
    if kind == "heavy_rows_wave":
        edge = (h // 2 + 7) // 8 * 8 + 8
        edge += 8 if edge % 128 == 0 else 0
    else:
        edge = (h // 2 + 127) // 128 * 128
    first = edge - h // 2
    assert first >= 0 and first + h <= m, f"{kind}: {h} rows around row {edge} do not fit {m} rows"
    return first


def structured_mask(kind, m, n, min_mean_row, rng, chunk=32):
    """[m, n] bool mask of one of STRUCTURED_KINDS with at least min_mean_row * m entries (what
    the LDS routes ask for: 16, or 4 for the 64-column SpMM and the tiled SDDMM).  `chunk`:
    the K-chunk (SpMM) or slab (SDDMM) whose partial last piece `last_chunk` fills."""
    rows, cols = np.arange(m)[:, None], np.arange(n)[None, :]
    need = int(np.ceil(min_mean_row * m))
    per_row = int(np.ceil(min_mean_row))
    assert m >= 2 and n >= 2 * per_row, (m, n, min_mean_row)
    if kind == "causal":            # row 0 holds column 0, the last row every column
        mask = cols <= rows * (n - 1) // (m - 1)
    elif kind == "band":
        centre = rows * n // m
        width = 0
        while np.count_nonzero(np.abs(cols - centre) <= width) < need:
            width += 1
        mask = np.abs(cols - centre) <= width
    elif kind == "global_columns_one_chunk":
        mask = np.broadcast_to(cols < per_row, (m, n))
    elif kind == "global_columns_per_chunk":   # one column per chunk, column n - 1 among them
        chunks = -(-n // chunk)
        held = {min((i * chunks // per_row) * chunk + (7 * i + i // chunks) % chunk, n - 2)
                for i in range(per_row - 1)} | {n - 1}
        assert len(held) == per_row, (sorted(held), per_row)
        mask = np.broadcast_to(np.isin(np.arange(n), sorted(held))[None, :], (m, n))
    elif kind.startswith("heavy_rows_"):
        h = max(2, -(-need // n))
        first = _heavy_first_row(kind, m, h)
        mask = np.broadcast_to((rows >= first) & (rows < first + h), (m, n))
    elif kind == "last_chunk":      # exactly the partial last chunk where that is long enough
        c = n % chunk if n % chunk >= per_row else per_row
        mask = np.broadcast_to(cols >= n - c, (m, n))
    elif kind == "block_diagonal":  # 64 x 64 blocks ending in the bottom-right corner: the last
        row_blocks, col_blocks = -(-m // 64), -(-n // 64)   # block is ragged in rows and columns
        mask = cols // 64 == np.maximum(col_blocks - row_blocks + rows // 64, 0)
    elif kind == "stride":
        s = max(1, n // per_row)
        mask = cols % s == rows % s
    elif kind == "alternating":     # even rows full, odd rows one entry, each in another column
        mask = (rows % 2 == 0) | (cols == (rows * 37 + 11) % n)
    elif kind == "corner":
        width = min(n, 100)
        height = -(-need // width)
        assert height <= m, (m, n, min_mean_row)
        mask = (rows < height) & (cols < width)
    else:
        assert kind == "uniform", kind
        density = min(1.0, 1.25 * min_mean_row / n + 4.0 / (m * n))
        mask = O.random_mask(m, n, 1.0 - density, round_to=1, rng=rng) != 0
    mask = np.ascontiguousarray(mask, dtype=bool)
    assert np.count_nonzero(mask) >= need, (kind, m, n, np.count_nonzero(mask), need)
    return mask


def structured_csr(kind, m, n, min_mean_row, rng, order="descending", shuffle_every=0, chunk=32):
    """(row_indices, row_offsets, column_indices), int32, of structured_mask(kind, ...).
    order: "descending" row lengths (what diffsort gives real callers, ties by row number) or
    "identity".  shuffle_every = 3: the columns of every third row in random order -- the
    order-independent path of the LDS kernels, as shuffle_columns is for the many-mask layout."""
    mask = structured_mask(kind, m, n, min_mean_row, rng, chunk=chunk)
    lengths = mask.sum(axis=1)
    row_offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    column_indices = np.nonzero(mask)[1].astype(np.int32)
    if order == "descending":
        row_indices = np.argsort(-lengths, kind="stable").astype(np.int32)
    else:
        assert order == "identity", order
        row_indices = np.arange(m, dtype=np.int32)
    if shuffle_every:
        for r in range(0, m, shuffle_every):
            a, b = int(row_offsets[r]), int(row_offsets[r + 1])
            if b - a > 1:
                column_indices[a:b] = column_indices[a:b][rng.permutation(b - a)]
    return row_indices, row_offsets, column_indices


def _row_view(a, row_offsets):
    """(values as [rows, width] or flat, row id per element or None)."""
    a = np.asarray(a, np.float64)
    if row_offsets is None:
        if a.ndim >= 2 and a.shape[-1] < 16:
            return a.reshape(-1, a.shape[-2] * a.shape[-1]), None
        return (a.reshape(-1, a.shape[-1]) if a.ndim >= 2 else a.reshape(1, -1)), None
    lengths = np.diff(np.asarray(row_offsets, np.int64))
    ids = np.repeat(np.arange(len(lengths)), lengths)
    return a.reshape(-1, a.shape[-1]), ids


def rel_err(got, expected, row_offsets=None):
    """Worst violation of the fp32 parity bound, as a multiple of 1: the test
    is ``rel_err(...) < 1e-4`` (the north star's tolerance).  Two criteria, both
    PER ROW of the output (the unit one wavefront group accumulates):

      (1) |got - want| / (|want| + rowmean|want|)       every element
      (2) |got - want| / |want|                         elements with
                                                         |want| > 1e-2 * rowmax|want|

    (1) is rtol*|want| + atol with atol = rtol * mean magnitude of the SAME
    row: a float32 sum of K products carries an absolute error ~1e-7*sum|a*b|,
    so entries that cancel to nearly zero cannot be held to a purely relative
    bound, but the slack they get comes from their own row, never from a
    larger row elsewhere in the tensor.  (2) is a pure relative check on
    every entry that is not a cancellation.

    A "row" is the last dimension for dense outputs; for CSR-ordered outputs
    ([nnz] or [R, nnz]) pass ``row_offsets`` and it is the CSR row.  Dense
    outputs narrower than 16 columns (n = 1, 7 ...) have no row to speak of: a
    single cancelling element would be its own scale, so there the scale is
    taken over the whole [m, n] matrix of the replica; likewise CSR rows of fewer
    than 16 entries take the scale of their replica.
    """
    got = np.asarray(got, np.float64)
    expected = np.asarray(expected, np.float64)
    if got.size == 0:
        return 0.0
    assert got.shape == expected.shape, (got.shape, expected.shape)
    w, ids = _row_view(expected, row_offsets)
    g = got.reshape(w.shape)
    aw = np.abs(w)
    err = np.abs(g - w)
    if ids is None:
        rowmean = aw.mean(axis=1, keepdims=True)
        rowmax = aw.max(axis=1, keepdims=True)
    else:
        rows = int(ids.max()) + 1 if ids.size else 0
        count = np.maximum(np.bincount(ids, minlength=rows), 1)
        rowmean = np.stack([np.bincount(ids, weights=r, minlength=rows) / count for r in aw])
        rowmax = np.zeros((aw.shape[0], rows))
        for r in range(aw.shape[0]):
            np.maximum.at(rowmax[r], ids, aw[r])
        # CSR rows of fewer than 16 entries are no scale either (a row of ONE entry
        # that cancels to nearly zero would be held to a relative bound of itself):
        # such rows take the replica's mean / maximum, like narrow dense outputs
        short = count < 16
        rowmean[:, short] = aw.mean(axis=1, keepdims=True)
        rowmax[:, short] = aw.max(axis=1, keepdims=True)
        rowmean, rowmax = rowmean[:, ids], rowmax[:, ids]
    worst = float(np.max(err / (aw + np.maximum(rowmean, 1e-30))))
    significant = aw > 1e-2 * rowmax
    if significant.any():
        worst = max(worst, float(np.max(err[significant] / aw[significant])))
    return worst


def rel_err_torch(got, want):
    """rel_err on device tensors (full-size checks): rows = last dimension,
    ``want`` in float64."""
    import torch
    want = want.to(torch.float64)
    err = (got.to(torch.float64) - want).abs()
    aw = want.abs()
    rowmean = aw.mean(dim=-1, keepdim=True).clamp_min(1e-30)
    rowmax = aw.amax(dim=-1, keepdim=True)
    worst = float((err / (aw + rowmean)).max())
    significant = aw > 1e-2 * rowmax
    if bool(significant.any()):
        worst = max(worst, float((err[significant] / aw[significant]).max()))
    return worst


# ---------------------------------------------------------------------------
# half storage (float16 / bfloat16): the oracle runs on the ROUNDED inputs, and what is
# left to compare is the arithmetic plus one rounding of the output
# ---------------------------------------------------------------------------
def ulp(want, dtype):
    """Spacing of the storage type at |want| (float16 subnormals included)."""
    import torch
    a = np.abs(np.asarray(want, np.float64))
    if dtype == torch.float16:
        return np.spacing(np.minimum(a, 65000.0).astype(np.float16)).astype(np.float64)
    if dtype == torch.bfloat16:
        return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 7)
    return np.zeros_like(a)


def half_err(got, want, dtype, row_offsets=None):
    """rel_err of what is left of |got - want| after ONE unit in the last place of
    the output's storage type (its rounding) has been taken off: the test is
    ``half_err(...) < 1e-4``, the float32 bound on the arithmetic."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    diff = got - want
    rest = np.sign(diff) * np.maximum(np.abs(diff) - ulp(want, dtype), 0.0)
    return rel_err(want + rest, want, row_offsets)


def rounded(x, dtype, dev):
    """(device tensor in `dtype`, the same values as float32 numpy)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev).to(dtype)
    return t, t.float().cpu().numpy()


# ---------------------------------------------------------------------------
# many-mask family: masks of mixed kinds and float64 references (torch, any device)
# ---------------------------------------------------------------------------
MASK_KINDS = ("empty", "single", "uniform", "band", "global", "heavy_row", "empty_rows")


def mask_of_kind(kind, m, n, rng):
    """One [m, n] 0/1 mask: empty; a single entry; uniform at density 0.02-1; a band (local
    window along the diagonal of the m x n rectangle); global tokens (full rows and columns
    over a 2 % background); one full row in a <= 5 % mask (more than 32 entries in one key
    chunk); uniform with forced empty rows."""
    mask = np.zeros((m, n), dtype=bool)
    if kind == "single":
        mask[rng.integers(0, m), rng.integers(0, n)] = True
    elif kind == "uniform":
        mask = rng.random((m, n)) < rng.uniform(0.02, 1.0)
    elif kind == "band":
        width = int(rng.integers(0, 17))
        centre = (np.arange(m)[:, None] * n) // max(m, 1)
        mask = np.abs(np.arange(n)[None, :] - centre) <= width
    elif kind == "global":
        mask = rng.random((m, n)) < 0.02
        mask[rng.choice(m, size=min(m, int(rng.integers(1, 4))), replace=False)] = True
        mask[:, rng.choice(n, size=min(n, int(rng.integers(1, 4))), replace=False)] = True
    elif kind == "heavy_row":
        mask = rng.random((m, n)) < rng.uniform(0.0, 0.05)
        mask[rng.integers(0, m)] = True
    elif kind == "empty_rows":
        mask = rng.random((m, n)) < rng.uniform(0.1, 0.6)
        mask[rng.choice(m, size=max(1, m // 8), replace=False)] = False
    else:
        assert kind == "empty", kind
    return mask


def shuffle_columns(column_indices, row_offsets, mask_id, m, first, rng, every=3):
    """Columns of every `every`-th row of mask `mask_id` (flat many-mask layout, its entries
    from `first`) in random order, in place: the order-independent path of those row blocks."""
    ro = row_offsets[mask_id * (m + 1):(mask_id + 1) * (m + 1)]
    for r in range(0, m, every):
        a, b = first + int(ro[r]), first + int(ro[r + 1])
        if b - a > 1:
            column_indices[a:b] = column_indices[a:b][rng.permutation(b - a)]


def many_mask_entries(nonzeros, row_offsets, column_indices, m, heads, device):
    """(replica, row, column, slot) long tensors of every served entry of a many-mask
    topology (flat or [b, m + 1] offsets), replica r under mask r // heads."""
    import torch
    ro = torch.as_tensor(row_offsets).reshape(-1).to(device=device, dtype=torch.int64)
    ci = torch.as_tensor(column_indices).reshape(-1).to(device=device, dtype=torch.int64)
    parts, first = [], 0
    for i, count in enumerate(int(c) for c in nonzeros):
        offs = ro[i * (m + 1):(i + 1) * (m + 1)]
        rows = torch.repeat_interleave(torch.arange(m, device=device), offs[1:] - offs[:-1])
        cols = ci[first:first + count]
        slots = torch.arange(count, device=device)
        for h in range(heads):
            parts.append((torch.full_like(slots, i * heads + h), rows, cols, slots))
        first += count
    if not parts:
        empty = torch.zeros(0, dtype=torch.int64, device=device)
        return empty, empty, empty, empty
    return tuple(torch.cat([p[j] for p in parts]) for j in range(4))


def ref_sddmm_many_mask(entries, width, lhs, rhs):
    """[R, width] float64: lhs[r, row] . rhs[r, col] at every entry, 0 past a replica's count
    (differentiable)."""
    import torch
    r, row, col, slot = entries
    out = torch.zeros(lhs.size(0), width, dtype=torch.float64, device=lhs.device)
    return out.index_put((r, slot), (lhs.double()[r, row] * rhs.double()[r, col]).sum(-1))


def ref_spmm_many_mask(entries, m, values, dense):
    """[R, m, N] float64: the sparse [m, k] of each replica (values[r, slot]) times dense[r]."""
    import torch
    r, row, col, slot = entries
    a = torch.zeros(dense.size(0), m, dense.size(1), dtype=torch.float64, device=dense.device)
    a = a.index_put((r, row, col), values.double()[r, slot])
    return a @ dense.double()


def ref_softmax_many_mask(entries, m, n, values, scale=1.0):
    """Row softmax of scale * values over each replica's entries, [R, values.size(1)] float64
    with zeros past a replica's count (differentiable)."""
    import torch
    r, row, col, slot = entries
    dense = torch.full((values.size(0), m, n), float("-inf"), dtype=torch.float64,
                       device=values.device)
    dense = dense.index_put((r, row, col), scale * values.double()[r, slot])
    probs = torch.softmax(dense, dim=-1)
    out = torch.zeros(values.shape, dtype=torch.float64, device=values.device)
    return out.index_put((r, slot), probs[r, row, col])


def ref_attention_many_mask(q, k, v, dense_masks, scale):
    """float64 dense masked softmax per replica, replica r under mask r // heads: q [R, m, d],
    k and v [R, n, d], dense_masks [b, m, n] bool -> (out [R, m, d], lse [R, m]); rows
    without entries give zeros and lse = -inf.  Differentiable (gradients of empty rows: 0)."""
    import torch
    q, k, v = (x.double() for x in (q, k, v))
    heads = q.size(0) // dense_masks.size(0)
    mask = torch.as_tensor(dense_masks).to(q.device).repeat_interleave(heads, 0)
    s = (scale * q @ k.transpose(1, 2)).masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    return torch.softmax(s, dim=-1).nan_to_num(0.0) @ v, lse
