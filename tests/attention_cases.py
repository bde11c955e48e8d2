"""Named masks for the fused attention kernels (csrc/attention.hip, attention_rows.hip,
attention_backward.hip), each built to put a stated edge of the kernels' hand-made logic in
front of them, and a numpy model of where the LDS-staged forward puts things: the row in every
row slot, the entries of every row per 128-key chunk, and the plan (row_ok and chunk table)
exactly as the pre-pass writes it.  numpy only, explicit seeds; no kernel and no oracle.

tests/test_attention_cases_cpu.py proves that the cases reach the edges they are named for and
enumerates what tests/test_gpu_attention_instances.py runs.
"""
import functools

import numpy as np

from transpose_cases import reference as transpose_reference

BM = 128            # query rows of a workgroup (kBM)
BK = 128            # key rows of an LDS stage (kBK)
WINDOW = 16         # entries of a window; two are prefetched per row and chunk
PREFETCHED = 32

# per (row, chunk) counts of the staged forward: both sides of `left > 4 / 8 / 12`, a full
# window, both prefetched windows full, the first on-demand window with one entry, a second
# on-demand window, a full chunk
CHUNK_COUNTS = (0, 1, 4, 5, 8, 9, 12, 13, 16, 17, 31, 32, 33, 48, 49, 128)
# list lengths of the row-group kernels (windows of 16, unroll of 4, scalar tail):
# test_gpu_attention_d128.EDGE_COUNTS plus a fourth window
ROWGROUP_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 32, 33, 48, 49)

CANARY_F32 = -12345.0
CANARY_HALF = -768.0          # exact in float16 and bfloat16
CANARY_INT = -7777777
GUARD = 16                    # canary elements in front of and behind every guarded region


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def dealt_index(slot, slots, per):
    """spmm_tiled_common.h: the entry of row_indices that row slot `slot` holds."""
    return (slot % per) * (slots // per) + slot // per


def slot_rows(row_indices, m):
    """[slots] the row in every row slot, slots = ceil(m / 128) * 128; -1: padding."""
    slots = ceil_div(m, BM) * BM
    entry = dealt_index(np.arange(slots), slots, BM)
    rows = np.full(slots, -1, dtype=np.int64)
    rows[entry < m] = np.asarray(row_indices, np.int64)[entry[entry < m]]
    return rows


def block_rows(row_indices, m):
    """[blocks, 128] the rows (or -1) that share a row block."""
    return slot_rows(row_indices, m).reshape(-1, BM)


def wave_sets(row_indices, m):
    """[slots / 4, 4] the rows (or -1) of the four row groups that share a wave and a `t`
    (slots block * 128 + wave * 8 + 4 t .. + 3): one `longest` each."""
    return slot_rows(row_indices, m).reshape(-1, 4)


def chunk_counts(row_offsets, column_indices, n):
    """[m, ceil(n / 128)] entries of each row per 128-key chunk."""
    ro = np.asarray(row_offsets, np.int64)
    m, nchunks = len(ro) - 1, ceil_div(n, BK)
    rows = np.repeat(np.arange(m), np.diff(ro))
    out = np.zeros((m, nchunks), dtype=np.int64)
    np.add.at(out, (rows, np.asarray(column_indices, np.int64) // BK), 1)
    return out


def plan_model(row_indices, row_offsets, column_indices, m, n):
    """(row_ok [slots], table [(nchunks + 1) * slots], defined [like table]) as
    chunk_table_body<128> writes them.  table[c * slots + slot] = position of the first entry
    of the slot's row in a chunk >= c (the row's end if none).  A row is ok iff its columns
    ascend strictly and lie in [0, n); padding slots: ok, zeros.  The pre-pass writes every word
    of an ok row once; in a row that is not ok an entry that breaks the order writes nothing and
    the others may write a word twice or not at all -- `defined` is False there (such a row's
    block gathers: the kernel does not read its table)."""
    ro = np.asarray(row_offsets, np.int64)
    ci = np.asarray(column_indices, np.int64)
    rows = slot_rows(row_indices, m)
    slots, nchunks = len(rows), ceil_div(n, BK)
    row_ok = np.ones(slots, dtype=np.int32)
    table = np.zeros((nchunks + 1, slots), dtype=np.int32)
    writes = np.ones((nchunks + 1, slots), dtype=np.int64)
    for slot, row in enumerate(rows):
        if row < 0:
            continue
        writes[:, slot] = 0
        p0, p1 = int(ro[row]), int(ro[row + 1])
        for p in range(p0, p1):
            cur, prev = int(ci[p]), (int(ci[p - 1]) if p > p0 else -1)
            if cur <= prev or cur >= n:
                row_ok[slot] = 0
                continue
            for c in range((prev // BK if prev >= 0 else -1) + 1, cur // BK + 1):
                table[c, slot] = p
                writes[c, slot] += 1
        last = -1
        if p1 > p0:
            lc = int(ci[p1 - 1])
            last = lc // BK if 0 <= lc < n else nchunks
        for c in range(last + 1, nchunks + 1):
            table[c, slot] = p1
            writes[c, slot] += 1
    return row_ok, table.reshape(-1), (writes == 1).reshape(-1)


def gathered_blocks(row_indices, row_offsets, column_indices, m, n):
    """[blocks] bool: the row block holds a row that is not ok and takes the gather path."""
    row_ok, _, _ = plan_model(row_indices, row_offsets, column_indices, m, n)
    return ~row_ok.reshape(-1, BM).all(axis=1)


def mask_plan_ints(slots, nchunks):
    """attention.hip: ints of one mask's region of a many-mask plan."""
    ints = ceil_div(slots, 64) * 64 + (nchunks + 1) * slots + 1
    return ceil_div(ints, 64) * 64


def row_ok_ints(slots):
    return ceil_div(4 * slots, 256) * 64


def transpose_numpy(row_offsets, column_indices, m, n):
    """(t_row_offsets [n + 1], t_column_indices [nnz], permutation [nnz]) of the stable
    transpose: slot t of the transposed mask holds original entry permutation[t]."""
    assert len(row_offsets) == m + 1
    return transpose_reference(row_offsets, column_indices, n)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class Case:
    """dense [m, n] bool and its CSR (int32); row_indices in the named order.  The columns of
    the rows in `reversed_rows` descend, those of `swapped_rows` have one pair exchanged."""

    def __init__(self, name, dense, order, reversed_rows=(), swapped_rows=(), seed=0):
        self.name, self.order = name, order
        self.dense = np.ascontiguousarray(dense, dtype=bool)
        self.m, self.n = self.dense.shape
        lengths = self.dense.sum(axis=1)
        self.row_offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
        ci = np.nonzero(self.dense)[1].astype(np.int32)
        for r in reversed_rows:
            a, b = self.row_offsets[r], self.row_offsets[r + 1]
            assert b - a >= 2, (name, r)
            ci[a:b] = ci[a:b][::-1].copy()
        for r in swapped_rows:
            a, b = self.row_offsets[r], self.row_offsets[r + 1]
            assert b - a >= 3, (name, r)
            mid = a + (b - a) // 2
            ci[[mid - 1, mid]] = ci[[mid, mid - 1]]
        self.column_indices = ci
        self.unsorted_rows = tuple(reversed_rows) + tuple(swapped_rows)
        if order == "by_length":        # what callers pass: longest first, ties by row number
            ri = np.argsort(-lengths, kind="stable")
        elif order == "identity":
            ri = np.arange(self.m)
        else:
            assert order == "permuted", order
            ri = np.random.default_rng(900 + seed).permutation(self.m)
        self.row_indices = ri.astype(np.int32)

    @property
    def nnz(self):
        return len(self.column_indices)

    @property
    def csr(self):
        return self.row_indices, self.row_offsets, self.column_indices

    @property
    def chunk_counts(self):
        return chunk_counts(self.row_offsets, self.column_indices, self.n)

    @property
    def gathered(self):
        return gathered_blocks(*self.csr, self.m, self.n)

    def transposed(self, order="by_length", seed=0):
        """(t_row_indices, t_row_offsets, t_column_indices, permutation), int32."""
        t_ro, t_ci, perm = transpose_numpy(self.row_offsets, self.column_indices, self.m, self.n)
        lengths = np.diff(t_ro)
        if order == "by_length":
            t_ri = np.argsort(-lengths, kind="stable")
        elif order == "identity":
            t_ri = np.arange(self.n)
        else:
            t_ri = np.random.default_rng(700 + seed).permutation(self.n)
        return t_ri.astype(np.int32), t_ro, t_ci, perm


def _fill(dense, row, chunk, count, rng, n):
    """`count` entries of `row` inside key chunk `chunk` (clipped to the chunk's width): a random
    subset that holds the chunk's first column for rows 0, 3, 6 .. and its last for even rows."""
    lo, hi = chunk * BK, min((chunk + 1) * BK, n)
    if lo >= n:
        return
    count = min(count, hi - lo)
    if count == 0:
        return
    cols = np.sort(rng.choice(np.arange(lo, hi), size=count, replace=False))
    if row % 2 == 0:
        cols[-1] = hi - 1
    if row % 3 == 0 and count > 1:
        cols[0] = lo
    dense[row, cols] = True


def designed_mask(m, n, seed, last_row_empty=False):
    """Rows by specification (counts per chunk), as many as fit m, then random short rows:
      rows 0..15   CHUNK_COUNTS[i] entries in chunk 0, CHUNK_COUNTS[(i + 5) % 16] in chunk 1,
                   one in chunk 2 for every third row
      rows 16..19  a `longest` set under the identity order: 40 / 2 / 0 (but 3 in chunk 1) / none
      rows 20..23  the same around chunk 1: 37 there / 1 there / 5 in chunk 0 only / none
      row 24       a gap chunk: 3 in chunk 0, none in chunk 1, 1 in chunk 2
      row 25       only in the last chunk
    and at the end of the mask, so that a padding slot follows under the identity order when
    m % 128 != 0: row m - 3 with 40 entries in chunk 0, row m - 2 with 2 in the last chunk, and
    the last row with ONE entry (or none: last_row_empty) -- the last entry of column_indices
    sits in a row of one entry, every prefetch past it clamps."""
    rng = np.random.default_rng(seed)
    nchunks = ceil_div(n, BK)
    dense = np.zeros((m, n), dtype=bool)
    specs = [(v, CHUNK_COUNTS[(i + 5) % 16], 1 if i % 3 == 0 else 0) for i, v in enumerate(CHUNK_COUNTS)]
    specs += [(40, 0, 0), (2, 0, 0), (0, 3, 0), (0, 0, 0)]
    specs += [(0, 37, 0), (0, 1, 0), (5, 0, 0), (0, 0, 0)]
    specs += [(3, 0, 1)]
    body = max(m - 3, 0)
    for row in range(body):
        if row < len(specs):
            for chunk, count in enumerate(specs[row]):
                _fill(dense, row, chunk, count, rng, n)
        elif row == len(specs):
            _fill(dense, row, nchunks - 1, 4, rng, n)
        else:
            for chunk in range(nchunks):
                if rng.random() < 0.6:
                    _fill(dense, row, chunk, int(rng.integers(0, 21)), rng, n)
    if m >= 3:
        _fill(dense, m - 3, 0, 40, rng, n)
        _fill(dense, m - 2, nchunks - 1, 2, rng, n)
    if not last_row_empty:
        dense[m - 1, min(n - 1, 70)] = True
    return dense


def rowgroup_mask(m, n, seed):
    """Row i < 12 holds ROWGROUP_COUNTS[i] entries and key column j < 12 holds
    ROWGROUP_COUNTS[j] query rows, both at once: the rows' entries lie in columns >= 12, the
    columns' in rows >= 12, the 12 x 12 corner is empty.  The other rows hold what the columns
    gave them plus 0..5 random entries in columns >= 12.  The last key column is seen by the row
    of ONE entry alone (its dK is 0 by cancellation: zero_row_error of the GPU tests)."""
    k = len(ROWGROUP_COUNTS)
    assert m >= k + max(ROWGROUP_COUNTS) and n - 1 >= k + max(ROWGROUP_COUNTS)
    rng = np.random.default_rng(seed)
    dense = np.zeros((m, n), dtype=bool)
    for i, count in enumerate(ROWGROUP_COUNTS):
        dense[i, k + rng.choice(n - 1 - k, size=count, replace=False)] = True
        dense[k + rng.choice(m - k, size=count, replace=False), i] = True
    single = ROWGROUP_COUNTS.index(1)
    dense[single] = False
    dense[single, n - 1] = True
    for row in range(k, m):
        extra = int(rng.integers(0, 6))
        dense[row, k + rng.choice(n - 1 - k, size=extra, replace=False)] = True
    return dense


STRUCTURED_SHAPES = ((260, 260), (200, 136))
STRUCTURED_KINDS = ("causal", "band8", "band40", "global", "block_diagonal", "stride", "dense_row")


def structured(kind, m, n, seed=0):
    """The masks attention is run with.  causal and stride are helpers.structured_mask's; band
    (|column - row * n / m| <= width / 2), global rows and columns over a 2 % background, 48 x 48
    diagonal blocks and one dense row in a 2 % mask are built here."""
    rng = np.random.default_rng(seed)
    rows, cols = np.arange(m)[:, None], np.arange(n)[None, :]
    if kind in ("causal", "stride"):
        from helpers import structured_mask   # (imports the oracle package: layout code only)
        return structured_mask(kind, m, n, 8, rng)
    if kind.startswith("band"):
        width = int(kind[4:])
        return np.abs(cols - rows * n // m) <= width // 2
    if kind == "global":
        dense = rng.random((m, n)) < 0.02
        dense[[3, m // 2, m - 1]] = True
        dense[:, [0, 127, n - 1]] = True
        return dense
    if kind == "block_diagonal":
        return rows // 48 == np.minimum(cols // 48, (m - 1) // 48)
    assert kind == "dense_row", kind
    dense = rng.random((m, n)) < 0.02
    dense[m // 3] = True
    return dense


def _unsorted(name, m, n, seed, unsorted, order="identity"):
    """A uniform mask of 12 .. 40 entries per row with reversed and swapped rows."""
    rng = np.random.default_rng(seed)
    dense = np.zeros((m, n), dtype=bool)
    for row in range(m):
        dense[row, rng.choice(n, size=int(rng.integers(12, 41)), replace=False)] = True
    reversed_rows, swapped_rows = unsorted
    return Case(name, dense, order, reversed_rows, swapped_rows, seed)


BUILDERS = {
    # the staged forward's per-chunk counts, `longest` sets, chunk and row-block geometry
    "edges_127x257_identity": lambda: Case("edges_127x257_identity", designed_mask(127, 257, 1), "identity"),
    "edges_129x256_by_length": lambda: Case("edges_129x256_by_length", designed_mask(129, 256, 2), "by_length"),
    "edges_260x255_permuted": lambda: Case("edges_260x255_permuted", designed_mask(260, 255, 3), "permuted", seed=3),
    "edges_128x129_last_row_empty": lambda: Case("edges_128x129_last_row_empty",
                                                 designed_mask(128, 129, 4, last_row_empty=True), "by_length"),
    "edges_127x257_last_row_empty": lambda: Case("edges_127x257_last_row_empty",
                                                 designed_mask(127, 257, 5, last_row_empty=True), "identity"),
    "edges_60x128_identity": lambda: Case("edges_60x128_identity", designed_mask(60, 128, 6), "identity"),
    "one_row_1x64": lambda: Case("one_row_1x64", designed_mask(1, 64, 7), "identity"),
    # order: m = 129 gives two row blocks, identity order deals even rows to block 0
    "one_block_gathers_129x256": lambda: _unsorted("one_block_gathers_129x256", 129, 256, 8, ((10,), (20,))),
    "every_block_gathers_129x256": lambda: _unsorted("every_block_gathers_129x256", 129, 256, 9, ((10, 11), (21,))),
    # (three blocks: rows 0, 1, 2 are the first slots of blocks 0, 1, 2)
    "every_block_gathers_260x64": lambda: _unsorted("every_block_gathers_260x64", 260, 64, 10, ((0, 1), (2,))),
    # the row-group kernels: designed row AND key-column counts
    "rowgroup_100x100": lambda: Case("rowgroup_100x100", rowgroup_mask(100, 100, 11), "by_length",
                                     reversed_rows=(8,)),
    "rowgroup_90x77": lambda: Case("rowgroup_90x77", rowgroup_mask(90, 77, 12), "permuted",
                                   reversed_rows=(9,), swapped_rows=(7,), seed=12),
}
for _m, _n in STRUCTURED_SHAPES:
    for _kind in STRUCTURED_KINDS:
        BUILDERS[f"{_kind}_{_m}x{_n}"] = (
            lambda kind=_kind, m=_m, n=_n: Case(f"{kind}_{m}x{n}", structured(kind, m, n, seed=m + n),
                                                "by_length"))

CASE_NAMES = tuple(BUILDERS)
EDGE_CASES = tuple(name for name in CASE_NAMES if name.startswith(("edges_", "one_", "every_")))
ROWGROUP_CASES = ("rowgroup_100x100", "rowgroup_90x77")
STRUCTURED_CASES = tuple(f"{kind}_{m}x{n}" for m, n in STRUCTURED_SHAPES for kind in STRUCTURED_KINDS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# ---------------------------------------------------------------------------
# many-mask batches: masks of one shape in the flat layout (row_indices [b * m] local row ids,
# row_offsets [b * (m + 1)] each starting at 0, column_indices concatenated, counts [b])
# ---------------------------------------------------------------------------
BATCHES = {
    "edges_127x257": ("edges_127x257_identity", "edges_127x257_last_row_empty"),
    "order_129x256": ("one_block_gathers_129x256", "every_block_gathers_129x256"),
    "edges_and_order_129x256": ("edges_129x256_by_length", "one_block_gathers_129x256"),
    "structured_260x260": ("causal_260x260", "dense_row_260x260"),
    "structured_200x136": ("band40_200x136", "global_200x136"),
}
EDGE_BATCHES = ("edges_127x257", "order_129x256", "edges_and_order_129x256")
STRUCTURED_BATCHES = ("structured_260x260", "structured_200x136")


class Batch:
    def __init__(self, name, cases):
        self.name, self.cases = name, cases
        self.m, self.n = cases[0].m, cases[0].n
        assert all((c.m, c.n) == (self.m, self.n) for c in cases)
        self.row_indices = np.concatenate([c.row_indices for c in cases]).astype(np.int32)
        self.row_offsets = np.concatenate([c.row_offsets for c in cases]).astype(np.int32)
        self.column_indices = np.concatenate([c.column_indices for c in cases]).astype(np.int32)
        self.nonzeros = [c.nnz for c in cases]
        self.dense = np.stack([c.dense for c in cases])

    def plan_model(self):
        """The whole many-mask plan as int32 words and which of them the model defines: one
        region per mask (row_ok, table, and in the LAST word of region `rank` the mask that
        starts rank-th: most entries first, ties by mask number)."""
        slots, nchunks = ceil_div(self.m, BM) * BM, ceil_div(self.n, BK)
        ints = mask_plan_ints(slots, nchunks)
        plan = np.zeros(len(self.cases) * ints, dtype=np.int32)
        defined = np.zeros(len(self.cases) * ints, dtype=bool)
        order = sorted(range(len(self.cases)), key=lambda i: (-self.nonzeros[i], i))
        for i, c in enumerate(self.cases):
            row_ok, table, table_defined = plan_model(*c.csr, c.m, c.n)
            base = i * ints
            plan[base:base + slots] = row_ok
            defined[base:base + slots] = True
            first = base + row_ok_ints(slots)
            plan[first:first + len(table)] = table
            defined[first:first + len(table)] = table_defined
            plan[(i + 1) * ints - 1] = order[i]
            defined[(i + 1) * ints - 1] = True
        return plan, defined


@functools.lru_cache(maxsize=None)
def batch(name):
    return Batch(name, [case(c) for c in BATCHES[name]])


# ---------------------------------------------------------------------------
# what the GPU file runs: (instance, case or batch, p)
# ---------------------------------------------------------------------------
STORAGE_PAIRS = (("float32", "float32"), ("float16", "float32"), ("float16", "float16"),
                 ("bfloat16", "float32"), ("bfloat16", "bfloat16"))
DROP_P = 0.25


def forward_instances():
    """The 20 instances of sparse_attention_kernel<T, TO, MANY, Drop...>."""
    return [(t, to, many, drop) for t, to in STORAGE_PAIRS for many in (False, True)
            for drop in (False, True)]


def forward_runs():
    """[(instance, case or batch name)]: every instance takes the edge cases (batches), the
    structured cases go to the single-mask instances in turn -- case j with dropout iff j is
    odd -- and the structured batches to every many-mask instance."""
    runs = []
    for inst in forward_instances():
        _, _, many, drop = inst
        if many:
            runs += [(inst, name) for name in EDGE_BATCHES + STRUCTURED_BATCHES]
        else:
            runs += [(inst, name) for name in EDGE_CASES]
            runs += [(inst, name) for j, name in enumerate(STRUCTURED_CASES) if (j % 2 == 1) == drop]
    return runs


def rowgroup_instances():
    """The 2 instances of attention_rows_forward_kernel (d = 128) and the 8 of the backward
    kernels: (kernel, d, drop)."""
    forward = [("rows_forward", 128, drop) for drop in (False, True)]
    backward = [(kernel, d, drop) for kernel in ("backward_rows", "backward_columns")
                for d in (64, 128) for drop in (False, True)]
    return forward + backward


BACKWARD_CASES = ROWGROUP_CASES + ("edges_127x257_identity", "causal_200x136", "global_200x136")
ROWS_FORWARD_CASES = ROWGROUP_CASES + ("edges_129x256_by_length", "band8_200x136")
T_ORDERS = ("by_length", "identity", "permuted")


def rowgroup_runs():
    runs = []
    for inst in rowgroup_instances():
        names = ROWS_FORWARD_CASES if inst[0] == "rows_forward" else BACKWARD_CASES
        runs += [(inst, name) for name in names]
    return runs
