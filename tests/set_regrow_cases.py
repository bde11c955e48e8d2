"""Shared by tests/test_set_regrow_cpu.py and tests/test_gpu_set_regrow.py: the rule of the
drop-and-grow step under generated scores (topology.regrow_per_row_random / regrow_total_random,
include/sputnik_hip.h "random scores that are never stored") restated in numpy on the Philox of
tests/philox_ref.py, and the inputs both files build.  CPU only; everything is an integer or a
bit copy."""
import numpy as np
import torch

from tests import philox_ref
from tests import regrow_total_cases as C
from torch_sputnik_amd import ops, topology

DEFAULT = ops.REGROW_KEY_MASK
MASKS = (0, 0x3, 0xff, DEFAULT)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
STATE = (2 ** 40 + 17, 4 * 10 ** 9)
PER_ROW_NAMES = ("column_indices", "values", "source")


def words(m, n, state, values):
    """uint32 [m, n]: word c & 3 of Philox(seed, (offset / 4, c >> 2, r)), r | 2**31 for the
    value stream"""
    seed, offset = (int(v) & 0xFFFFFFFFFFFFFFFF for v in state)
    assert offset % 4 == 0
    block = offset // 4
    rows = np.arange(m, dtype=np.uint32)[:, None] | np.uint32(0x80000000 if values else 0)
    columns = np.arange(n, dtype=np.uint32)[None, :]
    out = philox_ref.philox4x32_10((seed & 0xFFFFFFFF, seed >> 32),
                                   (block & 0xFFFFFFFF, block >> 32, columns >> np.uint32(2), rows))
    stacked = np.stack([np.broadcast_to(w, (m, n)) for w in out])
    pick = np.broadcast_to((columns & np.uint32(3)).astype(np.int64), (m, n))[None]
    return np.take_along_axis(stacked, pick, 0)[0]


def keys(m, n, state, key_mask=DEFAULT):
    return words(m, n, state, False) & np.uint32(key_mask)


def key_scores(m, n, state, key_mask=DEFAULT):
    """float32 [m, n] tensor whose bit patterns are the keys"""
    return torch.from_numpy(keys(m, n, state, key_mask).astype(np.int64).astype(np.int32)).view(torch.float32)


def value_image(m, n, state, bound, dtype):
    """[m, n] tensor of `dtype`: what random_csr stores at every position under `bound`"""
    q = (words(m, n, state, True) >> np.uint32(8)).astype(np.int64) - 2 ** 23
    scale = np.float32(bound / 2.0 ** 23)
    return torch.from_numpy(q.astype(np.float32) * scale).to(dtype)       # to nearest even


def _grown_bits(rows, columns, n, state, bound, dtype):
    m = int(rows.max()) + 1 if rows.size else 0
    if bound is None or not rows.size:
        return np.zeros(rows.size, dtype=np.int64)
    image = C.bits_of(value_image(m, n, state, bound, dtype)).numpy().astype(np.int64)
    return image[rows, columns]


def _assemble(values, entry_rows, old_columns, kept, grown_flat, n, state, bound):
    """the union of the kept entries and the grown flat positions, ascending -> (rows, columns,
    value bits, source)"""
    old_bits = C.bits_of(values).numpy().astype(np.int64)
    kept_flat = entry_rows[kept] * n + old_columns[kept]
    flat = np.concatenate([kept_flat, grown_flat]).astype(np.int64)
    source = np.concatenate([kept, np.full(grown_flat.size, -1)]).astype(np.int64)
    order = np.argsort(flat, kind="stable")
    flat, source = flat[order], source[order]
    assert np.unique(flat).size == flat.size          # no grown position among the kept ones
    rows, columns = flat // max(n, 1), flat % max(n, 1)
    grown = source < 0
    bits = np.where(grown, 0, old_bits[np.maximum(source, 0)]) if old_bits.size else np.zeros(0, dtype=np.int64)
    if grown.any():
        bits[grown] = _grown_bits(rows[grown], columns[grown], n, state, bound, values.dtype)
    bit_type = C.BITS[values.element_size()]
    return rows, columns, torch.from_numpy(bits).to(bit_type).view(values.dtype), torch.from_numpy(source)


def rule_per_row(values, row_offsets, column_indices, drop_counts, n, state, key_mask=DEFAULT, bound=None):
    """The rule per row: stable descending argsorts of the value keys over the row's entries
    (Kept) and of the generated keys over the row's open columns (Grown)."""
    m = row_offsets.numel() - 1
    offsets, old_columns = row_offsets.numpy().astype(np.int64), column_indices.numpy().astype(np.int64)
    value_keys = C.keys(values).numpy()
    score_keys = keys(m, n, state, key_mask).astype(np.int64)
    entry_rows = np.repeat(np.arange(m), offsets[1:] - offsets[:-1])
    kept, grown_flat = [], []
    for r in range(m):
        begin, end = offsets[r], offsets[r + 1]
        d = min(max(int(drop_counts[r]), 0), end - begin)
        order = np.argsort(-value_keys[begin:end], kind="stable")[: end - begin - d]
        kept.append(begin + order)
        row_keys = score_keys[r].copy()
        row_keys[old_columns[begin + order]] = -1
        grown = np.argsort(-row_keys, kind="stable")[:d]
        assert d == 0 or row_keys[grown].min() >= 0
        grown_flat.append(r * n + grown)
    kept = np.concatenate(kept + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    grown_flat = np.concatenate(grown_flat + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    rows, columns, new_values, source = _assemble(values, entry_rows, old_columns, kept, grown_flat, n, state, bound)
    assert np.array_equal(np.bincount(rows, minlength=m), offsets[1:] - offsets[:-1])     # the rows keep their lengths
    return torch.from_numpy(columns).to(torch.int32), new_values, source


def rule_total(values, row_offsets, column_indices, d, n, state, key_mask=DEFAULT, bound=None):
    """The rule matrix-wide: stable descending argsorts over entry indices (Kept) and over flat
    indices (Grown)."""
    m = row_offsets.numel() - 1
    nnz = values.numel()
    offsets, old_columns = row_offsets.numpy().astype(np.int64), column_indices.numpy().astype(np.int64)
    entry_rows = np.repeat(np.arange(m), offsets[1:] - offsets[:-1])
    kept = np.argsort(-C.keys(values).numpy(), kind="stable")[: nnz - d].astype(np.int64)
    score_keys = keys(m, n, state, key_mask).astype(np.int64).reshape(-1)
    score_keys[entry_rows[kept] * n + old_columns[kept]] = -1
    grown_flat = np.argsort(-score_keys, kind="stable")[:d].astype(np.int64)
    assert d == 0 or score_keys[grown_flat].min() >= 0
    rows, columns, new_values, source = _assemble(values, entry_rows, old_columns, kept, grown_flat, n, state, bound)
    new_offsets = torch.zeros(m + 1, dtype=torch.int32)
    new_offsets[1:] = torch.from_numpy(np.cumsum(np.bincount(rows, minlength=m)))
    row_indices = torch.argsort(new_offsets[1:] - new_offsets[:-1], stable=True).to(torch.int32)
    return row_indices, new_offsets, torch.from_numpy(columns).to(torch.int32), new_values, source


def state_tensor(state, device="cpu"):
    return torch.tensor(state, dtype=torch.int64, device=device)


def torch_per_row(values, row_offsets, column_indices, drop_counts, n, state, key_mask=DEFAULT, bound=None):
    """topology.regrow_per_row_random on CPU tensors (the torch path)"""
    return topology.regrow_per_row_random(values, row_offsets, column_indices, drop_counts, n, grow_bound=bound,
                                          rng_state=state_tensor(state), key_mask=key_mask)


def torch_total(values, row_offsets, column_indices, d, n, state, key_mask=DEFAULT, bound=None):
    return topology.regrow_total_random(values, row_offsets, column_indices, d, n, grow_bound=bound,
                                        rng_state=state_tensor(state), key_mask=key_mask)


def assert_same(got, want, names, where=""):
    assert len(got) == len(want) == len(names)
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where, g.dtype, w.dtype, g.shape, w.shape)
        g, w = g.cpu(), w.cpu()
        same = torch.equal(C.bits_of(g), C.bits_of(w)) if name == "values" else torch.equal(g, w)
        assert same, (name, where)


def pattern(m, n, density, dtype, generator):
    """(values, row_offsets, column_indices) of an m x n pattern: density 0 = all rows empty,
    1 = all rows full, else ragged rows of about that share with an empty and a full row among
    them where there is room; quantised values (ties) without specials among them"""
    if density == 0.0:
        lengths = torch.zeros(m, dtype=torch.int64)
    elif density == 1.0:
        lengths = torch.full((m,), n, dtype=torch.int64)
    else:
        lengths = torch.binomial(torch.full((m,), float(n)), torch.full((m,), density), generator=generator).long()
        if m >= 3:
            lengths[m // 2], lengths[m - 1] = 0, n
    row_offsets, column_indices = C.csr(lengths, n, generator)
    values = C.quantised(column_indices.numel(), dtype, generator, special=False)
    return values, row_offsets, column_indices


DROPS = ("none", "one", "third", "all")


def drop_counts(row_offsets, how):
    lengths = (row_offsets[1:] - row_offsets[:-1]).to(torch.int32)
    if how == "none":
        return torch.zeros_like(lengths)
    if how == "one":
        return torch.minimum(lengths, torch.ones_like(lengths))
    if how == "third":
        return torch.div(lengths + 2, 3, rounding_mode="floor").to(torch.int32)
    return lengths.clone()


def drop_total(nnz, how):
    return {"none": 0, "one": min(1, nnz), "third": (nnz + 2) // 3, "all": nnz}[how]
