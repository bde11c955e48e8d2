"""Shared by tests/test_regrow_total_cpu.py and tests/test_gpu_regrow_total.py: the rule of the
matrix-wide drop-and-grow step (topology.regrow_total) stated by brute force, and the inputs
both files build.  CPU tensors only; everything is an integer or a bit copy."""
import torch

from torch_sputnik_amd import topology

BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
RANKED = (torch.float32, torch.float16, torch.bfloat16)
NAMES = ("row_indices", "row_offsets", "column_indices", "values", "source")


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()])


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def width(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def keys(x):
    """the bit pattern without the sign, as an int64; other dtypes rank as float32"""
    x = (x if x.dtype in RANKED else x.float()).contiguous()
    if x.element_size() == 2:
        return x.view(torch.int16).to(torch.int64) & 0x7fff
    return x.view(torch.int32).to(torch.int64) & 0x7fffffff


def brute_force(values, row_offsets, column_indices, d, scores):
    """The rule itself: stable descending argsorts of the keys over entry indices (Kept) and over
    flat indices (Grown), then the union as a CSR pattern."""
    m, n = scores.shape
    nnz = values.numel()
    lengths = (row_offsets[1:] - row_offsets[:-1]).to(torch.int64)
    flat = torch.repeat_interleave(torch.arange(m), lengths) * n + column_indices.to(torch.int64)
    kept_entries = torch.argsort(keys(values), descending=True, stable=True)[: nnz - d]
    ranked = scores if scores.dtype in RANKED else scores.float()
    limit = int(keys(torch.tensor([torch.finfo(ranked.dtype).max], dtype=ranked.dtype))[0])
    score_keys = keys(ranked).clamp(max=limit).reshape(-1)
    score_keys[flat[kept_entries]] = -1                                  # Kept is not open
    grown = torch.argsort(score_keys, descending=True, stable=True)[:d]
    assert d == 0 or int(score_keys[grown].min()) >= 0
    entry = torch.full((m * n,), -1, dtype=torch.int64)
    entry[flat[kept_entries]] = kept_entries
    new_flat = torch.sort(torch.cat([flat[kept_entries], grown])).values
    source = entry[new_flat]
    old_bits = bits_of(values)
    new_bits = torch.where(source >= 0, old_bits[source.clamp(min=0)], torch.zeros(1, dtype=old_bits.dtype))
    new_rows = torch.div(new_flat, max(n, 1), rounding_mode="floor")
    new_offsets = torch.zeros(m + 1, dtype=torch.int32)
    new_offsets[1:] = torch.cumsum(torch.bincount(new_rows, minlength=m), 0)
    row_indices = torch.argsort(new_offsets[1:] - new_offsets[:-1], stable=True).to(torch.int32)
    return (row_indices, new_offsets, (new_flat - new_rows * n).to(torch.int32), new_bits.view(values.dtype), source)


def torch_path(values, row_offsets, column_indices, d, scores):
    """topology.regrow_total with the device build off"""
    topology.enable_device_build(False)
    try:
        return topology.regrow_total(values, row_offsets, column_indices, d, scores)
    finally:
        topology.enable_device_build(True)


def assert_same(got, want, where=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where, g.dtype, w.dtype, g.shape, w.shape)
        g, w = g.cpu(), w.cpu()
        same = torch.equal(bits_of(g), bits_of(w)) if name == "values" else torch.equal(g, w)
        assert same, (name, where)


def specials(dtype):
    """NaN, +-inf, +-0, the largest finite value, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.375, -0.375,
                                    torch.finfo(dtype).max], dtype=dtype), from_bits([1], dtype)])


def quantised(shape, dtype, generator, quantum=0.125, special=True):
    """few distinct magnitudes, multiples of the quantum (many ties, signs mixed), with the
    special values among them"""
    x = ((torch.randn(shape, generator=generator) / quantum).round() * quantum).to(dtype)
    if special:
        flat, s = x.reshape(-1), specials(dtype)
        flat[1::5][: s.numel()] = s[: flat[1::5].numel()]
    return x


def csr(lengths, n, generator):
    """row_offsets and ascending random columns of rows of these lengths"""
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    row_offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    columns = [torch.sort(torch.randperm(n, generator=generator)[: int(k)]).values for k in lengths]
    return row_offsets, torch.cat(columns + [torch.zeros(0, dtype=torch.int64)]).to(torch.int32)


def random_case(m, n, value_dtype, score_dtype, generator):
    """ragged random rows, quantised values and scores -> (values, row_offsets, column_indices, scores)"""
    lengths = torch.randint(0, n + 1, (m,), generator=generator)
    row_offsets, column_indices = csr(lengths, n, generator)
    values = quantised(column_indices.numel(), value_dtype, generator)
    scores = quantised((m, n), score_dtype, generator)
    return values, row_offsets, column_indices, scores
