"""CPU: per-row drop-and-grow without a device -- the torch path of topology.regrow_per_row
against an independent statement of the rule (a Python loop per row, sorting (-key, column)),
SparseLinear.update_topology(per_row=True) on a CPU module, the host-only launch query and the
argument errors.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def bits_of(t):
    """integer view of a tensor's elements (value bits compare exactly, NaN included)"""
    return t.contiguous().view(BITS[t.element_size()])


def numpy_keys(x):
    """bit pattern without the sign, as int64 -- stated with numpy alone"""
    if x.element_size() == 2:
        return x.contiguous().view(torch.int16).numpy().astype(np.int64) & 0x7fff
    return x.contiguous().view(torch.int32).numpy().astype(np.int64) & 0x7fffffff


def loop_rule(values, row_offsets, column_indices, drop_counts, scores):
    """(column_indices, value bits, source) of the new pattern, row by row"""
    value_keys = numpy_keys(values)
    limit = int(numpy_keys(torch.tensor([torch.finfo(scores.dtype).max], dtype=scores.dtype))[0])
    score_keys = np.minimum(numpy_keys(scores), limit)
    old_bits = bits_of(values).numpy()
    offsets, columns, counts = row_offsets.numpy(), column_indices.numpy(), drop_counts.numpy()
    n = scores.shape[1]
    new_columns, new_bits, source = [], [], []
    for r in range(scores.shape[0]):
        begin, end = int(offsets[r]), int(offsets[r + 1])
        drop = min(max(int(counts[r]), 0), end - begin)
        by_key = sorted(range(begin, end), key=lambda i: (-value_keys[i], columns[i]))
        kept = {int(columns[i]): i for i in by_key[:end - begin - drop]}
        free = [c for c in range(n) if c not in kept]
        grown = sorted(free, key=lambda c: (-score_keys[r, c], c))[:drop]
        for c in sorted(list(kept) + grown):
            new_columns.append(c)
            source.append(kept.get(c, -1))
            new_bits.append(old_bits[kept[c]] if c in kept else 0)
    return (np.array(new_columns, np.int32), np.array(new_bits, old_bits.dtype), np.array(source, np.int64))


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def specials(dtype):
    """NaN, +-inf, +-0, the largest finite value, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.375, -0.375,
                                    torch.finfo(dtype).max], dtype=dtype), from_bits([1], dtype)])


def quantised(shape, dtype, generator):
    """few distinct magnitudes: many ties, signs mixed"""
    return ((torch.randn(shape, generator=generator) / 0.25).round() * 0.25).to(dtype)


def pattern(m, n, value_dtype, score_dtype, generator):
    """A ragged CSR pattern with an empty row, a full row, an all-equal row and an all-zero row,
    the special values among values and scores."""
    lengths = torch.randint(1, n, (m,), generator=generator)
    lengths[2], lengths[3] = 0, n
    columns = [torch.sort(torch.randperm(n, generator=generator)[:int(k)]).values for k in lengths]
    row_offsets = torch.zeros(m + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    column_indices = torch.cat(columns).to(torch.int32)
    values = quantised(column_indices.numel(), value_dtype, generator)
    values[row_offsets[4]:row_offsets[5]] = -1.5
    values[row_offsets[5]:row_offsets[6]] = 0.0
    s = specials(value_dtype)
    values[1::7][:s.numel()] = s[:values[1::7].numel()]
    values[row_offsets[3]:row_offsets[3] + 4] = torch.tensor([float("nan"), -0.0, float("inf"), 0.0], dtype=value_dtype)
    scores = quantised((m, n), score_dtype, generator)
    scores[4] = 2.0
    scores[5] = 0.0
    s = specials(score_dtype)
    scores.view(-1)[2::11][:s.numel()] = s[:scores.view(-1)[2::11].numel()]
    return values, row_offsets, column_indices, scores, lengths.to(torch.int32)


def drop_cases(lengths, generator):
    yield "none", torch.zeros_like(lengths)
    yield "one", torch.ones_like(lengths)
    yield "all but one", lengths - 1
    yield "all", lengths.clone()
    yield "random", (torch.rand(lengths.numel(), generator=generator) * (lengths + 1)).to(torch.int32)
    yield "clamped", torch.where(torch.arange(lengths.numel()) % 2 == 0, lengths + 5, torch.full_like(lengths, -3))


def check_against_loop(values, row_offsets, column_indices, drop_counts, scores, note=""):
    got = topology.regrow_per_row(values, row_offsets, column_indices, drop_counts, scores)
    want = loop_rule(values, row_offsets, column_indices, drop_counts, scores)
    assert got[0].dtype == torch.int32 and got[1].dtype == values.dtype and got[2].dtype == torch.int64
    for g, w, name in zip((got[0], bits_of(got[1]), got[2]), want, ("column_indices", "values", "source")):
        assert np.array_equal(g.numpy(), w), (name, note)
    return got


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
@pytest.mark.parametrize("value_dtype", DTYPES, **ids)
def test_torch_path_matches_the_loop_rule(value_dtype, score_dtype):
    generator = torch.Generator().manual_seed(21)
    values, row_offsets, column_indices, scores, lengths = pattern(9, 13, value_dtype, score_dtype, generator)
    for note, drop_counts in drop_cases(lengths, generator):
        new_columns, new_values, source = check_against_loop(values, row_offsets, column_indices, drop_counts,
                                                             scores, note)
        if note == "none":
            assert torch.equal(new_columns, column_indices) and torch.equal(bits_of(new_values), bits_of(values))
            assert torch.equal(source, torch.arange(values.numel()))
        if note == "all":
            assert bool((source == -1).all()) and not bits_of(new_values).any()
    # a full row keeps its columns whatever it drops; grown entries are +0.0 with source -1
    full = slice(int(row_offsets[3]), int(row_offsets[4]))
    new_columns, new_values, source = topology.regrow_per_row(values, row_offsets, column_indices,
                                                              torch.full_like(lengths, 5), scores)
    assert torch.equal(new_columns[full], torch.arange(13, dtype=torch.int32))
    assert int((source[full] == -1).sum()) == 5
    assert not bits_of(new_values)[full][source[full] == -1].any()


def test_the_clamp_and_the_ties_by_column():
    """NaN / inf scores tie with the largest finite value: growth goes by column among them;
    constant scores grow the lowest free columns; constant values drop the highest columns."""
    for dtype in DTYPES:
        n = 12
        row_offsets = torch.tensor([0, 4, 8], dtype=torch.int32)
        column_indices = torch.tensor([1, 4, 6, 9, 0, 1, 2, 3], dtype=torch.int32)
        values = torch.tensor([2.0, -2.0, 2.0, -2.0, 1.0, 1.0, 1.0, 1.0], dtype=dtype)
        scores = torch.zeros(2, n, dtype=dtype)
        scores[0, 3], scores[0, 5], scores[0, 7], scores[0, 10] = (float("inf"), torch.finfo(dtype).max, float("nan"),
                                                                   -float("inf"))
        scores[1] = -0.5
        drop_counts = torch.tensor([3, 2], dtype=torch.int32)
        new_columns, new_values, source = check_against_loop(values, row_offsets, column_indices, drop_counts, scores)
        # row 0: the ties drop columns 4, 6, 9; the clamped scores tie: columns 3, 5, 7 before 10
        assert new_columns[:4].tolist() == [1, 3, 5, 7] and source[:4].tolist() == [0, -1, -1, -1]
        # row 1: keeps columns 0, 1; every other column ties: 2 and 3 come back, at zero
        assert new_columns[4:].tolist() == [0, 1, 2, 3] and source[4:].tolist() == [4, 5, -1, -1]
        assert new_values[6:].tolist() == [0.0, 0.0]


def test_other_dtypes_rank_as_float():
    generator = torch.Generator().manual_seed(22)
    values, row_offsets, column_indices, scores, lengths = pattern(7, 10, torch.float32, torch.float32, generator)
    finite = torch.nan_to_num(values, nan=3.0, posinf=4.0, neginf=-4.0)
    drop_counts = lengths // 2
    want = topology.regrow_per_row(finite, row_offsets, column_indices, drop_counts, scores)
    got = topology.regrow_per_row(finite.double(), row_offsets, column_indices, drop_counts, scores.double())
    assert got[1].dtype == torch.float64 and torch.equal(got[1], want[1].double())
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


# ---- SparseLinear.update_topology(per_row=True) on a CPU module (no kernel involved) ----

OUT, IN = 12, 20


def cpu_module(density=0.3, seed=5, dtype=torch.float32, per_row=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(OUT, IN, generator=g).to(dtype)
    return SparseLinear.from_dense(w, density=density, per_row=per_row)


def flat_positions(module):
    lengths = (module.row_offsets[1:] - module.row_offsets[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(module.output_features), lengths)
    return rows * module.input_features + module.column_indices.to(torch.int64)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), **ids)
def test_update_topology_per_row_on_a_cpu_module(dtype):
    module = cpu_module(dtype=dtype)
    k = round(0.3 * IN)
    assert torch.equal(module.row_offsets, torch.arange(OUT + 1, dtype=torch.int32) * k)
    parameter, nnz = module.values, module.values.numel()
    old = (module.row_indices, module.row_offsets, module.column_indices)
    old_copies = [t.clone() for t in old]
    old_values = module.values.detach().clone()
    assert functional._is_static(*old)
    g =torch.Generator().manual_seed(6)
    scores = torch.randn(OUT, IN, generator=g)
    scores[0, 0], scores[3, 7], scores[5, 5] = float("nan"), float("inf"), float("-inf")
    d = int(np.floor(np.float64(k) * 0.34))
    assert d == 2
    want = loop_rule(old_values, old[1], old[2], torch.full((OUT,), d, dtype=torch.int32), scores)

    source = module.update_topology(0.34, scores, per_row=True)

    assert module.values is parameter and module.values.numel() == nnz
    assert torch.equal(module.row_offsets, old_copies[1]) and torch.equal(module.row_indices, old_copies[0])
    assert np.array_equal(module.column_indices.numpy(), want[0])
    assert np.array_equal(bits_of(module.values.detach()).numpy(), want[1])
    assert source.dtype == torch.int64 and np.array_equal(source.numpy(), want[2])
    grown = source == -1
    assert torch.equal(grown.reshape(OUT, k).sum(1), torch.full((OUT,), d))
    assert torch.equal(bits_of(module.values.detach())[~grown], bits_of(old_values)[source[~grown]])
    assert torch.equal(old_copies[2][source[~grown]], module.column_indices[~grown])
    assert not bits_of(module.values.detach())[grown].any()                      # exactly +0.0
    # the old index tensors are replaced -- clones for the unchanged ones --, not written to
    assert all(new is not o for new, o in zip((module.row_indices, module.row_offsets, module.column_indices), old))
    assert all(torch.equal(t, c) for t, c in zip(old, old_copies))
    assert functional._is_static(module.row_indices, module.row_offsets, module.column_indices)
    assert not any(functional._is_static(t) for t in old)        # the old ones are unregistered


def test_update_topology_per_row_no_op_and_generator():
    module = cpu_module()
    nnz = module.values.numel()
    before = [t.clone() for t in (module.values.detach(), module.row_indices, module.row_offsets,
                                  module.column_indices)]
    indices = (module.row_indices, module.row_offsets, module.column_indices)
    for fraction in (0.0, 0.9 / IN):                                  # not even a full row drops one
        source = module.update_topology(fraction, per_row=True)
        assert torch.equal(source, torch.arange(nnz))
        assert all(a is b for a, b in zip(indices, (module.row_indices, module.row_offsets, module.column_indices)))
    source = module.update_topology(0.9 / 6, torch.ones(OUT, IN), per_row=True)   # floor(6 * 0.15) = 0 in every row
    assert torch.equal(source, torch.arange(nnz))
    assert all(torch.equal(a, b) for a, b in zip(before, (module.values.detach(), module.row_indices,
                                                          module.row_offsets, module.column_indices)))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            module.update_topology(bad, per_row=True)
    with pytest.raises(ValueError):
        module.update_topology(0.5, torch.zeros(OUT, IN + 1), per_row=True)
    # SET: random growth, reproducible with the generator's seed, row lengths unchanged
    patterns = []
    for seed in (11, 11, 12):
        module = cpu_module()
        source = module.update_topology(0.5, generator=torch.Generator().manual_seed(seed), per_row=True)
        assert torch.equal((source == -1).reshape(OUT, 6).sum(1), torch.full((OUT,), 3))
        assert torch.equal(module.row_offsets, before[2])
        patterns.append(flat_positions(module))
    assert torch.equal(patterns[0], patterns[1]) and not torch.equal(patterns[0], patterns[2])


def test_dropped_positions_are_eligible_again_per_row():
    module = cpu_module()
    flat = flat_positions(module)
    scores = torch.zeros(OUT, IN)
    scores.view(-1)[flat] = -1.0           # the largest |scores| sit on the present pattern
    source = module.update_topology(0.5, scores, per_row=True)
    assert torch.equal(flat_positions(module), flat)          # dropped entries grow back ...
    grown = source == -1
    assert int(grown.sum()) == 3 * OUT
    assert not bits_of(module.values.detach())[grown].any()   # ... at zero


def test_matrix_wide_step_is_unchanged():
    """per_row=False is today's route: the same result as the call without the keyword, which
    loses the row balance per_row=True keeps."""
    g = torch.Generator().manual_seed(7)
    scores = torch.randn(OUT, IN, generator=g)
    results = []
    for kwargs in (dict(), dict(per_row=False)):
        module = cpu_module()
        source = module.update_topology(0.3, scores, **kwargs)
        results.append((source, module.values.detach().clone(), module.row_indices, module.row_offsets,
                        module.column_indices))
    assert all(torch.equal(a, b) for a, b in zip(*results))
    lengths = results[0][3][1:] - results[0][3][:-1]
    assert int(lengths.min()) != int(lengths.max())
    for seed in (3, 3):
        module = cpu_module()
        source = module.update_topology(0.3, generator=torch.Generator().manual_seed(seed), per_row=False)
        results.append((source, module.column_indices))
    assert all(torch.equal(a, b) for a, b in zip(results[-2], results[-1]))


# ---- the host-only query, the C entry and the argument errors ----

def test_launch_query_is_host_only_and_consistent():
    for score_bytes in (2, 4):
        for value_bytes in (2, 4):
            limit = capi.csr_regrow_launch_shape(2, 1, score_bytes, value_bytes)["max_n"]
            assert limit >= 16384
            assert capi.csr_regrow_launch_shape(2, 16384, score_bytes, value_bytes)["served"]
            assert capi.csr_regrow_launch_shape(2, limit, score_bytes, value_bytes)["served"]
            beyond = capi.csr_regrow_launch_shape(2, limit + 1, score_bytes, value_bytes)
            assert not beyond["served"] and beyond["max_n"] == limit and beyond["grid"] == -1
            for n in (1, 16, 17, 64, 65, 100, 257, 2048, 16384, limit):
                shape = capi.csr_regrow_launch_shape(100, n, score_bytes, value_bytes)
                walk = capi.dense_to_csr_launch_shape(1, 100, n, score_bytes)
                assert shape["value_digit_passes"] == value_bytes and shape["score_digit_passes"] == score_bytes
                assert shape["rows_per_wave"] == min(walk["rows_per_wave"], 8)
                assert shape["elements_per_lane"] == walk["elements_per_lane"] == 16 // score_bytes
                assert shape["rows_per_workgroup"] == 4 * shape["rows_per_wave"]
                assert shape["grid"] == -(-100 // shape["rows_per_workgroup"])
                # 256 bins and two bits per column for every row of the workgroup, inside 64 KiB
                assert shape["lds_bytes"] == shape["rows_per_workgroup"] * (1024 + 8 * -(-n // 32)) <= 65536
                # a group covers a row of an instance with several rows per wave in one step
                if shape["rows_per_wave"] > 1:
                    assert n <= (64 // shape["rows_per_wave"]) * shape["elements_per_lane"]
    assert capi.csr_regrow_launch_shape(0, 0, 4, 4)["grid"] == 0
    for args in ((4, 4, 1, 4), (4, 4, 4, 8), (4, 4, 3, 2), (-1, 4, 4, 4), (4, -1, 2, 2), (65536, 32768, 2, 4)):
        with pytest.raises(RuntimeError):
            capi.csr_regrow_launch_shape(*args)


def test_c_abi_rejects_bad_arguments_without_a_device():
    lib = capi.lib()
    invalid = -1   # SPUTNIK_HIP_INVALID_ARGUMENT
    limit = capi.csr_regrow_launch_shape(2, 1, 4, 4)["max_n"]
    buffer = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buffer) + 15) // 16 * 16          # host memory: every call is rejected before a launch
    #        m  n  nnz  offsets columns values vb counts scores sb stride  key limit  ws    bytes  outputs
    calls = (
        (4, 4, 4, None, None, None, 4, None, None, 3, 4, 0x7f7fffff, None, 0, None, None, None),     # score width
        (4, 4, 4, None, None, None, 8, None, None, 4, 4, 0x7f7fffff, None, 0, None, None, None),     # value width
        (4, 4, 4, p, p, p, 4, p, p, 4, -4, 0x7f7fffff, None, 0, p, p, p),                            # negative stride
        (4, 4, -1, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p),                            # negative nnz
        (-1, 4, 4, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p),                            # negative m
        (2, limit + 1, 4, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p),                     # beyond the bitmap
        (65536, 32768, 4, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p),                     # m * n
        (4, 4, 4, p, p, p, 4, p, p, 2, 4, 0x7f7fffff, None, 0, p, p, p),                             # key limit of another width
        (4, 4, 4, None, None, None, 4, None, None, 4, 4, 0x7f7fffff, None, 0, None, None, None),     # no pointers
        (4, 4, 4, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, None),                          # no source
        (4, 4, 4, p, p, p + 2, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p),                         # misaligned values
        (4, 4, 4, p, p, p, 2, p, p + 1, 2, 4, 0x7bff, None, 0, p, p, p),                             # misaligned scores
        (4, 4, 4, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p + 2, p),                         # misaligned out values
        (4, 4, 4, p, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p + 4),                         # misaligned source
        (4, 4, 4, p + 2, p, p, 4, p, p, 4, 4, 0x7f7fffff, None, 0, p, p, p),                         # misaligned offsets
    )
    for call in calls:
        assert lib.sputnik_hip_csr_regrow(*call, None) == invalid, call
    # m = 0 or nnz = 0: nothing to launch, whatever the pointers
    assert lib.sputnik_hip_csr_regrow(0, 4, 4, None, None, None, 4, None, None, 4, 4, 0x7f7fffff, None, 0,
                                      None, None, None, None) == 0
    assert lib.sputnik_hip_csr_regrow(4, 4, 0, None, None, None, 2, None, None, 2, 4, 0x7f7f, None, 0,
                                      None, None, None, None) == 0
    assert lib.sputnik_hip_csr_regrow_workspace_bytes(100, 7, 50) == 0


def test_argument_errors():
    values = torch.ones(5)
    row_offsets = torch.tensor([0, 2, 5], dtype=torch.int32)
    column_indices = torch.tensor([0, 3, 1, 2, 5], dtype=torch.int32)
    drop_counts = torch.tensor([1, 1], dtype=torch.int32)
    scores = torch.zeros(2, 6)
    good = dict(values=values, row_offsets=row_offsets, column_indices=column_indices, drop_counts=drop_counts,
                scores=scores)
    bad = (dict(scores=scores.reshape(-1)), dict(scores=torch.zeros(3, 6)), dict(row_offsets=row_offsets.long()),
           dict(row_offsets=row_offsets[:2]), dict(column_indices=column_indices[:4]),
           dict(column_indices=column_indices.long()), dict(drop_counts=drop_counts.long()),
           dict(drop_counts=torch.zeros(3, dtype=torch.int32)), dict(values=values.reshape(5, 1)),
           dict(values=torch.ones(4)))
    for fn in (ops.csr_regrow, topology.regrow_per_row):
        for change in bad:
            with pytest.raises(ValueError):
                fn(**{**good, **change})
    with pytest.raises(ValueError):
        ops.csr_regrow(**{**good, "values": values.double()})
    with pytest.raises(ValueError):
        ops.csr_regrow(**{**good, "scores": scores.double()})
    with pytest.raises(RuntimeError):
        ops.csr_regrow(**good)                               # CPU tensors: the op is device only
    assert len(topology.regrow_per_row(**good)) == 3
