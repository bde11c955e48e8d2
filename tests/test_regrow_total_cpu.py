"""CPU: the matrix-wide drop-and-grow step (topology.regrow_total, the matrix-wide branch of
SparseLinear.update_topology) on CPU tensors against a brute-force statement of the rule, and the
host-only queries of the device step.  Everything is an integer or a bit copy: every comparison
is exact."""
import pytest
import torch

from tests import regrow_total_cases as C
from torch_sputnik_amd import SparseLinear, capi, ops, topology

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
ids = dict(ids=lambda d: str(d).split(".")[-1])


def check(values, row_offsets, column_indices, d, scores, note=""):
    want = C.brute_force(values, row_offsets, column_indices, d, scores)
    where = f"{tuple(scores.shape)} {scores.dtype} values {values.dtype} d {d} {note}"
    got = topology.regrow_total(values, row_offsets, column_indices, d, scores)
    C.assert_same(got, want, where)
    C.assert_same(topology.regrow_total_composed(values, row_offsets, column_indices, d, scores), want, where)
    assert int(got[1][-1]) == values.numel() and int((got[4] == -1).sum()) == d
    return got


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
@pytest.mark.parametrize("value_dtype", DTYPES, **ids)
def test_ragged_patterns_with_ties_and_specials(value_dtype, score_dtype):
    """Empty rows, full rows and random ones; quantised values and scores (many ties) with NaN,
    +-inf, +-0, finfo.max and a denormal among both; every count edge."""
    generator = torch.Generator().manual_seed(71)
    m, n = 13, 37
    lengths = torch.randint(0, n + 1, (m,), generator=generator)
    lengths[0], lengths[3], lengths[4], lengths[12] = 0, n, 0, n
    row_offsets, column_indices = C.csr(lengths, n, generator)
    values = C.quantised(column_indices.numel(), value_dtype, generator)
    scores = C.quantised((m, n), score_dtype, generator)
    nnz = values.numel()
    for d in (0, 1, nnz // 3, nnz - 1, nnz):
        if d > m * n - (nnz - d):
            continue
        got = check(values, row_offsets, column_indices, d, scores)
        if d == 0:
            assert torch.equal(got[2], column_indices) and torch.equal(got[1], row_offsets)
            assert torch.equal(got[4], torch.arange(nnz))
        if d == nnz:
            assert bool((got[4] == -1).all()) and not C.bits_of(got[3]).any()


def test_count_edges():
    generator = torch.Generator().manual_seed(72)
    # no entries
    for m, n in ((5, 7), (0, 7), (3, 0), (0, 0)):
        empty = (torch.zeros(0), torch.zeros(m + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
        got = check(*empty, 0, C.quantised((m, n), torch.float32, generator))
        assert got[0].tolist() == list(range(m)) and got[2].numel() == 0
    # a full pattern: what is grown is exactly what was dropped
    m, n = 6, 9
    row_offsets, column_indices = C.csr([n] * m, n, generator)
    values = C.quantised(m * n, torch.float32, generator)
    for d in (0, 1, 20, m * n):
        got = check(values, row_offsets, column_indices, d, C.quantised((m, n), torch.float16, generator))
        assert torch.equal(got[2], column_indices) and torch.equal(got[1], row_offsets)
    # one row, one column
    check(torch.tensor([2.0]), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), 1,
          torch.tensor([[3.0]]))
    with pytest.raises(ValueError):
        topology.regrow_total(values, row_offsets, column_indices, m * n + 1, torch.zeros(m, n))
    with pytest.raises(ValueError):
        topology.regrow_total(values, row_offsets, column_indices, -1, torch.zeros(m, n))
    with pytest.raises(ValueError):
        topology.regrow_total(values, row_offsets[:-1], column_indices, 1, torch.zeros(m, n))
    with pytest.raises(RuntimeError):
        ops.csr_regrow_total(values, row_offsets, column_indices, 1, torch.zeros(m, n))      # CPU tensors


def test_all_scores_equal_and_all_values_equal():
    """Constant scores: Grown is the first d open positions in row-major order.  Constant values:
    the drop takes the highest entry indices."""
    generator = torch.Generator().manual_seed(73)
    m, n = 7, 19
    values, row_offsets, column_indices, _ = C.random_case(m, n, torch.float32, torch.float32, generator)
    nnz = values.numel()
    d = min(nnz, m * n - nnz) // 2 + 1
    got = check(values, row_offsets, column_indices, d, torch.full((m, n), -2.5))
    lengths = (got[1][1:] - got[1][:-1]).to(torch.int64)
    flat = torch.repeat_interleave(torch.arange(m), lengths) * n + got[2]
    kept = set(flat[got[4] >= 0].tolist())
    free = [p for p in range(m * n) if p not in kept]
    assert flat[got[4] == -1].tolist() == free[:d]
    constant = torch.full((nnz,), 0.75)
    constant[1::2] = -0.75
    got = check(constant, row_offsets, column_indices, d, C.quantised((m, n), torch.float32, generator))
    assert got[4][got[4] >= 0].tolist() == list(range(nnz - d))


def test_other_dtypes_rank_as_float():
    generator = torch.Generator().manual_seed(74)
    values, row_offsets, column_indices, scores = C.random_case(9, 21, torch.float32, torch.float32, generator)
    d = values.numel() // 4
    # float64 scores whose float32 images tie
    double = scores.double() + 1e-12 * torch.randn(9, 21, generator=generator, dtype=torch.float64)
    want = check(values, row_offsets, column_indices, d, double.float())
    C.assert_same(check(values, row_offsets, column_indices, d, double, note="float64 scores"), want)
    got = check(values.double(), row_offsets, column_indices, d, scores, note="float64 values")
    assert got[3].dtype == torch.float64


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), **ids)
def test_update_topology_is_regrow_total_on_the_layers_arrays(dtype):
    generator = torch.Generator().manual_seed(75)
    out_f, in_f = 24, 40
    module = SparseLinear.from_dense(torch.randn(out_f, in_f, generator=generator).to(dtype), density=0.3)
    parameter, nnz = module.values, module.values.numel()
    old = (module.values.detach().clone(), module.row_offsets, module.column_indices, module.row_indices)
    scores = torch.randn(out_f, in_f, generator=generator)
    scores[1, 2], scores[3, 4], scores[5, 6] = float("nan"), float("inf"), -float("inf")
    d = int(0.3 * nnz)
    want = topology.regrow_total(old[0], old[1], old[2], d, scores)
    C.assert_same(want, C.brute_force(old[0], old[1], old[2], d, scores))
    source = module.update_topology(0.3, scores)
    assert module.values is parameter and module.values.numel() == nnz
    C.assert_same((module.row_indices, module.row_offsets, module.column_indices, module.values.detach(), source),
                  want)
    assert all(new is not t for new, t in zip((module.row_offsets, module.column_indices, module.row_indices),
                                              old[1:]))
    assert int((source == -1).sum()) == d
    # SET: random scores from the generator, drawn as before
    seeded = torch.Generator().manual_seed(5)
    random_scores = torch.rand(out_f, in_f, generator=seeded)
    before = (module.values.detach().clone(), module.row_offsets, module.column_indices)
    want = topology.regrow_total(*before, int(0.2 * nnz), random_scores)
    source = module.update_topology(0.2, generator=torch.Generator().manual_seed(5))
    C.assert_same((module.row_indices, module.row_offsets, module.column_indices, module.values.detach(), source),
                  want)
    # d = 0 changes nothing
    kept = (module.row_indices, module.row_offsets, module.column_indices)
    assert torch.equal(module.update_topology(0.0, scores), torch.arange(nnz))
    assert all(a is b for a, b in zip(kept, (module.row_indices, module.row_offsets, module.column_indices)))


def test_queries_are_host_only():
    """served and the limits at the last row and column served and one beyond; the launch
    count; the workspace bytes, counted from the layout."""
    shape = capi.csr_regrow_total_launch_shape(2048, 2048, 838860, 4, 4)
    assert shape["served"] and shape["max_m"] == 16384 and shape["rows_per_wave"] == 1
    assert shape["value_digit_passes"] == 4 and shape["score_digit_passes"] == 4 and shape["launches"] == 16
    assert shape["lds_bytes"] == shape["rows_per_workgroup"] * 8 * 64 and shape["grid"] == 512
    topk = capi.csr_topk_launch_shape(2048, 2048, 838860, 4, True)
    assert (shape["value_rows_per_wave"], shape["value_rows_grid"], shape["flat_grid"]) == \
        (topk["rows_per_wave"], topk["rows_grid"], topk["flat_grid"])
    walk = capi.dense_to_csr_launch_shape(1, 2048, 2048, 4)
    assert all(shape[k] == walk[k] for k in ("rows_per_wave", "elements_per_lane", "rows_per_workgroup", "grid"))
    half = capi.csr_regrow_total_launch_shape(100, 30, 500, 2, 2)
    assert half["launches"] == 12 and half["elements_per_lane"] == 8 and half["rows_per_wave"] == 16
    max_m, max_n = shape["max_m"], shape["max_n"]
    assert max_n >= capi.csr_regrow_launch_shape(1, 1, 4, 4)["max_n"]
    assert capi.csr_regrow_total_launch_shape(max_m, 8, 100, 4, 4)["served"]
    beyond = capi.csr_regrow_total_launch_shape(max_m + 1, 8, 100, 4, 4)
    assert not beyond["served"] and beyond["max_m"] == max_m and beyond["grid"] == -1
    widest = capi.csr_regrow_total_launch_shape(3, max_n, 100, 2, 4)
    assert widest["served"] and widest["lds_bytes"] == 64 * 1024
    beyond = capi.csr_regrow_total_launch_shape(3, max_n + 1, 100, 2, 4)
    assert not beyond["served"] and beyond["max_n"] == max_n
    assert capi.csr_regrow_total_launch_shape(0, 5, 0, 4, 4)["launches"] == 0
    assert capi.csr_regrow_total_launch_shape(5, 5, 0, 4, 4)["launches"] == 1
    for bad in ((-1, 8, 1, 4, 4), (8, -1, 1, 4, 4), (8, 8, -1, 4, 4), (8, 8, 1, 3, 4), (8, 8, 1, 4, 8),
                (1 << 15, 1 << 16, 1, 4, 4)):
        with pytest.raises(RuntimeError):
            capi.csr_regrow_total_launch_shape(*bad)
    m, n = 2048, 2048
    select = 4 * 256 + 1 + 2 * m                      # bins, threshold, quotas and tie counts
    assert capi.csr_regrow_total_workspace_bytes(m, n, 838860) == 4 * (2 * select + m + 1 + 2 * m * (n // 32))
    assert capi.csr_regrow_total_workspace_bytes(3, 33, 5) == 4 * (2 * (1025 + 6) + 4 + 2 * 3 * 2)
    assert capi.csr_regrow_total_workspace_bytes(-1, 8, 1) == 0
