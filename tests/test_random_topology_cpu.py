"""CPU: the torch path of the random topologies (topology.random_csr, SparseLinear.random)
against a numpy restatement of the rule written here -- tests/philox_ref's Philox4x32-10, a
stable argsort of the keys and the value formula; it does not call the product's Philox -- and
topology.erk_densities.  Everything is an integer or a bit pattern: every comparison is exact."""
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from torch_sputnik_amd import SparseLinear, ops, topology

LO = 0xFFFFFFFF
CPU = torch.device("cpu")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
SHAPES = ((1, 1), (3, 5), (8, 16), (17, 33), (5, 257))
STATES = ((1, 0), (2 ** 40 + 17, 4 * 10 ** 9))      # the second one exercises the high words


def words(m, n, seed, offset, values):
    """int64 [m, n]: word c & 3 of Philox(seed, (offset / 4, c >> 2, r)), r | 2**31 for the values"""
    assert offset % 4 == 0
    c = offset // 4
    r = (np.arange(m, dtype=np.uint64)[:, None] | np.uint64(0x80000000 if values else 0)).astype(np.uint32)
    e = np.arange(n, dtype=np.int64)[None, :]
    stacked = np.stack(P.philox4x32_10((seed & LO, seed >> 32), (c & LO, c >> 32, (e >> 2).astype(np.uint32), r)))
    return np.take_along_axis(stacked, np.broadcast_to((e & 3)[None], (1, m, n)), 0)[0].astype(np.int64)


def value_bits(q, bound, dtype):
    """float32(q) * float32(bound / 2**23), rounded to nearest even into dtype, as integers"""
    x = q.astype(np.float32) * np.float32(bound / 2.0 ** 23)
    if dtype == torch.float32:
        return x.view(np.int32).astype(np.int64)
    if dtype == torch.float16:
        return x.astype(np.float16).view(np.int16).astype(np.int64)
    bits = x.view(np.uint32).astype(np.uint64)           # bfloat16: the upper half, ties to even
    return ((bits + np.uint64(0x7FFF) + ((bits >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) \
        .astype(np.uint16).view(np.int16).astype(np.int64)


def restated(m, n, per_row, total, dtype, bound, seed, offset, key_mask=0x7FFFFFFF):
    """-> (row_indices, row_offsets, column_indices, value bits), int64 arrays"""
    keys = words(m, n, seed, offset, False) & key_mask
    if per_row is not None:
        kept = np.argsort(-keys, axis=1, kind="stable")[:, :per_row]
        flat = (np.sort(kept, axis=1) + np.arange(m)[:, None] * n).reshape(-1)
        row_offsets = np.arange(m + 1) * per_row
        row_indices = np.arange(m)
    else:
        flat = np.sort(np.argsort(-keys.reshape(-1), kind="stable")[:total])
        lengths = np.bincount(flat // n, minlength=m)
        row_offsets = np.concatenate([[0], np.cumsum(lengths)])
        row_indices = np.argsort(lengths, kind="stable")
    q = (words(m, n, seed, offset, True).reshape(-1)[flat] >> 8) - 2 ** 23
    return row_indices, row_offsets, flat % n, value_bits(q, bound, dtype)


def as_arrays(values, row_indices, row_offsets, column_indices):
    views = {4: torch.int32, 2: torch.int16}
    return (row_indices.numpy().astype(np.int64), row_offsets.numpy().astype(np.int64),
            column_indices.numpy().astype(np.int64),
            values.contiguous().view(views[values.element_size()]).numpy().astype(np.int64))


def assert_equal(got, want, where):
    for name, g, w in zip(("row_indices", "row_offsets", "column_indices", "values"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), f"{name} differs: {where}"


def counts(most):
    return sorted({0, min(1, most), most // 3 + (1 if most > 2 else 0), most})


def check_structure(m, n, count, per_row, bound, values, row_indices, row_offsets, column_indices):
    nnz = count * m if per_row else count
    assert values.numel() == nnz and column_indices.numel() == nnz
    assert row_indices.dtype == row_offsets.dtype == column_indices.dtype == torch.int32
    assert row_offsets.numel() == m + 1 and int(row_offsets[0]) == 0 and int(row_offsets[-1]) == nnz
    lengths = row_offsets[1:] - row_offsets[:-1]
    assert bool((lengths >= 0).all())
    if per_row:
        assert bool((lengths == count).all())
    assert torch.equal(row_indices, torch.argsort(lengths, stable=True).to(torch.int32))   # diffsort's order
    assert sorted(row_indices.tolist()) == list(range(m))
    for r in range(m):
        columns = column_indices[int(row_offsets[r]):int(row_offsets[r + 1])].tolist()
        assert all(a < b for a, b in zip(columns, columns[1:])), "ascending, no duplicates"
        assert all(0 <= c < n for c in columns)
    assert bool((values.float().abs() <= bound).all())


@pytest.mark.parametrize("state", STATES, ids=("low", "high"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_torch_path_equals_the_restatement(shape, state):
    m, n = shape
    seed, offset = state
    rng_state = torch.tensor([seed, offset], dtype=torch.int64)
    for per_row in (False, True):
        for count in counts(n if per_row else m * n):
            for dtype in DTYPES:
                bound = 0.75
                got = topology.random_csr(m, n, nonzeros=count, per_row=per_row, dtype=dtype, bound=bound,
                                          rng_state=rng_state)
                assert got[0].dtype == dtype
                want = restated(m, n, count if per_row else None, None if per_row else count, dtype, bound,
                                seed, offset)
                where = f"{m}x{n} {'per row' if per_row else 'total'} {count} {dtype} state {state}"
                assert_equal(as_arrays(*got), want, where)
                check_structure(m, n, count, per_row, bound, *got)


def helper(m, n, per_row, total, key_mask, dtype=torch.float32, bound=1.0, seed=7, offset=8):
    row_indices, row_offsets, column_indices, values = topology._random_csr_torch(
        m, n, per_row, total, dtype, ops.random_value_scale(bound), seed, offset, CPU, key_mask=key_mask)
    return values, row_indices, row_offsets, column_indices


def test_equal_keys_keep_the_first_positions():
    """key_mask = 0: every key ties, the lowest flat indices (columns, per row) win"""
    m, n = 5, 33
    for total in (0, 1, 40, 99, m * n):
        _, _, row_offsets, column_indices = helper(m, n, None, total, 0)
        lengths = (row_offsets[1:] - row_offsets[:-1]).tolist()
        flat = [r * n + c for r in range(m) for c in column_indices[int(row_offsets[r]):int(row_offsets[r + 1])].tolist()]
        assert flat == list(range(total)) and sum(lengths) == total
    for k in (0, 1, 7, n):
        _, _, row_offsets, column_indices = helper(m, n, k, None, 0)
        assert column_indices.tolist() == list(range(k)) * m
        assert row_offsets.tolist() == [r * k for r in range(m + 1)]


@pytest.mark.parametrize("shape", ((8, 16), (17, 33), (5, 257)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_everywhere_equal_the_restatement(shape):
    """key_mask = 0x7: eight distinct keys, ties in every row"""
    m, n = shape
    for per_row in (False, True):
        for count in counts(n if per_row else m * n):
            k, total = (count, None) if per_row else (None, count)
            got = helper(m, n, k, total, 0x7, torch.float16, 0.5)
            assert_equal(as_arrays(*got), restated(m, n, k, total, torch.float16, 0.5, 7, 8, key_mask=0x7),
                         f"{m}x{n} {'per row' if per_row else 'total'} {count} under key_mask 7")
            check_structure(m, n, count, per_row, 0.5, *got)


def test_default_bound_and_arguments():
    """bound=None is 1 / sqrt(max(1, entries per row)); counts follow magnitude_prune"""
    m, n = 8, 64
    state = torch.tensor([3, 0], dtype=torch.int64)
    for per_row, kwargs, per in ((True, dict(density=0.25), 16), (False, dict(nonzeros=128), 16),
                                 (False, dict(nonzeros=4), 0.5), (True, dict(nonzeros=0), 0)):
        values, _, row_offsets, _ = topology.random_csr(m, n, per_row=per_row, rng_state=state, **kwargs)
        bound = 1.0 / math.sqrt(max(1.0, per))
        explicit = topology.random_csr(m, n, per_row=per_row, rng_state=state, bound=bound, **kwargs)[0]
        assert torch.equal(values, explicit)
        assert bool((values.abs() <= bound).all())
        if values.numel() >= 64:
            assert float(values.abs().max()) > 0.8 * bound     # (128 uniform draws: all below 0.8 has p = 4e-13)
    assert topology.random_csr(m, n, density=0.3)[0].numel() == round(0.3 * m * n)
    assert topology.random_csr(m, n, density=0.3, per_row=True)[0].numel() == round(0.3 * n) * m
    values, _, _, _, used = topology.random_csr(m, n, density=0.1, return_rng_state=True)
    assert used.dtype == torch.int64 and used.numel() == 2 and int(used[1]) == 0
    assert torch.equal(values, topology.random_csr(m, n, density=0.1, rng_state=used)[0])
    torch.manual_seed(5)
    first = topology.random_csr(m, n, density=0.1)
    torch.manual_seed(5)
    assert all(torch.equal(a, b) for a, b in zip(first, topology.random_csr(m, n, density=0.1)))
    for bad in (dict(), dict(density=0.1, nonzeros=3), dict(density=1.5), dict(nonzeros=m * n + 1),
                dict(nonzeros=n + 1, per_row=True), dict(density=0.1, dtype=torch.float64),
                dict(density=0.1, rng_state=torch.tensor([1, 2], dtype=torch.int64))):
        with pytest.raises(ValueError):
            topology.random_csr(m, n, **bad)
    with pytest.raises(RuntimeError):
        ops.random_csr(m, n, total=4, device="cpu")


def test_every_position_is_equally_likely():
    """Deterministic: seed 1, offsets 4 d for d = 0 .. 255, 8 x 16, K = 32 and k = 4.  Every
    position is kept Binomial(256, 1/4) times; matrix-wide a row's total over the draws has
    the variance of 256 hypergeometric draws.  |z| <= 4 for all of them (the restatement gives
    2.31 and 2.17 for the positions and 1.5 for the rows)."""
    m, n, draws = 8, 16, 256
    hits = {False: np.zeros((m, n)), True: np.zeros((m, n))}
    for d in range(draws):
        state = torch.tensor([1, 4 * d], dtype=torch.int64)
        for per_row in (False, True):
            _, _, row_offsets, column_indices = topology.random_csr(m, n, nonzeros=4 if per_row else 32,
                                                                    per_row=per_row, rng_state=state)
            rows = np.repeat(np.arange(m), np.diff(row_offsets.numpy()))
            hits[per_row][rows, column_indices.numpy()] += 1
    for per_row in (False, True):
        z = (hits[per_row] - draws / 4) / math.sqrt(draws * 0.25 * 0.75)
        print(f"per_row {per_row}: position |z| max {np.abs(z).max():.2f}")
        assert np.abs(z).max() <= 4.0
    assert np.array_equal(hits[True].sum(1), np.full(m, 4.0 * draws))
    sd = math.sqrt(draws * 32 * (1 / 8) * (7 / 8) * 96 / 127)
    z = (hits[False].sum(1) - 4.0 * draws) / sd
    print(f"matrix-wide: row |z| max {np.abs(z).max():.2f}")
    assert np.abs(z).max() <= 4.0


def test_erk_densities():
    shapes = [(10, 784), (300, 784), (100, 300), (4096, 1024), (1024, 4096)]
    got = topology.erk_densities(shapes, 0.1)
    assert np.allclose(got, [1.0, 0.33742, 0.97615, 0.089369, 0.089369], rtol=0, atol=1e-5)
    assert got[0] == 1.0 and all(isinstance(d, float) and 0.0 < d <= 1.0 for d in got)
    sizes = [o * i for o, i in shapes]
    assert abs(sum(d * s for d, s in zip(got, sizes)) / sum(sizes) - 0.1) < 1e-12
    assert np.allclose(topology.erk_densities([(64, 128)] * 3, 0.3), [0.3] * 3, rtol=0, atol=1e-15)
    assert topology.erk_densities(shapes, 1.0) == [1.0] * len(shapes)
    uniform = topology.erk_densities(shapes, 0.2, power=0.0)
    assert np.allclose(uniform, [0.2] * len(shapes), rtol=0, atol=1e-15)
    assert topology.erk_densities([], 0.5) == []
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            topology.erk_densities(shapes, bad)
    with pytest.raises(ValueError):
        topology.erk_densities([(0, 4)], 0.5)


@pytest.mark.parametrize("per_row", (False, True))
def test_sparse_linear_random_on_the_cpu(per_row):
    in_f, out_f = 48, 24
    state = torch.tensor([11, 4], dtype=torch.int64)
    layer = SparseLinear.random(in_f, out_f, density=0.25, per_row=per_row, rng_state=state)
    assert (layer.input_features, layer.output_features) == (in_f, out_f)
    assert isinstance(layer.values, torch.nn.Parameter) and layer.values.requires_grad
    assert layer.values.dtype == torch.float32 and layer.values.device.type == "cpu"
    assert "values" in dict(layer.named_parameters())
    nnz = round(0.25 * in_f) * out_f if per_row else round(0.25 * in_f * out_f)
    assert layer.values.numel() == nnz == layer.column_indices.numel() == int(layer.row_offsets[-1])
    assert layer.row_indices.numel() == out_f and layer.row_offsets.numel() == out_f + 1
    lengths = layer.row_offsets[1:] - layer.row_offsets[:-1]
    if per_row:
        assert bool((lengths == round(0.25 * in_f)).all())
    want = topology.random_csr(out_f, in_f, density=0.25, per_row=per_row, rng_state=state)
    assert all(torch.equal(a, b) for a, b in zip(
        (layer.values.detach(), layer.row_indices, layer.row_offsets, layer.column_indices), want))
    half = SparseLinear.random(in_f, out_f, nonzeros=5, dtype=torch.bfloat16)
    assert half.values.dtype == torch.bfloat16 and half.values.numel() == 5

    generator = torch.Generator().manual_seed(3)
    source = layer.update_topology(0.3, generator=generator, per_row=per_row)
    assert source.numel() == nnz and layer.values.numel() == nnz
    assert int((source < 0).sum()) > 0 and int(layer.row_offsets[-1]) == nnz
    source = layer.prune_to(density=0.1, per_row=per_row)
    kept = round(0.1 * in_f) * out_f if per_row else round(0.1 * in_f * out_f)
    assert layer.values.numel() == kept == source.numel() == int(layer.row_offsets[-1])
