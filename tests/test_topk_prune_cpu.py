"""CPU: magnitude pruning and regrowth without a device -- the torch path of
topology.magnitude_prune / topology.topk_to_csr against an independent numpy statement of the
selection rule, the host-only launch query, the argument errors, and
SparseLinear.update_topology on a CPU module.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, ops, topology

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def bits_of(t):
    """integer view of a tensor's elements (value bits compare exactly, NaN included)"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def numpy_keys(x):
    """bit pattern without the sign, as int64 -- stated with numpy alone"""
    if x.element_size() == 2:
        return (x.contiguous().view(torch.int16).numpy().astype(np.int64)) & 0x7fff
    return (x.contiguous().view(torch.int32).numpy().astype(np.int64)) & 0x7fffffff


def numpy_rule(x, per_row=None, total=None):
    """(row_offsets, column_indices, flat positions) of the kept set: np.lexsort on
    (index, -key) -- largest key first, lowest index among equals."""
    keys = numpy_keys(x)
    m, n = keys.shape
    if per_row is not None:
        columns = [np.sort(np.lexsort((np.arange(n), -keys[r]))[:per_row]) for r in range(m)]
        flat = np.concatenate([r * n + c for r, c in enumerate(columns)]) if m else np.zeros(0, np.int64)
    else:
        flat = np.sort(np.lexsort((np.arange(m * n), -keys.reshape(-1)))[:total])
    flat = flat.astype(np.int64)
    rows = flat // max(n, 1)
    offsets = np.zeros(m + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return offsets.astype(np.int32), (flat - rows * n).astype(np.int32), flat


def special_matrix(dtype, m=7, n=9, seed=0):
    """NaN, +-inf, +-0, a denormal, an all-equal row, an all-zero row and x / -x pairs"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, n, generator=g).to(dtype)
    x[0, 1], x[0, 3], x[0, 4] = float("nan"), float("inf"), float("-inf")
    x[0, 5], x[0, 6] = 0.0, -0.0
    x[1] = 1.5                                             # all equal
    x[2] = 0.0                                             # all zero
    x[3, 0:8:2] = -x[3, 1:8:2]                             # x / -x pairs
    x[3, 8] = -x[3, 0]
    denormal = torch.tensor([1], dtype=torch.int16 if dtype != torch.float32 else torch.int32).view(dtype)
    x[4, 2] = denormal[0]
    x[4, 3] = 0.0
    x[5, 0], x[5, 8] = -2.0, 2.0
    return x


def check_against_rule(x, got, per_row=None, total=None, values_from=None):
    row_indices, row_offsets, column_indices, values = got
    offsets, columns, flat = numpy_rule(x, per_row, total)
    assert row_offsets.dtype == row_indices.dtype == column_indices.dtype == torch.int32
    assert np.array_equal(row_offsets.numpy(), offsets)
    assert np.array_equal(column_indices.numpy(), columns)
    lengths = torch.from_numpy(offsets[1:] - offsets[:-1])
    assert torch.equal(row_indices, torch.argsort(lengths, stable=True).to(torch.int32))
    source = x if values_from is None else values_from
    assert values.dtype == source.dtype
    assert torch.equal(bits_of(values), bits_of(source).reshape(-1)[torch.from_numpy(flat)])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_torch_path_matches_the_numpy_rule(dtype):
    x = special_matrix(dtype)
    m, n = x.shape
    for k in (0, 1, n - 1, n, 4):
        check_against_rule(x, topology.topk_to_csr(x, per_row=k), per_row=k)
        values, ri, ro, ci = topology.magnitude_prune(x, nonzeros=k, per_row=True)
        check_against_rule(x, (ri, ro, ci, values), per_row=k)
    for K in (0, 1, m * n - 1, m * n, 20):
        check_against_rule(x, topology.topk_to_csr(x, total=K), total=K)
        values, ri, ro, ci = topology.magnitude_prune(x, nonzeros=K)
        check_against_rule(x, (ri, ro, ci, values), total=K)


def test_unique_keys_agree_with_topk():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 33, generator=g)
    _, _, ci, values = topology.topk_to_csr(x, per_row=5)
    want = torch.sort(torch.topk(x.abs(), 5, dim=1).indices, dim=1).values
    assert torch.equal(ci.reshape(12, 5).to(torch.int64), want)
    assert torch.equal(values.reshape(12, 5), x.gather(1, want))


def test_density_counts_and_other_dtypes():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(10, 14, generator=g)
    values, ri, ro, ci = topology.magnitude_prune(x, density=0.2)
    assert values.numel() == ci.numel() == round(0.2 * 140) and int(ro[-1]) == 28
    values, ri, ro, ci = topology.magnitude_prune(x, density=0.25, per_row=True)
    assert torch.equal(ro, torch.arange(11, dtype=torch.int32) * round(0.25 * 14))
    assert torch.equal(ri, torch.arange(10, dtype=torch.int32))
    # other dtypes rank as .float() and keep their own values
    x64 = x.double()
    got = topology.magnitude_prune(x64, nonzeros=17)
    want = topology.magnitude_prune(x, nonzeros=17)
    assert got[0].dtype == torch.float64 and torch.equal(got[0], want[0].double())
    assert all(torch.equal(a, b) for a, b in zip(got[1:], want[1:]))
    xi = torch.randint(-50, 50, (6, 8), generator=g)
    values, _, ro, ci = topology.magnitude_prune(xi, nonzeros=3, per_row=True)
    assert values.dtype == torch.int64
    check_against_rule(xi.float(), (torch.arange(6, dtype=torch.int32), ro, ci, values), per_row=3, values_from=xi)
    # values_from: another dtype, an integer payload
    payload = torch.arange(140, dtype=torch.int32).reshape(10, 14)
    check_against_rule(x, topology.topk_to_csr(x, total=31, values_from=payload), total=31, values_from=payload)


def test_launch_query_is_host_only():
    limit = capi.csr_row_order_route(1, 1, 0)["capacity"]
    limit = capi.csr_row_order_route(1, limit + 1, 0)["capacity"]
    assert limit == 16384
    assert capi.topk_to_csr_launch_shape(limit, 8, 4, True)["served"]
    assert not capi.topk_to_csr_launch_shape(limit + 1, 8, 4, True)["served"]
    assert capi.topk_to_csr_launch_shape(limit + 1, 8, 4, False)["served"]     # per row: no sort
    for element_bytes in (2, 4):
        for n in (1, 16, 17, 100, 257, 2048):
            for total in (False, True):
                shape = capi.topk_to_csr_launch_shape(100, n, element_bytes, total)
                walk = capi.dense_to_csr_launch_shape(1, 100, n, element_bytes)
                assert shape["digit_passes"] == element_bytes
                assert {k: shape[k] for k in walk} == walk and shape["grid"] >= 1
    assert capi.topk_to_csr_launch_shape(0, 0, 4, False)["grid"] == 0
    for args in ((4, 4, 1, False), (4, 4, 8, True), (4, 4, 3, False), (-1, 4, 4, False), (4, -1, 2, True),
                 (65536, 32768, 2, False)):
        with pytest.raises(RuntimeError):
            capi.topk_to_csr_launch_shape(*args)


def test_c_abi_rejects_bad_arguments_without_a_device():
    lib = capi.lib()
    invalid = -1   # SPUTNIK_HIP_INVALID_ARGUMENT
    null = [None] * 5
    calls = (
        (4, 4, None, 3, 4, 0, 1, None, 4, 4, None, 0) + tuple(null),       # element width
        (4, 4, None, 4, 4, 0, 5, None, 4, 4, None, 0) + tuple(null),       # per_row count above n
        (4, 4, None, 4, 4, 1, 17, None, 4, 4, None, 0) + tuple(null),      # total count above m * n
        (4, 4, None, 4, 4, 1, -1, None, 4, 4, None, 0) + tuple(null),      # negative count
        (16385, 4, None, 4, 4, 1, 1, None, 4, 4, None, 0) + tuple(null),   # total mode beyond the row order
        (4, 4, None, 4, 4, 0, 1, None, 4, 4, None, 0) + tuple(null),       # no pointers
    )
    for call in calls:
        assert lib.sputnik_hip_topk_to_csr(*call, None) == invalid
    assert capi.lib().sputnik_hip_topk_to_csr_workspace_bytes(100, 7, 0) == 800
    assert capi.lib().sputnik_hip_topk_to_csr_workspace_bytes(100, 7, 1) == 4 * (4 * 256 + 1 + 200)


def test_argument_errors():
    x = torch.randn(4, 6)
    for fn in (ops.topk_to_csr, topology.topk_to_csr):
        with pytest.raises(ValueError):
            fn(x)                                            # neither
        with pytest.raises(ValueError):
            fn(x, per_row=1, total=1)                        # both
        for kwargs in (dict(per_row=-1), dict(per_row=7), dict(total=-1), dict(total=25)):
            with pytest.raises(ValueError):
                fn(x, **kwargs)
        with pytest.raises(ValueError):
            fn(x, per_row=1, values_from=torch.zeros(4, 5))  # mismatched shape
        with pytest.raises(ValueError):
            fn(x.reshape(-1), per_row=1)
    with pytest.raises(ValueError):
        ops.topk_to_csr(x, per_row=1, values_from=torch.zeros(4, 6, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.topk_to_csr(x.double(), per_row=1)
    with pytest.raises(RuntimeError):
        ops.topk_to_csr(x, per_row=1)                        # CPU tensors: the op is device only
    for kwargs in (dict(), dict(density=0.5, nonzeros=3), dict(density=1.5), dict(density=-0.1),
                   dict(nonzeros=25), dict(nonzeros=7, per_row=True), dict(nonzeros=-1)):
        with pytest.raises(ValueError):
            topology.magnitude_prune(x, **kwargs)


# ---- SparseLinear.from_dense / update_topology on a CPU module (no kernel involved) ----

def cpu_module(out_f=12, in_f=20, density=0.3, seed=5, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(out_f, in_f, generator=g).to(dtype)
    return SparseLinear.from_dense(w, density=density), w


def flat_positions(module):
    lengths = (module.row_offsets[1:] - module.row_offsets[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(module.output_features), lengths)
    return rows * module.input_features + module.column_indices.to(torch.int64)


def expected_update(module, d, scores):
    """Kept and Grown, stated on their own with numpy: (kept old indices, grown flat positions)"""
    values = module.values.detach()
    nnz = values.numel()
    keys = numpy_keys(values.reshape(1, -1)).reshape(-1)
    kept = np.sort(np.lexsort((np.arange(nnz), -keys))[:nnz - d])
    flat = flat_positions(module).numpy()
    s = scores.detach().abs()
    largest = torch.finfo(s.dtype).max
    s = torch.where(torch.isfinite(s), s, torch.full_like(s, largest))
    skeys = numpy_keys(s).reshape(-1)
    eligible = np.ones(skeys.size, bool)
    eligible[flat[kept]] = False
    candidates = np.nonzero(eligible)[0]
    grown = candidates[np.lexsort((candidates, -skeys[candidates]))[:d]]
    return kept, np.sort(grown)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("float32", "bfloat16"))
def test_update_topology_on_a_cpu_module(dtype):
    module, w = cpu_module(dtype=dtype)
    assert module.values.dtype == dtype and module.values.numel() == round(0.3 * 240)
    parameter, nnz = module.values, module.values.numel()
    old_values, old_flat = module.values.detach().clone(), flat_positions(module)
    old_indices = (module.row_indices, module.row_offsets, module.column_indices)
    old_index_copies = [t.clone() for t in old_indices]
    g = torch.Generator().manual_seed(6)
    scores = torch.randn(12, 20, generator=g)
    scores[0, 0], scores[3, 7], scores[5, 5], scores[11, 19] = float("nan"), float("inf"), float("-inf"), 0.0
    d = int(0.3 * nnz)
    kept, grown = expected_update(module, d, scores)

    source = module.update_topology(0.3, scores)

    assert module.values is parameter and module.values.numel() == nnz
    assert int(module.row_offsets[-1]) == nnz and module.column_indices.numel() == nnz
    new_flat = flat_positions(module)
    want_flat = np.sort(np.concatenate([old_flat.numpy()[kept], grown]))
    assert np.array_equal(new_flat.numpy(), want_flat)
    # non-finite scores count as the largest finite value: they are grown first where eligible
    for r, c in ((0, 0), (3, 7), (5, 5)):
        assert r * 20 + c in set(new_flat.tolist())
    assert source.dtype == torch.int64 and source.shape == (nnz,)
    is_grown = torch.from_numpy(np.isin(new_flat.numpy(), grown))
    assert torch.equal(source == -1, is_grown) and int(is_grown.sum()) == d
    assert np.array_equal(np.sort(source[~is_grown].numpy()), kept)
    assert torch.equal(old_flat[source[~is_grown]], new_flat[~is_grown])
    assert torch.equal(bits_of(module.values.detach()[~is_grown]), bits_of(old_values[source[~is_grown]]))
    assert torch.equal(bits_of(module.values.detach()[is_grown]), torch.zeros(d, dtype=bits_of(old_values).dtype))
    # the old index tensors are replaced, not written to
    assert all(new is not old for new, old in zip((module.row_indices, module.row_offsets, module.column_indices),
                                                  old_indices))
    assert all(torch.equal(t, c) for t, c in zip(old_indices, old_index_copies))
    assert torch.equal(module.row_indices, topology.diffsort(module.row_offsets))


def test_update_topology_no_op_and_generator():
    module, _ = cpu_module()
    before = [t.clone() for t in (module.values.detach(), module.row_indices, module.row_offsets,
                                  module.column_indices)]
    indices = (module.row_indices, module.row_offsets, module.column_indices)
    source = module.update_topology(0.0)
    assert torch.equal(source, torch.arange(module.values.numel()))
    source = module.update_topology(0.9 / module.values.numel())        # d = int(0.9) = 0
    assert torch.equal(source, torch.arange(module.values.numel()))
    assert all(a is b for a, b in zip(indices, (module.row_indices, module.row_offsets, module.column_indices)))
    assert all(torch.equal(a, b) for a, b in zip(before, (module.values.detach(), module.row_indices,
                                                          module.row_offsets, module.column_indices)))
    # SET: random growth, reproducible with the generator's seed
    patterns = []
    for seed in (11, 11, 12):
        module, _ = cpu_module()
        source = module.update_topology(0.4, generator=torch.Generator().manual_seed(seed))
        assert int((source == -1).sum()) == int(0.4 * module.values.numel())
        patterns.append(flat_positions(module))
    assert torch.equal(patterns[0], patterns[1]) and not torch.equal(patterns[0], patterns[2])


def test_dropped_positions_are_eligible_again():
    module, _ = cpu_module()
    nnz = module.values.numel()
    flat = flat_positions(module)
    scores = torch.zeros(12, 20)
    scores.view(-1)[flat] = 1.0            # the largest scores sit on the present pattern
    source = module.update_topology(0.25, scores)
    assert torch.equal(flat_positions(module), flat)          # dropped entries grow back ...
    grown = source == -1
    assert int(grown.sum()) == int(0.25 * nnz)
    assert torch.equal(module.values.detach()[grown], torch.zeros(int(grown.sum())))   # ... at zero
