"""CPU: the drop-and-grow step under generated scores -- SET's step without a dense tensor
(topology.regrow_per_row_random / regrow_total_random, SparseLinear.set_update) -- on CPU tensors
against a numpy restatement of the rule (tests/set_regrow_cases.py: the Philox of
tests/philox_ref.py, stable argsorts per row and matrix-wide), and the host-only queries of the
device step.  Everything is an integer or a bit copy: every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import regrow_total_cases as C
from tests import set_regrow_cases as S
from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

SHAPES = ((1, 1), (5, 3), (7, 17), (12, 64))
ids = dict(ids=lambda d: str(d).split(".")[-1])


def properties_per_row(old, new, n, where):
    """nnz and the row lengths stay (the offsets are not returned: the slots are the row's own);
    kept entries are carried bit for bit; no grown column is among the kept ones; columns ascend"""
    values, row_offsets, column_indices = old
    new_columns, new_values, source = new
    assert new_columns.numel() == values.numel() == source.numel(), where
    old_bits, new_bits = C.bits_of(values), C.bits_of(new_values)
    for r in range(row_offsets.numel() - 1):
        begin, end = int(row_offsets[r]), int(row_offsets[r + 1])
        row, src = new_columns[begin:end].tolist(), source[begin:end]
        assert row == sorted(set(row)) and all(0 <= c < n for c in row), where       # ascending, no column twice
        kept = src >= 0
        assert bool(((src[kept] >= begin) & (src[kept] < end)).all()), where
        assert torch.equal(new_columns[begin:end][kept], column_indices[src[kept]]), where
        assert torch.equal(new_bits[begin:end][kept], old_bits[src[kept]]), where
        if end - begin == n:                                   # a full row regrows what it dropped
            assert row == list(range(n)), where


@pytest.mark.parametrize("dtype", S.DTYPES, **ids)
@pytest.mark.parametrize("m,n", SHAPES)
def test_per_row_against_the_rule(m, n, dtype):
    generator = torch.Generator().manual_seed(100 * m + n)
    for density in (0.0, 0.3, 1.0):
        old = S.pattern(m, n, density, dtype, generator)
        for how in S.DROPS:
            drops = S.drop_counts(old[1], how)
            for key_mask in S.MASKS:
                for bound in (None, 0.5):
                    where = f"{m}x{n} {dtype} density {density} drop {how} mask {key_mask:#x} bound {bound}"
                    got = S.torch_per_row(*old, drops, n, S.STATE, key_mask, bound)
                    S.assert_same(got, S.rule_per_row(*old, drops, n, S.STATE, key_mask, bound), S.PER_ROW_NAMES, where)
                    properties_per_row(old, got, n, where)
                    assert int((got[2] < 0).sum()) == int(drops.sum()), where
                    if bound is None:
                        assert not C.bits_of(got[1])[got[2] < 0].any(), where       # +0.0


@pytest.mark.parametrize("dtype", S.DTYPES, **ids)
@pytest.mark.parametrize("m,n", SHAPES)
def test_total_against_the_rule(m, n, dtype):
    generator = torch.Generator().manual_seed(200 * m + n)
    for density in (0.0, 0.3, 1.0):
        old = S.pattern(m, n, density, dtype, generator)
        nnz = old[0].numel()
        for how in S.DROPS:
            d = S.drop_total(nnz, how)
            for key_mask in S.MASKS:
                for bound in (None, 0.5):
                    where = f"{m}x{n} {dtype} density {density} drop {how} mask {key_mask:#x} bound {bound}"
                    got = S.torch_total(*old, d, n, S.STATE, key_mask, bound)
                    S.assert_same(got, S.rule_total(*old, d, n, S.STATE, key_mask, bound), C.NAMES, where)
                    row_indices, row_offsets, columns, values, source = got
                    assert int(row_offsets[-1]) == nnz == columns.numel() and int((source < 0).sum()) == d, where
                    kept = source >= 0
                    assert torch.equal(C.bits_of(values)[kept], C.bits_of(old[0])[source[kept]]), where
                    assert torch.equal(columns[kept], old[2][source[kept]]), where
                    flat = torch.repeat_interleave(torch.arange(m), (row_offsets[1:] - row_offsets[:-1]).long()) * n \
                        + columns.long()
                    assert bool((flat[1:] > flat[:-1]).all()), where               # ascending, no position twice
                    if density == 1.0:                          # a full pattern regrows what it dropped
                        assert torch.equal(columns, old[2]) and torch.equal(row_offsets, old[1]), where
                    if d == 0:
                        assert torch.equal(source, torch.arange(nnz)) and torch.equal(columns, old[2]), where


def test_the_step_is_the_stored_one_under_key_scores():
    """the rule as the header states it: regrow_per_row / regrow_total under dense float32 scores
    whose bits are the keys; a key is finite and non-negative"""
    generator = torch.Generator().manual_seed(5)
    m, n = 12, 64
    scores = S.key_scores(m, n, S.STATE)
    assert bool(torch.isfinite(scores).all()) and bool((scores >= 0).all())
    assert float(torch.tensor([ops.REGROW_KEY_MASK], dtype=torch.int32).view(torch.float32)) < 2.0
    old = S.pattern(m, n, 0.3, torch.float32, generator)
    drops = S.drop_counts(old[1], "third")
    S.assert_same(S.torch_per_row(*old, drops, n, S.STATE), topology.regrow_per_row(*old, drops, scores),
                  S.PER_ROW_NAMES)
    d = S.drop_total(old[0].numel(), "third")
    S.assert_same(S.torch_total(*old, d, n, S.STATE), topology.regrow_total(*old, d, scores), C.NAMES)


def test_grown_values_are_those_of_random_csr():
    """a grown position stores what random_csr stores there under the same state and bound"""
    m, n, bound = 7, 17, 0.5
    state = S.state_tensor(S.STATE)
    for dtype in S.DTYPES:
        values, _, row_offsets, column_indices = topology.random_csr(m, n, density=1.0, dtype=dtype, bound=bound,
                                                                     rng_state=state)
        image = values.view(m, n)                              # (every position, in order)
        assert torch.equal(C.bits_of(image), C.bits_of(S.value_image(m, n, S.STATE, bound, dtype)))
        generator = torch.Generator().manual_seed(6)
        old = S.pattern(m, n, 0.3, dtype, generator)
        d = old[0].numel() // 2
        _, new_offsets, columns, new_values, source = S.torch_total(*old, d, n, S.STATE, bound=bound)
        rows = torch.repeat_interleave(torch.arange(m), (new_offsets[1:] - new_offsets[:-1]).long())
        grown = source < 0
        assert torch.equal(C.bits_of(new_values)[grown], C.bits_of(image)[rows[grown], columns[grown].long()])


def test_every_open_position_is_equally_likely():
    """One row of 4096 columns whose 2048 entries are all dropped: every column is open and 2048
    are grown, so a column is grown with probability 1/2.  Over 2000 offsets of one seed its
    count is Binomial(2000, 1/2): mean 1000, standard deviation sqrt(500) = 22.4; every column
    lies within 5 of them (the chance that one of 4096 does not is 0.2 %, and the state is fixed:
    the largest deviation at this seed is 3.85)."""
    n, length, draws = 4096, 2048, 2000
    generator = torch.Generator().manual_seed(11)
    row_offsets, column_indices = C.csr([length], n, generator)
    values = torch.randn(length, generator=generator)
    drops = torch.tensor([length], dtype=torch.int32)
    counts = np.zeros(n, dtype=np.int64)
    for draw in range(draws):
        columns, _, source = S.torch_per_row(values, row_offsets, column_indices, drops, n, (1234, 4 * draw))
        assert bool((source < 0).all())
        counts[columns.numpy()] += 1
    mean, deviation = draws * length / n, (draws * 0.25) ** 0.5
    worst = np.abs(counts - mean).max() / deviation
    print(f"largest deviation of a column's grow count: {worst:.2f} standard deviations")
    assert worst < 5.0


def test_launch_shape_queries_are_host_only():
    for value_bytes in (2, 4):
        shape = capi.csr_regrow_random_launch_shape(2, 61440, 100, value_bytes, False)
        stored = capi.csr_regrow_launch_shape(2, 61440, 4, value_bytes)
        assert shape["served"] and shape["max_n"] == 61440 and shape["max_m"] == -1
        assert all(shape[name] == stored[name] for name in stored)
        assert shape["score_digit_passes"] == 4 and shape["value_digit_passes"] == value_bytes
        assert shape["launches"] == 1 and shape["elements_per_lane"] == 4
        unserved = capi.csr_regrow_random_launch_shape(2, 61441, 100, value_bytes, False)
        assert not unserved["served"] and unserved["max_n"] == 61440 and unserved["launches"] == -1
        # matrix-wide: the row order and the scan serve 16384 rows, the planes 65536 columns
        shape = capi.csr_regrow_random_launch_shape(16384, 64, 5000, value_bytes, True)
        stored = capi.csr_regrow_total_launch_shape(16384, 64, 5000, 4, value_bytes)
        assert shape["served"] and shape["max_m"] == 16384 and shape["max_n"] == 65536
        assert all(shape[name] == stored[name] for name in shape)
        assert shape["score_digit_passes"] == 4 and shape["launches"] == 8 + value_bytes + 4
        assert not capi.csr_regrow_random_launch_shape(16385, 64, 5000, value_bytes, True)["served"]
        assert capi.csr_regrow_random_launch_shape(16385, 64, 5000, value_bytes, False)["served"]
        assert capi.csr_regrow_random_launch_shape(4, 65536, 100, value_bytes, True)["served"]
        assert not capi.csr_regrow_random_launch_shape(4, 65537, 100, value_bytes, True)["served"]
        # without entries: the row order and the lane that publishes the state
        assert capi.csr_regrow_random_launch_shape(5, 64, 0, value_bytes, True)["launches"] == 2
        assert capi.csr_regrow_random_launch_shape(0, 64, 0, value_bytes, True)["launches"] == 1
    for n in (1, 16, 17, 64, 129, 1000):                        # the walk is the build's for 4-byte elements
        walk = capi.dense_to_csr_launch_shape(1, 65, n, 4)
        shape = capi.csr_regrow_random_launch_shape(65, n, 100, 4, True)
        assert all(shape[name] == walk[name] for name in ("rows_per_wave", "elements_per_lane", "rows_per_workgroup", "grid"))
    assert capi.csr_regrow_random_workspace_bytes(65, 129, 100, False) == 0
    assert capi.csr_regrow_random_workspace_bytes(65, 129, 100, True) == capi.csr_regrow_total_workspace_bytes(65, 129, 100)
    with pytest.raises(RuntimeError):
        capi.csr_regrow_random_launch_shape(2, 64, 10, 8, False)
    with pytest.raises(RuntimeError):
        capi.csr_regrow_random_launch_shape(-1, 64, 10, 4, True)


def test_argument_checks():
    generator = torch.Generator().manual_seed(7)
    m, n = 5, 9
    values, row_offsets, column_indices = S.pattern(m, n, 0.5, torch.float32, generator)
    drops = S.drop_counts(row_offsets, "one")
    state = S.state_tensor(S.STATE)
    assert ops.REGROW_KEY_MASK == 0x3fffffff
    with pytest.raises(ValueError):
        topology.regrow_per_row_random(values, row_offsets, column_indices, drops, n, key_mask=0x40000000)
    with pytest.raises(ValueError):
        topology.regrow_total_random(values, row_offsets, column_indices, 1, n, key_mask=-1)
    with pytest.raises(ValueError):
        topology.regrow_total_random(values, row_offsets, column_indices, values.numel() + 1, n)
    with pytest.raises(ValueError):
        topology.regrow_total_random(values, row_offsets, column_indices, 1, n, grow_bound=float("inf"))
    with pytest.raises(ValueError):
        topology.regrow_per_row_random(values, row_offsets, column_indices, drops, n, grow_bound=-1.0)
    with pytest.raises(ValueError):
        topology.regrow_per_row_random(values, row_offsets, column_indices, drops[:-1], n)
    with pytest.raises(ValueError):
        topology.regrow_per_row_random(values, row_offsets, column_indices, drops.long(), n)
    with pytest.raises(ValueError):
        topology.regrow_total_random(values, row_offsets, column_indices, 1, n, rng_state=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        topology.regrow_total_random(values, row_offsets, column_indices, 1, n, rng_state=torch.tensor([1, 6]))
    with pytest.raises(RuntimeError):
        ops.csr_regrow_random(values, row_offsets, column_indices, drops, n, rng_state=state)      # CPU tensors
    with pytest.raises(RuntimeError):
        ops.csr_regrow_total_random(values, row_offsets, column_indices, 1, n, rng_state=state)
    # without a state a CPU call draws a seed from torch's CPU generator, offset 0
    torch.manual_seed(3)
    first = topology.regrow_total_random(values, row_offsets, column_indices, 5, n, return_rng_state=True)
    torch.manual_seed(3)
    again = topology.regrow_total_random(values, row_offsets, column_indices, 5, n, return_rng_state=True)
    assert int(first[5][1]) == 0 and torch.equal(first[5], again[5])
    S.assert_same(first[:5], again[:5], C.NAMES)
    S.assert_same(topology.regrow_total_random(values, row_offsets, column_indices, 5, n, rng_state=first[5]), first[:5],
                  C.NAMES)
    # other dtypes take the rule in torch as well
    double = topology.regrow_total_random(values.double(), row_offsets, column_indices, 5, n, grow_bound=0.5,
                                          rng_state=state)
    single = topology.regrow_total_random(values, row_offsets, column_indices, 5, n, grow_bound=0.5, rng_state=state)
    assert double[3].dtype == torch.float64 and torch.equal(double[2], single[2])
    assert torch.equal(double[3].float(), single[3])


@pytest.mark.parametrize("per_row", (False, True))
def test_set_update_on_a_cpu_module(per_row):
    torch.manual_seed(21)
    in_f, out_f = 24, 10
    layer = SparseLinear.random(in_f, out_f, density=0.25, per_row=per_row)
    parameter, nnz = layer.values, layer.values.numel()
    optimizer = torch.optim.SGD([parameter], lr=0.1, momentum=0.9)
    parameter.grad = torch.arange(nnz, dtype=torch.float32)
    optimizer.step()
    momentum = optimizer.state[parameter]["momentum_buffer"].clone()
    twin = SparseLinear.random(in_f, out_f, density=0.25, per_row=per_row)
    twin._set_topology(torch.nn.Parameter(layer.values.detach().clone()), layer.row_indices.clone(),
                       layer.row_offsets.clone(), layer.column_indices.clone())
    old = (parameter.detach().clone(), layer.row_indices, layer.row_offsets, layer.column_indices)
    state = S.state_tensor(S.STATE)

    source, used = layer.set_update(0.3, per_row=per_row, grow_bound=0.25, rng_state=state, return_rng_state=True)
    assert torch.equal(used, state)
    assert layer.values is parameter and isinstance(layer.values, torch.nn.Parameter)       # the optimizer keeps its handle
    for before, now in zip(old[1:], (layer.row_indices, layer.row_offsets, layer.column_indices)):
        assert now is not before
    assert functional._is_static(layer.row_indices, layer.row_offsets, layer.column_indices)     # re-registered,
    assert not functional._is_static(*old[1:])                                                  # the old ones are not
    # the step is the topology function's, on the old arrays
    if per_row:
        lengths = old[2][1:] - old[2][:-1]
        drops = torch.floor(lengths.to(torch.float64) * 0.3).to(torch.int32)
        want = S.rule_per_row(old[0], old[2], old[3], drops, in_f, S.STATE, bound=0.25)
        S.assert_same((layer.column_indices, layer.values.detach(), source), want, S.PER_ROW_NAMES)
        assert torch.equal(layer.row_offsets, old[2]) and torch.equal(layer.row_indices, old[1])
        dropped = int(drops.sum())
    else:
        dropped = int(0.3 * nnz)
        want = S.rule_total(old[0], old[2], old[3], dropped, in_f, S.STATE, bound=0.25)
        S.assert_same((layer.row_indices, layer.row_offsets, layer.column_indices, layer.values.detach(), source), want,
                      C.NAMES)
    assert int((source < 0).sum()) == dropped > 0
    grown = layer.values.detach()[source < 0]
    assert bool((grown.abs() <= 0.25).all()) and bool((grown != 0).any())
    topology.remap_optimizer_state(optimizer, parameter, layer.values, source)
    remapped = optimizer.state[parameter]["momentum_buffer"]
    assert torch.equal(remapped[source >= 0], momentum[source[source >= 0]]) and not remapped[source < 0].any()
    # grow_bound=None grows zeros at the same positions
    zero_source = twin.set_update(0.3, per_row=per_row, rng_state=state)
    assert torch.equal(zero_source, source) and torch.equal(twin.column_indices, layer.column_indices)
    assert not twin.values.detach()[source < 0].any()
    assert torch.equal(twin.values.detach()[source >= 0], layer.values.detach()[source >= 0])
    # the shortcuts: nothing changes, nothing is drawn
    indices = (layer.row_indices, layer.row_offsets, layer.column_indices)
    for fraction in (0.0, 1e-9):
        same, drawn = layer.set_update(fraction, per_row=per_row, return_rng_state=True)
        assert torch.equal(same, torch.arange(nnz)) and drawn is None
        assert all(a is b for a, b in zip(indices, (layer.row_indices, layer.row_offsets, layer.column_indices)))
    for fraction in (-0.1, 1.5):
        with pytest.raises(ValueError, match="update_topology: drop_fraction"):
            layer.set_update(fraction, per_row=per_row)
    # update_topology keeps its behaviour, generator= included
    a = layer.update_topology(0.3, generator=torch.Generator().manual_seed(4), per_row=per_row)
    assert a.numel() == nnz and int((a < 0).sum()) == dropped
