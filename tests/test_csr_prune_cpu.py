"""CPU: gradual magnitude pruning without a device -- the torch path of topology.prune_csr
against a Python loop per row, the cubic schedule topology.gradual_density, the optimizer
hand-over topology.remap_optimizer_state and SparseLinear.prune_to.  Everything is an integer
or a bit copy: every comparison is exact."""
import ctypes

import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, ops, topology

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {2: torch.int16, 4: torch.int32}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()])


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def key_of(values, i):
    """the rule, restated on one Python integer: the bit pattern without the sign"""
    width = values.element_size() * 8
    return (int(bits_of(values)[i]) & ((1 << width) - 1)) & ((1 << (width - 1)) - 1)


def pattern(m, n, dtype, generator):
    """A CSR pattern of an m x n matrix with an empty row, a full row and short rows; values of
    few distinct magnitudes, mixed signs, NaN, +-inf, +-0 and the smallest denormal."""
    lengths = torch.randint(0, n + 1, (m,), generator=generator)
    lengths[0], lengths[m // 2], lengths[m - 1] = 2, 0, n
    columns = [torch.sort(torch.randperm(n, generator=generator)[:int(length)]).values for length in lengths]
    row_offsets = torch.zeros(m + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    column_indices = torch.cat(columns).to(torch.int32)
    nnz = column_indices.numel()
    values = ((torch.randn(nnz, generator=generator) / 0.25).round() * 0.25).to(dtype)
    special = torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.5, -0.5], dtype=dtype),
                         from_bits([1], dtype)])
    values[1::4][: special.numel()] = special[: values[1::4].numel()]
    return values, row_offsets, column_indices


def by_loop(values, row_offsets, per_row=None, total=None):
    """the kept entry indices, ascending: a Python loop over rows (per row) or entries (total)"""
    offsets = row_offsets.tolist()
    if total is not None:
        ranked = sorted(range(values.numel()), key=lambda i: (-key_of(values, i), i))
        return sorted(ranked[:total])
    kept = []
    for r in range(len(offsets) - 1):
        ranked = sorted(range(offsets[r], offsets[r + 1]), key=lambda i: (-key_of(values, i), i))
        kept += sorted(ranked[:per_row])
    return kept


def check_against_loop(case, n, per_row=None, total=None):
    values, row_offsets, column_indices = case
    m = row_offsets.numel() - 1
    row_indices, new_offsets, new_columns, new_values, source = topology.prune_csr(
        values, row_offsets, column_indices, n, per_row=per_row, total=total)
    want = by_loop(values, row_offsets, per_row=per_row, total=total)
    assert source.dtype == torch.int64 and source.tolist() == want
    assert new_columns.dtype == torch.int32 and torch.equal(new_columns, column_indices[want])
    assert new_values.dtype == values.dtype and torch.equal(bits_of(new_values), bits_of(values)[want])
    rows = torch.bucketize(torch.tensor(want, dtype=torch.int64), row_offsets[1:].to(torch.int64), right=True)
    want_offsets = torch.zeros(m + 1, dtype=torch.int32)
    want_offsets[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0)
    assert new_offsets.dtype == torch.int32 and torch.equal(new_offsets, want_offsets)
    lengths = new_offsets[1:] - new_offsets[:-1]
    assert row_indices.dtype == torch.int32
    assert torch.equal(row_indices, torch.argsort(lengths, stable=True).to(torch.int32))
    return new_offsets, source


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_prune_csr_against_a_loop(dtype):
    generator = torch.Generator().manual_seed(31)
    for m, n in ((7, 13), (9, 70)):
        case = pattern(m, n, dtype, generator)
        nnz = case[0].numel()
        for k in (0, 1, 3, n):
            new_offsets, _ = check_against_loop(case, n, per_row=k)
            lengths = case[1][1:] - case[1][:-1]
            assert torch.equal(new_offsets[1:] - new_offsets[:-1], lengths.clamp(max=k))
        for K in (0, 1, nnz // 2, nnz - 1, nnz):
            new_offsets, source = check_against_loop(case, n, total=K)
            assert source.numel() == K and int(new_offsets[-1]) == K


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_prune_csr_ties_go_to_the_lower_index(dtype):
    """all magnitudes equal: the first k of every row, the first K of the matrix"""
    generator = torch.Generator().manual_seed(32)
    _, row_offsets, column_indices = pattern(7, 13, dtype, generator)
    nnz = column_indices.numel()
    values = torch.where(torch.arange(nnz) % 2 == 0, 1.5, -1.5).to(dtype)
    _, _, _, _, source = topology.prune_csr(values, row_offsets, column_indices, 13, total=nnz // 2)
    assert source.tolist() == list(range(nnz // 2))
    check_against_loop((values, row_offsets, column_indices), 13, per_row=2)
    check_against_loop((values, row_offsets, column_indices), 13, total=nnz // 2 + 1)


def test_prune_csr_other_dtypes_rank_as_float():
    generator = torch.Generator().manual_seed(33)
    values, row_offsets, column_indices = pattern(9, 70, torch.float32, generator)
    finite = torch.nan_to_num(values, nan=3.0, posinf=4.0, neginf=-4.0)
    want = topology.prune_csr(finite, row_offsets, column_indices, 70, total=100)
    got = topology.prune_csr(finite.double(), row_offsets, column_indices, 70, total=100)
    assert got[3].dtype == torch.float64 and torch.equal(got[3], want[3].double())
    assert all(torch.equal(g, w) for g, w in zip(got[:3] + got[4:], want[:3] + want[4:]))


def test_prune_csr_argument_errors():
    generator = torch.Generator().manual_seed(34)
    values, row_offsets, column_indices = pattern(7, 13, torch.float32, generator)
    nnz = values.numel()
    good = dict(values=values, row_offsets=row_offsets, column_indices=column_indices)
    for bad in (dict(), dict(per_row=1, total=1), dict(per_row=-1), dict(total=-1), dict(total=nnz + 1),
                dict(per_row=14)):
        with pytest.raises(ValueError):
            topology.prune_csr(**good, n=13, **bad)
    for fn, extra in ((topology.prune_csr, dict(n=13)), (ops.csr_topk, dict())):
        with pytest.raises(ValueError):
            fn(**{**good, "row_offsets": row_offsets.long()}, total=1, **extra)
        with pytest.raises(ValueError):
            fn(**{**good, "column_indices": column_indices[:-1]}, total=1, **extra)
        with pytest.raises(ValueError):
            fn(**{**good, "values": values.reshape(1, -1)}, total=1, **extra)
    with pytest.raises(ValueError):
        ops.csr_topk(values.double(), row_offsets, column_indices, total=1)
    with pytest.raises(RuntimeError):
        ops.csr_topk(**good, total=1)                        # CPU tensors: the op is device only


def test_launch_shape_query_is_host_only():
    limit = capi.csr_row_order_route(1, 1, 0)["capacity"] * 8
    assert limit == 16384
    for total in (False, True):
        assert capi.csr_topk_launch_shape(limit, 8, 100, 4, total)["served"]
        beyond = capi.csr_topk_launch_shape(limit + 1, 8, 100, 4, total)
        assert not beyond["served"] and beyond["rows_per_wave"] == -1
    for value_bytes in (2, 4):
        v = 16 // value_bytes
        previous = None
        for mean in range(0, 64 * v + 2):
            shape = capi.csr_topk_launch_shape(10, 4096, 10 * mean + 9, value_bytes, False)
            assert shape["elements_per_lane"] == v and shape["digit_passes"] == value_bytes
            assert shape["group_lanes"] * shape["rows_per_wave"] == 64
            assert shape["rows_per_workgroup"] == 4 * shape["rows_per_wave"]
            # the narrowest group whose one step covers the mean row length
            assert mean <= shape["group_lanes"] * v or shape["group_lanes"] == 64
            assert shape["group_lanes"] == 4 or mean > shape["group_lanes"] // 2 * v
            assert shape["rows_grid"] == -(-10 // shape["rows_per_workgroup"]) and shape["flat_grid"] == 0
            assert previous is None or shape["group_lanes"] >= previous
            previous = shape["group_lanes"]
        assert previous == 64
    assert capi.csr_topk_launch_shape(100, 100, 2048 * 8 * 3, 2, True)["flat_grid"] == 4      # 3 * 2048 + 2 pieces
    assert capi.csr_topk_launch_shape(100, 100, 0, 2, True)["flat_grid"] == 0
    assert capi.csr_topk_launch_shape(0, 0, 0, 4, False)["rows_grid"] == 0
    for args in ((-1, 4, 4, 4, False), (4, -1, 4, 4, False), (4, 4, -1, 4, False), (4, 4, 4, 8, False),
                 (4, 4, 4, 1, True)):
        with pytest.raises(RuntimeError):
            capi.csr_topk_launch_shape(*args)


def test_c_abi_rejects_bad_arguments_without_a_device():
    lib = capi.lib()
    invalid = -1   # SPUTNIK_HIP_INVALID_ARGUMENT
    buffer = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buffer) + 15) // 16 * 16          # host memory: every call is rejected before a launch
    big = 1 << 20
    #    m  n  nnz offsets columns values vb mode count ws bytes  row_indices offsets columns values source capacity
    calls = (
        (4, 8, 16, p, p, p, 8, 1, 5, p, big, p, p, p, p, p, 16),             # value width
        (4, 8, 16, p, p, p, 1, 1, 5, p, big, p, p, p, p, p, 16),             # value width
        (4, 8, 16, p, p, p, 4, 2, 5, p, big, p, p, p, p, p, 16),             # neither mode
        (-1, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, p, 16),            # negative m
        (4, -1, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, p, 16),            # negative n
        (4, 8, -1, p, p, p, 4, 1, 0, p, big, p, p, p, p, p, 16),             # negative nnz
        (4, 8, 16, p, p, p, 4, 1, -1, p, big, p, p, p, p, p, 16),            # negative count
        (4, 8, 16, p, p, p, 4, 1, 17, p, big, p, p, p, p, p, 32),            # total count above nnz
        (4, 8, 16, p, p, p, 4, 0, 9, None, 0, p, p, p, p, p, 16),            # per-row count above n
        (16385, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, p, 16),         # beyond the row order
        (16385, 8, 16, p, p, p, 4, 0, 5, None, 0, p, p, p, p, p, 16),
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, p, 4),              # capacity below count
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, p, -1),             # negative capacity
        (4, 8, 16, None, p, p, 4, 1, 5, p, big, p, p, p, p, p, 16),          # no offsets
        (4, 8, 16, p, None, p, 4, 1, 5, p, big, p, p, p, p, p, 16),          # no columns
        (4, 8, 16, p, p, None, 4, 1, 5, p, big, p, p, p, p, p, 16),          # no values
        (4, 8, 16, p, p, p + 2, 4, 1, 5, p, big, p, p, p, p, p, 16),         # misaligned values
        (4, 8, 16, p + 2, p, p, 4, 1, 5, p, big, p, p, p, p, p, 16),         # misaligned offsets
        (4, 8, 16, p, p, p, 4, 1, 5, None, big, p, p, p, p, p, 16),          # no workspace
        (4, 8, 16, p, p, p, 4, 1, 5, p, 64, p, p, p, p, p, 16),              # workspace too small
        (4, 8, 16, p, p, p, 4, 1, 5, p + 2, big, p, p, p, p, p, 16),         # misaligned workspace
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, None, p, p, p, p, 16),          # total mode: no row_indices
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, None, p, p, p, 16),          # no out offsets
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, None, p, p, 16),          # total mode is one call
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, None, p, 16),          # no out values
        (4, 8, 16, p, p, p, 2, 1, 5, p, big, p, p, p, p + 1, p, 16),         # misaligned out values
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, None, 16),          # no source
        (4, 8, 16, p, p, p, 4, 1, 5, p, big, p, p, p, p, p + 4, 16),         # misaligned source
        (4, 8, 16, p, p, p, 4, 0, 5, None, 0, None, p, None, None, None, 0),    # per row: neither half
        (4, 8, 16, None, None, None, 4, 0, 5, None, 0, p, p, None, None, None, 0),    # offsets half: no offsets
        (4, 8, 16, p, p, p, 4, 0, 5, None, 0, None, p, p, p, None, 16),      # fill half: no source
    )
    for call in calls:
        assert lib.sputnik_hip_csr_topk(*call, None) == invalid, call
    assert lib.sputnik_hip_csr_topk_workspace_bytes(100, 7, 50, 0) == 0
    assert lib.sputnik_hip_csr_topk_workspace_bytes(100, 7, 50, 1) == 4 * (4 * 256 + 1 + 200)


# ---- the schedule ----

def test_gradual_density():
    d = topology.gradual_density
    assert d(100, 100, 1100, 0.9, 0.1) == 0.9 and d(1100, 100, 1100, 0.9, 0.1) == 0.1     # the end points
    assert d(0, 100, 1100, 0.9, 0.1) == 0.9 and d(5000, 100, 1100, 0.9, 0.1) == 0.1        # the clamps
    assert d(600, 100, 1100, 0.9, 0.1) == 0.1 + (0.9 - 0.1) / 8                            # the midpoint
    assert d(3, 0, 4, 1.0, 0.0) == 1.0 / 64
    trace = [d(t, 100, 1100, 0.9, 0.1) for t in range(0, 1300, 7)]
    assert all(isinstance(x, float) for x in trace)
    assert all(a >= b for a, b in zip(trace, trace[1:])) and min(trace) == 0.1 and max(trace) == 0.9
    assert d(7, 7, 7, 0.5, 0.25) in (0.5, 0.25)                                            # an empty ramp
    with pytest.raises(ValueError):
        d(0, 10, 5, 0.9, 0.1)


# ---- the module and the optimizer hand-over ----

OUT, IN, BATCH, SEQ = 12, 20, 2, 3


def cpu_layer(seed, density=0.5, per_row=False):
    """A CPU SparseLinear.  (Its forward has no CPU kernel: the one real optimizer step is
    driven by a gradient assigned to ``values``.)"""
    generator = torch.Generator().manual_seed(seed)
    w = (torch.randn(OUT, IN, generator=generator) / 0.5).round() * 0.5          # many ties
    layer = SparseLinear.from_dense(w, density=density, per_row=per_row)
    return layer, generator


def one_step(layer, optimizer, generator):
    layer.values.grad = torch.randn(layer.values.numel(), generator=generator)
    optimizer.step()
    layer.values.grad = None


def make_optimizers(layer):
    return (torch.optim.SGD([layer.values], lr=0.1, momentum=0.9),
            torch.optim.Adam([{"params": [layer.bias]}, {"params": [layer.values], "lr": 0.01}]))


@pytest.mark.parametrize("which", (0, 1), ids=("sgd", "adam"))
@pytest.mark.parametrize("per_row", (False, True), ids=("matrix", "per_row"))
def test_remap_after_prune_to(which, per_row):
    layer, generator = cpu_layer(41)
    optimizer = make_optimizers(layer)[which]
    one_step(layer, optimizer, generator)
    old = layer.values
    before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizer.state[old].items()}
    assert any(torch.is_tensor(v) and v.shape == old.shape for v in before.values())
    source = layer.prune_to(density=0.25, per_row=per_row)
    new = layer.values
    assert new is not old and new.numel() == source.numel() < old.numel()
    topology.remap_optimizer_state(optimizer, old, new, source)

    assert old not in optimizer.state and new in optimizer.state
    held = [p for group in optimizer.param_groups for p in group["params"]]
    assert not any(p is old for p in held) and sum(p is new for p in held) == 1
    if which == 1:                                           # the slot and its group's options are kept
        assert optimizer.param_groups[1]["params"][0] is new and optimizer.param_groups[1]["lr"] == 0.01
    state = optimizer.state[new]
    assert set(state) == set(before)
    for name, was in before.items():
        if torch.is_tensor(was) and was.shape == old.shape:
            assert state[name].shape == new.shape and state[name].dtype == was.dtype
            assert torch.equal(state[name].view(torch.int32), was.view(torch.int32)[source]), name
        elif torch.is_tensor(was):
            assert torch.equal(state[name], was), name       # step
        else:
            assert state[name] == was, name
    kept = new.detach().clone()
    one_step(layer, optimizer, generator)
    assert layer.values is new and not torch.equal(new.detach(), kept)


@pytest.mark.parametrize("which", (0, 1), ids=("sgd", "adam"))
@pytest.mark.parametrize("per_row", (False, True), ids=("matrix", "per_row"))
def test_remap_after_update_topology(which, per_row):
    layer, generator = cpu_layer(42, per_row=per_row)
    optimizer = make_optimizers(layer)[which]
    one_step(layer, optimizer, generator)
    parameter = layer.values
    before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizer.state[parameter].items()}
    source = layer.update_topology(0.3, torch.randn(OUT, IN, generator=generator), per_row=per_row)
    assert layer.values is parameter and int((source == -1).sum()) > 0
    topology.remap_optimizer_state(optimizer, parameter, parameter, source)
    state = optimizer.state[parameter]
    grown, carried = source == -1, source >= 0
    for name, was in before.items():
        if torch.is_tensor(was) and was.shape == parameter.shape:
            assert torch.equal(state[name][grown], torch.zeros(int(grown.sum())))
            assert torch.equal(state[name].view(torch.int32)[carried], was.view(torch.int32)[source[carried]]), name
        elif torch.is_tensor(was):
            assert torch.equal(state[name], was), name
    assert sum(p is parameter for group in optimizer.param_groups for p in group["params"]) == 1
    one_step(layer, optimizer, generator)


def test_remap_without_state_and_with_a_stranger():
    layer, _ = cpu_layer(43)
    optimizer = torch.optim.SGD([layer.values], lr=0.1, momentum=0.9)
    old = layer.values
    source = layer.prune_to(nonzeros=30)
    topology.remap_optimizer_state(optimizer, old, layer.values, source)     # no step taken: only the slot moves
    assert optimizer.param_groups[0]["params"][0] is layer.values and len(optimizer.state) == 0
    with pytest.raises(ValueError):
        topology.remap_optimizer_state(optimizer, old, layer.values, source)     # old is gone already
    with pytest.raises(ValueError):
        topology.remap_optimizer_state(optimizer, layer.values, layer.values, source[:-1])


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), **ids)
def test_prune_to_on_cpu(dtype):
    generator = torch.Generator().manual_seed(44)
    w = ((torch.randn(OUT, IN, generator=generator) / 0.5).round() * 0.5).to(dtype)
    for kwargs, prune in ((dict(density=0.25), dict(total=round(0.25 * OUT * IN))),
                          (dict(nonzeros=7), dict(total=7)), (dict(nonzeros=0), dict(total=0)),
                          (dict(density=0.25, per_row=True), dict(per_row=5)),
                          (dict(nonzeros=3, per_row=True), dict(per_row=3)),
                          (dict(nonzeros=IN, per_row=True), dict(per_row=IN))):
        layer = SparseLinear.from_dense(w, density=0.5)
        layer.values.requires_grad_(kwargs.get("nonzeros") != 7)
        layer.values.grad = torch.zeros_like(layer.values) if layer.values.requires_grad else None
        layer.dense_grad = marker = torch.zeros(1)
        old = (layer.values, layer.row_indices, layer.row_offsets, layer.column_indices)
        copies = [t.detach().clone() for t in old]
        want = topology.prune_csr(old[0].detach(), old[2], old[3], IN, **prune)
        source = layer.prune_to(**kwargs)
        assert torch.equal(source, want[4])
        assert torch.equal(layer.row_indices, want[0]) and torch.equal(layer.row_offsets, want[1])
        assert torch.equal(layer.column_indices, want[2])
        assert torch.equal(bits_of(layer.values.detach()), bits_of(want[3]))
        assert isinstance(layer.values, torch.nn.Parameter) and layer.values is not old[0]
        assert layer.values.requires_grad == old[0].requires_grad and layer.values.grad is None
        assert layer.values.dtype == dtype and layer.dense_grad is marker
        assert all(torch.equal(t.detach(), c) for t, c in zip(old, copies))       # the old arrays are not written to
        assert dict(layer.named_parameters())["values"] is layer.values

    layer = SparseLinear.from_dense(w, density=0.5)
    parameter, nnz = layer.values, layer.values.numel()
    indices = (layer.row_indices, layer.row_offsets, layer.column_indices)
    for kwargs in (dict(nonzeros=nnz), dict(nonzeros=nnz + 1), dict(density=0.5), dict(density=1.0)):
        source = layer.prune_to(**kwargs)                    # at or above nnz: nothing changes
        assert layer.values is parameter and torch.equal(source, torch.arange(nnz))
        assert all(a is b for a, b in zip(indices, (layer.row_indices, layer.row_offsets, layer.column_indices)))
    for bad in (dict(), dict(density=0.5, nonzeros=3), dict(density=1.5), dict(density=-0.1), dict(nonzeros=-1),
                dict(nonzeros=OUT * IN + 1), dict(nonzeros=IN + 1, per_row=True)):
        with pytest.raises(ValueError):
            layer.prune_to(**bad)
    assert layer.values is parameter
