"""GPU: random topologies drawn on the device (csrc/topology.hip; ops.random_csr,
topology.random_csr, SparseLinear.random) against the torch path of the same rule on the CPU
with the same rng_state.  Integers and value bits: every comparison is exact.  The torch path
itself is held to a numpy restatement in tests/test_random_topology_cpu.py."""
import pytest
import torch

from helpers import rel_err_torch
from torch_sputnik_amd import SparseLinear, capi, ops, topology

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
DEFAULT = ops.RANDOM_KEY_MASK
WIDTHS = (1, 3, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 513, 1000)
STATE = (2 ** 40 + 17, 4 * 10 ** 9)
BITS = {4: torch.int32, 2: torch.int16}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def bits(values):
    return values.contiguous().view(BITS[values.element_size()])


def assert_same(got, want, where):
    """(row_indices, row_offsets, column_indices, values) of the device against the CPU's"""
    for name, g, w in zip(("row_indices", "row_offsets", "column_indices", "values"), got, want):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, f"{name}: {where}"
        same = torch.equal(bits(g).cpu(), bits(w)) if name == "values" else torch.equal(g.cpu(), w)
        assert same, f"{name} differs: {where}"


def torch_path(m, n, per_row, total, dtype, bound, state, key_mask=DEFAULT):
    return topology._random_csr_torch(m, n, per_row, total, dtype, ops.random_value_scale(bound), state[0], state[1],
                                      CPU, key_mask=key_mask)


def check(m, n, per_row, total, dtype=torch.float32, bound=0.5, state=STATE, key_mask=DEFAULT):
    where = f"{m}x{n} per_row {per_row} total {total} {dtype} key_mask {key_mask:#x}"
    given = torch.tensor(state, dtype=torch.int64, device="cuda")
    got = ops.random_csr(m, n, per_row=per_row, total=total, dtype=dtype, bound=bound, device="cuda",
                         rng_state=given, key_mask=key_mask)
    assert got[4].tolist() == list(state)
    assert_same(got[:4], torch_path(m, n, per_row, total, dtype, bound, state, key_mask), where)
    return got


def counts(most):
    return sorted({0, min(1, most), most // 3 + (1 if most > 2 else 0), most})


def both_modes(m, n, dtype=torch.float32, key_mask=DEFAULT):
    for k in counts(n):
        check(m, n, k, None, dtype, key_mask=key_mask)
    for total in counts(m * n):
        check(m, n, None, total, dtype, key_mask=key_mask)


def test_launch_shape():
    """the walk is the build's for 4-byte elements; 1 launch per row, 9 matrix-wide"""
    seen = set()
    for n in WIDTHS:
        shape = capi.random_csr_launch_shape(65, n, False)
        walk = capi.dense_to_csr_launch_shape(1, 65, n, 4)
        assert all(shape[name] == walk[name] for name in ("rows_per_wave", "elements_per_lane", "rows_per_workgroup", "grid"))
        assert shape["served"] and shape["digit_passes"] == 4 and shape["launches"] == 1
        assert capi.random_csr_launch_shape(65, n, True)["launches"] == 9
        seen.add(shape["rows_per_wave"])
    assert seen == {16, 8, 4, 2, 1}                       # every lane-group width of the walk
    assert capi.random_csr_workspace_bytes(65, 129, False) == 0
    assert capi.random_csr_workspace_bytes(65, 129, True) == 4 * (4 * 256 + 1 + 2 * 65)


@pytest.mark.parametrize("n", WIDTHS)
def test_device_equals_torch_path(n):
    """every lane-group width (n <= 16, 32, 64, 128, 256) and step count (up to 4 at n = 1000), rows
    short of, equal to and beyond a wave's groups"""
    for m in (1, 5, 65):
        both_modes(m, n)


@pytest.mark.parametrize("n", (16, 64))
@pytest.mark.parametrize("m", (63, 64, 130))
def test_workgroup_edges(m, n):
    both_modes(m, n)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), **ids)
def test_half_values(dtype):
    for m, n in ((5, 3), (65, 17), (5, 129), (65, 513)):
        both_modes(m, n, dtype)
    # a step of 2**-24: float16 results reach its denormals and round to nearest even there
    check(65, 129, None, 2000, dtype, bound=2.0 ** -1)
    check(65, 129, 40, None, dtype, bound=2.0 ** -10)


@pytest.mark.parametrize("key_mask", (0x7, 0))
def test_forced_ties(key_mask):
    for m, n in ((5, 4), (65, 33), (5, 257), (130, 64), (65, 1000)):
        both_modes(m, n, key_mask=key_mask)
    if key_mask == 0:     # all keys equal: the first positions
        m, n = 65, 129
        _, row_offsets, column_indices, _, _ = check(m, n, None, 1000, key_mask=0)
        assert column_indices.tolist() == [i % n for i in range(1000)]
        assert row_offsets.tolist() == [min(r * n, 1000) for r in range(m + 1)]
        assert check(m, n, 7, None, key_mask=0)[2].tolist() == list(range(7)) * m


def test_scan_limits():
    """matrix-wide: 16384 rows are served, 16385 are not and take the torch path"""
    m, n = 16384, 4
    assert capi.random_csr_launch_shape(m, n, True)["served"]
    check(m, n, None, 20000)
    assert not capi.random_csr_launch_shape(m + 1, n, True)["served"]
    assert capi.random_csr_launch_shape(m + 1, n, False)["served"]
    with pytest.raises(RuntimeError):
        ops.random_csr(m + 1, n, total=20000, device="cuda")
    given = torch.tensor(STATE, dtype=torch.int64, device="cuda")
    values, row_indices, row_offsets, column_indices = topology.random_csr(m + 1, n, nonzeros=20000, bound=0.5,
                                                                           device="cuda", rng_state=given)
    assert_same((row_indices, row_offsets, column_indices, values),
                torch_path(m + 1, n, None, 20000, torch.float32, 0.5, STATE), "16385 x 4 through topology")
    check(m + 1, n, 2, None)                               # (per row: no row order, no limit)


@pytest.mark.parametrize("per_row", (False, True))
def test_generator(per_row):
    m, n = 65, 129
    kwargs = dict(per_row=20) if per_row else dict(total=1500)

    def run(**more):
        return ops.random_csr(m, n, dtype=torch.float32, bound=0.5, device="cuda", **kwargs, **more)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))

    torch.manual_seed(1234)
    first, second = run(), run()
    assert not same(first, second)
    assert int(first[4][0]) == int(second[4][0]) == 1234
    assert int(second[4][1]) - int(first[4][1]) == 4
    assert same(run(rng_state=second[4]), second)          # a replay consumes nothing ...
    third = run()
    assert int(third[4][1]) - int(second[4][1]) == 4       # ... of the generator
    torch.manual_seed(1234)
    again = run()
    assert same(first, again) and torch.equal(first[4], again[4])
    state = tuple(first[4].tolist())
    assert_same(first[:4], torch_path(m, n, kwargs.get("per_row"), kwargs.get("total"), torch.float32, 0.5, state),
                "a fresh draw against the torch path at the state it published")
    # the torch path on the GPU draws the same 4 of the same generator
    torch.manual_seed(1234)
    topology.enable_device_build(False)
    try:
        fallback = topology.random_csr(m, n, nonzeros=20 if per_row else 1500, per_row=per_row, bound=0.5,
                                       device="cuda", return_rng_state=True)
    finally:
        topology.enable_device_build(True)
    assert torch.equal(fallback[4], first[4]) and fallback[0].is_cuda
    assert same((fallback[1], fallback[2], fallback[3], fallback[0]), first)
    # count 0: nothing to select, the state is published all the same
    generator = torch.cuda.default_generators[torch.cuda.current_device()]
    offset = generator.get_offset()
    empty = ops.random_csr(m, n, dtype=torch.float32, device="cuda", **{name: 0 for name in kwargs})
    assert empty[3].numel() == 0 and empty[1].tolist() == [0] * (m + 1) and empty[0].tolist() == list(range(m))
    assert empty[4].tolist() == [1234, offset] and generator.get_offset() == offset + 4


def test_no_dense_temporary():
    """1024 x 1024, K = 104858, float32: outputs and workspace are about 0.9 MB; an [m, n]
    float32 image alone would be 4 MiB"""
    m = n = 1024
    total = 104858

    def run():
        return ops.random_csr(m, n, total=total, dtype=torch.float32, device="cuda")

    run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - before
    print(f"peak over the call: {raised} bytes")
    assert raised < 2 * 1024 * 1024
    assert out[3].numel() == total and int(out[1][-1]) == total


@pytest.mark.parametrize("per_row", (False, True))
def test_captured_into_a_graph(per_row):
    """The call neither synchronises nor reads back: captured on a side stream, every replay
    draws a new pattern, the one the torch path gives at the rng_state the replay wrote."""
    m, n = 65, 129
    kwargs = dict(per_row=20) if per_row else dict(total=1500)

    def run():
        return ops.random_csr(m, n, dtype=torch.float32, bound=0.5, device="cuda", **kwargs)

    torch.manual_seed(77)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                               # (warm-up on the capturing stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = run()
    replays = []
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in captured])
        state = tuple(captured[4].tolist())
        assert state[0] == 77 and state[1] % 4 == 0
        assert_same(captured[:4], torch_path(m, n, kwargs.get("per_row"), kwargs.get("total"), torch.float32, 0.5, state),
                    f"replay {replay} against the torch path at {state}")
    assert int(replays[1][4][1]) != int(replays[0][4][1])
    assert not torch.equal(replays[0][2], replays[1][2])


def dense_weight(layer):
    out_f, in_f = layer.output_features, layer.input_features
    lengths = (layer.row_offsets[1:] - layer.row_offsets[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(out_f, device=lengths.device), lengths)
    weight = torch.zeros(out_f, in_f, dtype=torch.float64, device=lengths.device)
    weight[rows, layer.column_indices.long()] = layer.values.detach().double()
    return weight


@pytest.mark.parametrize("per_row", (False, True))
def test_sparse_linear_random(per_row):
    in_f, out_f, batch, seq = 256, 128, 2, 24
    torch.manual_seed(9)
    layer = SparseLinear.random(in_f, out_f, density=0.2, per_row=per_row, device="cuda")
    nnz = round(0.2 * in_f) * out_f if per_row else round(0.2 * in_f * out_f)
    assert layer.values.is_cuda and layer.values.numel() == nnz == int(layer.row_offsets[-1])
    assert isinstance(layer.values, torch.nn.Parameter)
    bound = 1.0 / (nnz / out_f) ** 0.5
    largest = float(layer.values.detach().abs().max())
    assert 0.9 * bound < largest <= bound
    assert abs(float(layer.values.detach().mean())) < 4 * bound / (3 * nnz) ** 0.5      # (sd of the mean: bound / sqrt(3 nnz))
    x = torch.randn(batch, seq, in_f, device="cuda")

    def forward_is_consistent(what):
        want = torch.matmul(dense_weight(layer), x.double().transpose(1, 2))      # [B, out, S]
        assert rel_err_torch(layer(x), want) < 1e-4, what

    forward_is_consistent("the drawn layer")
    scores = torch.randn(out_f, in_f, device="cuda")
    source = layer.update_topology(0.3, scores, per_row=per_row)
    assert source.numel() == nnz and int((source < 0).sum()) > 0
    forward_is_consistent("after update_topology")
    layer.prune_to(density=0.1, per_row=per_row)
    assert layer.values.numel() == (round(0.1 * in_f) * out_f if per_row else round(0.1 * in_f * out_f))
    forward_is_consistent("after prune_to")
