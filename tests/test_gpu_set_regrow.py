"""GPU: the drop-and-grow step under generated scores on the device (csrc/topology.hip;
ops.csr_regrow_random, ops.csr_regrow_total_random, SparseLinear.set_update) against the torch
path of the same rule on the CPU with the same rng_state, and against the stored-score kernels
(ops.csr_regrow, ops.csr_regrow_total) given the keys as a float32 tensor.  Integers and value
bits: every comparison is exact.  The torch path itself is held to a numpy restatement in
tests/test_set_regrow_cpu.py.

The axes -- widths, rows, densities, drops, key masks, dtypes, grow bounds, the two modes -- are
not multiplied out (27648 cases): test_device_equals_torch_path takes every (n, m, density, drop,
mode) and deals (key_mask, dtype, grow_bound) round over them, so that every triple meets every
width; the tests below it take every key mask, and every dtype with every bound, through both modes
at shapes of every lane-group width."""
import itertools

import pytest
import torch

from helpers import rel_err_torch
from tests import regrow_total_cases as C
from tests import set_regrow_cases as S
from torch_sputnik_amd import SparseLinear, capi, ops, topology

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 513, 1000)
DENSITIES = (0.0, 0.3, 1.0)
BOUNDS = (None, 0.5)
TRIPLES = tuple(itertools.product(S.MASKS, S.DTYPES, BOUNDS))
MODES = ("per_row", "total")
ids = dict(ids=lambda d: str(d).split(".")[-1])


def names(mode):
    return S.PER_ROW_NAMES if mode == "per_row" else C.NAMES


def on_gpu(tensors):
    return tuple(t.cuda() for t in tensors)


def device_step(mode, old, drop, n, key_mask=S.DEFAULT, bound=None, rng_state=None):
    """the op of the mode on GPU tensors -> (the step's tensors, rng_state)"""
    op = ops.csr_regrow_random if mode == "per_row" else ops.csr_regrow_total_random
    out = op(*old, drop.cuda() if torch.is_tensor(drop) else drop, n, grow_bound=bound, rng_state=rng_state,
             key_mask=key_mask)
    assert all(t.is_cuda for t in out)
    return out[:-1], out[-1]


def torch_step(mode, old, drop, n, state, key_mask=S.DEFAULT, bound=None):
    return (S.torch_per_row if mode == "per_row" else S.torch_total)(*old, drop, n, state, key_mask, bound)


def drop_of(mode, old, how):
    return S.drop_counts(old[1], how) if mode == "per_row" else S.drop_total(old[0].numel(), how)


def check(mode, old, how, n, key_mask=S.DEFAULT, bound=None, state=S.STATE, where=""):
    """the device step at `state` against the torch path on the CPU"""
    drop = drop_of(mode, old, how)
    where = f"{mode} {old[1].numel() - 1}x{n} nnz {old[0].numel()} {old[0].dtype} drop {how} mask {key_mask:#x} " \
            f"bound {bound} {where}"
    got, used = device_step(mode, on_gpu(old), drop, n, key_mask, bound, S.state_tensor(state, "cuda"))
    assert used.tolist() == list(state), where
    S.assert_same(got, torch_step(mode, old, drop, n, state, key_mask, bound), names(mode), where)
    return got


def sweep(m_values, n, generator, deal=0):
    """every (m, density, drop, mode) at width n, the (key_mask, dtype, bound) triples dealt round"""
    i = 0
    for m in m_values:
        for density in DENSITIES:
            patterns = {}
            for how in S.DROPS:
                for mode in MODES:
                    key_mask, dtype, bound = TRIPLES[(7 * i + 5 * (i // len(TRIPLES)) + deal) % len(TRIPLES)]
                    i += 1
                    if dtype not in patterns:
                        patterns[dtype] = S.pattern(m, n, density, dtype, generator)
                    check(mode, patterns[dtype], how, n, key_mask, bound, where=f"density {density}")


def test_launch_shape():
    """the walk is the build's for 4-byte elements, four score passes; per row one launch and the
    limits of the stored-score steps at 4-byte scores"""
    seen = set()
    for n in WIDTHS:
        walk = capi.dense_to_csr_launch_shape(1, 65, n, 4)
        total = capi.csr_regrow_random_launch_shape(65, n, 100, 4, True)
        per_row = capi.csr_regrow_random_launch_shape(65, n, 100, 4, False)
        assert all(total[name] == walk[name] for name in ("rows_per_wave", "elements_per_lane", "rows_per_workgroup", "grid"))
        assert per_row["rows_per_wave"] == min(walk["rows_per_wave"], 8)
        assert total["served"] and per_row["served"] and total["score_digit_passes"] == per_row["score_digit_passes"] == 4
        assert total["launches"] == 16 and per_row["launches"] == 1
        seen.add(total["rows_per_wave"])
    assert seen == {16, 8, 4, 2, 1}                           # every lane-group width of the walk


@pytest.mark.parametrize("n", WIDTHS)
def test_device_equals_torch_path(n):
    """every lane-group width (n <= 16, 32, 64, 128, 256) and step count (up to 4 at n = 1000); rows
    short of, equal to and beyond a wave's groups; empty, ragged and full patterns; every drop"""
    sweep((1, 5, 65), n, torch.Generator().manual_seed(300 + n), deal=WIDTHS.index(n))


@pytest.mark.parametrize("n", (16, 64))
@pytest.mark.parametrize("m", (63, 64, 130))
def test_workgroup_edges(m, n):
    sweep((m,), n, torch.Generator().manual_seed(400 + m + n), deal=m + n)


@pytest.mark.parametrize("key_mask", S.MASKS, ids=hex)
def test_key_masks(key_mask):
    """Few key bits force ties; mask 0 makes every key tie, and matrix-wide the quota then has to
    be handed across rows and workgroups by the scan: Grown is the first d open positions."""
    generator = torch.Generator().manual_seed(500 + key_mask % 97)
    for m, n in ((5, 4), (65, 33), (5, 257), (130, 64), (65, 1000)):
        for density in (0.3, 1.0):
            old = S.pattern(m, n, density, torch.float32, generator)
            for how in ("one", "third", "all"):
                for mode in MODES:
                    check(mode, old, how, n, key_mask, 0.5 if how == "third" else None)
    if key_mask == 0:
        m, n = 130, 64                                          # 9 workgroups of 16 rows
        old = S.pattern(m, n, 0.3, torch.float32, generator)
        nnz = old[0].numel()
        _, row_offsets, columns, _, source = check("total", old, "all", n, 0)
        assert bool((source < 0).all())                         # everything dropped, so every position is open:
        assert columns.tolist() == [i % n for i in range(nnz)]  # the first nnz of them, row-major
        assert row_offsets.tolist() == [min(r * n, nnz) for r in range(m + 1)]


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("dtype", S.DTYPES, **ids)
def test_dtypes_and_grow_bounds(dtype, bound):
    generator = torch.Generator().manual_seed(600)
    for m, n in ((5, 3), (65, 17), (63, 64), (5, 129), (65, 513)):
        old = S.pattern(m, n, 0.3, dtype, generator)
        for how in ("third", "all"):
            for mode in MODES:
                got = check(mode, old, how, n, bound=bound)
                grown = got[-1] < 0
                if bound is None:
                    assert not C.bits_of(got[-2])[grown].any()          # +0.0
                else:
                    assert bool((got[-2][grown].float().abs() <= bound).all())
    if bound is not None:      # a step of 2**-24: float16 results reach its denormals and round to nearest even there
        old = S.pattern(65, 129, 0.3, dtype, generator)
        for mode in MODES:
            check(mode, old, "all", 129, bound=2.0 ** -1)
            check(mode, old, "third", 129, bound=2.0 ** -10)
            check(mode, old, "third", 129, bound=0.0)


def test_widest_row():
    """per row, n = 61440: one row per wave, 64 KiB of LDS, 60 steps"""
    m, n = 2, 61440
    assert capi.csr_regrow_random_launch_shape(m, n, 100, 4, False)["lds_bytes"] == 65536
    generator = torch.Generator().manual_seed(700)
    old = S.pattern(m, n, 0.3, torch.float32, generator)
    check("per_row", old, "third", n, bound=0.5)
    with pytest.raises(RuntimeError):
        ops.csr_regrow_random(*on_gpu(S.pattern(m, n + 1, 0.01, torch.float32, generator)),
                              torch.zeros(m, dtype=torch.int32, device="cuda"), n + 1)


def test_beyond_the_limits_takes_the_torch_path():
    """matrix-wide above 16384 rows: the op raises, topology takes the rule in torch on the GPU"""
    m, n = 16385, 4
    generator = torch.Generator().manual_seed(701)
    old = S.pattern(m, n, 0.3, torch.float32, generator)
    state = S.state_tensor(S.STATE, "cuda")
    with pytest.raises(RuntimeError):
        ops.csr_regrow_total_random(*on_gpu(old), 100, n, rng_state=state)
    got = topology.regrow_total_random(*on_gpu(old), 100, n, grow_bound=0.5, rng_state=state)
    assert all(t.is_cuda for t in got)
    S.assert_same(got, S.torch_total(*old, 100, n, S.STATE, bound=0.5), C.NAMES)
    check("per_row", old, "one", n)                            # (per row: no row order, no limit)


@pytest.mark.parametrize("mode", MODES)
def test_device_against_the_stored_score_kernels(mode):
    """The same calls against ops.csr_regrow / ops.csr_regrow_total under a float32 score tensor on
    the GPU whose bits are the keys (numpy Philox): a check that does not pass through the torch
    path.  Grown values: zeros as the stored kernels write them, or the numpy value stream."""
    generator = torch.Generator().manual_seed(800)
    stored = ops.csr_regrow if mode == "per_row" else ops.csr_regrow_total
    i = 0
    for m, n in ((1, 1), (5, 3), (65, 17), (64, 64), (130, 16), (5, 129), (65, 257), (5, 1000)):
        for density in DENSITIES:
            for how in S.DROPS:
                key_mask, dtype, bound = TRIPLES[(7 * i) % len(TRIPLES)]
                i += 1
                old = S.pattern(m, n, density, dtype, generator)
                drop = drop_of(mode, old, how)
                where = f"{mode} {m}x{n} density {density} drop {how} mask {key_mask:#x} {dtype} bound {bound}"
                got, _ = device_step(mode, on_gpu(old), drop, n, key_mask, bound, S.state_tensor(S.STATE, "cuda"))
                scores = S.key_scores(m, n, S.STATE, key_mask).cuda()
                want = stored(*on_gpu(old), drop.cuda() if torch.is_tensor(drop) else drop, scores)
                S.assert_same(got[:-2], want[:-2], names(mode)[:-2], where)         # the pattern
                assert torch.equal(got[-1], want[-1]), where                        # source
                grown = (got[-1] < 0).cpu()
                values, zeros = C.bits_of(got[-2]).cpu(), C.bits_of(want[-2]).cpu()
                assert torch.equal(values[~grown], zeros[~grown]) and not zeros[grown].any(), where
                if bound is None:
                    assert not values[grown].any(), where
                else:
                    offsets = (old[1] if mode == "per_row" else got[1].cpu()).long()
                    rows = torch.repeat_interleave(torch.arange(m), offsets[1:] - offsets[:-1])
                    image = C.bits_of(S.value_image(m, n, S.STATE, bound, dtype))
                    assert torch.equal(values[grown], image[rows[grown], got[-3].cpu().long()[grown]]), where


@pytest.mark.parametrize("mode", MODES)
def test_generator(mode):
    """torch.manual_seed makes runs repeat; a call draws 4 of the device generator's offset; the
    state it returns reproduces it on the GPU and on the CPU"""
    m, n = 65, 129
    generator = torch.Generator().manual_seed(900)
    old = S.pattern(m, n, 0.3, torch.float32, generator)
    drop = drop_of(mode, old, "third")
    gpu = on_gpu(old)

    def run(**more):
        got, state = device_step(mode, gpu, drop, n, bound=0.5, **more)
        return got + (state,)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a[:-1], b[:-1]))

    torch.manual_seed(1234)
    first, second = run(), run()
    assert not same(first, second)
    assert int(first[-1][0]) == int(second[-1][0]) == 1234
    assert int(second[-1][1]) - int(first[-1][1]) == 4
    assert same(run(rng_state=second[-1]), second)             # a replay consumes nothing ...
    third = run()
    assert int(third[-1][1]) - int(second[-1][1]) == 4         # ... of the generator
    torch.manual_seed(1234)
    again = run()
    assert same(first, again) and torch.equal(first[-1], again[-1])
    state = tuple(first[-1].tolist())
    S.assert_same(first[:-1], torch_step(mode, old, drop, n, state, bound=0.5), names(mode),
                  "a fresh draw against the torch path at the state it published")
    # the torch path on the GPU draws the same 4 of the same generator
    torch.manual_seed(1234)
    topology.enable_device_build(False)
    try:
        function = topology.regrow_per_row_random if mode == "per_row" else topology.regrow_total_random
        fallback = function(*gpu, drop.cuda() if torch.is_tensor(drop) else drop, n, grow_bound=0.5,
                            return_rng_state=True)
    finally:
        topology.enable_device_build(True)
    assert torch.equal(fallback[-1], first[-1]) and fallback[0].is_cuda
    S.assert_same(fallback[:-1], first[:-1], names(mode))
    # no entries: nothing to select, the state is published all the same
    device_generator = torch.cuda.default_generators[torch.cuda.current_device()]
    offset = device_generator.get_offset()
    empty = on_gpu(S.pattern(m, n, 0.0, torch.float32, generator))
    got, state = device_step(mode, empty, drop_of(mode, empty, "all"), n)
    assert got[-1].numel() == 0 and state.tolist() == [1234, offset] and device_generator.get_offset() == offset + 4
    if mode == "total":
        assert got[1].tolist() == [0] * (m + 1) and got[0].tolist() == list(range(m))


@pytest.mark.parametrize("mode", MODES)
def test_captured_into_a_graph(mode):
    """The call neither synchronises nor reads back: captured on a side stream, every replay
    draws new scores, and the step is the one the torch path gives at the rng_state the replay
    wrote."""
    m, n = 65, 129
    generator = torch.Generator().manual_seed(1000)
    old = S.pattern(m, n, 0.3, torch.float32, generator)
    drop = drop_of(mode, old, "third")
    gpu = on_gpu(old)
    drop_gpu = drop.cuda() if torch.is_tensor(drop) else drop
    op = ops.csr_regrow_random if mode == "per_row" else ops.csr_regrow_total_random

    def run():
        return op(*gpu, drop_gpu, n, grow_bound=0.5)

    torch.manual_seed(77)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                   # (warm-up on the capturing stream)
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
        state = tuple(captured[-1].tolist())
        assert state[0] == 77 and state[1] % 4 == 0
        S.assert_same(captured[:-1], torch_step(mode, old, drop, n, state, bound=0.5), names(mode),
                      f"replay {replay} against the torch path at {state}")
    assert int(replays[1][-1][1]) != int(replays[0][-1][1])
    assert not torch.equal(replays[0][-3], replays[1][-3])     # other values: other positions were grown


def test_no_dense_array():
    """1024 x 1024 at density 0.1, float32: outputs, planes and workspace of one set_update come to
    about 2 MB; one [out, in] float32 score image alone is 4.2 MB."""
    size = 1024
    torch.manual_seed(5)
    layer = SparseLinear.random(size, size, density=0.1, device="cuda")
    layer.set_update(0.3)                                       # (warm-up)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    source = layer.set_update(0.3)
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - before
    print(f"peak over set_update: {raised} bytes; one score image: {size * size * 4} bytes")
    assert raised < size * size * 4
    assert int((source < 0).sum()) == int(0.3 * layer.values.numel())
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    layer.update_topology(0.3, grow_scores=None)
    torch.cuda.synchronize()
    print(f"peak over update_topology(grow_scores=None): {torch.cuda.max_memory_allocated() - before} bytes")


def dense_weight(layer):
    out_f, in_f = layer.output_features, layer.input_features
    lengths = (layer.row_offsets[1:] - layer.row_offsets[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(out_f, device=lengths.device), lengths)
    weight = torch.zeros(out_f, in_f, dtype=torch.float64, device=lengths.device)
    weight[rows, layer.column_indices.long()] = layer.values.detach().double()
    return weight


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("per_row", (False, True))
def test_module_and_its_cpu_twin(per_row, bound):
    in_f, out_f, batch, seq = 256, 128, 2, 24
    drawn = S.state_tensor((9, 40))
    layer = SparseLinear.random(in_f, out_f, density=0.2, per_row=per_row, device="cuda", rng_state=drawn.cuda())
    twin = SparseLinear.random(in_f, out_f, density=0.2, per_row=per_row, rng_state=drawn)
    parameter, nnz = layer.values, layer.values.numel()
    state = S.state_tensor(S.STATE)
    source, used = layer.set_update(0.3, per_row=per_row, grow_bound=bound, rng_state=state.cuda(), return_rng_state=True)
    twin_source = twin.set_update(0.3, per_row=per_row, grow_bound=bound, rng_state=state)
    assert layer.values is parameter and source.is_cuda and used.tolist() == list(S.STATE)
    S.assert_same((layer.row_indices, layer.row_offsets, layer.column_indices, layer.values.detach(), source),
                  (twin.row_indices, twin.row_offsets, twin.column_indices, twin.values.detach(), twin_source), C.NAMES)
    grown = source < 0
    assert source.numel() == nnz and int(grown.sum()) > 0
    assert bool((layer.values.detach()[grown] != 0).any()) == (bound is not None)
    x = torch.randn(batch, seq, in_f, device="cuda")
    want = torch.matmul(dense_weight(layer), x.double().transpose(1, 2))      # [B, out, S]
    assert rel_err_torch(layer(x), want) < 1e-4
    # without a state the step draws from the device generator and repeats under the same seed
    torch.manual_seed(31)
    a = layer.set_update(0.3, per_row=per_row, grow_bound=bound, return_rng_state=True)
    assert int(a[1][0]) == 31 and a[1].is_cuda and int((a[0] < 0).sum()) > 0
    assert rel_err_torch(layer(x), torch.matmul(dense_weight(layer), x.double().transpose(1, 2))) < 1e-4


def test_binding_checks():
    """The argument checks of the binding itself, reached through torch.ops.torch_sputnik directly
    (ops.py turns the same inputs away before the binding sees them): every bad input is a
    host-side rejection before any launch, a RuntimeError."""
    T = torch.ops.torch_sputnik
    m, n = 4, 8
    values, row_offsets, column_indices = on_gpu(S.pattern(m, n, 0.5, torch.float32, torch.Generator().manual_seed(1100)))
    nnz = values.numel()
    drops = torch.ones(m, dtype=torch.int32, device="cuda")
    state = S.state_tensor(S.STATE, "cuda")

    def per_row(v=values, ro=row_offsets, ci=column_indices, d=drops, width=n, scale=-1.0, st=state, mask=S.DEFAULT):
        return T.csr_regrow_random(v, ro, ci, d, width, scale, st, mask)

    def total(v=values, ro=row_offsets, ci=column_indices, d=2, width=n, scale=-1.0, st=state, mask=S.DEFAULT):
        return T.csr_regrow_total_random(v, ro, ci, d, width, scale, st, mask)

    assert len(per_row()) == 4 and len(total()) == 6 and per_row(st=None)[3].is_cuda
    for op in (per_row, total):
        for bad in (dict(mask=S.DEFAULT + 1), dict(mask=-1), dict(scale=float("inf")), dict(width=-1),
                    dict(v=values.double()), dict(v=values.cpu()), dict(v=values[:-1]), dict(ro=row_offsets.cpu()),
                    dict(ro=row_offsets.long()), dict(ci=column_indices.long()), dict(ci=column_indices.cpu()),
                    dict(st=state.cpu()), dict(st=state.int()), dict(st=torch.zeros(3, dtype=torch.int64, device="cuda"))):
            with pytest.raises(RuntimeError):
                op(**bad)
                pytest.fail(f"{op.__name__} accepted {bad}")
    for bad in (dict(d=drops[:-1]), dict(d=drops.long()), dict(d=drops.cpu()), dict(width=61441)):
        with pytest.raises(RuntimeError):
            per_row(**bad)
            pytest.fail(f"per_row accepted {bad}")
    for bad in (dict(d=-1), dict(d=nnz + 1), dict(width=65537)):
        with pytest.raises(RuntimeError):
            total(**bad)
            pytest.fail(f"total accepted {bad}")
