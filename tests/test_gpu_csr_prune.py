"""GPU: top-k over the entries of a CSR pattern, written out as a smaller CSR pattern
(csrc/topology.hip; ops.csr_topk, topology.prune_csr, SparseLinear.prune_to) against the torch
path on the CPU copy of the same input.  Everything is an integer or a bit copy: every
comparison is exact.

Instance parameters (group width, elements per lane, rows per workgroup, digit passes, the row
limit) come from the host query the launches themselves decide by."""
import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

pytestmark = pytest.mark.gpu

W = 64
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {2: torch.int16, 4: torch.int32}
NAMES = ("row_indices", "row_offsets", "column_indices", "values", "source")
ids = dict(ids=lambda d: str(d).split(".")[-1])


def width(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()]) if t.is_floating_point() else t


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[width(dtype)]).view(dtype)


def csr(lengths, n, generator):
    """row_offsets and ascending random columns for rows of these lengths"""
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    row_offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    keys = torch.rand(lengths.numel(), n, generator=generator)
    order = torch.argsort(keys, dim=1)                         # a random subset of every row's columns
    taken = torch.arange(n)[None, :] < lengths[:, None]
    mask = torch.zeros(lengths.numel(), n, dtype=torch.bool).scatter_(1, order, taken)
    return row_offsets, mask.nonzero()[:, 1].to(torch.int32)


def specials(dtype):
    """NaN, +-inf, +-0, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.375, -0.375],
                                   dtype=dtype), from_bits([1], dtype)])


def quantised(count, dtype, generator, quantum=0.125):
    """few distinct magnitudes (many ties, signs mixed) with the special values among them"""
    x = ((torch.randn(count, generator=generator) / quantum).round() * quantum).to(dtype)
    s = specials(dtype)
    x[1::5][: s.numel()] = s[: x[1::5].numel()]
    return x


def random_case(lengths, n, dtype, generator):
    row_offsets, column_indices = csr(lengths, n, generator)
    return quantised(column_indices.numel(), dtype, generator), row_offsets, column_indices


def same(got, want, where=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where, g.shape, w.shape)
        assert torch.equal(bits_of(g).cpu(), bits_of(w).cpu()), (name, where)


def check(case, n, per_row=None, total=None, note=""):
    """ops.csr_topk on the device copies against the torch path on the CPU tensors.  Returns the
    device result."""
    want = topology.prune_csr(*case, n, per_row=per_row, total=total)
    got = ops.csr_topk(*(t.cuda() for t in case), per_row=per_row, total=total)
    assert all(g.is_cuda for g in got)
    assert got[4].dtype == torch.int64 and all(got[i].dtype == torch.int32 for i in (0, 1, 2))
    same(got, want, f"m={case[1].numel() - 1} nnz={case[0].numel()} {case[0].dtype} per_row={per_row} total={total} {note}")
    return got


def shape_of(case, n, total=False):
    return capi.csr_topk_launch_shape(case[1].numel() - 1, n, case[0].numel(), case[0].element_size(), total)


def boundaries(value_bytes):
    """Every mean row length that is the last of a group width, read from the query: [(mean,
    rows per workgroup there, rows per workgroup one above)]."""
    found, previous = [], None
    v = capi.csr_topk_launch_shape(1, 1, 1, value_bytes, False)["elements_per_lane"]
    for mean in range(0, W * v + 2):
        shape = capi.csr_topk_launch_shape(8, 8 * W * v, 8 * mean, value_bytes, False)
        if previous is not None and shape["group_lanes"] != previous["group_lanes"]:
            found.append((mean - 1, previous["rows_per_workgroup"], shape["rows_per_workgroup"]))
        previous = shape
    assert len(found) == 4 and previous["group_lanes"] == W     # groups of 4 -> 8 -> 16 -> 32 -> 64 lanes
    return v, found


def lengths_around(mean, m, generator):
    """m row lengths of sum mean * m exactly -- the query sees this mean -- in rows of 2 * mean
    columns: an empty row and a full row among them (m >= 2), the others scattered in pairs."""
    n = 2 * mean
    lengths = [mean] * m
    if m >= 2:
        lengths[0], lengths[1] = 0, n
    for i in range(2, m - 1, 2):
        d = int(torch.randint(0, mean + 1, (1,), generator=generator))
        lengths[i], lengths[i + 1] = mean - d, mean + d
    return lengths, max(n, 1)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_every_instance_at_its_edges(dtype):
    generator = torch.Generator().manual_seed(2025)
    v, found = boundaries(width(dtype))
    assert capi.csr_topk_launch_shape(8, 8, 8, width(dtype), True)["digit_passes"] == width(dtype)
    for last, r_at, r_above in found:
        for mean, r in ((last, r_at), (last + 1, r_above)):
            for m in sorted({1, r - 1, r, r + 1}):
                lengths, n = lengths_around(mean, m, generator)
                case = random_case(lengths, n, dtype, generator)
                nnz = case[0].numel()
                for total in (False, True):
                    shape = shape_of(case, n, total)
                    assert shape["rows_per_workgroup"] == r and shape["group_lanes"] * r == 4 * W
                    assert shape["elements_per_lane"] == v
                for k in sorted({1, (n + 2) // 3, n - 1}):
                    check(case, n, per_row=k)
                for K in sorted({1, (nnz + 2) // 3, nnz - 1}):
                    check(case, n, total=K)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_long_rows_take_several_steps(dtype):
    """One long row under the widest group, and under the narrowest (a short mean): the walk
    loops; row starts fall at every alignment relative to a 16-byte load."""
    generator = torch.Generator().manual_seed(2026)
    v = 16 // width(dtype)
    long = 2 * W * v + 3
    for lengths, lanes in (((long, 0, 1), W), ((1, long, 0), W), ([long] + [3, 0, 5, 2, 1, 4, 7] * 30, 4),
                           ([2, 1, 6, 3] * 16 + [9 * v + 1], 4)):
        case = random_case(lengths, long + 5, dtype, generator)
        assert shape_of(case, long + 5)["group_lanes"] == lanes
        nnz = case[0].numel()
        for k in (1, 2, long // 3, long - 1):
            check(case, long + 5, per_row=k)
        for K in (1, nnz // 3, nnz - 1):
            check(case, long + 5, total=K)
    starts = set((case[1][:-1] % v).tolist())
    assert starts == set(range(v))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_count_edges(dtype):
    generator = torch.Generator().manual_seed(2027)
    for lengths, n in (((3, 0, 9, 5, 9), 9), ((70,), 70), ((1,), 1), ((0, 0, 0, 0, 0), 6), ((0,), 3), ((), 4),
                       ([300, 7, 0, 120] * 3, 300)):
        case = random_case(lengths, n, dtype, generator)
        nnz, m = case[0].numel(), len(lengths)
        for k in sorted({0, 1, n - 1, n}):
            got = check(case, n, per_row=k)
            assert int(got[1][-1]) == got[2].numel() == sum(min(length, k) for length in lengths)
        for K in sorted({0, min(1, nnz), max(nnz - 1, 0), nnz}):
            got = check(case, n, total=K)
            assert got[2].numel() == K and int(got[1][-1]) == K and got[0].numel() == m


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_all_values_equal(dtype):
    """Only the index decides: the first k entries of every row, the first K of the arrays --
    the quota ends at a row start, in the middle of a row and in the middle of a walk step."""
    generator = torch.Generator().manual_seed(2028)
    v = 16 // width(dtype)
    lengths = [5 * W * v // 2, 0, 3, W * v, 77, 1]
    n = max(lengths)
    row_offsets, column_indices = csr(lengths, n, generator)
    nnz = column_indices.numel()
    values = torch.where(torch.arange(nnz) % 3 == 0, -2.5, 2.5).to(dtype)
    case = (values, row_offsets, column_indices)
    step = shape_of(case, n)["group_lanes"] * v
    assert step < lengths[0]
    for k in (1, 2, step - 1, step, step + 1, n - 1):
        got = check(case, n, per_row=k)
        starts = row_offsets[:-1].to(torch.int64)
        want = torch.cat([starts[r] + torch.arange(min(lengths[r], k)) for r in range(len(lengths))])
        assert torch.equal(got[4].cpu(), want)
    for K in (1, step // 2, step, step + v + 1, lengths[0] - 1, lengths[0], lengths[0] + 2, lengths[0] + 3 + step + 5,
              nnz - 1):
        got = check(case, n, total=K)
        assert torch.equal(got[4].cpu(), torch.arange(K))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_threshold_group_over_rows_and_workgroups(dtype):
    """Two magnitudes; the lower one is the threshold group, spread over every row and over
    several workgroups of the flat walk.  The quota ends in each of them."""
    generator = torch.Generator().manual_seed(2029)
    m, length, n = 40, 640, 700
    row_offsets, column_indices = csr([length] * m, n, generator)
    nnz = m * length
    values = torch.where(torch.rand(nnz, generator=generator) < 0.1, 3.0, -1.0).to(dtype)
    values = values * torch.where(torch.rand(nnz, generator=generator) < 0.5, -1.0, 1.0).to(dtype)
    case = (values, row_offsets, column_indices)
    assert shape_of(case, n, True)["flat_grid"] >= 2
    above = int((values.abs() == 3.0).sum())
    for quota in (0, 1, length // 2, nnz // 3, nnz // 2 + 7, nnz - above - 1):
        got = check(case, n, total=above + quota)
        lengths = (got[1][1:] - got[1][:-1]).cpu()
        assert int(lengths.sum()) == above + quota
    check(case, n, total=above - 5)                        # the threshold group is the upper one
    check(case, n, per_row=length // 5)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_digits(dtype):
    """Keys that differ only in ONE 8-bit digit, one case per digit pass: every pass has to decide."""
    passes = width(dtype)
    generator = torch.Generator().manual_seed(2030)
    for p in range(passes):
        shift = 8 * (passes - 1 - p)
        rest = sum(0x21 << (8 * q) for q in range(passes) if 8 * q != shift)
        digits = list(range(0x80 if p == 0 else 0x100))           # (the sign is no part of the key)
        patterns = [(d << shift) | rest for d in digits] * 3
        values = from_bits(patterns, dtype)[torch.randperm(len(patterns), generator=generator)]
        bits = values.view(BITS[passes])
        negative = bits | torch.tensor(-(1 << (8 * passes - 1)), dtype=BITS[passes])
        values = torch.where(torch.rand(bits.numel(), generator=generator) < 0.5, bits, negative).view(dtype)
        keys = topology.magnitude_keys(values)
        assert sorted(set(keys.tolist())) == sorted((d << shift) | rest for d in digits)      # (bits survived)
        nnz = values.numel()
        lengths = [nnz // 4, 0, nnz // 2, nnz - nnz // 4 - nnz // 2]
        row_offsets, column_indices = csr(lengths, nnz, generator)
        case = (values, row_offsets, column_indices)
        for k in (1, 2, 50, nnz // 4 - 1):
            check(case, nnz, per_row=k, note=f"pass {p}")
        for K in (1, 7, nnz // 3, nnz - 2):
            check(case, nnz, total=K, note=f"pass {p}")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_scan_block_edges_and_the_row_limit(dtype):
    generator = torch.Generator().manual_seed(2031)
    for m in (1023, 1024, 1025):
        lengths = torch.randint(0, 4, (m,), generator=generator)
        case = random_case(lengths, 3, dtype, generator)
        nnz = case[0].numel()
        for K in (1, m, nnz - 1):
            check(case, 3, total=K)
        check(case, 3, per_row=2)
    limit = 16384
    for m in (limit, limit + 1):
        lengths = torch.randint(0, 3, (m,), generator=generator)
        case = random_case(lengths, 2, dtype, generator)
        assert shape_of(case, 2, True)["served"] == shape_of(case, 2, False)["served"] == (m == limit)
        if m == limit:
            check(case, 2, total=limit // 2)
            check(case, 2, per_row=1)
            continue
        device = [t.cuda() for t in case]
        for kwargs in (dict(total=limit // 2), dict(per_row=1)):
            with pytest.raises(RuntimeError):
                ops.csr_topk(*device, **kwargs)
            got = topology.prune_csr(*device, 2, **kwargs)          # ... answered by the torch path
            assert all(g.is_cuda for g in got)
            same(got, topology.prune_csr(*case, 2, **kwargs))


def test_prune_csr_routes():
    generator = torch.Generator().manual_seed(2032)
    lengths = torch.randint(0, 91, (70,), generator=generator)
    case = random_case(lengths, 90, torch.float32, generator)
    finite = (torch.nan_to_num(case[0], nan=3.0, posinf=4.0, neginf=-4.0),) + case[1:]
    for kwargs in (dict(total=1234), dict(per_row=9)):
        want = topology.prune_csr(*finite, 90, **kwargs)
        results = [topology.prune_csr(finite[0].cuda().requires_grad_(), finite[1].cuda(), finite[2].cuda(), 90,
                                      **kwargs)]
        topology.enable_device_build(False)
        try:
            results.append(topology.prune_csr(*(t.cuda() for t in finite), 90, **kwargs))
        finally:
            topology.enable_device_build(True)
        for got in results:
            assert all(g.is_cuda for g in got) and not got[3].requires_grad
            same(got, want)
        wide = topology.prune_csr(finite[0].double().cuda(), finite[1].cuda(), finite[2].cuda(), 90, **kwargs)
        assert wide[3].dtype == torch.float64 and torch.equal(wide[3].cpu(), want[3].double())   # ranked as .float()
        assert all(torch.equal(g.cpu(), w) for g, w in zip(wide[:3] + wide[4:], want[:3] + want[4:]))


def test_reproducible():
    generator = torch.Generator().manual_seed(2033)
    case = random_case([110] * 600, 1100, torch.float32, generator)
    assert case[0].numel() == 66000
    device = [t.cuda() for t in case]
    for kwargs in (dict(per_row=40), dict(total=22000)):
        first, second = ops.csr_topk(*device, **kwargs), ops.csr_topk(*device, **kwargs)
        same(first, second)
        check(case, 1100, **kwargs)


def test_total_mode_is_capturable():
    """Total mode neither synchronises nor reads back, and its allocations are torch's own per
    call: it is captured into a graph on a side stream, and each replay on new values in the
    captured buffers equals the eager call.  (Per-row mode reads one integer back.)"""
    generator = torch.Generator().manual_seed(2034)
    lengths = torch.randint(0, 301, (70,), generator=generator)
    case = random_case(lengths, 300, torch.float32, generator)
    device = [t.cuda() for t in case]
    K = case[0].numel() // 3
    ops.csr_topk(*device, total=K)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.csr_topk(*device, total=K)
    for _ in range(2):
        fresh = (quantised(case[0].numel(), torch.float32, generator),) + case[1:]
        device[0].copy_(fresh[0])
        graph.replay()
        torch.cuda.synchronize()
        same(captured, ops.csr_topk(*device, total=K))
        same(captured, topology.prune_csr(*fresh, 300, total=K))


# ---- the module ----

OUT, IN, BATCH, SEQ = 64, 96, 2, 8


def explicit_module(values, row_indices, row_offsets, column_indices):
    """A SparseLinear on a given pattern, explicit zeros included"""
    module = SparseLinear(IN, OUT).to(values.device)
    module.values = torch.nn.Parameter(values.detach().clone())
    module.row_indices, module.row_offsets, module.column_indices = (
        row_indices.clone(), row_offsets.clone(), column_indices.clone())
    functional.register_static_topology(module.row_indices, module.row_offsets, module.column_indices)
    return module


def forward_backward(module, x_host):
    x = x_host.cuda().requires_grad_()
    module.values.grad = None
    y = module(x)
    y.backward(torch.ones_like(y) * 0.5)
    return y.detach(), module.values.grad.clone(), x.grad.clone()


@pytest.mark.parametrize("per_row", (False, True), ids=("matrix", "per_row"))
@pytest.mark.parametrize("input_dtype", (torch.float32, torch.float16), **ids)
def test_prune_to_serves_no_stale_state(input_dtype, per_row):
    generator = torch.Generator().manual_seed(2035)
    w = torch.randn(OUT, IN, generator=generator)
    module = SparseLinear.from_dense(w.cuda(), density=0.5, per_row=per_row)
    x_host = torch.randn(BATCH, SEQ, IN, generator=generator).to(input_dtype)
    forward_backward(module, x_host)           # plans, transposed topology and images of the OLD pattern exist
    with torch.no_grad():
        module(x_host.cuda())
    optimizer = torch.optim.Adam([module.values], lr=0.1)
    optimizer.step()
    old = module.values
    old_state = {name: t.clone() for name, t in optimizer.state[old].items()}
    old_arrays = (old.detach().clone(), module.row_offsets.clone(), module.column_indices.clone())

    source = module.prune_to(density=0.25, per_row=per_row)

    # the same step on a CPU module of the same pattern
    twin = SparseLinear(IN, OUT)
    twin.values = torch.nn.Parameter(old_arrays[0].cpu())
    twin.row_offsets, twin.column_indices = old_arrays[1].cpu(), old_arrays[2].cpu()
    twin.row_indices = topology.diffsort(twin.row_offsets)
    twin_source = twin.prune_to(density=0.25, per_row=per_row)
    assert source.is_cuda and torch.equal(source.cpu(), twin_source)
    for name in ("row_indices", "row_offsets", "column_indices"):
        assert torch.equal(getattr(module, name).cpu(), getattr(twin, name)), name
    assert torch.equal(module.values.detach().view(torch.int32).cpu(), twin.values.detach().view(torch.int32))
    assert module.values is not old and isinstance(module.values, torch.nn.Parameter)
    assert module.values.requires_grad and module.values.grad is None
    assert torch.equal(old.detach(), old_arrays[0])
    if per_row:                                              # the layer stays row balanced
        assert torch.equal(module.row_offsets.cpu(), torch.arange(OUT + 1, dtype=torch.int32) * 24)
    else:
        assert module.values.numel() == round(0.25 * OUT * IN)

    topology.remap_optimizer_state(optimizer, old, module.values, source)
    state = optimizer.state[module.values]
    assert old not in optimizer.state and torch.equal(state["step"], old_state["step"])
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(state[name].view(torch.int32), old_state[name].view(torch.int32)[source]), name
    for round_ in range(2):
        fresh = explicit_module(module.values, module.row_indices, module.row_offsets, module.column_indices)
        got, want = forward_backward(module, x_host), forward_backward(fresh, x_host)
        for g, w_, name in zip(got, want, ("forward", "values.grad", "input.grad")):
            assert torch.equal(g, w_), (name, round_)
        with torch.no_grad():
            assert torch.equal(module(x_host.cuda()), fresh(x_host.cuda()))
        before = module.values.detach().clone()
        optimizer.step()                        # the carried Adam trains the new Parameter
        assert not torch.equal(module.values.detach(), before)
