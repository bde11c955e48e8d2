"""GPU: top-k selection written out as a CSR topology (csrc/topology.hip; ops.topk_to_csr,
topology.magnitude_prune, SparseLinear.from_dense / update_topology) against the torch path on
the CPU copy of the same input.  Everything is an integer or a bit copy: every comparison is
exact.

Instance parameters (rows per wave, elements per lane, rows per workgroup, digit passes, the
row limit of total mode) come from the host query the launches themselves decide by."""
import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

pytestmark = pytest.mark.gpu

W = 64
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {2: torch.int16, 4: torch.int32}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()])


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def check(host, per_row=None, total=None, values_from=None, device=None, device_values=None, note=""):
    """ops.topk_to_csr on the device copy (or the given device view of the same numbers)
    against the torch path on the CPU tensor.  Returns the device result."""
    want = topology.topk_to_csr(host, per_row=per_row, total=total, values_from=values_from)
    scores = host.cuda() if device is None else device
    if device_values is None and values_from is not None:
        device_values = values_from.cuda()
    got = ops.topk_to_csr(scores, per_row=per_row, total=total, values_from=device_values)
    where = f"{tuple(host.shape)} {host.dtype} per_row={per_row} total={total} {note}"
    for g, w, name in zip(got, want, ("row_indices", "row_offsets", "column_indices", "values")):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (name, where)
        if name == "values":
            assert torch.equal(bits_of(g).cpu(), bits_of(w)), (name, where)
        else:
            assert g.dtype == torch.int32 and torch.equal(g.cpu(), w), (name, where)
    return got


def specials(dtype):
    """NaN, +-inf, +-0, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.375, -0.375],
                                   dtype=dtype), from_bits([1], dtype)])


def random_scores(m, n, dtype, generator, quantum=0.125):
    """Few distinct magnitudes (many ties, signs mixed), one all-equal row, one all-zero row and
    the special values where they fit."""
    x = (torch.randn(m, n, generator=generator) / quantum).round() * quantum
    if m > 2:
        x[m // 2] = -1.5
        x[m - 1] = 0.0
    x = x.to(dtype)
    flat = x.reshape(-1)
    s = specials(dtype)
    flat[1::5][: s.numel()] = s[: flat[1::5].numel()]
    return x


def boundaries(element_bytes):
    """Every n that is the last of a rows-per-wave instance, read from the query."""
    v = capi.topk_to_csr_launch_shape(1, 1, element_bytes, False)["elements_per_lane"]
    found, previous = [], None
    for n in range(1, W * v + 2):
        rows = capi.topk_to_csr_launch_shape(1, n, element_bytes, False)["rows_per_wave"]
        if previous is not None and rows != previous:
            found.append(n - 1)
        previous = rows
    assert len(found) == 4 and previous == 1   # 16 -> 8 -> 4 -> 2 -> 1 rows per wave
    return v, found


def shapes(element_bytes):
    v, found = boundaries(element_bytes)
    widths = {1, W - 1, W, W + 1, W * v - 1, W * v, W * v + 1, 2 * W * v + 3}
    for n in found:
        widths |= {n, n + 1}
    for n in sorted(widths):
        shape = capi.topk_to_csr_launch_shape(1, n, element_bytes, True)
        assert shape == capi.topk_to_csr_launch_shape(1, n, element_bytes, False)
        r = shape["rows_per_workgroup"]
        for m in sorted({1, r - 1, r, r + 1}):
            yield m, n


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_every_instance_at_its_edges(dtype):
    generator = torch.Generator().manual_seed(2024)
    element_bytes = torch.empty(0, dtype=dtype).element_size()
    assert capi.topk_to_csr_launch_shape(8, 8, element_bytes, True)["digit_passes"] == element_bytes
    for m, n in shapes(element_bytes):
        host = random_scores(m, n, dtype, generator)
        for k in sorted({min(n, 1), (n + 2) // 3, n - 1}):
            check(host, per_row=k)
        for K in sorted({min(m * n, 1), (m * n + 2) // 3, m * n - 1}):
            check(host, total=K)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_scan_block_edges_and_the_row_limit(dtype):
    generator = torch.Generator().manual_seed(5)
    for m in (1023, 1024, 1025):
        host = random_scores(m, 3, dtype, generator)
        for K in (1, m, 2 * m + 1):
            check(host, total=K)
        check(host, per_row=2)
    limit = 16384
    assert capi.topk_to_csr_launch_shape(limit, 2, 4, True)["served"]
    assert not capi.topk_to_csr_launch_shape(limit + 1, 2, 4, True)["served"]
    host = random_scores(limit + 1, 2, dtype, generator)
    check(host, per_row=1)                              # equal lengths: no sort, no row limit
    with pytest.raises(RuntimeError):
        ops.topk_to_csr(host.cuda(), total=limit)
    got = topology.magnitude_prune(host.cuda(), nonzeros=limit)    # ... answered by the torch path
    want = topology.magnitude_prune(host, nonzeros=limit)
    assert all(g.is_cuda and torch.equal(bits_of(g).cpu() if g.is_floating_point() else g.cpu(),
                                         bits_of(w) if w.is_floating_point() else w)
               for g, w in zip(got, want))
    if dtype == torch.float32:
        host = random_scores(limit, 2, dtype, generator)
        check(host, total=limit + 7)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_count_edges(dtype):
    generator = torch.Generator().manual_seed(6)
    for m, n in ((1, 1), (3, 5), (9, 70), (6, 300), (2, 1100)):
        host = random_scores(m, n, dtype, generator)
        for k in sorted({0, 1, n - 1, n}):
            got = check(host, per_row=k)
            assert got[2].numel() == m * k
        for K in sorted({0, 1, m * n - 1, m * n}):
            got = check(host, total=K)
            assert got[2].numel() == K and int(got[1][-1]) == K
    for m, n in ((0, 5), (4, 0), (0, 0)):
        host = torch.zeros(m, n, dtype=dtype)
        check(host, per_row=0)
        check(host, total=0)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_constant_matrix(dtype):
    """Every element ties: the first k columns, the first K flat positions."""
    for m, n in ((5, 9), (7, 130), (3, 1030)):
        host = torch.full((m, n), -2.5, dtype=dtype)
        for k in (1, n // 2, n - 1):
            got = check(host, per_row=k)
            assert torch.equal(got[2].cpu().reshape(m, k), torch.arange(k, dtype=torch.int32).expand(m, k))
        for K in (1, n - 1, n, n + 1, 2 * n + n // 2, m * n - 1):
            got = check(host, total=K)
            lengths = (got[1][1:] - got[1][:-1]).cpu().tolist()
            assert lengths == [max(0, min(n, K - r * n)) for r in range(m)]


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_tie_groups_across_the_steps_of_the_walk(dtype):
    element_bytes = torch.empty(0, dtype=dtype).element_size()
    n = 1100
    shape = capi.topk_to_csr_launch_shape(4, n, element_bytes, False)
    step = (W // shape["rows_per_wave"]) * shape["elements_per_lane"]     # columns of one step
    assert 2 * step < n
    for columns in ((62, 63, 64, 65), (step - 2, step - 1, step, step + 1), (5, step - 1, 2 * step - 1, n - 1),
                    (step - 1, step, 2 * step - 1, 2 * step)):
        host = torch.full((4, n), 0.25, dtype=dtype)
        host[:, 7] = 3.0                                   # one element above the group
        host[1] = host[1].flip(0).neg()                    # (signs do not matter)
        host[:, list(columns)] = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=dtype)    # the tie group
        ties = len(columns)
        for quota in (1, ties - 1, ties):
            got = check(host, per_row=1 + quota)
            assert got[2].cpu().reshape(4, -1)[0].tolist() == sorted([7] + list(columns[:quota]))
        # views of the same rows: off the 16-byte alignment the steps fall elsewhere
        base = torch.zeros(4, n + 5, dtype=dtype)
        base[:, 3:3 + n] = host
        device = base.cuda()[:, 3:3 + n]
        assert device.stride(0) == n + 5 and not device.is_contiguous()
        check(host, per_row=3, device=device, note="sliced view")
        check(host, total=4 + 2 * ties + 1, device=device, note="sliced view")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_total_quota_over_several_rows(dtype):
    """The tie group spread over rows; the quota ends at a row's first tie, mid-row, at its
    last tie and exactly at a row end.  Rows wholly below the threshold come out empty."""
    m, n = 7, 300
    host = torch.full((m, n), 0.125, dtype=dtype)
    host[0, 10], host[3, 299], host[6, 0] = 9.0, -9.0, 8.0                 # above the ties
    tie_columns = {1: (0, 150, 299), 2: (), 3: (4, 270), 4: (63, 64, 255, 256), 5: (), 6: (299,)}
    for r, columns in tie_columns.items():
        host[r, list(columns)] = torch.tensor([2.0, -2.0] * 2, dtype=dtype)[: len(columns)]
    ties = sum(len(c) for c in tie_columns.values())
    for quota in range(ties + 1):
        got = check(host, total=3 + quota)
        lengths = (got[1][1:] - got[1][:-1]).cpu().tolist()
        assert lengths[2] == 0 and lengths[5] == 0 and sum(lengths) == 3 + quota
    got = check(host, total=3 + ties + 5)                  # beyond the ties: the next group begins
    assert int(got[1][1]) == 1 + 5


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_digits(dtype):
    """Keys that differ only in the lowest byte, only in the highest byte and across a byte
    boundary (0x..00ff / 0x..0100), with the special values among them."""
    element_bytes = torch.empty(0, dtype=dtype).element_size()
    top = 8 * (element_bytes - 1)
    generator = torch.Generator().manual_seed(8)
    low = [0x3c00 << (top - 8) | b for b in range(256)]                               # lowest byte only
    high = [(b << top) | 0x21 for b in range(1, 0x78)]                                 # highest byte only
    carry = [0x00ff, 0x0100, 0x01ff, 0x0200, 0x00fe, 0x0101]
    if element_bytes == 4:
        carry += [0x00ffff, 0x010000, 0x00ff00, 0x3f00ffff, 0x3f010000, 0x3effffff, 0x3f000000]
    else:
        carry += [0x3cff, 0x3d00, 0x3bff, 0x3c00]
    for patterns in (low, high, carry, low + high + carry):
        base = from_bits(patterns, dtype)
        signs = torch.where(torch.rand(base.numel(), generator=generator) < 0.5, -1.0, 1.0).to(dtype)
        row = torch.cat([base * signs, specials(dtype), base[: 5]])
        n = row.numel()
        host = torch.stack([row[torch.randperm(n, generator=generator)] for _ in range(6)])
        assert torch.equal(topology.magnitude_keys(host).sort(1).values[0],
                           topology.magnitude_keys(row).sort().values)            # (bits survived)
        for k in (1, 2, n // 2, n - 3):
            check(host, per_row=k)
        for K in (1, 7, 3 * n + 1, 6 * n - 2):
            check(host, total=K)


def test_views_and_values_from():
    generator = torch.Generator().manual_seed(9)
    big = random_scores(40, 331, torch.float16, generator)
    device = big.cuda()
    rows = device[::2]                                                     # row-strided
    assert rows.stride(0) == 2 * 331 and not rows.is_contiguous()
    check(big[::2], per_row=17, device=rows)
    check(big[::2], total=999, device=rows)
    sliced = device[1:, 3:300]                                             # odd n, rows off 16 bytes
    assert sliced.size(1) % 2 == 1 and sliced.stride(1) == 1 and (sliced.data_ptr() % 16) != 0
    check(big[1:, 3:300], per_row=40, device=sliced)
    check(big[1:, 3:300], total=2000, device=sliced)
    columns = device[:, ::2]                                               # last stride 2: copied
    check(big[:, ::2], total=500, device=columns)
    expanded = device[:1].expand(5, 331)                                   # row stride 0
    check(big[:1].expand(5, 331), total=333, device=expanded)

    scores = random_scores(33, 129, torch.float32, generator)
    payload16 = torch.randn(33, 129, generator=generator).to(torch.bfloat16)
    payload16[0, :3] = torch.tensor([float("nan"), -0.0, float("inf")], dtype=torch.bfloat16)
    payload32 = torch.randint(-2 ** 31, 2 ** 31 - 1, (33, 129), generator=generator, dtype=torch.int64).to(torch.int32)
    for payload in (payload16, payload32, payload16.to(torch.float16).view(torch.int16)):
        check(scores, per_row=129, values_from=payload)
        check(scores, per_row=30, values_from=payload)
        check(scores, total=1500, values_from=payload)
    half = scores.to(torch.float16)
    check(half, total=1500, values_from=payload32)
    wide = torch.zeros(33, 200, dtype=torch.int32)
    wide[:, 7:136] = payload32
    check(scores, total=777, values_from=payload32, device_values=wide.cuda()[:, 7:136])
    with pytest.raises(ValueError):
        ops.topk_to_csr(scores.cuda(), total=5, values_from=payload32.cuda()[:, :100])
    with pytest.raises(ValueError):
        ops.topk_to_csr(scores.cuda(), total=5, values_from=payload32.cuda().to(torch.int64))
    with pytest.raises(ValueError):
        ops.topk_to_csr(scores.cuda(), total=5, values_from=payload32)     # on another device


def test_magnitude_prune_routes():
    generator = torch.Generator().manual_seed(10)
    host = random_scores(70, 90, torch.float32, generator)
    for kwargs in (dict(density=0.2), dict(density=0.1, per_row=True), dict(nonzeros=1234),
                   dict(nonzeros=9, per_row=True)):
        want = topology.magnitude_prune(host, **kwargs)
        results = [topology.magnitude_prune(host.cuda().requires_grad_(), **kwargs)]
        topology.enable_device_build(False)
        try:
            results.append(topology.magnitude_prune(host.cuda(), **kwargs))
        finally:
            topology.enable_device_build(True)
        results.append(topology.magnitude_prune(host.double().cuda(), **kwargs))       # ranked as .float()
        for got in results:
            assert not got[0].requires_grad
            assert torch.equal(got[0].float().view(torch.int32).cpu(), want[0].view(torch.int32))
            assert all(g.is_cuda and torch.equal(g.cpu(), w) for g, w in zip(got[1:], want[1:]))


def test_reproducible():
    generator = torch.Generator().manual_seed(11)
    device = random_scores(600, 1100, torch.float32, generator).cuda()
    for kwargs in (dict(per_row=110), dict(total=66000)):
        first = ops.topk_to_csr(device, **kwargs)
        second = ops.topk_to_csr(device, **kwargs)
        assert all(torch.equal(bits_of(a), bits_of(b)) for a, b in zip(first, second))
    check(device.cpu(), total=66000)
    check(device.cpu(), per_row=110)


def test_total_mode_is_capturable():
    """Total mode neither synchronises nor reads back, its allocations are torch's own per call
    and every launch is a kernel (the bins are cleared by one, not by a memset): it is captured
    into a graph on a side stream, and each replay on new scores in the captured buffer equals
    the eager call."""
    generator = torch.Generator().manual_seed(2035)
    m, n = 70, 300
    K = m * n // 3
    scores = random_scores(m, n, torch.float32, generator).cuda()
    ops.topk_to_csr(scores, total=K)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.topk_to_csr(scores, total=K)
    for _ in range(2):
        fresh = random_scores(m, n, torch.float32, generator)
        scores.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = check(fresh, total=K, device=scores)        # eager op == the torch path on the CPU tensor
        for c, e in zip(captured, eager):
            assert c.dtype == e.dtype and c.shape == e.shape and torch.equal(bits_of(c), bits_of(e))


# ---- the modules ----

OUT, IN, BATCH, SEQ = 64, 96, 2, 8


def explicit_module(values, row_indices, row_offsets, column_indices):
    """A SparseLinear on a given pattern, explicit zeros included"""
    module = SparseLinear(IN, OUT).to(values.device)
    module.values = torch.nn.Parameter(values.detach().clone())
    module.row_indices, module.row_offsets, module.column_indices = (
        row_indices.clone(), row_offsets.clone(), column_indices.clone())
    functional.register_static_topology(module.row_indices, module.row_offsets, module.column_indices)
    return module


@pytest.mark.parametrize("input_dtype", (torch.float32, torch.float16), **ids)
def test_from_dense_forward(input_dtype):
    generator = torch.Generator().manual_seed(12)
    w = torch.randn(OUT, IN, generator=generator)
    K = round(0.25 * OUT * IN)
    _, ro, ci, _ = topology.topk_to_csr(w, total=K)                       # the CPU rule
    mask = torch.zeros(OUT, IN)
    lengths = (ro[1:] - ro[:-1]).to(torch.int64)
    mask[torch.repeat_interleave(torch.arange(OUT), lengths), ci.to(torch.int64)] = 1.0
    assert int(mask.sum()) == K
    reference = SparseLinear(IN, OUT).cuda()
    with torch.no_grad():
        reference.weight.copy_((w * mask).cuda())
    reference.setup_sparse_tensors()
    module = SparseLinear.from_dense(w.cuda(), density=0.25)
    assert module.values.is_cuda and module.values.dtype == torch.float32 and module.values.numel() == K
    assert isinstance(module.values, torch.nn.Parameter) and module.values.requires_grad
    for name in ("row_indices", "row_offsets", "column_indices"):
        assert torch.equal(getattr(module, name), getattr(reference, name)), name
    assert torch.equal(module.values.detach(), reference.values.detach())
    x = torch.randn(BATCH, SEQ, IN, generator=generator).to(input_dtype).cuda()
    with torch.no_grad():
        got, want = module(x), reference(x)
    assert got.shape == (BATCH, OUT, SEQ) and torch.equal(got, want)
    per_row = SparseLinear.from_dense(w.cuda(), density=0.25, per_row=True)
    assert torch.equal(per_row.row_offsets.cpu(), torch.arange(OUT + 1, dtype=torch.int32) * 24)
    with torch.no_grad():
        assert per_row(x).shape == (BATCH, OUT, SEQ)


def forward_backward(module, x_host):
    x = x_host.cuda().requires_grad_()
    module.values.grad = None
    y = module(x)
    y.backward(torch.ones_like(y) * 0.5)
    return y.detach(), module.values.grad.clone(), x.grad.clone()


@pytest.mark.parametrize("input_dtype", (torch.float32, torch.float16), **ids)
def test_update_topology_serves_no_stale_state(input_dtype):
    generator = torch.Generator().manual_seed(13)
    w = torch.randn(OUT, IN, generator=generator)
    module = SparseLinear.from_dense(w.cuda(), density=0.25)
    parameter, nnz = module.values, module.values.numel()
    x_host = torch.randn(BATCH, SEQ, IN, generator=generator).to(input_dtype)
    forward_backward(module, x_host)           # plans, transposed topology and images of the OLD pattern exist
    with torch.no_grad():
        module(x_host.cuda())
    optimizer = torch.optim.SGD(module.parameters(), lr=0.1)
    old = (module.values.detach().clone(), module.row_offsets.clone(), module.column_indices.clone())

    scores = torch.randn(OUT, IN, generator=generator)
    scores[1, 2], scores[3, 4] = float("nan"), float("inf")
    source = module.update_topology(0.3, scores.cuda())

    # the same step on a CPU module of the same pattern
    twin = SparseLinear(IN, OUT)
    twin.values = torch.nn.Parameter(old[0].cpu())
    twin.row_offsets, twin.column_indices = old[1].cpu(), old[2].cpu()
    twin.row_indices = topology.diffsort(twin.row_offsets)
    twin_source = twin.update_topology(0.3, scores)
    assert torch.equal(source.cpu(), twin_source) and int((source == -1).sum()) == int(0.3 * nnz)
    for name in ("row_indices", "row_offsets", "column_indices"):
        assert torch.equal(getattr(module, name).cpu(), getattr(twin, name)), name
    assert torch.equal(module.values.detach().view(torch.int32).cpu(), twin.values.detach().view(torch.int32))
    assert module.values is parameter and module.values.numel() == nnz
    assert torch.equal(module.values.detach()[source == -1], torch.zeros(int(0.3 * nnz), device="cuda"))

    for round_ in range(2):
        fresh = explicit_module(module.values, module.row_indices, module.row_offsets, module.column_indices)
        got, want = forward_backward(module, x_host), forward_backward(fresh, x_host)
        for g, w_, name in zip(got, want, ("forward", "values.grad", "input.grad")):
            assert torch.equal(g, w_), (name, round_)
        with torch.no_grad():
            assert torch.equal(module(x_host.cuda()), fresh(x_host.cuda()))
        before = module.values.detach().clone()
        optimizer.step()                        # the optimizer still holds THE parameter
        assert module.values is parameter and not torch.equal(module.values.detach(), before)
        assert (module.values.detach()[source == -1] != 0).any()           # grown entries train
