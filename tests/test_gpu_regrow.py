"""GPU: per-row drop-and-grow of a CSR topology (csrc/topology.hip; ops.csr_regrow,
topology.regrow_per_row, SparseLinear.update_topology(per_row=True)) against the torch path on
the CPU copy of the same input.  Everything is an integer or a bit copy: every comparison is
exact.

Instance parameters (rows per wave, elements per lane, rows per workgroup, digit passes, the
widest row) come from the host query the launch itself decides by."""
import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

pytestmark = pytest.mark.gpu

W = 64
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
VALUE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)     # 4- and 2-byte words
BITS = {2: torch.int16, 4: torch.int32}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()])


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def width(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def check(values, row_offsets, column_indices, drop_counts, scores, device_scores=None, note=""):
    """ops.csr_regrow on the device copies (or the given device view of the same scores) against
    the torch path on the CPU tensors.  Returns the device result."""
    want = topology.regrow_per_row(values, row_offsets, column_indices, drop_counts, scores)
    got = ops.csr_regrow(values.cuda(), row_offsets.cuda(), column_indices.cuda(), drop_counts.cuda(),
                         scores.cuda() if device_scores is None else device_scores)
    where = f"{tuple(scores.shape)} {scores.dtype} values {values.dtype} {note}"
    for g, w, name in zip(got, want, ("column_indices", "values", "source")):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (name, where)
        same = torch.equal(bits_of(g).cpu(), bits_of(w)) if name == "values" else torch.equal(g.cpu(), w)
        assert same, (name, where)
    return got


def specials(dtype):
    """NaN, +-inf, +-0, the largest finite value, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.375, -0.375,
                                    torch.finfo(dtype).max], dtype=dtype), from_bits([1], dtype)])


def quantised(shape, dtype, generator, quantum=0.125):
    """few distinct magnitudes (many ties, signs mixed) with the special values among them"""
    x = ((torch.randn(shape, generator=generator) / quantum).round() * quantum).to(dtype)
    flat, s = x.reshape(-1), specials(dtype)
    flat[1::5][: s.numel()] = s[: flat[1::5].numel()]
    return x


def csr(lengths, n, generator):
    """row_offsets and ascending random columns of rows of these lengths"""
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    row_offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    columns = [torch.sort(torch.randperm(n, generator=generator)[: int(k)]).values for k in lengths]
    return row_offsets, torch.cat(columns + [torch.zeros(0, dtype=torch.int64)]).to(torch.int32)


def random_case(m, n, value_dtype, score_dtype, generator):
    lengths = torch.randint(0, n + 1, (m,), generator=generator)
    row_offsets, column_indices = csr(lengths, n, generator)
    values = quantised(column_indices.numel(), value_dtype, generator)
    scores = quantised((m, n), score_dtype, generator)
    drop_counts = (torch.rand(m, generator=generator) * (lengths + 1)).to(torch.int32)
    return values, row_offsets, column_indices, drop_counts, scores


def boundaries(score_bytes):
    """Every n that is the last of a rows-per-wave instance, read from the query."""
    v = capi.csr_regrow_launch_shape(1, 1, score_bytes, 4)["elements_per_lane"]
    found, previous = [], None
    for n in range(1, W * v + 2):
        rows = capi.csr_regrow_launch_shape(1, n, score_bytes, 4)["rows_per_wave"]
        if previous is not None and rows != previous:
            found.append(n - 1)
        previous = rows
    assert len(found) == 3 and previous == 1   # 8 -> 4 -> 2 -> 1 rows per wave
    return v, found


def shapes(score_bytes):
    v, found = boundaries(score_bytes)
    widths = {1, 31, 32, 33, W - 1, W, W + 1, W * v - 1, W * v, W * v + 1, 2 * W * v + 3}
    for n in found:
        widths |= {n, n + 1}
    for n in sorted(widths):
        shape = capi.csr_regrow_launch_shape(1, n, score_bytes, 4)
        assert shape == capi.csr_regrow_launch_shape(1, n, score_bytes, 2) | {"value_digit_passes": 4}
        r = shape["rows_per_workgroup"]
        for m in sorted({1, r - 1, r, r + 1} - {0}):
            yield m, n


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
def test_every_instance_at_its_edges(score_dtype):
    generator = torch.Generator().manual_seed(2025)
    shape = capi.csr_regrow_launch_shape(8, 8, width(score_dtype), 2)
    assert shape["served"] and shape["score_digit_passes"] == width(score_dtype) and shape["value_digit_passes"] == 2
    for i, (m, n) in enumerate(shapes(width(score_dtype))):
        for value_dtype in (VALUE_DTYPES[0], VALUE_DTYPES[1 + i % 2]):
            check(*random_case(m, n, value_dtype, score_dtype, generator))


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
@pytest.mark.parametrize("value_dtype", VALUE_DTYPES[:2], **ids)
def test_ragged_rows(value_dtype, score_dtype):
    """Lengths 0, 1, n and random ones in one matrix, among them a row longer than one step of
    its group over the entries (64 lanes) and rows of several steps; d_r = 0, 1, len_r and
    random: the running counts of old bits and of ties cross the steps."""
    generator = torch.Generator().manual_seed(31)
    m, n = 70, 1100
    lengths = torch.randint(0, 60, (m,), generator=generator)
    lengths[0], lengths[1], lengths[2], lengths[3], lengths[4], lengths[69] = 0, 1, n, 65, 700, n
    row_offsets, column_indices = csr(lengths, n, generator)
    values = quantised(column_indices.numel(), value_dtype, generator)
    scores = quantised((m, n), score_dtype, generator)
    random_counts = (torch.rand(m, generator=generator) * (lengths + 1)).to(torch.int32)
    for note, drop_counts in (("none", torch.zeros(m, dtype=torch.int32)), ("one", torch.ones(m, dtype=torch.int32)),
                              ("all", lengths.to(torch.int32)), ("random", random_counts)):
        got = check(values, row_offsets, column_indices, drop_counts, scores, note=note)
        if note == "none":
            assert torch.equal(got[0].cpu(), column_indices) and torch.equal(got[2].cpu(), torch.arange(values.numel()))
        if note == "all":
            assert bool((got[2] == -1).all()) and not bits_of(got[1]).any()


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_ties(dtype):
    """Constant scores: the growth takes the lowest free columns.  Constant values: the drop
    takes the highest columns.  Both over rows of several steps."""
    generator = torch.Generator().manual_seed(32)
    for m, n, length in ((5, 9, 4), (7, 130, 70), (3, 1100, 600)):
        row_offsets, column_indices = csr([length] * m, n, generator)
        values = quantised(m * length, dtype, generator)
        drop = length // 2
        drop_counts = torch.full((m,), drop, dtype=torch.int32)
        got = check(values, row_offsets, column_indices, drop_counts, torch.full((m, n), -2.5, dtype=dtype),
                    note="constant scores")
        for r in range(m):
            new = got[0][r * length:(r + 1) * length].cpu()
            kept = new[got[2][r * length:(r + 1) * length].cpu() >= 0].tolist()
            free = [c for c in range(n) if c not in set(kept)]
            assert sorted(kept + free[:drop]) == new.tolist()
        constant = torch.full((m * length,), 0.75, dtype=dtype)
        constant[1::2] = -0.75
        got = check(constant, row_offsets, column_indices, drop_counts, quantised((m, n), dtype, generator),
                    note="constant values")
        source = got[2].cpu().reshape(m, length)
        kept = torch.arange(m)[:, None] * length + torch.arange(length - drop)[None, :]
        assert torch.equal(torch.sort(source, dim=1, descending=True).values[:, :length - drop].flip(1), kept)


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
def test_tie_groups_across_the_steps_of_the_walk(score_dtype):
    n = 1100
    shape = capi.csr_regrow_launch_shape(4, n, width(score_dtype), 4)
    step = (W // shape["rows_per_wave"]) * shape["elements_per_lane"]     # columns of one step
    assert 2 * step < n
    generator = torch.Generator().manual_seed(33)
    for columns in ((62, 63, 64, 65), (step - 2, step - 1, step, step + 1), (5, step - 1, 2 * step - 1, n - 1),
                    (step - 1, step, 2 * step - 1, 2 * step)):
        scores = torch.full((4, n), 0.25, dtype=score_dtype)
        scores[:, 7] = 3.0                                   # one column above the group
        scores[1] = scores[1].neg()                          # (signs do not matter)
        scores[:, list(columns)] = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=score_dtype)    # the tie group
        row_offsets = torch.arange(5, dtype=torch.int32) * 6
        column_indices = torch.tensor([0, 1, 2, 3, 4, n - 2] * 4, dtype=torch.int32)
        values = torch.arange(24, 0, -1).to(torch.float32)
        for quota in (1, 3, 4):
            got = check(values, row_offsets, column_indices, torch.full((4,), 1 + quota, dtype=torch.int32), scores)
            kept = [0, 1, 2, 3, 4, n - 2][: 6 - 1 - quota]
            assert got[0][:6].cpu().tolist() == sorted(kept + [7] + list(columns[:quota]))
        # a view of the same rows: off the 16-byte alignment the steps fall elsewhere
        base = torch.zeros(4, n + 5, dtype=score_dtype)
        base[:, 3:3 + n] = scores
        device = base.cuda()[:, 3:3 + n]
        assert device.stride(0) == n + 5 and not device.is_contiguous()
        check(values, row_offsets, column_indices, torch.full((4,), 3, dtype=torch.int32), scores, device_scores=device,
              note="sliced view")
    # the value ties of a row of several steps over its entries: q_v ends inside a later step
    length = 300
    row_offsets, column_indices = csr([length] * 2, n, generator)
    values = torch.full((2 * length,), 0.5)
    values[:length:7] = 4.0
    for keep in (1, 43, 44, 150, 299):
        check(values, row_offsets, column_indices, torch.full((2,), length - keep, dtype=torch.int32),
              quantised((2, n), score_dtype, generator), note=f"value ties, keep {keep}")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_digits(dtype):
    """Keys that differ only in the lowest byte, only in the highest byte and across a byte
    boundary, as values and as scores, with the special values among them."""
    element_bytes = width(dtype)
    top = 8 * (element_bytes - 1)
    generator = torch.Generator().manual_seed(34)
    low = [0x3c00 << (top - 8) | b for b in range(256)]                               # lowest byte only
    high = [(b << top) | 0x21 for b in range(1, 0x78)]                                 # highest byte only
    carry = [0x00ff, 0x0100, 0x01ff, 0x0200, 0x00fe, 0x0101]
    if element_bytes == 4:
        carry += [0x00ffff, 0x010000, 0x00ff00, 0x3f00ffff, 0x3f010000, 0x3effffff, 0x3f000000]
    else:
        carry += [0x3cff, 0x3d00, 0x3bff, 0x3c00]
    other = torch.float16 if dtype == torch.float32 else torch.float32
    for patterns in (low, high, carry, low + high + carry):
        base = from_bits(patterns, dtype)
        signs = torch.where(torch.rand(base.numel(), generator=generator) < 0.5, -1.0, 1.0).to(dtype)
        row = torch.cat([base * signs, specials(dtype), base[: 5]])
        n, m = row.numel(), 6
        dense = torch.stack([row[torch.randperm(n, generator=generator)] for _ in range(m)])
        assert torch.equal(topology.magnitude_keys(dense).sort(1).values[0], topology.magnitude_keys(row).sort().values)
        # as scores, over a sparse pattern of plain values
        lengths = torch.randint(0, n + 1, (m,), generator=generator)
        row_offsets, column_indices = csr(lengths, n, generator)
        plain = quantised(column_indices.numel(), other, generator)
        for fraction in (0.1, 0.5, 1.0):
            check(plain, row_offsets, column_indices, (lengths * fraction).to(torch.int32), dense, note="scores")
        # as values: every row full, so the old values are the dense rows themselves
        full_offsets = torch.arange(m + 1, dtype=torch.int32) * n
        full_columns = torch.arange(n, dtype=torch.int32).repeat(m)
        for drop in (1, 2, n // 2, n - 3):
            check(dense.reshape(-1), full_offsets, full_columns, torch.full((m,), drop, dtype=torch.int32),
                  quantised((m, n), other, generator), note="values")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_clamp(dtype):
    """NaN and inf scores count as the largest finite value: against finfo.max they tie by column."""
    n = 200
    scores = torch.full((3, n), 1.0, dtype=dtype)
    scores[:, 150], scores[:, 20], scores[:, 90], scores[:, 199] = (float("nan"), torch.finfo(dtype).max,
                                                                    float("inf"), -float("inf"))
    scores[2, 5] = -torch.finfo(dtype).max
    row_offsets = torch.tensor([0, 3, 6, 9], dtype=torch.int32)
    column_indices = torch.tensor([0, 1, 2, 0, 2, 90, 0, 1, 2], dtype=torch.int32)
    values = torch.tensor([3.0, 2.0, 1.0, 1.0, 2.0, 3.0, 3.0, 2.0, 1.0], dtype=torch.float32)   # row 1 keeps column 90 longest
    for drop, grown in ((1, [[20], [20], [5]]), (2, [[20, 90], [20, 150], [5, 20]]),
                        (3, [[20, 90, 150]] * 2 + [[5, 20, 90]])):
        got = check(values, row_offsets, column_indices, torch.full((3,), drop, dtype=torch.int32), scores)
        for r in range(3):
            row = slice(3 * r, 3 * r + 3)
            assert got[0][row][got[2][row] == -1].cpu().tolist() == grown[r]


def test_views_and_clamped_counts():
    generator = torch.Generator().manual_seed(35)
    big = quantised((40, 331), torch.float16, generator)
    device = big.cuda()

    def case(m, n, value_dtype):
        lengths = torch.randint(0, n + 1, (m,), generator=generator)
        row_offsets, column_indices = csr(lengths, n, generator)
        values = quantised(column_indices.numel(), value_dtype, generator)
        # counts outside 0 .. len_r are clamped
        drop_counts = torch.randint(-5, n + 6, (m,), generator=generator).to(torch.int32)
        return values, row_offsets, column_indices, drop_counts

    rows = device[::2]                                                     # row-strided
    assert rows.stride(0) == 2 * 331 and not rows.is_contiguous()
    check(*case(20, 331, torch.float32), big[::2], device_scores=rows)
    sliced = device[1:, 3:300]                                             # odd n, rows off 16 bytes
    assert sliced.size(1) % 2 == 1 and sliced.stride(1) == 1 and (sliced.data_ptr() % 16) != 0
    check(*case(39, 297, torch.bfloat16), big[1:, 3:300], device_scores=sliced)
    columns = device[:, ::2]                                               # last stride 2: copied
    check(*case(40, 166, torch.float32), big[:, ::2], device_scores=columns)
    expanded = device[:1].expand(5, 331)                                   # row stride 0
    check(*case(5, 331, torch.float16), big[:1].expand(5, 331), device_scores=expanded)
    wide = quantised((9, 77), torch.float32, generator)
    wide_device = wide.cuda()[:, 1:]                                       # float32 rows off 16 bytes
    assert (wide_device.data_ptr() % 16) != 0
    check(*case(9, 76, torch.float16), wide[:, 1:], device_scores=wide_device)
    for m, n in ((0, 5), (4, 0), (0, 0)):
        empty = (torch.zeros(0), torch.zeros(m + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
                 torch.zeros(m, dtype=torch.int32), torch.zeros(m, n))
        assert all(t.numel() == 0 for t in check(*empty))
    values, row_offsets, column_indices, drop_counts = case(4, 331, torch.float32)
    with pytest.raises(RuntimeError):
        ops.csr_regrow(values, row_offsets, column_indices, drop_counts, big[:4])            # CPU tensors
    with pytest.raises(ValueError):
        ops.csr_regrow(values.cuda(), row_offsets.cuda(), column_indices.cuda(), drop_counts.cuda(), big[:4])
    with pytest.raises(ValueError):
        ops.csr_regrow(values.cuda().double(), row_offsets.cuda(), column_indices.cuda(), drop_counts.cuda(),
                       device[:4])


def test_the_widest_row_and_beyond():
    generator = torch.Generator().manual_seed(36)
    limit = capi.csr_regrow_launch_shape(2, 1, 2, 4)["max_n"]
    assert limit >= 16384 and capi.csr_regrow_launch_shape(2, limit, 2, 4)["served"]
    assert not capi.csr_regrow_launch_shape(2, limit + 1, 2, 4)["served"]
    for n in (limit, limit + 1):
        lengths = torch.tensor([n // 3, 1000])
        row_offsets, column_indices = csr(lengths, n, generator)
        column_indices[-1] = n - 1                                         # the last bit of the bitmap
        values = quantised(column_indices.numel(), torch.float32, generator)
        scores = quantised((2, n), torch.float16, generator)
        scores[1, n - 2] = 100.0
        drop_counts = torch.tensor([n // 5, 400], dtype=torch.int32)
        want = topology.regrow_per_row(values, row_offsets, column_indices, drop_counts, scores)
        on_device = [t.cuda() for t in (values, row_offsets, column_indices, drop_counts, scores)]
        if n > limit:
            with pytest.raises(RuntimeError):
                ops.csr_regrow(*on_device)
        got = topology.regrow_per_row(*on_device)          # beyond the limit: answered by the torch path
        assert all(g.is_cuda for g in got)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[2].cpu(), want[2])
        assert torch.equal(bits_of(got[1]).cpu(), bits_of(want[1]))
        if n == limit:
            check(values, row_offsets, column_indices, drop_counts, scores)


def test_routes_agree():
    generator = torch.Generator().manual_seed(37)
    case = random_case(33, 90, torch.float32, torch.float32, generator)
    want = topology.regrow_per_row(*case)
    results = [topology.regrow_per_row(*(t.cuda() for t in case))]
    topology.enable_device_build(False)
    try:
        results.append(topology.regrow_per_row(*(t.cuda() for t in case)))
    finally:
        topology.enable_device_build(True)
    results.append(topology.regrow_per_row(*(t.cuda() for t in case[:4]), case[4].double().cuda()))   # ranked as .float()
    for got in results:
        assert all(g.is_cuda for g in got)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[2].cpu(), want[2])
        assert torch.equal(bits_of(got[1]).cpu(), bits_of(want[1]))


def test_reproducible_and_capturable():
    """Two calls give equal tensors.  The call neither synchronises nor reads back and its
    allocations are torch's own per call: it is captured into a graph, and the replay on new
    inputs in the captured buffers equals the eager call."""
    generator = torch.Generator().manual_seed(38)
    case = [t.cuda() for t in random_case(70, 1100, torch.float32, torch.float32, generator)]
    first, second = ops.csr_regrow(*case), ops.csr_regrow(*case)
    assert all(torch.equal(bits_of(a) if a.is_floating_point() else a, bits_of(b) if b.is_floating_point() else b)
               for a, b in zip(first, second))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.csr_regrow(*case)
    fresh = random_case(70, 1100, torch.float32, torch.float32, generator)
    fresh_offsets, fresh_columns = csr((case[1][1:] - case[1][:-1]).cpu(), 1100, generator)    # nnz is captured
    fresh = (quantised(fresh_columns.numel(), torch.float32, generator), fresh_offsets, fresh_columns, fresh[3],
             fresh[4])
    for static, new in zip(case, fresh):
        static.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.csr_regrow(*case)
    assert all(torch.equal(bits_of(a) if a.is_floating_point() else a, bits_of(b) if b.is_floating_point() else b)
               for a, b in zip(captured, eager))
    check(*fresh)


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


@pytest.mark.parametrize("input_dtype", (torch.float32, torch.float16), **ids)
def test_update_topology_per_row_serves_no_stale_state(input_dtype):
    generator = torch.Generator().manual_seed(39)
    w = torch.randn(OUT, IN, generator=generator)
    module = SparseLinear.from_dense(w.cuda(), density=0.25, per_row=True)
    k = 24
    balanced = torch.arange(OUT + 1, dtype=torch.int32) * k
    assert torch.equal(module.row_offsets.cpu(), balanced)
    parameter, nnz = module.values, module.values.numel()
    x_host = torch.randn(BATCH, SEQ, IN, generator=generator).to(input_dtype)
    forward_backward(module, x_host)           # plans, transposed topology and images of the OLD pattern exist
    with torch.no_grad():
        module(x_host.cuda())
    optimizer = torch.optim.SGD(module.parameters(), lr=0.1)
    d = int(k * 0.3)

    for step in range(2):
        old = (module.values.detach().clone(), module.row_indices, module.row_offsets, module.column_indices)
        scores = torch.randn(OUT, IN, generator=generator)
        scores[1, 2], scores[3, 4] = float("nan"), float("inf")
        source = module.update_topology(0.3, scores.cuda(), per_row=True)

        # the same step on a CPU module of the same pattern
        twin = SparseLinear(IN, OUT)
        twin.values = torch.nn.Parameter(old[0].cpu())
        twin.row_indices, twin.row_offsets, twin.column_indices = (t.cpu() for t in old[1:])
        twin_source = twin.update_topology(0.3, scores, per_row=True)
        assert torch.equal(source.cpu(), twin_source)
        assert torch.equal((source == -1).reshape(OUT, k).sum(1).cpu(), torch.full((OUT,), d))
        for name in ("row_indices", "row_offsets", "column_indices"):
            assert torch.equal(getattr(module, name).cpu(), getattr(twin, name)), name
        assert torch.equal(module.row_offsets.cpu(), balanced)                 # the rows keep their lengths
        assert all(getattr(module, name) is not t for name, t in
                   zip(("row_indices", "row_offsets", "column_indices"), old[1:]))
        assert torch.equal(module.values.detach().view(torch.int32).cpu(), twin.values.detach().view(torch.int32))
        assert module.values is parameter and module.values.numel() == nnz
        assert not module.values.detach()[source == -1].view(torch.int32).any()
        assert torch.equal(module.values.detach()[source >= 0], old[0][source[source >= 0]])

        fresh = explicit_module(module.values, module.row_indices, module.row_offsets, module.column_indices)
        got, want = forward_backward(module, x_host), forward_backward(fresh, x_host)
        for g, w_, name in zip(got, want, ("forward", "values.grad", "input.grad")):
            assert torch.equal(g, w_), (name, step)
        with torch.no_grad():
            assert torch.equal(module(x_host.cuda()), fresh(x_host.cuda()))
        before = module.values.detach().clone()
        optimizer.step()                        # the optimizer still holds THE parameter
        assert module.values is parameter and not torch.equal(module.values.detach(), before)
        assert (module.values.detach()[source == -1] != 0).any()           # grown entries train
