"""GPU: the matrix-wide drop-and-grow step of a CSR topology on the device (csrc/topology.hip;
ops.csr_regrow_total, topology.regrow_total, SparseLinear.update_topology / rigl_update with
per_row=False) against the torch path on the CPU copy of the same input AND against a
brute-force statement of the rule (tests/regrow_total_cases.py).  Everything is an integer or a
bit copy: every comparison is exact.

Instance parameters (rows per wave, elements per lane, rows per workgroup, the limits) come from
the host query the launches themselves decide by."""
import pytest
import torch

from tests import regrow_total_cases as C
from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

pytestmark = pytest.mark.gpu

W = 64
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
VALUE_DTYPES = {4: torch.float32, 2: torch.bfloat16}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def check(values, row_offsets, column_indices, d, scores, device_scores=None, note=""):
    """ops.csr_regrow_total on the device copies (or the given device view of the same scores)
    against the torch path and the brute force on the CPU tensors.  Returns the device result."""
    where = f"{tuple(scores.shape)} {scores.dtype} values {values.dtype} d {d} {note}"
    want = C.brute_force(values, row_offsets, column_indices, d, scores)
    C.assert_same(C.torch_path(values, row_offsets, column_indices, d, scores), want, "torch path " + where)
    got = ops.csr_regrow_total(values.cuda(), row_offsets.cuda(), column_indices.cuda(), d,
                               scores.cuda() if device_scores is None else device_scores)
    assert all(g.is_cuda for g in got)
    C.assert_same(got, want, where)
    return got


def counts(nnz, generator):
    """d = 0, 1, random, nnz - 1, nnz"""
    return sorted({0, min(1, nnz), int(torch.randint(0, nnz + 1, (1,), generator=generator)), max(nnz - 1, 0), nnz})


def boundaries(score_bytes):
    """Every n that is the last of a rows-per-wave instance, read from the query."""
    v = capi.csr_regrow_total_launch_shape(1, 1, 1, score_bytes, 4)["elements_per_lane"]
    found, previous = [], None
    for n in range(1, W * v + 2):
        rows = capi.csr_regrow_total_launch_shape(1, n, 1, score_bytes, 4)["rows_per_wave"]
        if previous is not None and rows != previous:
            found.append(n - 1)
        previous = rows
    assert found == [4 * v, 8 * v, 16 * v, 32 * v] and previous == 1     # 16 -> 8 -> 4 -> 2 -> 1 rows per wave
    return v, found


@pytest.mark.parametrize("value_bytes", (4, 2))
@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
def test_every_instance_at_its_edges(score_dtype, value_bytes):
    generator = torch.Generator().manual_seed(2026)
    value_dtype = VALUE_DTYPES[value_bytes] if score_dtype != torch.bfloat16 or value_bytes == 4 else torch.float16
    v, found = boundaries(C.width(score_dtype))
    widths = {1, 2 * W * v + 3}
    for n in found:
        widths |= {n - 1, n, n + 1}
    for n in sorted(widths):
        shape = capi.csr_regrow_total_launch_shape(1, n, 1, C.width(score_dtype), value_bytes)
        assert shape["served"] and shape["value_digit_passes"] == value_bytes
        assert shape["score_digit_passes"] == C.width(score_dtype)
        r = shape["rows_per_workgroup"]
        for m in sorted({1, r - 1, r, r + 1} - {0}):
            case = C.random_case(m, n, value_dtype, score_dtype, generator)
            nnz = case[0].numel()
            check(*case[:3], int(torch.randint(0, nnz + 1, (1,), generator=generator)), case[3])


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
def test_ragged_extremes(score_dtype):
    """Empty rows, full rows, a row that loses every entry while another gains; then Kept
    confined to the last rows and Grown to the first: the lengths move a long way."""
    generator = torch.Generator().manual_seed(41)
    m, n = 70, 300
    lengths = torch.randint(0, 60, (m,), generator=generator)
    lengths[0], lengths[1], lengths[2], lengths[3], lengths[4], lengths[69] = 0, 1, n, 65, 290, n
    row_offsets, column_indices = C.csr(lengths, n, generator)
    values = C.quantised(column_indices.numel(), torch.float32, generator, special=False)
    scores = C.quantised((m, n), score_dtype, generator)
    values[row_offsets[4]:row_offsets[5]] = 1e-3            # row 4 loses every entry ...
    scores[4] = 0.0
    scores[0] = 50.0                                        # ... while the empty row 0 fills up
    nnz = values.numel()
    for d in counts(nnz, generator) + [290 + n]:
        got = check(values, row_offsets, column_indices, d, scores)
        if d == 290 + n:
            new_lengths = (got[1][1:] - got[1][:-1]).cpu()
            assert int(new_lengths[0]) == n and int(new_lengths[4]) == 0
    # Kept in the last rows, Grown in the first
    half = m // 2
    lengths = torch.cat([torch.randint(20, 60, (half,), generator=generator), torch.full((m - half,), 40)])
    row_offsets, column_indices = C.csr(lengths, n, generator)
    values = torch.rand(column_indices.numel(), generator=generator) + 0.5
    values[: int(row_offsets[half])] *= 1e-3
    scores = (torch.rand(m, n, generator=generator) + 0.5).to(score_dtype)
    scores[half:] *= 1e-3
    d = int(row_offsets[half])
    got = check(values, row_offsets, column_indices, d, scores)
    new_lengths = (got[1][1:] - got[1][:-1]).cpu()
    assert torch.equal(new_lengths[half:], lengths[half:].to(torch.int32)) and int(new_lengths[:half].sum()) == d
    assert bool((got[4][:d] == -1).all()) and bool((got[4][d:] >= 0).all())


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_ties(dtype):
    """Quantised values: equal keys straddle T_v inside a row, across rows and across workgroups,
    and the quota is handed down the rows.  Constant scores: Grown is the first d open positions
    in row-major order, the quota ending mid-row and mid-piece."""
    generator = torch.Generator().manual_seed(42)
    for m, n, length in ((5, 9, 4), (7, 130, 70), (70, 300, 100)):
        shape = capi.csr_regrow_total_launch_shape(m, n, m * length, C.width(dtype), C.width(dtype))
        assert shape["grid"] > 1 or m < 70                 # the last shape spans several workgroups
        row_offsets, column_indices = C.csr([length] * m, n, generator)
        nnz = m * length
        values = C.quantised(nnz, dtype, generator, quantum=0.5)
        v = shape["elements_per_lane"]
        # the quota of open positions ends in the middle of a row and of a lane's piece
        for d in sorted({1, (n - length) + v // 2 + 1, 2 * (n - length) + (n - length) // 2 + 1, nnz // 2} & set(range(nnz + 1))):
            got = check(values, row_offsets, column_indices, d, torch.full((m, n), -2.5, dtype=dtype),
                        note="constant scores")
            lengths = (got[1][1:] - got[1][:-1]).to(torch.int64).cpu()
            flat = torch.repeat_interleave(torch.arange(m), lengths) * n + got[2].cpu()
            source = got[4].cpu()
            kept = set(flat[source >= 0].tolist())
            free = [p for p in range(m * n) if p not in kept]
            assert flat[source == -1].tolist() == free[:d]
        constant = torch.full((nnz,), 0.75, dtype=dtype)
        constant[1::2] = -0.75
        for d in (1, length // 2, length + 3, nnz - length - 1):
            got = check(constant, row_offsets, column_indices, d, C.quantised((m, n), dtype, generator),
                        note="constant values")
            source = got[4].cpu()
            assert torch.sort(source[source >= 0]).values.tolist() == list(range(nnz - d))


@pytest.mark.parametrize("score_dtype", DTYPES, **ids)
def test_tie_groups_across_the_steps_of_the_walk(score_dtype):
    n = 1100
    shape = capi.csr_regrow_total_launch_shape(4, n, 24, C.width(score_dtype), 4)
    step = (W // shape["rows_per_wave"]) * shape["elements_per_lane"]     # columns of one step
    assert 2 * step < n
    generator = torch.Generator().manual_seed(43)
    row_offsets = torch.arange(5, dtype=torch.int32) * 6
    column_indices = torch.tensor([0, 1, 2, 3, 4, n - 2] * 4, dtype=torch.int32)
    values = torch.arange(24, 0, -1).to(torch.float32)
    for columns in ((62, 63, 64, 65), (step - 2, step - 1, step, step + 1), (5, step - 1, 2 * step - 1, n - 1),
                    (step - 1, step, 2 * step - 1, 2 * step)):
        scores = torch.full((4, n), 0.25, dtype=score_dtype)
        scores[:, 7] = 3.0                                   # one column above the group
        scores[1] = scores[1].neg()                          # (signs do not matter)
        scores[:, list(columns)] = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=score_dtype)    # the tie group
        for d in (5, 6, 7, 4 + 4 + 3, 4 + 16 + 2):
            check(values, row_offsets, column_indices, d, scores)
        # a view of the same rows: off the 16-byte alignment the steps fall elsewhere
        base = torch.zeros(4, n + 5, dtype=score_dtype)
        base[:, 3:3 + n] = scores
        device = base.cuda()[:, 3:3 + n]
        assert device.stride(0) == n + 5 and not device.is_contiguous()
        check(values, row_offsets, column_indices, 4 + 6, scores, device_scores=device, note="sliced view")
    # the value ties of rows of several steps over their entries: the quota ends inside a later step
    length = 300
    row_offsets, column_indices = C.csr([length] * 2, n, generator)
    values = torch.full((2 * length,), 0.5)
    values[:length:7] = 4.0
    for keep in (1, 43, 44, 150, 299, 300, 301, 599):
        check(values, row_offsets, column_indices, 2 * length - keep, C.quantised((2, n), score_dtype, generator),
              note=f"value ties, keep {keep}")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_digits(dtype):
    """Keys that differ only in the lowest byte, only in the highest byte, only in a middle byte
    and across a byte boundary, as values and as scores, with the special values among them."""
    element_bytes = C.width(dtype)
    top = 8 * (element_bytes - 1)
    generator = torch.Generator().manual_seed(44)
    families = [[0x3c00 << (top - 8) | b for b in range(256)],                           # lowest byte only
                [(b << top) | 0x21 for b in range(1, 0x78)]]                             # highest byte only
    if element_bytes == 4:
        families += [[0x3f000021 | (b << 8) for b in range(256)], [0x3f002100 | (b << 16) for b in range(128)]]
    carry = [0x00ff, 0x0100, 0x01ff, 0x0200, 0x00fe, 0x0101]
    if element_bytes == 4:
        carry += [0x00ffff, 0x010000, 0x00ff00, 0x3f00ffff, 0x3f010000, 0x3effffff, 0x3f000000]
    else:
        carry += [0x3cff, 0x3d00, 0x3bff, 0x3c00]
    other = torch.float16 if dtype == torch.float32 else torch.float32
    for patterns in families + [carry, sum(families, []) + carry]:
        base = C.from_bits(patterns, dtype)
        signs = torch.where(torch.rand(base.numel(), generator=generator) < 0.5, -1.0, 1.0).to(dtype)
        row = torch.cat([base * signs, C.specials(dtype), base[: 5]])
        n, m = row.numel(), 6
        dense = torch.stack([row[torch.randperm(n, generator=generator)] for _ in range(m)])
        # as scores, over a sparse pattern of plain values
        lengths = torch.randint(0, n + 1, (m,), generator=generator)
        row_offsets, column_indices = C.csr(lengths, n, generator)
        plain = C.quantised(column_indices.numel(), other, generator)
        for fraction in (0.1, 0.5, 1.0):
            check(plain, row_offsets, column_indices, int(plain.numel() * fraction), dense, note="scores")
        # as values: every row full, so the old values are the dense rows themselves
        full_offsets = torch.arange(m + 1, dtype=torch.int32) * n
        full_columns = torch.arange(n, dtype=torch.int32).repeat(m)
        for d in (1, 2, m * n // 2, m * n - 3):
            check(dense.reshape(-1), full_offsets, full_columns, d, C.quantised((m, n), other, generator),
                  note="values")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_clamp_and_the_specials(dtype):
    """NaN and +-inf scores tie with finfo.max and lose to a lower flat index holding it; NaN and
    inf values rank above every finite one; denormals rank by their bits; -0.0 ties with 0.0."""
    n = 200
    largest = torch.finfo(dtype).max
    scores = torch.full((3, n), 1.0, dtype=dtype)
    scores[0, 150], scores[0, 20], scores[1, 90], scores[2, 199] = float("nan"), largest, float("inf"), -float("inf")
    scores[1, 5] = -largest
    row_offsets = torch.tensor([0, 3, 6, 9], dtype=torch.int32)
    column_indices = torch.tensor([0, 1, 2, 0, 2, 90, 0, 1, 2], dtype=torch.int32)
    values = torch.tensor([9.0, 8.0, 7.0, 6.0, 5.0, 1.0, 4.0, 3.0, 2.0], dtype=torch.float32)
    order = [(0, 20), (0, 150), (1, 5), (1, 90), (2, 199)]              # the clamped ties, by flat index
    for d in range(1, 6):
        got = check(values, row_offsets, column_indices, d, scores)
        lengths = (got[1][1:] - got[1][:-1]).to(torch.int64).cpu()
        rows = torch.repeat_interleave(torch.arange(3), lengths)
        grown = got[4].cpu() == -1
        assert list(zip(rows[grown].tolist(), got[2].cpu()[grown].tolist())) == order[:d]
    # values: NaN > inf > finite; denormals by their bits; -0.0 == 0.0 by index
    special = torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), largest, 1.0, 0.0, -0.0, 0.0, -0.0],
                                      dtype=dtype), C.from_bits([1, 2, 3], dtype)])
    k = special.numel()
    generator = torch.Generator().manual_seed(45)
    values = special[torch.randperm(k, generator=generator)].repeat(2)
    row_offsets, column_indices = C.csr([k // 2, k - k // 2, k // 3, k - k // 3], n, generator)
    grow = C.quantised((4, n), dtype, generator)
    for d in range(0, 2 * k + 1):
        got = check(values, row_offsets, column_indices, d, grow, note="special values")
    assert not C.bits_of(got[3]).any()


def test_count_edges():
    generator = torch.Generator().manual_seed(46)
    values, row_offsets, column_indices, scores = C.random_case(37, 90, torch.float32, torch.float16, generator)
    nnz = values.numel()
    got = check(values, row_offsets, column_indices, 0, scores)
    assert torch.equal(got[4].cpu(), torch.arange(nnz)) and torch.equal(got[2].cpu(), column_indices)
    assert torch.equal(got[1].cpu(), row_offsets) and torch.equal(C.bits_of(got[3]).cpu(), C.bits_of(values))
    got = check(values, row_offsets, column_indices, nnz, scores)
    assert bool((got[4] == -1).all()) and not C.bits_of(got[3]).any()
    check(values, row_offsets, column_indices, 1, scores)
    check(values, row_offsets, column_indices, nnz - 1, scores)
    for m, n in ((5, 7), (0, 7), (3, 0), (0, 0), (2049, 3)):              # no entries
        empty = (torch.zeros(0), torch.zeros(m + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
        got = check(*empty, 0, torch.zeros(m, n))
        assert got[0].cpu().tolist() == list(range(m)) and not got[1].any() and got[2].numel() == 0
    # a full pattern: Grown is exactly what was dropped
    m, n = 9, 70
    row_offsets, column_indices = C.csr([n] * m, n, generator)
    values = C.quantised(m * n, torch.bfloat16, generator)
    for d in (0, 1, 100, m * n):
        got = check(values, row_offsets, column_indices, d, C.quantised((m, n), torch.float32, generator))
        assert torch.equal(got[2].cpu(), column_indices) and torch.equal(got[1].cpu(), row_offsets)
    on_device = [t.cuda() for t in (values, row_offsets, column_indices)]
    with pytest.raises(ValueError):
        ops.csr_regrow_total(*on_device, m * n + 1, torch.zeros(m, n).cuda())
    with pytest.raises(ValueError):
        ops.csr_regrow_total(*on_device, -1, torch.zeros(m, n).cuda())
    with pytest.raises(ValueError):
        ops.csr_regrow_total(*on_device, 1, torch.zeros(m, n))                          # scores on the CPU
    with pytest.raises(ValueError):
        ops.csr_regrow_total(on_device[0].double(), *on_device[1:], 1, torch.zeros(m, n).cuda())
    with pytest.raises(RuntimeError):
        ops.csr_regrow_total(values, row_offsets, column_indices, 1, torch.zeros(m, n))  # CPU tensors


def test_views_and_mixed_dtypes():
    generator = torch.Generator().manual_seed(47)
    big = C.quantised((40, 331), torch.float16, generator)
    device = big.cuda()

    def case(m, n, value_dtype):
        lengths = torch.randint(0, n + 1, (m,), generator=generator)
        row_offsets, column_indices = C.csr(lengths, n, generator)
        values = C.quantised(column_indices.numel(), value_dtype, generator)
        return values, row_offsets, column_indices, int(torch.randint(0, values.numel() + 1, (1,), generator=generator))

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
    wide = C.quantised((9, 77), torch.float32, generator)
    wide_device = wide.cuda()[:, 1:]                                       # float32 rows off 16 bytes
    assert (wide_device.data_ptr() % 16) != 0
    check(*case(9, 76, torch.float16), wide[:, 1:], device_scores=wide_device)
    check(*case(9, 76, torch.bfloat16), wide[:, 1:].to(torch.bfloat16))
    # values as a view: entries off 16 bytes
    values, row_offsets, column_indices, d = case(9, 76, torch.float16)
    padded = torch.cat([torch.zeros(3, dtype=torch.float16), values]).cuda()[3:]
    assert padded.data_ptr() % 16 != 0
    got = ops.csr_regrow_total(padded, row_offsets.cuda(), column_indices.cuda(), d, wide_device)
    C.assert_same(got, C.brute_force(values, row_offsets, column_indices, d, wide[:, 1:]))


@pytest.mark.parametrize("m", (1023, 1024, 1025, 16384))
def test_scan_and_row_limits(m):
    generator = torch.Generator().manual_seed(48)
    n = 8
    values, row_offsets, column_indices, scores = C.random_case(m, n, torch.float32, torch.float32, generator)
    values = C.quantised(values.numel(), torch.float32, generator, quantum=1.0)          # ties down the rows
    scores = C.quantised((m, n), torch.float32, generator, quantum=1.0)
    check(values, row_offsets, column_indices, values.numel() // 3, scores)


def test_beyond_the_limits_and_the_widest_row():
    generator = torch.Generator().manual_seed(49)
    shape = capi.csr_regrow_total_launch_shape(3, 8, 8, 2, 4)
    max_m, max_n = shape["max_m"], shape["max_n"]
    for m, n, score_dtype in ((max_m + 1, 8, torch.float32), (3, max_n + 1, torch.float16), (3, max_n, torch.float16)):
        lengths = torch.randint(0, 9, (m,), generator=generator) if m > 3 else torch.tensor([5, 0, 8])
        row_offsets, column_indices = C.csr(lengths, n, generator)
        if m == 3:
            column_indices[-1] = n - 1                                     # the last bit of the planes
        values = C.quantised(column_indices.numel(), torch.float32, generator)
        scores = C.quantised((m, n), score_dtype, generator)
        scores[m - 1, n - 2] = 100.0
        d = values.numel() // 2
        served = capi.csr_regrow_total_launch_shape(m, n, values.numel(), C.width(score_dtype), 4)["served"]
        assert served == (m <= max_m and n <= max_n)
        on_device = [values.cuda(), row_offsets.cuda(), column_indices.cuda(), d, scores.cuda()]
        if served:
            check(values, row_offsets, column_indices, d, scores)
        else:
            with pytest.raises(RuntimeError):
                ops.csr_regrow_total(*on_device)
        got = topology.regrow_total(*on_device)            # beyond the limits: answered by the torch path
        assert all(g.is_cuda for g in got)
        C.assert_same(got, C.torch_path(values, row_offsets, column_indices, d, scores))


def test_routes_agree():
    generator = torch.Generator().manual_seed(50)
    values, row_offsets, column_indices, scores = C.random_case(33, 90, torch.float32, torch.float32, generator)
    d = values.numel() // 3
    want = C.brute_force(values, row_offsets, column_indices, d, scores)
    on_device = [values.cuda(), row_offsets.cuda(), column_indices.cuda(), d, scores.cuda()]
    C.assert_same(topology.regrow_total(*on_device), want)
    C.assert_same(topology.regrow_total_composed(*on_device), want)                     # the device top-k inside
    C.assert_same(C.torch_path(*on_device), want)
    C.assert_same(topology.regrow_total(*on_device[:4], scores.double().cuda()), want)   # ranked as .float()
    C.assert_same(topology.regrow_total(on_device[0].double(), *on_device[1:]),
                  C.brute_force(values.double(), row_offsets, column_indices, d, scores))


def test_reproducible_and_capturable():
    """Two calls give equal tensors.  The call neither synchronises nor reads back and its
    allocations are torch's own per call: it is captured into a graph on a side stream, and every
    replay on new values and scores in the captured buffers equals the eager call and the torch
    path."""
    generator = torch.Generator().manual_seed(51)
    m, n = 70, 1100
    values, row_offsets, column_indices, scores = C.random_case(m, n, torch.float32, torch.float32, generator)
    d = values.numel() // 3
    static = [values.cuda(), row_offsets.cuda(), column_indices.cuda(), scores.cuda()]

    def run():
        return ops.csr_regrow_total(static[0], static[1], static[2], d, static[3])

    first, second = run(), run()
    C.assert_same(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                             # (warm-up on the capturing stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = run()
    for replay in range(2):
        new_values = C.quantised(values.numel(), torch.float32, generator)
        new_scores = C.quantised((m, n), torch.float32, generator)
        static[0].copy_(new_values)
        static[3].copy_(new_scores)
        graph.replay()
        torch.cuda.synchronize()
        C.assert_same(captured, run(), f"replay {replay} against the eager call")
        C.assert_same(captured, C.torch_path(new_values, row_offsets, column_indices, d, new_scores),
                      f"replay {replay} against the torch path")
        C.assert_same(captured, C.brute_force(new_values, row_offsets, column_indices, d, new_scores))


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
def test_update_topology_serves_no_stale_state(input_dtype):
    generator = torch.Generator().manual_seed(52)
    w = torch.randn(OUT, IN, generator=generator)
    module = SparseLinear.from_dense(w.cuda(), density=0.25)
    parameter, nnz = module.values, module.values.numel()
    x_host = torch.randn(BATCH, SEQ, IN, generator=generator).to(input_dtype)
    forward_backward(module, x_host)           # plans, transposed topology and images of the OLD pattern exist
    with torch.no_grad():
        module(x_host.cuda())
    optimizer = torch.optim.SGD(module.parameters(), lr=0.1)
    d = int(0.3 * nnz)

    for step in range(2):
        old = (module.values.detach().clone(), module.row_indices, module.row_offsets, module.column_indices)
        scores = torch.randn(OUT, IN, generator=generator)
        scores[1, 2], scores[3, 4] = float("nan"), float("inf")
        source = module.update_topology(0.3, scores.cuda())

        # the same step on a CPU module of the same pattern
        twin = SparseLinear(IN, OUT)
        twin.values = torch.nn.Parameter(old[0].cpu())
        twin.row_indices, twin.row_offsets, twin.column_indices = (t.cpu() for t in old[1:])
        twin_source = twin.update_topology(0.3, scores)
        want = C.brute_force(old[0].cpu(), old[2].cpu(), old[3].cpu(), d, scores)
        C.assert_same((twin.row_indices, twin.row_offsets, twin.column_indices, twin.values.detach(), twin_source), want)
        C.assert_same((module.row_indices, module.row_offsets, module.column_indices, module.values.detach(), source),
                      want)
        assert int((source == -1).sum()) == d
        assert all(getattr(module, name) is not t for name, t in
                   zip(("row_indices", "row_offsets", "column_indices"), old[1:]))
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


def test_rigl_update_is_update_topology_on_the_collected_gradient():
    generator = torch.Generator().manual_seed(53)
    out_f, in_f, seq, batch = 256, 128, 128, 2
    w = torch.randn(out_f, in_f, generator=generator).cuda()
    twins = [SparseLinear.from_dense(w, density=0.2).collect_dense_grad() for _ in range(2)]
    x = torch.randn(batch, seq, in_f, generator=generator).cuda()
    for layer in twins:
        y = layer(x)
        y.backward(torch.ones_like(y) * 0.5)
    assert torch.equal(twins[0].dense_grad, twins[1].dense_grad)
    old = [t.cpu() for t in (twins[0].values.detach(), twins[0].row_offsets, twins[0].column_indices)]
    scores = twins[1].dense_grad.clone()
    source = twins[0].rigl_update(0.3)
    want_source = twins[1].update_topology(0.3, grow_scores=scores)
    assert torch.equal(source, want_source) and int((source < 0).sum()) == int(0.3 * old[0].numel())
    for name in ("row_indices", "row_offsets", "column_indices"):
        assert torch.equal(getattr(twins[0], name), getattr(twins[1], name))
    assert torch.equal(twins[0].values.detach(), twins[1].values.detach())
    C.assert_same((twins[0].row_indices, twins[0].row_offsets, twins[0].column_indices, twins[0].values.detach(),
                   source), C.brute_force(*old, int(0.3 * old[0].numel()), scores.cpu()))
