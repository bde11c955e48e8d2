"""GPU: every launch instance of the sparse softmax kernel (csrc/softmax.hip), forward and
backward, against the float64 oracle on the operands as stored.

The kernel is one template, sparse_softmax_rows_kernel<T, LPR, BASE, V, BACKWARD, DEPTH, NT>:
six float32 and four half classes (LPR, BASE, V), two directions, three prefetch depths, four
nontemporal modes, a run length chosen at run time, and per row a fast path (aligned 16-byte
pieces, clamped and masked; pieces BASE..V-1 switched on per wave) or three strided passes.
The uniform random masks of the other softmax tests reach one path per class with the default
knobs.  Here the masks are skewed on purpose -- short rows, rows past BASE pieces, rows past
the window, empty rows, a row of one entry -- so that every launch mixes the three ways a row
is served; `sputnik_hip_sparse_softmax_route` (host only) says which instance a call takes,
and every test asserts the one it means to reach.  `serve_counts` restates the few lines of
the kernel's `fetch` that decide a row's path, from the operands' real addresses.

Bounds are the project's: rel_err < 1e-4 (float32), half_err < 1e-4 (one unit in the last
place of the stored output taken off first).
"""
import numpy as np
import pytest
import torch

from oracle import sputnik_oracle as O
from tests.helpers import half_err, rel_err, rel_err_torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
CANARY = -7.25          # exact in float32 / float16 / bfloat16; no softmax output
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
KNOBS = ("SPUTNIK_HIP_SOFTMAX_RPG", "SPUTNIK_HIP_SOFTMAX_DEPTH", "SPUTNIK_HIP_SOFTMAX_NT")

# (storage, short, long_a, long_b, class): rows of short +- 2 entries, two of long_a (inside the
# window, past BASE pieces; None where BASE == V), two of long_b (past the window)
FLOAT_TABLE = [
    (10, 70, 200, (16, 1, 2)),
    (60, 150, 260, (16, 2, 3)),
    (120, 250, 300, (16, 3, 4)),
    (170, 400, 600, (32, 2, 4)),
    (300, None, 600, (32, 4, 4)),
    (700, None, 1030, (64, 4, 4)),
]
HALF_TABLE = [
    (60, 190, 260, (16, 1, 2)),
    (150, 300, 500, (16, 2, 3)),
    (300, 600, 1000, (32, 2, 3)),
    (700, None, 1030, (64, 2, 2)),
]
CASES = ([(torch.float32,) + row for row in FLOAT_TABLE]
         + [(dt,) + row for dt in (torch.float16, torch.bfloat16) for row in HALF_TABLE])


def case_id(case):
    dtype, short, _, _, cls = case
    return f"{str(dtype).split('.')[-1]}-{cls[0]}_{cls[1]}_{cls[2]}-short{short}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def capi():
    from torch_sputnik_amd import capi
    assert "gfx950" in capi.version()
    return capi


@pytest.fixture
def knobs(capi, monkeypatch):
    """set(rpg=, depth=, nt=): the softmax developer knobs for the calls that follow; all three
    are removed again, and the library told to look, when the test ends.  (monkeypatch then
    puts back whatever the variables held before the test, without another look: a knob set
    from outside the test run stays switched off in the library until its next reload, as
    with the knob fixtures of conftest.py.)"""
    def set_knobs(rpg=None, depth=None, nt=None):
        for name, value in zip(KNOBS, (rpg, depth, nt)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(value))
        capi.reload_options()
    set_knobs()
    try:
        yield set_knobs
    finally:
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        capi.reload_options()


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def entries_per_piece(dtype):
    return 4 if dtype == torch.float32 else 8


def skewed_offsets(m, short, long_a, long_b, seed, odd=False):
    """Row offsets of a mask with rows of short +- 2 entries, except two rows of long_a (if any),
    two of long_b, two empty rows and one row of a single entry; rows 0 and m - 1 keep entries.
    `odd`: an odd entry count, so that consecutive replicas differ in alignment."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(short - 2, short + 3, size=m)
    special = rng.choice(np.arange(1, m - 1), size=7, replace=False)
    if long_a is not None:
        lens[special[0:2]] = long_a
    lens[special[2:4]] = long_b
    lens[special[4:6]] = 0
    lens[special[6]] = 1
    if odd and int(lens.sum()) % 2 == 0:
        lens[0] += 1
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def topology(ro):
    """(row_indices, column_indices) that go with the offsets: the softmax reads neither, the
    oracle checks their shapes."""
    m, nnz = len(ro) - 1, int(ro[-1])
    return np.arange(m, dtype=np.int32), np.zeros(nnz, dtype=np.int32)


def stored(x, dtype):
    """x rounded to the storage type, as float32 numpy: what the kernel reads."""
    return torch.from_numpy(np.asarray(x, np.float32)).to(dtype).float().numpy()


def want_forward(x, ro, scale):
    ri, ci = topology(ro)
    return O.sparse_softmax_scaled(np.asarray(x, np.float64), ri, ro, ci, scale)


def err_of(got, want, dtype, ro):
    return rel_err(got, want, ro) if dtype == torch.float32 else half_err(got, want, dtype, ro)


class Operand:
    """[rows, nnz] values inside a flat device buffer: row r at `start + r * stride`, the buffer's
    first byte on a 16-byte boundary, so row 0 sits `phase` entries into a piece.  Everything
    around the rows holds `fill` (NaN for inputs, the canary for outputs), at least one piece
    before and after."""

    def __init__(self, dev, dtype, rows, nnz, phase=0, stride=None, fill=float("nan"), values=None):
        e = entries_per_piece(dtype)
        self.rows, self.nnz = rows, nnz
        self.stride = nnz if stride is None else stride
        self.start = e + phase
        size = self.start + (rows - 1) * self.stride + nnz + 2 * e
        self.buf = torch.full((size,), fill, dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.fill = fill
        if values is not None:
            self.region().copy_(torch.from_numpy(np.asarray(values, np.float32)).to(dev).to(dtype))
        else:
            self.region().fill_(float("nan"))

    def region(self):
        return torch.as_strided(self.buf, (self.rows, self.nnz), (self.stride, 1), self.start)

    def arg(self):
        return self.buf[self.start:]

    def address(self):
        """of row 0, in elements"""
        return self.buf.data_ptr() // self.buf.element_size() + self.start

    def take(self):
        """The rows (a copy), after checking that nothing around them changed, bit for bit."""
        got = self.region().clone()
        self.region().fill_(self.fill)
        bits = torch.int32 if self.buf.dtype == torch.float32 else torch.int16
        untouched = torch.full((1,), self.fill, dtype=self.buf.dtype, device=self.buf.device).view(bits)
        assert bool((self.buf.view(bits) == untouched).all()), "a write outside the output's rows"
        return got


def launch(capi, dev, dtype, ro_d, m, replicas, a, b, scale, phases=(0, 0, 0), strides=(None, None, None),
           float_entry=False, out=None):
    """One call of the kernel library.  a [R, nnz]: scores (forward, b is None) or the softmax
    output (backward, b = the gradient [R, nnz], or [1, nnz] with stride 0).  Returns (result
    rows as a device tensor, the three operands)."""
    nnz = a.shape[1]
    op_a = Operand(dev, dtype, a.shape[0], nnz, phases[0], strides[0], values=a)
    op_out = out if out is not None else Operand(dev, dtype, replicas, nnz, phases[2], strides[2], fill=CANARY)
    ri_d = torch.zeros(m, dtype=torch.int32, device=dev)
    ci_d = torch.zeros(nnz, dtype=torch.int32, device=dev)
    if b is None:
        fn = capi.sparse_softmax_scaled_batched if float_entry else capi.sparse_softmax_typed
        fn(m, replicas, op_a.arg(), ri_d, ro_d, ci_d, scale, op_out.arg(),
           values_stride=op_a.stride, out_stride=op_out.stride)
        return op_out.take(), (op_a, None, op_out)
    op_b = Operand(dev, dtype, b.shape[0], nnz, phases[1], strides[1], values=b)
    fn = capi.sparse_softmax_backward_batched if float_entry else capi.sparse_softmax_backward_typed
    fn(m, replicas, op_a.arg(), op_b.arg(), ro_d, scale, op_out.arg(), nonzeros=nnz,
       softmax_out_stride=op_a.stride, grad_out_stride=op_b.stride, grad_values_stride=op_out.stride)
    return op_out.take(), (op_a, op_b, op_out)


def serve_counts(ro, cls, dtype, replicas, ops):
    """How the kernel serves the rows of a call -- the arithmetic of its `fetch` and of
    launch_rows' `same_phase`, from the operands' addresses and strides -- as a dict of
    counts over all replicas (fast: BASE pieces suffice; extra: the row itself reaches past
    them; strided) and the per-(replica, row) arrays `kind` (0 empty, 1 fast, 2 extra,
    3 strided) and `first_piece` (start of the first aligned piece, relative to the replica)."""
    lpr, base, v = cls
    e = entries_per_piece(dtype)
    present = [op for op in ops if op is not None]
    op_a = present[0]
    nnz = op_a.nnz
    alike = all(op.stride == op_a.stride for op in present)
    same_phase = (alike and 2 * e <= nnz < (1 << 28)
                  and all(op.address() % e == op_a.address() % e for op in present))
    p0 = np.asarray(ro[:-1], np.int64)
    p1 = np.asarray(ro[1:], np.int64)
    kind = np.zeros((replicas, len(p0)), np.int64)
    first = np.zeros((replicas, len(p0)), np.int64)
    for r in range(replicas):
        phase = (op_a.address() + r * op_a.stride) % e
        lo_lim = -(r * op_a.stride)
        hi_lim = (replicas - 1 - r) * op_a.stride + nnz
        qmin = lo_lim + ((-(lo_lim + phase)) & (e - 1))
        qmax = ((hi_lim - e + phase) & ~(e - 1)) - phase
        s = p0 - ((p0 + phase) & (e - 1))
        last_piece = ((p1 - 1 + phase) & ~(e - 1)) - phase
        fast = same_phase & (p1 - s <= lpr * e * v) & (s >= qmin) & (last_piece <= qmax)
        extra = fast & (p1 - s > base * e * lpr)
        kind[r] = np.where(p1 == p0, 0, np.where(extra, 2, np.where(fast, 1, 3)))
        first[r] = s
    return {"fast": int((kind == 1).sum()), "extra": int((kind == 2).sum()),
            "strided": int((kind == 3).sum()), "kind": kind, "first_piece": first}


def assert_class(capi, m, nnz, replicas, dtype, backward, cls, **more):
    route = capi.sparse_softmax_route(m, nnz, replicas, dtype, backward)
    assert (route["lanes_per_row"], route["base_pieces"], route["pieces"]) == cls, (route, cls)
    for key, value in more.items():
        assert route[key] == value, (key, route)
    return route


class Problem:
    """A skewed mask with values for both directions and their float64 references (computed
    once per scale, shared by the calls of a test)."""

    def __init__(self, dev, dtype, m, short, long_a, long_b, seed, replicas=3, odd=False):
        self.dtype, self.m, self.replicas = dtype, m, replicas
        self.ro = skewed_offsets(m, short, long_a, long_b, seed, odd)
        self.nnz = int(self.ro[-1])
        self.ro_d = torch.from_numpy(self.ro).to(dev)
        rng = np.random.default_rng(seed + 1)
        self.x = stored(rng.uniform(-6, 6, (replicas, self.nnz)), dtype)
        # backward: y from the float64 forward, rounded to the storage type; g uniform in [-1, 1]
        self.y = {}
        self.g = stored(rng.uniform(-1, 1, (replicas, self.nnz)), dtype)
        self._want = {}

    def want(self, backward, scale):
        key = (backward, scale)
        if key not in self._want:
            if not backward:
                self._want[key] = want_forward(self.x, self.ro, scale)
            else:
                self.y[scale] = stored(want_forward(self.x, self.ro, scale), self.dtype)
                self._want[key] = O.sparse_softmax_backward(self.y[scale], self.g, self.ro, scale)
        return self._want[key]

    def operands(self, backward, scale):
        self.want(backward, scale)
        return (self.y[scale], self.g) if backward else (self.x, None)


# ---------------------------------------------------------------------------------------------
# A. every class, both directions, three storage types
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_class_both_directions(capi, dev, knobs, case):
    dtype, short, long_a, long_b, cls = case
    for m in (37, 150):
        prob = Problem(dev, dtype, m, short, long_a, long_b, seed=1000 + m + short)
        for backward in (False, True):
            assert_class(capi, m, prob.nnz, 3, dtype, backward, cls, depth=1, nontemporal=0)
            for scale in (1.0, 0.125):
                a, b = prob.operands(backward, scale)
                got, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, a, b, scale)
                counts = serve_counts(prob.ro, cls, dtype, 3, ops)
                assert counts["fast"] > 0 and counts["strided"] > 0, counts
                if cls[1] < cls[2]:
                    assert counts["extra"] > 0, counts
                got = got.float().cpu().numpy()
                tag = (case_id(case), m, backward, scale)
                assert not np.isnan(got).any(), tag
                err = err_of(got, prob.want(backward, scale), dtype, prob.ro)
                print(tag, "err", err)
                assert err < TOL, tag


# ---------------------------------------------------------------------------------------------
# B. phases
# ---------------------------------------------------------------------------------------------
PHASE_CASES = [(torch.float32,) + FLOAT_TABLE[1], (torch.float16,) + HALF_TABLE[1],
               (torch.bfloat16,) + HALF_TABLE[0]]


@pytest.mark.parametrize("case", PHASE_CASES, ids=case_id)
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_every_phase_and_mismatched_phases(capi, dev, knobs, case, backward):
    """Every alignment of the operands inside a 16-byte piece, with an odd entry count (each
    replica at another phase), NaN around every input and a canary around the output; operands
    aligned alike take the fast path, three mismatched combinations the strided passes."""
    dtype, short, long_a, long_b, cls = case
    e = entries_per_piece(dtype)
    m, scale = 37, 0.125
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=77 + short, odd=True)
    assert prob.nnz % 2 == 1
    assert_class(capi, m, prob.nnz, 3, dtype, backward, cls)
    a, b = prob.operands(backward, scale)
    want = prob.want(backward, scale)
    for phase in range(e):
        got, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, a, b, scale, phases=(phase,) * 3)
        counts = serve_counts(prob.ro, cls, dtype, 3, ops)
        assert counts["fast"] > 0 and counts["extra"] > 0 and counts["strided"] > 0, (phase, counts)
        got = got.float().cpu().numpy()
        assert not np.isnan(got).any(), phase
        assert err_of(got, want, dtype, prob.ro) < TOL, phase
    mismatched = [(1, 2, 1), (1, 1, 2), (0, e - 1, 2)] if backward else [(1, 1, 2), (0, 0, e - 1), (3, 3, 0)]
    for phases in mismatched:
        got, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, a, b, scale, phases=phases)
        counts = serve_counts(prob.ro, cls, dtype, 3, ops)
        assert counts["fast"] == 0 and counts["extra"] == 0 and counts["strided"] > 0, (phases, counts)
        got = got.float().cpu().numpy()
        assert not np.isnan(got).any(), phases
        assert err_of(got, want, dtype, prob.ro) < TOL, phases


# ---------------------------------------------------------------------------------------------
# C. strides
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,float_entry", [(torch.float32, True), (torch.float32, False),
                                               (torch.float16, False)],
                         ids=["float32_entry", "float32_typed", "float16_typed"])
def test_strides(capi, dev, knobs, dtype, float_entry):
    """Replica strides other than the entry count: equal padded strides (fast path; NaN in the
    inputs' pads, the output's pads untouched), an input padded differently from the output, a
    gradient broadcast with stride 0, a padded softmax output next to dense operands (all
    strided passes: launch_rows' strides_alike)."""
    short, long_a, long_b, cls = FLOAT_TABLE[1] if dtype == torch.float32 else HALF_TABLE[1]
    m, scale, replicas = 37, 0.125, 3
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=5 + short)
    n = prob.nnz
    for backward in (False, True):
        assert_class(capi, m, n, replicas, dtype, backward, cls)
        a, b = prob.operands(backward, scale)
        want = prob.want(backward, scale)
        layouts = [((n + 1,) * 3, True), ((n + 5,) * 3, True), ((n + 3, n + 3, n), False),
                   ((n, n, n + 2), False)]
        if backward:
            layouts += [((n + 4, n, n), False), ((n, n + 1, n + 2), False)]
        for strides, fast in layouts:
            got, ops = launch(capi, dev, dtype, prob.ro_d, m, replicas, a, b, scale, strides=strides,
                              float_entry=float_entry)
            counts = serve_counts(prob.ro, cls, dtype, replicas, ops)
            if fast:
                assert counts["fast"] > 0 and counts["extra"] > 0 and counts["strided"] > 0, (strides, counts)
            else:
                assert counts["fast"] == 0 and counts["extra"] == 0, (strides, counts)
            got = got.float().cpu().numpy()
            assert not np.isnan(got).any(), (backward, strides)
            assert err_of(got, want, dtype, prob.ro) < TOL, (backward, strides)
    # one gradient row for all replicas
    y = prob.y[scale]
    want = O.sparse_softmax_backward(y, np.broadcast_to(prob.g[:1], y.shape), prob.ro, scale)
    got, ops = launch(capi, dev, dtype, prob.ro_d, m, replicas, y, prob.g[:1], scale, strides=(n, 0, n),
                      float_entry=float_entry)
    assert serve_counts(prob.ro, cls, dtype, replicas, ops)["fast"] == 0
    got = got.float().cpu().numpy()
    assert not np.isnan(got).any()
    assert err_of(got, want, dtype, prob.ro) < TOL


# ---------------------------------------------------------------------------------------------
# D. knobs: prefetch depth, rows per group, nontemporal hints
# ---------------------------------------------------------------------------------------------
KNOB_CASES = [(torch.float32,) + FLOAT_TABLE[2], (torch.float16,) + HALF_TABLE[2],
              (torch.float32,) + FLOAT_TABLE[5]]
KNOB_COMBOS = ([dict(depth=d, rpg=r) for d in (2, 3) for r in (1, 2, 3, 5, 16)]
               + [dict(depth=1, nt=t, rpg=r) for t in (0, 1, 2, 3) for r in (1, 2, 5, 16)])


@pytest.mark.parametrize("case", KNOB_CASES, ids=case_id)
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_knobs_give_the_default_bits(capi, dev, knobs, case, backward):
    """Depth 2 and 3 x run lengths 1, 2, 3, 5, 16 and the four nontemporal modes (depth 1: the
    deeper rings are built without the hint) x run lengths 1, 2, 5, 16: each against float64
    and bit-identical to the default instance -- a row's lane assignment and the order of its
    reductions depend on none of the three, and a piece that a neighbouring row of the wave
    switched on adds -inf to the maximum and 0 to the sums."""
    dtype, short, long_a, long_b, cls = case
    scale = 0.125
    for m in (150, 37):
        prob = Problem(dev, dtype, m, short, long_a, long_b, seed=300 + m + short)
        a, b = prob.operands(backward, scale)
        want = prob.want(backward, scale)
        knobs()
        assert_class(capi, m, prob.nnz, 3, dtype, backward, cls, rows_per_group=1, depth=1, nontemporal=0)
        default, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, a, b, scale)
        counts = serve_counts(prob.ro, cls, dtype, 3, ops)
        assert counts["fast"] > 0 and counts["strided"] > 0 and (cls[1] == cls[2] or counts["extra"] > 0)
        assert err_of(default.float().cpu().numpy(), want, dtype, prob.ro) < TOL, (m, "default")
        for combo in KNOB_COMBOS:
            knobs(**combo)
            assert_class(capi, m, prob.nnz, 3, dtype, backward, cls, rows_per_group=combo["rpg"],
                         depth=combo["depth"], nontemporal=combo.get("nt", 0))
            got, _ = launch(capi, dev, dtype, prob.ro_d, m, 3, a, b, scale)
            host = got.float().cpu().numpy()
            assert not np.isnan(host).any(), (m, combo)
            assert err_of(host, want, dtype, prob.ro) < TOL, (m, combo)
            assert torch.equal(got.view(torch.uint8), default.view(torch.uint8)), (m, combo)


# ---------------------------------------------------------------------------------------------
# E. the automatic two rows per group
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,short,long_a,long_b,cls", [
    (512, 10, 70, 200, (16, 1, 2)), (515, 10, 70, 200, (16, 1, 2)),
    (128, 700, None, 1030, (64, 4, 4)), (129, 700, None, 1030, (64, 4, 4))],
    ids=["16_1_2-m512", "16_1_2-m515", "64_4_4-m128", "64_4_4-m129"])
def test_automatic_two_rows_per_group(capi, dev, knobs, m, short, long_a, long_b, cls):
    """No knob set: 128 replicas put m * replicas at the rule's threshold, so the two-row ring
    runs as the benchmarked sizes run it.  m = 515 and 129 are no multiple of the rows one wave
    covers (2 x 64 / LPR): the last wave's lane broadcast of row bounds and its `it0 + J <
    rows_per_group` tail see rows past m.  Eight replicas' worth of values, repeated (the
    float64 reference is computed once per distinct replica)."""
    dtype, replicas, distinct, scale = torch.float32, 128, 8, 0.125
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=m, replicas=distinct)
    for backward in (False, True):
        route = assert_class(capi, m, prob.nnz, replicas, dtype, backward, cls, rows_per_group=2, depth=1,
                             nontemporal=0)
        if m in (515, 129):
            assert m % (2 * 64 // route["lanes_per_row"]) != 0
        a, b = prob.operands(backward, scale)
        tile = lambda x: np.tile(x, (replicas // distinct, 1))
        got, ops = launch(capi, dev, dtype, prob.ro_d, m, replicas, tile(a), None if b is None else tile(b), scale)
        counts = serve_counts(prob.ro, cls, dtype, replicas, ops)
        assert counts["fast"] > 0 and counts["strided"] > 0 and (cls[1] == cls[2] or counts["extra"] > 0)
        got = got.cpu().numpy()
        assert not np.isnan(got).any()
        want = prob.want(backward, scale)
        worst = max(rel_err(got[i:i + distinct], want, prob.ro) for i in range(0, replicas, distinct))
        assert worst < TOL, (backward, worst)


# ---------------------------------------------------------------------------------------------
# F. more replicas than one grid's y dimension holds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_replica_slices(capi, dev, knobs, dtype):
    """65535 + 3 replicas of a mask of 3 rows and 41 entries: the second launch of the slice
    loop serves the last three, which carry values of their own, with buffer limits relative
    to the slice."""
    ro = np.array([0, 17, 22, 41], np.int32)
    m, nnz, replicas, scale = 3, 41, 65535 + 3, 0.5
    ro_d = torch.from_numpy(ro).to(dev)
    rng = np.random.default_rng(41)
    x4 = stored(rng.uniform(-6, 6, (4, nnz)), dtype)
    g4 = stored(rng.uniform(-1, 1, (4, nnz)), dtype)
    y4 = stored(want_forward(x4, ro, scale), dtype)
    spread = lambda v: np.concatenate([np.broadcast_to(v[:1], (65535, nnz)), v[1:]])
    for backward in (False, True):
        assert_class(capi, m, nnz, replicas, dtype, backward, (16, 1, 2))
        want4 = O.sparse_softmax_backward(y4, g4, ro, scale) if backward else want_forward(x4, ro, scale)
        a, b = (spread(y4), spread(g4)) if backward else (spread(x4), None)
        got, ops = launch(capi, dev, dtype, ro_d, m, replicas, a, b, scale)
        assert not bool(torch.isnan(got).any())
        # the first 65535 replicas hold the same values at eight (four) alignments: compare the
        # distinct results, and the last three, with float64
        head = np.ascontiguousarray(got[:65535].float().cpu().numpy())
        head = np.unique(head.view(np.dtype((np.void, 4 * nnz))).ravel()).view(np.float32).reshape(-1, nnz)
        assert 1 <= len(head) <= 64
        for row in head:
            assert err_of(row[None], want4[:1], dtype, ro) < TOL, backward
        assert err_of(got[65535:].float().cpu().numpy(), want4[1:], dtype, ro) < TOL, backward


# ---------------------------------------------------------------------------------------------
# G. tiny calls and special values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float16", "bfloat16"])
def test_tiny_entry_counts(capi, dev, knobs, dtype):
    """1, 2E - 1 and 2E entries (E per 16-byte piece): below 2E no row takes the fast path."""
    e = entries_per_piece(dtype)
    rng = np.random.default_rng(3)
    for lens in ((1, 0), (e, e - 1), (e + 1, e - 1)):
        ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        nnz, m, scale = int(ro[-1]), 2, 0.5
        ro_d = torch.from_numpy(ro).to(dev)
        x = stored(rng.uniform(-6, 6, (3, nnz)), dtype)
        g = stored(rng.uniform(-1, 1, (3, nnz)), dtype)
        want = want_forward(x, ro, scale)
        y = stored(want, dtype)
        for phase in (0, 1, e - 1):
            for backward in (False, True):
                assert_class(capi, m, nnz, 3, dtype, backward, (16, 1, 2))
                a, b = (y, g) if backward else (x, None)
                got, ops = launch(capi, dev, dtype, ro_d, m, 3, a, b, scale, phases=(phase,) * 3)
                counts = serve_counts(ro, (16, 1, 2), dtype, 3, ops)
                if nnz < 2 * e:
                    assert counts["fast"] == 0 and counts["extra"] == 0, counts
                got = got.float().cpu().numpy()
                assert not np.isnan(got).any(), (lens, phase, backward)
                ref = O.sparse_softmax_backward(y, g, ro, scale) if backward else want
                assert err_of(got, ref, dtype, ro) < TOL, (lens, phase, backward)


@pytest.mark.parametrize("case", PHASE_CASES, ids=case_id)
def test_masked_scores_give_exact_zeros(capi, dev, knobs, case):
    """Rows where some, not all, scores are -inf: exact zeros there, in fast and strided rows,
    and a gradient of exactly zero through them."""
    dtype, short, long_a, long_b, cls = case
    m, scale = 37, 0.125
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=11 + short, odd=True)
    rng = np.random.default_rng(12)
    x = prob.x.copy()
    masked = rng.random(x.shape) < 0.3
    masked[:, prob.ro[:-1][np.diff(prob.ro) > 0]] = False     # every row keeps its first score
    x[masked] = -np.inf
    assert_class(capi, m, prob.nnz, 3, dtype, False, cls)
    got, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, x, None, scale, phases=(1, 1, 1))
    counts = serve_counts(prob.ro, cls, dtype, 3, ops)
    assert counts["fast"] > 0 and counts["extra"] > 0 and counts["strided"] > 0, counts
    got = got.float().cpu().numpy()
    want = want_forward(x, prob.ro, scale)
    assert np.all(want[masked] == 0.0) and np.all(got[masked] == 0.0)
    assert not np.isnan(got).any()
    assert err_of(got, want, dtype, prob.ro) < TOL
    y = stored(want, dtype)
    assert_class(capi, m, prob.nnz, 3, dtype, True, cls)
    dx, _ = launch(capi, dev, dtype, prob.ro_d, m, 3, y, prob.g, scale, phases=(1, 1, 1))
    dx = dx.float().cpu().numpy()
    assert np.all(dx[masked] == 0.0) and not np.isnan(dx).any()
    assert err_of(dx, O.sparse_softmax_backward(y, prob.g, prob.ro, scale), dtype, prob.ro) < TOL


@pytest.mark.parametrize("case", PHASE_CASES, ids=case_id)
def test_large_scores_and_where_the_maximum_sits(capi, dev, knobs, case):
    """Scores around 1e3 (the maximum must come off before the exponential), with the row
    maximum in an `extra` piece, in the partial first piece of a fast row, and in a strided
    row."""
    dtype, short, long_a, long_b, cls = case
    lpr, base, _ = cls
    e = entries_per_piece(dtype)
    m = 37
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=21 + short, odd=True)
    rng = np.random.default_rng(22)
    lens = np.diff(prob.ro)
    # spacing of bfloat16 at 1e3 is 4: steps of 4 below the maximum keep the rounded inputs apart
    x = 1000.0 - 4.0 * rng.integers(1, 5, (3, prob.nnz))
    p0 = prob.ro[:-1].astype(np.int64)
    top = np.where(lens == long_a, p0 + lens - 1,                  # last entry: past BASE pieces
                   np.where(lens == long_b, p0 + lens // 2, p0))   # strided row / first entry
    top = top[lens > 0]
    x[:, top] = 1008.0
    x = stored(x, dtype)
    assert np.all(x[:, top] == 1008.0)
    assert_class(capi, m, prob.nnz, 3, dtype, False, cls)
    got, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, x, None, 1.0, phases=(1, 1, 1))
    counts = serve_counts(prob.ro, cls, dtype, 3, ops)
    kind, first = counts["kind"], counts["first_piece"]
    rows_a, rows_b = np.flatnonzero(lens == long_a), np.flatnonzero(lens == long_b)
    # the placements are what the docstring says, for some replica each
    assert np.any((kind[:, rows_a] == 2) & (p0[rows_a] + lens[rows_a] - 1 - first[:, rows_a] >= base * e * lpr))
    assert np.all(kind[:, rows_b] == 3)
    plain = np.flatnonzero((lens > 1) & (lens != long_a) & (lens != long_b))
    assert np.any((kind[:, plain] == 1) & (first[:, plain] < p0[plain]))
    got = got.float().cpu().numpy()
    assert not np.isnan(got).any()
    assert err_of(got, want_forward(x, prob.ro, 1.0), dtype, prob.ro) < TOL


def test_float16_scores_near_the_largest_finite_value(capi, dev, knobs):
    """float16 scores near +-6e4 (the type's largest is 65504) with scale 1/8: widened before
    the scale is applied; steps of 32 (the spacing there) give differences of 4 after it."""
    dtype = torch.float16
    short, long_a, long_b, cls = HALF_TABLE[0]
    m, scale = 37, 0.125
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=31, odd=True)
    rng = np.random.default_rng(32)
    sign = np.where(rng.random(m) < 0.5, -1.0, 1.0)[np.repeat(np.arange(m), np.diff(prob.ro))]
    x = sign * 60000.0 + 32.0 * rng.integers(0, 9, (3, prob.nnz))
    assert np.array_equal(stored(x, dtype), x.astype(np.float32))
    assert_class(capi, m, prob.nnz, 3, dtype, False, cls)
    got, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, x, None, scale, phases=(3, 3, 3))
    counts = serve_counts(prob.ro, cls, dtype, 3, ops)
    assert counts["fast"] > 0 and counts["extra"] > 0 and counts["strided"] > 0, counts
    got = got.float().cpu().numpy()
    assert not np.isnan(got).any()
    assert half_err(got, want_forward(x, prob.ro, scale), dtype, prob.ro) < TOL


# ---------------------------------------------------------------------------------------------
# H. the automatic nontemporal forward
# ---------------------------------------------------------------------------------------------
def test_automatic_nontemporal_forward(capi, dev, knobs):
    """An output of 128 MB in one grid slice takes nontemporal stores on its own (the
    512-replica row of the benchmark): against a float64 softmax computed on the device, and
    the bits of the same call with the hint switched off."""
    m, replicas, scale = 64, 1024, 0.125
    lens = 512 + (np.arange(m) % 5)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz, widest = int(ro[-1]), int(lens.max())
    assert replicas * nnz * 4 >= 128 << 20
    ro_d = torch.from_numpy(ro).to(dev)
    ri_d = torch.zeros(m, dtype=torch.int32, device=dev)
    ci_d = torch.zeros(nnz, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    x = (torch.rand(replicas, nnz, device=dev, generator=gen) - 0.5) * 48.0
    assert_class(capi, m, nnz, replicas, torch.float32, False, (64, 4, 4), rows_per_group=2, depth=1,
                 nontemporal=2)
    out = torch.full_like(x, float("nan"))
    capi.sparse_softmax_typed(m, replicas, x, ri_d, ro_d, ci_d, scale, out)
    # float64 reference: the rows as segments of a [replicas, m, widest] array, -inf past a row's end
    slot = torch.arange(widest, device=dev)[None, :]
    inside = slot < torch.from_numpy(lens).to(dev)[:, None]
    index = (ro_d[:-1].long()[:, None] + slot).clamp_max(nnz - 1)
    segments = (x.double() * scale)[:, index].masked_fill(~inside, float("-inf"))
    want = torch.softmax(segments, dim=-1)
    del segments
    got = out[:, index].masked_fill(~inside, 0.0)
    assert not bool(torch.isnan(out).any())
    assert rel_err_torch(got, want) < TOL
    del want, got
    knobs(nt=0)
    assert_class(capi, m, nnz, replicas, torch.float32, False, (64, 4, 4), rows_per_group=2, depth=1,
                 nontemporal=0)
    plain = torch.full_like(x, float("nan"))
    capi.sparse_softmax_typed(m, replicas, x, ri_d, ro_d, ci_d, scale, plain)
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))


# ---------------------------------------------------------------------------------------------
# I. the gradient written over the incoming gradient
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(torch.float32,) + FLOAT_TABLE[1], (torch.float16,) + HALF_TABLE[1]],
                         ids=case_id)
def test_backward_in_place_over_the_gradient(capi, dev, knobs, case):
    """grad_values may be the very tensor grad_out (the benchmark's backward step calls it so):
    the same bits as with an output of its own, two rows per group."""
    dtype, short, long_a, long_b, cls = case
    m, scale = 150, 0.125
    prob = Problem(dev, dtype, m, short, long_a, long_b, seed=91 + short)
    y, g = prob.operands(True, scale)
    knobs(rpg=2)
    assert_class(capi, m, prob.nnz, 3, dtype, True, cls, rows_per_group=2)
    apart, ops = launch(capi, dev, dtype, prob.ro_d, m, 3, y, g, scale)
    counts = serve_counts(prob.ro, cls, dtype, 3, ops)
    assert counts["fast"] > 0 and counts["extra"] > 0 and counts["strided"] > 0, counts
    assert err_of(apart.float().cpu().numpy(), prob.want(True, scale), dtype, prob.ro) < TOL
    y_d = torch.from_numpy(y).to(dev).to(dtype)
    g_d = torch.from_numpy(g).to(dev).to(dtype)
    assert y_d.data_ptr() % 16 == 0 and g_d.data_ptr() % 16 == 0      # as `ops`: phase 0 throughout
    capi.sparse_softmax_backward_typed(m, 3, y_d, g_d, prob.ro_d, scale, g_d)
    assert torch.equal(g_d.view(torch.uint8), apart.view(torch.uint8))
