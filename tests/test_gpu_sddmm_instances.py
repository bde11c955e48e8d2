"""GPU: every instance of the LDS-tiled SDDMM kernels (csrc/sddmm_tiled.hip) at its slab, window
and walk edges, on the run list of tests/sddmm_cases.py (tests/test_sddmm_cases_cpu.py proves
what the list reaches).  Per run:

  1. the route is asserted with capi.sddmm_launch_shape before any launch, under the run's knobs,
     with and without the walk knob;
  2. the plan goes into a workspace inside a buffer of canary ints and is compared with the
     numpy model bit for bit on the defined words; the guards must be intact;
  3. the product runs planned and unplanned into `out`, a slice of a canary buffer with
     out_stride = nonzeros + 3 and 16 guard elements on each side (NaN for float32, -768 for
     half), on operands with replica strides of rows * k + 16 elements and NaN in the gaps;
     every element is written, no canary inside survives, none outside moves (the summed
     form's scratch vectors the same way);
  4. planned and unplanned give identical bits, and so does the run under the walk knob (every
     entry is computed by exactly one workgroup with the same instruction sequence, whichever
     row blocks that workgroup walks: a derived equality, no tolerance);
  5. the result is held to float64 at the suite's bounds: float32 output rel_err < 1e-4, half
     output half_err < 1e-4, the summed form the same on the sum.

Small-integer operands must give exactly the integer products (every entry added once per panel,
walked accumulating runs among them); a many-mask batch of three masks runs with and without the
knob; torch.ops.torch_sputnik.sddmm takes a few runs as well.

The pair-flat kernel (csrc/sddmm_flat.hip) runs in the same harness on a mask whose (row block,
slab) tiles hold designed step counts around its round capacity, in both geometries."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers
import sddmm_cases as S
from torch_sputnik_amd import capi

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
KNOB_NAMES = ("SPUTNIK_HIP_SDDMM_KERNEL", "SPUTNIK_HIP_SDDMM_FLAT", "SPUTNIK_HIP_SDDMM_DEBUG",
              "SPUTNIK_HIP_SDDMM_SLAB", "SPUTNIK_HIP_SDDMM_PANEL")
PAD = 16        # elements between the replicas of lhs and of rhs
RUNS = S.runs()


@pytest.fixture
def knobs(monkeypatch):
    """Sets the SPUTNIK_HIP_SDDMM_* knobs and has the library read them; restored afterwards."""
    def set_knobs(env):
        for name in KNOB_NAMES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        capi.reload_options()
    yield set_knobs
    monkeypatch.undo()
    capi.reload_options()


def dev():
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def canary_of(dtype):
    return float("nan") if dtype == torch.float32 else S.CANARY_HALF


def kept_canary(t):
    """bool tensor: where `t` still holds its canary."""
    return torch.isnan(t) if t.dtype == torch.float32 else t == (S.CANARY_INT if t.dtype == torch.int32
                                                                 else S.CANARY_HALF)


def guarded(numel, dtype):
    """(buffer, view): `numel` elements with GUARD canary elements on each side."""
    fill = S.CANARY_INT if dtype == torch.int32 else canary_of(dtype)
    buf = torch.full((S.GUARD + numel + S.GUARD,), fill, dtype=dtype, device=dev())
    return buf, buf[S.GUARD:S.GUARD + numel]


def guards_intact(buf, numel):
    return bool(kept_canary(buf[:S.GUARD]).all()) and bool(kept_canary(buf[S.GUARD + numel:]).all())


def strided(x, dtype):
    """[R, rows, k] float32 numpy -> (flat device buffer in `dtype` with PAD elements of NaN behind
    every replica, stride in elements, the stored values as float32 numpy)."""
    replicas, rows, k = x.shape
    stride = rows * k + PAD
    buf = torch.full((replicas * stride,), float("nan"), dtype=dtype, device=dev())
    stored = torch.from_numpy(x).to(dev()).to(dtype)
    buf.view(replicas, stride)[:, :rows * k] = stored.reshape(replicas, rows * k)
    return buf, stride, stored.float().cpu().numpy()


class Problem:
    """A run's topology and operands on the device, its float64 reference, and its calls."""

    def __init__(self, run, integers=False):
        self.run, self.case, self.config = run, run.case, run.config
        c = self.case
        self.in_dtype, self.out_dtype = DTYPES[self.config.in_type], DTYPES[self.config.out_type]
        self.ri, self.ro, self.ci = (torch.from_numpy(a).to(dev()) for a in c.csr)
        lhs, rhs = S.operands(run, integers=integers)
        self.lhs, self.lhs_stride, lhs_stored = strided(lhs, self.in_dtype)
        self.rhs, self.rhs_stride, rhs_stored = strided(rhs, self.in_dtype)
        self.want = S.reference(c.row_offsets, c.column_indices, lhs_stored, rhs_stored,
                                summed=self.config.summed)
        self.model = S.workspace_model(*c.csr, c.m, c.n, self.config.rows)

    def workspace(self):
        c, k = self.case, self.config.k
        query = capi.sddmm_sum_workspace_bytes if self.config.summed else capi.sddmm_workspace_bytes
        nbytes = query(c.m, k, c.n, c.nnz)
        assert nbytes > 0 and nbytes % 4 == 0 and nbytes // 4 >= len(self.model[0])
        return guarded(nbytes // 4, torch.int32)

    def plan(self):
        c, k = self.case, self.config.k
        buf, ws = self.workspace()
        fn = capi.lib().sputnik_hip_sddmm_sum_plan if self.config.summed else capi.lib().sputnik_hip_sddmm_plan
        status = fn(c.m, k, c.n, c.nnz, _p(self.ri), _p(self.ro), _p(self.ci), _p(ws),
                    ws.numel() * 4, _stream())
        assert status == 0, status
        self.check_plan(buf, ws)
        return buf, ws

    def check_plan(self, buf, ws):
        words, defined = self.model
        got = ws[:len(words)].cpu().numpy()
        wrong = np.nonzero((got != words) & defined)[0]
        assert wrong.size == 0, (self.run.id, "plan differs from the model at words", wrong[:8],
                                 got[wrong[:8]], words[wrong[:8]])
        assert guards_intact(buf, ws.numel()), (self.run.id, "a guard of the workspace moved")

    def launch(self, planned, ws_pair=None, entry="typed"):
        """The product into a fresh guarded output: float [R, nnz] (summed: [nnz]) of the bits
        written, after every canary check."""
        c, config = self.case, self.config
        if ws_pair is None:
            ws_pair = self.workspace()
        ws_buf, ws = ws_pair
        lib = capi.lib()
        head = (c.m, config.k, c.n, c.nnz, self.run.replicas, _p(self.ri), _p(self.ro), _p(self.ci),
                _p(self.lhs), self.lhs_stride, _p(self.rhs), self.rhs_stride)
        if config.summed:
            parts = self.run.replicas * config.panels_on_z
            scratch_bytes = capi.sddmm_sum_scratch_bytes(c.m, config.k, c.n, c.nnz, self.run.replicas)
            assert scratch_bytes >= 4 * parts * c.nnz
            sbuf, scratch = guarded(scratch_bytes // 4, torch.float32)
            obuf, out = guarded(c.nnz, torch.float32)
            if entry == "batched":
                fn = lib.sputnik_hip_sddmm_sum_batched_planned if planned else lib.sputnik_hip_sddmm_sum_batched
                status = fn(*head, _p(out), _p(ws), ws.numel() * 4, _p(scratch), scratch_bytes, _stream())
            else:
                status = lib.sputnik_hip_sddmm_sum_typed(
                    *head, capi.TYPE_CODES[self.in_dtype], _p(out), _p(ws), ws.numel() * 4, int(planned),
                    _p(scratch), scratch_bytes, _stream())
            assert status == 0, (self.run.id, status)
            assert guards_intact(sbuf, scratch.numel()), (self.run.id, "a guard of the scratch moved")
            assert not bool(kept_canary(scratch[:parts * c.nnz]).any()), (self.run.id, "a partial product is missing")
            assert bool(kept_canary(scratch[parts * c.nnz:]).all()), (self.run.id, "written behind the partial vectors")
            assert guards_intact(obuf, c.nnz) and not bool(kept_canary(out).any()), (self.run.id, "out")
            result = out.clone()
        else:
            stride = c.nnz + 3
            obuf, out = guarded(self.run.replicas * stride, self.out_dtype)
            if entry == "batched":
                fn = lib.sputnik_hip_sddmm_batched_planned if planned else lib.sputnik_hip_sddmm_batched
                status = fn(*head, _p(out), stride, _p(ws), ws.numel() * 4, _stream())
            else:
                status = lib.sputnik_hip_sddmm_typed(
                    *head, capi.TYPE_CODES[self.in_dtype], _p(out), stride, capi.TYPE_CODES[self.out_dtype],
                    _p(ws), ws.numel() * 4, int(planned), _stream())
            assert status == 0, (self.run.id, status)
            rows = out.view(self.run.replicas, stride)
            assert guards_intact(obuf, out.numel()), (self.run.id, "a guard of out moved")
            assert not bool(kept_canary(rows[:, :c.nnz]).any()), (self.run.id, "an output element was not written")
            assert bool(kept_canary(rows[:, c.nnz:]).all()), (self.run.id, "written between the replicas' outputs")
            result = rows[:, :c.nnz].clone()
        if not planned:
            self.check_plan(ws_buf, ws)     # (the call planned for itself)
        else:
            assert guards_intact(ws_buf, ws.numel())
        return result

    def error(self, got):
        c = self.case
        got = got.float().cpu().numpy().astype(np.float64)
        want = self.want
        if self.config.summed:
            got, want = got[None], want[None]
        if self.out_dtype != torch.float32:
            return helpers.half_err(got, want, self.out_dtype, c.row_offsets)
        return helpers.rel_err(got, want, c.row_offsets)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int16 if a.element_size() == 2
                                                                      else torch.int32) ==
                                                               b.view(torch.int16 if b.element_size() == 2
                                                                      else torch.int32)).all())


def assert_route(run, walked, planned):
    c, config = run.case, run.config
    got = capi.sddmm_launch_shape(c.m, config.k, c.n, c.nnz, run.replicas, DTYPES[config.in_type],
                                  DTYPES[config.out_type], planned=planned, summed=config.summed)
    assert got == run.launch_shape(walked), (run.id, walked, planned, got)
    return got


@pytest.mark.parametrize("run", RUNS, ids=lambda run: run.id)
def test_instance_at_its_edges(run, knobs):
    config = run.config
    float32_entries = config.in_type == "float32"
    # 1. the route, before anything is launched
    for walked in (False, True) if run.walked_y else (False,):
        knobs(config.knobs(walked))
        for planned in (False, True):
            shape = assert_route(run, walked, planned)
        if walked:
            assert shape["grid_y"] == run.walked_y < shape["row_blocks"]
    knobs(config.knobs(False))
    problem = Problem(run)
    # 2. the plan against the model, in a guarded workspace
    plan = problem.plan()
    # 3. planned and unplanned, every canary checked; 4. identical bits
    planned = problem.launch(True, plan)
    unplanned = problem.launch(False)
    assert same_bits(planned, unplanned), (run.id, "planned and unplanned differ")
    if float32_entries:     # (the float32 entry points of the C interface: the same path)
        assert same_bits(planned, problem.launch(True, plan, entry="batched")), run.id
        assert same_bits(planned, problem.launch(False, entry="batched")), run.id
    if run.walked_y:
        knobs(config.knobs(True))
        assert_route(run, True, True)
        walked = problem.launch(True, plan)
        differ = (walked.float() != planned.float()) | (walked.isnan() != planned.isnan())
        assert same_bits(walked, planned), (run.id, "walked and unwalked differ at", differ.nonzero()[:8].tolist())
        assert same_bits(problem.launch(False), planned), (run.id, "walked, unplanned")
    # 5. float64
    err = problem.error(planned)
    print(f"{run.id}: error {err:.3e} of 1e-4")
    assert err < 1e-4, (run.id, err)


EXACT_RUNS = [run for run in RUNS if run.case_name == "edges_1283x313_identity_last1" and run.walked_y == 5
              and run.config.out_type == "float32" and run.config.name in (
                  "float32_float32_plain_k384_stationary128x128",
                  "float32_float32_plain_k192_stationary64x256_knob8",
                  "float32_float32_sum_k512_stationary256x80",
                  "float32_float32_plain_k192_quad64x256",
                  "float16_float32_plain_k192_quad64x256",
                  "bfloat16_float32_plain_k512_quad256x64",
                  "bfloat16_float32_sum_k512_quad256x80")]


def test_exact_runs_are_all_there():
    assert len(EXACT_RUNS) == 7
    assert {(r.config.family, r.config.in_type == "float32") for r in EXACT_RUNS} == {
        ("stationary", True), ("quad", True), ("quad", False)}
    assert sum(r.config.passes > 1 for r in EXACT_RUNS) >= 4      # walked accumulating runs


@pytest.mark.parametrize("run", EXACT_RUNS, ids=lambda run: run.id)
def test_small_integers_give_the_exact_products(run, knobs):
    """|x| <= 4: every product and every sum is an integer that float32 holds (at most 16 k), so
    the result must EQUAL the float64 reference -- an entry added twice, or a panel left out or
    overwritten, shows as a whole number's difference.  Walked and unwalked."""
    problem = Problem(run, integers=True)
    assert np.abs(problem.want).max() <= 16 * run.config.k * (run.replicas if run.config.summed else 1) < 2 ** 24
    for walked in (False, True):
        knobs(run.config.knobs(walked))
        assert_route(run, walked, False)
        got = problem.launch(False).cpu().numpy().astype(np.float64)
        wrong = np.argwhere(got != problem.want)
        assert wrong.size == 0, (run.id, walked, wrong[:8].tolist())


@functools.lru_cache(maxsize=None)
def many_mask_batch():
    """Three masks of 523 x 313 with different entry counts in the flat many-mask layout; the
    first (rows by length) and the second (identity) hold unsorted rows."""
    masks = [S.case("edges_523x313_by_length_last2", 256),
             S.designed_case("many_523x313_identity", 523, 313, 256, "identity", "last1", 21),
             S.Case("many_523x313_thin", np.random.default_rng(22).random((523, 313)) < 0.03, None, "by_length")]
    assert len({c.nnz for c in masks}) == 3 and all(c.nnz >= 4 * c.m for c in masks)
    return masks


def test_many_masks_with_and_without_the_walk_knob(knobs):
    masks = many_mask_batch()
    m, n, k, heads, replicas = 523, 313, 64, 2, 6
    counts = [c.nnz for c in masks]
    largest = max(counts)
    ri = torch.from_numpy(np.concatenate([c.row_indices for c in masks])).to(dev())
    ro = torch.from_numpy(np.concatenate([c.row_offsets for c in masks])).to(dev())
    ci = torch.from_numpy(np.concatenate([c.column_indices for c in masks])).to(dev())
    rng = np.random.default_rng(23)
    lhs = torch.from_numpy(rng.uniform(-1, 1, (replicas, m, k)).astype(np.float32)).to(dev())
    rhs = torch.from_numpy(rng.uniform(-1, 1, (replicas, n, k)).astype(np.float32)).to(dev())
    entries = helpers.many_mask_entries(counts, ro, ci, m, heads, dev())
    width = largest + 3
    want = helpers.ref_sddmm_many_mask(entries, width, lhs, rhs).cpu().numpy()
    results = []
    for walked in (False, True):
        knobs(dict(S.BASE_KNOBS, **({"SPUTNIK_HIP_SDDMM_DEBUG": str(S.WALK)} if walked else {})))
        shape = capi.sddmm_launch_shape(m, k, n, largest, replicas, mask_heads=heads)
        assert (shape["family"], shape["panel_width"], shape["slab_rows"]) == ("quad", 64, 256), shape
        assert shape["grid_y"] == shape["row_blocks"] == 3 and shape["grid_z"] == replicas, shape
        nbytes = capi.sddmm_many_mask_workspace_bytes(len(masks), m, k, n, largest)
        assert nbytes > 0
        ws_buf, ws = guarded(nbytes // 4, torch.int32)
        obuf, out = guarded(replicas * width, torch.float32)
        capi.sddmm_many_mask(len(masks), m, k, n, counts, replicas, ri, ro, ci, lhs, rhs,
                             out.view(replicas, width), ws)
        assert guards_intact(ws_buf, ws.numel()) and guards_intact(obuf, out.numel())
        rows = out.view(replicas, width)
        # every mask's plan region against the model
        region = nbytes // 4 // len(masks)
        for i, c in enumerate(masks):
            words, defined = S.workspace_model(*c.csr, m, n, 256)
            got = ws[i * region:i * region + len(words)].cpu().numpy()
            assert not ((got != words) & defined).any(), (i, "plan")
        for r in range(replicas):
            count = counts[r // heads]
            assert not bool(torch.isnan(rows[r, :count]).any()) and bool(torch.isnan(rows[r, count:]).all()), r
            err = helpers.rel_err(rows[r, :count].cpu().numpy()[None], want[r, :count][None],
                                  masks[r // heads].row_offsets)
            assert err < 1e-4, (r, walked, err)
        results.append(rows.clone())
    assert same_bits(results[0], results[1])


OPS_RUNS = [run for run in RUNS if run.config.name in ("float32_float32_plain_k192_quad64x256",
                                                       "float32_float32_plain_k768_stationary256x128")
            and run.case_name in ("edges_779x313_permuted_last33", "edges_203xslab+1_identity_last_empty")]


@pytest.mark.parametrize("run", OPS_RUNS, ids=lambda run: run.id)
def test_torch_ops_entry(run, knobs):
    """torch.ops.torch_sputnik.sddmm on contiguous operands under the run's knobs: the bits of the
    C entry point, within the float64 bound."""
    import torch_sputnik as ts
    assert len(OPS_RUNS) == 4
    c, config = run.case, run.config
    knobs(config.knobs(False))
    assert_route(run, False, False)
    problem = Problem(run)
    lhs, rhs = S.operands(run)
    got = ts.sddmm(c.m, c.n, problem.ri, problem.ro, problem.ci, torch.from_numpy(lhs).to(dev()),
                   torch.from_numpy(rhs).to(dev()))
    assert got.shape == (run.replicas, c.nnz)
    assert problem.error(got) < 1e-4
    assert same_bits(got.contiguous(), problem.launch(False))


# ---------------------------------------------------------------------------
# the pair-flat kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("run", S.flat_runs(), ids=lambda run: run.id)
def test_pair_flat_kernel_at_its_round_edges(run, knobs):
    """Planned calls on the mask whose tiles hold 0, 1, fewer than the compute waves, kCap - 1,
    kCap, kCap + 1 and 2 kCap + 1 steps (tests/test_sddmm_cases_cpu.py counts them): the plan's
    tile_start words must give exactly those step counts, the product is guarded and strided
    like every other run, held to float64 -- and, on float32 outputs, to the exact integers."""
    c, config = run.case, run.config
    g = S.FLAT_GEOMETRIES[config.flat]
    knobs(config.knobs(False))
    assert_route(run, False, True)
    problem = Problem(run)
    plan = problem.plan()
    # the pair-flat plan sits behind the tables (256-byte aligned): steps before every tile, all
    # steps, the geometry's tag
    steps = S.flat_steps(c, config.flat).reshape(-1)
    first = len(problem.model[0])
    assert first * 4 % 256 == 0
    words = plan[1][first:first + len(steps) + 2].cpu().numpy()
    assert np.array_equal(np.diff(words[:len(steps) + 1]), steps) and words[0] == 0, (run.id, words, steps)
    assert words[len(steps) + 1] == (g["block"] << 16) | (g["slab"] << 4) | 0x5
    got = problem.launch(True, plan)
    assert same_bits(got, problem.launch(True, plan)), (run.id, "not repeatable")
    err = problem.error(got)
    print(f"{run.id}: error {err:.3e} of 1e-4")
    assert err < 1e-4, (run.id, err)
    if config.out_type == "float32":
        exact = Problem(run, integers=True)
        result = exact.launch(True, plan).cpu().numpy().astype(np.float64)
        wrong = np.argwhere(result != exact.want)
        assert wrong.size == 0, (run.id, wrong[:8].tolist())
