"""GPU: the flat-stream SpMM -- the pre-pass spmm_flat_fill_kernel and the three generated loops
spmm_flat_kernel<0 / 1 / 2> (csrc/spmm_flat.hip, csrc/gen_spmm_flat.py) -- on the run list of
tests/spmm_flat_cases.py (tests/test_spmm_flat_cases_cpu.py proves what the list reaches).  Per run:

  1. the route is asserted with capi.spmm_launch_shape under the run's knobs before any launch;
  2. sputnik_hip_spmm_plan writes into a workspace inside a buffer of canary ints: every byte the
     model defines equals the model, every other byte and both guards are still canary; a
     difference is reported as (group, chunk, field) or (group, window, entry, field); the plan
     is compared again after the products (the main kernel only reads it);
  3. all three loops run through sputnik_hip_spmm_batched_planned on the one plan, and the
     density's own loop through _batched and _bias_batched (bias + ReLU), into `out`, one float
     past 16-byte alignment inside a NaN-filled guarded buffer with replica strides of
     m * n + 3, on a dense operand with strides of k * n + 3 and NaN in the gaps: every element
     is written, no NaN survives inside, nothing moves outside;
  4. bits: every call twice; the three loops agree; planned == unplanned; a second row order
     gives the same bits; bias / ReLU == max(product + bias, 0) of those bits; where n is a
     multiple of 4 the visit-per-row 512-column kernel gives the same bits on the same operands
     (one chain of fused multiply-adds per output element in storage order, on the stream and on
     the order-independent path alike); the forced XCD codes give the bits of code 0;
  5. float64: helpers.rel_err < 1e-4.

Small-integer operands must give exactly the integer products in every loop under every
mapping; one run goes through torch.ops.torch_sputnik.spmm."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import spmm_flat_cases as F
from torch_sputnik_amd import capi

pytestmark = pytest.mark.gpu

KNOB_NAMES = ("SPUTNIK_HIP_SPMM_KERNEL", "SPUTNIK_HIP_SPMM_SPARSE", "SPUTNIK_HIP_SPMM_MEDIUM",
              "SPUTNIK_HIP_SPMM_DEBUG")
RUNS = F.runs()
WORST = {"rel_err": 0.0, "run": None}
CANARY_BYTES = np.array([F.CANARY_INT], dtype=np.int32).view(np.uint8)


@pytest.fixture
def knobs(monkeypatch):
    """Sets the SPUTNIK_HIP_SPMM_* knobs and has the library read them; restored afterwards."""
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
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def guarded(numel, dtype):
    """(buffer, view): `numel` elements with GUARD canary elements on each side."""
    fill = F.CANARY_INT if dtype == torch.int32 else float("nan")
    buf = torch.full((F.GUARD + numel + F.GUARD,), fill, dtype=dtype, device=dev())
    return buf, buf[F.GUARD:F.GUARD + numel]


def kept_canary(t):
    return t == F.CANARY_INT if t.dtype == torch.int32 else torch.isnan(t)


def guards_intact(buf, numel):
    return bool(kept_canary(buf[:F.GUARD]).all()) and bool(kept_canary(buf[F.GUARD + numel:]).all())


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def assert_route(run, knobs, loop=None):
    c = run.case
    knobs(run.knobs(loop))
    got = capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 4)
    assert (got["family"], got["table_offset"]) == ("flat", 0), (run.id, got)
    if loop is not None:
        assert capi.spmm_kernel_name(c.m, c.k, run.n, c.nnz, run.replicas) == f"spmm_flat_kernel<{loop}>"
    return got


class Problem:
    """A run's topology and operands on the device and its calls."""

    def __init__(self, run, integers=False, other_order=False, operands_of=None):
        self.run, self.case = run, run.case
        c = self.case
        ri = c.other_order() if other_order else c.row_indices
        self.ri, self.ro, self.ci = (torch.from_numpy(np.ascontiguousarray(a)).to(dev())
                                     for a in (ri, c.row_offsets, c.column_indices))
        self.model = F.plan(run.case_name, run.n, other_order)
        assert self.model.layout.bytes == capi.spmm_workspace_bytes(c.m, c.k, run.n, c.nnz)
        if run.plan_only:
            return
        if operands_of is not None:         # the same operands under another row order
            for name in ("host", "values", "values_stride", "dense_stride", "dense", "dense_plain", "bias"):
                setattr(self, name, getattr(operands_of, name))
            return
        values, dense, bias = F.operands(run, integers=integers)
        self.host = (values, dense, bias)
        self.values = torch.from_numpy(values).to(dev())
        self.values_stride = 0 if run.shared else c.nnz
        self.dense_stride = c.k * run.n + F.STRIDE_PAD
        self.dense = torch.full((run.replicas * self.dense_stride,), float("nan"), device=dev())
        self.dense_plain = torch.from_numpy(dense).to(dev())
        self.dense.view(run.replicas, self.dense_stride)[:, :c.k * run.n] = self.dense_plain.reshape(run.replicas, -1)
        self.bias = torch.from_numpy(bias).to(dev())

    def want(self):
        values, dense, _ = self.host
        return F.expected(self.run, values, dense)

    def workspace(self):
        return guarded(self.model.layout.bytes // 4, torch.int32)

    def check_plan(self, buf, ws, when):
        model = self.model
        got = ws.cpu().numpy().view(np.uint8)
        want = np.where(model.defined, model.bytes, np.tile(CANARY_BYTES, len(got) // 4))
        wrong = np.nonzero(got != want)[0]
        if wrong.size:
            at = int(wrong[0])
            kind = "differs from the model" if model.defined[at] else "was written but is not part of the plan"
            raise AssertionError((self.run.id, when, f"byte {at} {kind}", model.describe(at),
                                  f"got {got[at // 4 * 4:at // 4 * 4 + 4].tolist()} want {want[at // 4 * 4:at // 4 * 4 + 4].tolist()}",
                                  f"{wrong.size} bytes differ"))
        assert guards_intact(buf, ws.numel()), (self.run.id, when, "a guard of the workspace moved")

    def plan(self):
        c = self.case
        buf, ws = self.workspace()
        status = capi.lib().sputnik_hip_spmm_plan(c.m, c.k, self.run.n, c.nnz, _p(self.ri), _p(self.ro), _p(self.ci),
                                                  _p(ws), ws.numel() * 4, _stream())
        assert status == 0, status
        self.check_plan(buf, ws, "after the pre-pass")
        return buf, ws

    def launch(self, entry, ws_pair=None, relu=False):
        """One product into a fresh guarded output -> float [R, m, n] of the bits written, after
        every canary check.  entry: "planned" (on ws_pair), "batched" or "bias" (plan for
        themselves into a fresh guarded workspace)."""
        c, run = self.case, self.run
        planned = entry == "planned"
        ws_buf, ws = ws_pair if planned else self.workspace()
        size = c.m * run.n
        stride = size + F.STRIDE_PAD
        obuf, view = guarded(F.OUT_OFFSET + run.replicas * stride, torch.float32)
        out = view[F.OUT_OFFSET:]
        assert out.data_ptr() % 16 == 4
        lib = capi.lib()
        head = (c.m, c.k, run.n, c.nnz, run.replicas, _p(self.ri), _p(self.values), self.values_stride,
                _p(self.ro), _p(self.ci), _p(self.dense), self.dense_stride)
        tail = (_p(out), stride, _p(ws), ws.numel() * 4, _stream())
        if entry == "bias":
            status = lib.sputnik_hip_spmm_bias_batched(*head, _p(self.bias), int(relu), *tail)
        elif planned:
            status = lib.sputnik_hip_spmm_batched_planned(*head, *tail)
        else:
            status = lib.sputnik_hip_spmm_batched(*head, *tail)
        assert status == 0, (run.id, entry, status)
        rows = out.view(run.replicas, stride)
        assert guards_intact(obuf, view.numel()), (run.id, entry, "a guard of out moved")
        assert bool(torch.isnan(view[:F.OUT_OFFSET]).all()), (run.id, entry, "written in front of out")
        missing = torch.isnan(rows[:, :size]).nonzero()
        assert missing.numel() == 0, (run.id, entry, "output elements not written (replica, element)", missing[:4].tolist())
        assert bool(torch.isnan(rows[:, size:]).all()), (run.id, entry, "written between the replicas' outputs")
        self.check_plan(ws_buf, ws, f"after {entry}")
        return rows[:, :size].reshape(run.replicas, c.m, run.n).clone()

    def twice(self, entry, ws_pair=None, **kw):
        first = self.launch(entry, ws_pair, **kw)
        assert same_bits(first, self.launch(entry, ws_pair, **kw)), (self.run.id, entry, "not repeatable")
        return first

    def wide512(self):
        """The same operands, aligned and dense-packed, through the visit-per-row 512-column kernel
        (the caller has set its knob)."""
        c, run = self.case, self.run
        got = capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 16)
        assert got["family"] == "wide512", (run.id, got)
        _, ws = guarded(got["workspace_bytes"] // 4, torch.int32)
        obuf, out = guarded(run.replicas * c.m * run.n, torch.float32)
        status = capi.lib().sputnik_hip_spmm_batched(
            c.m, c.k, run.n, c.nnz, run.replicas, _p(self.ri), _p(self.values), self.values_stride, _p(self.ro),
            _p(self.ci), _p(self.dense_plain), c.k * run.n, _p(out), c.m * run.n, _p(ws), ws.numel() * 4, _stream())
        assert status == 0 and guards_intact(obuf, out.numel())
        return out.view(run.replicas, c.m, run.n).clone()


def where_differ(a, b):
    return (a.view(torch.int32) != b.view(torch.int32)).nonzero()[:4].tolist()


@pytest.mark.parametrize("run", RUNS, ids=lambda run: run.id)
def test_flat_run_at_its_edges(run, knobs):
    # 1. the route, before anything is launched
    assert_route(run, knobs)
    problem = Problem(run)
    # 2. the plan against the model, in a guarded workspace
    plan = problem.plan()
    if run.plan_only:
        return
    # 3. the three loops on the one plan; 4. identical bits
    by_loop = []
    for loop in range(3):
        assert_route(run, knobs, loop)
        by_loop.append(problem.twice("planned", plan))
    for loop in (1, 2):
        assert same_bits(by_loop[0], by_loop[loop]), (run.id, f"loop {loop} differs from loop 0 at (replica, row, column)",
                                                      where_differ(by_loop[0], by_loop[loop]))
    planned = by_loop[0]
    assert_route(run, knobs)
    unplanned = problem.twice("batched")
    assert same_bits(planned, unplanned), (run.id, "planned and unplanned differ", where_differ(planned, unplanned))
    with_bias = problem.twice("bias", relu=True)
    derived = torch.clamp_min(planned + problem.bias[None, :, None], 0.0)
    assert torch.equal(with_bias, derived), (run.id, "the epilogue is not max(product + bias, 0)")
    # a second row order of the same matrix
    other = Problem(run, other_order=True, operands_of=problem)
    reordered = other.launch("planned", other.plan())
    assert same_bits(reordered, planned), (run.id, "the row order changes the bits at", where_differ(reordered, planned))
    # the visit-per-row kernel on the same operands
    if run.wide512:
        knobs({"SPUTNIK_HIP_SPMM_KERNEL": "wide512"})
        visit = problem.wide512()
        assert same_bits(visit, planned), (run.id, "the 512-column visit-per-row kernel gives other bits at",
                                           where_differ(visit, planned))
    # 5. float64
    err = helpers.rel_err(planned.cpu().numpy().astype(np.float64), problem.want())
    if err > WORST["rel_err"]:
        WORST.update(rel_err=err, run=run.id)
    print(f"{run.id}: error {err:.3e} of 1e-4 (worst so far {WORST['rel_err']:.3e} in {WORST['run']})")
    assert err < 1e-4, (run.id, err)


def test_forced_xcd_codes_give_the_bits_of_code_0(knobs):
    """Eight column tiles under the forced XCD column codes 0..3 (and code 2 where the row blocks
    do not divide, which must fall to the next mapping): one plan, the same bits."""
    for case_name in ("map_1024x64", "map_256x64"):
        runs = [run for run in RUNS if run.case_name == case_name and run.n == 3588]
        assert runs and all(run.debug & F.XCD_FORCED for run in runs)
        base = F.Run(case_name, 3588, debug=F.xcd(0))
        assert_route(base, knobs)
        problem = Problem(base)
        want = problem.launch("batched")
        for run in runs:
            assert_route(run, knobs)
            got = Problem(run).launch("batched")
            assert same_bits(got, want), (run.id, run.mapping(), where_differ(got, want))


def test_nothing_staged_gives_the_same_plan_bytes(knobs):
    """SPUTNIK_HIP_SPMM_DEBUG bit 0x1000: the fill kernel assembles no group's stream in LDS.  The
    workspace must hold the same bytes as with staging (canaries included)."""
    pair = [run for run in RUNS if run.case_name == "staging_256x352"]
    assert sorted(run.debug for run in pair) == [0, F.STAGE_ALL_OFF]
    got = []
    for run in sorted(pair, key=lambda run: run.debug):
        assert_route(run, knobs)
        problem = Problem(run)
        staged = problem.model.staged(run.debug)
        assert staged.any() != bool(run.debug) and not staged[5]
        _, ws = problem.plan()
        got.append(ws.clone())
    assert torch.equal(got[0], got[1])


EXACT = [(run, loop) for run in RUNS for loop in range(3)
         if run.id.startswith(("counts_248x352-n384", "groups_256x352-n1155", "lengths_256x352-n1152", "unsorted_a",
                               "long_256x2080", "kedge_256x33", "map_")) and not run.plan_only]


def test_exact_runs_cover_every_loop_under_every_mapping():
    assert {(run.mapping(), loop) for run, loop in EXACT} == \
        {(mapping, loop) for mapping in ("xcd1", "xcd2", "xcd3", "eighths", "linear") for loop in range(3)}


@pytest.mark.parametrize("run,loop", EXACT, ids=lambda v: v.id if isinstance(v, F.Run) else f"loop{v}")
def test_small_integers_give_the_exact_products(run, loop, knobs):
    """Values +-1..3, dense -4..4: every product and every partial sum is an integer that float32
    holds, so the result must EQUAL the float64 reference in any order of summation -- an entry
    taken twice, left out, or multiplied with its neighbour's strip shows as a whole number."""
    assert_route(run, knobs, loop)
    problem = Problem(run, integers=True)
    want = problem.want()
    assert np.abs(want).max() <= 12 * run.case.k < 2 ** 24
    got = problem.launch("batched").cpu().numpy().astype(np.float64)
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, (run.id, loop, "(replica, row, column)", wrong[:8].tolist(),
                             got[tuple(wrong[0])], want[tuple(wrong[0])])


def test_torch_ops_entry(knobs):
    """torch.ops.torch_sputnik.spmm on contiguous operands under the flat knob: the bits of the C
    entry point, within the float64 bound."""
    import torch_sputnik as ts
    run = F.Run("groups_256x352", 384, 1, shared=False)
    c = run.case
    assert_route(run, knobs)
    problem = Problem(run)
    got = ts.spmm(c.m, c.k, problem.values[0], problem.ri, problem.ro, problem.ci, problem.dense_plain[0])
    got = got.reshape(1, c.m, run.n).contiguous()
    assert helpers.rel_err(got.cpu().numpy().astype(np.float64), problem.want()) < 1e-4
    assert same_bits(got, problem.launch("batched"))
