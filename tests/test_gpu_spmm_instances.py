"""GPU: every instance of the LDS-tiled SpMM kernels that share chunk_table_body -- the eight of
spmm_tiled_kernel<Cfg, SPARSE> (csrc/spmm_tiled.hip), spmm_tiled64_kernel unsplit and with its K
split (csrc/spmm_tiled64.hip) -- at its chunk and window edges, on the run list of
tests/spmm_cases.py (tests/test_spmm_cases_cpu.py proves what the list reaches).  Per run:

  1. the route is asserted with capi.spmm_launch_shape before any launch, under the run's knobs;
  2. sputnik_hip_spmm_plan writes into a workspace inside a buffer of canary ints; the tables at
     the offsets the query reports are compared with the numpy model bit for bit on the defined
     words, and every other word of the workspace must still be a canary;
  3. the product runs through sputnik_hip_spmm_batched_planned, _batched and _bias_batched into
     `out`, a slice of a NaN-filled buffer with out_stride = m * n + 16 and 16 guard elements on
     each side, on a dense operand with replica strides of k * n + 16 elements and NaN in the
     gaps: every element is written, no NaN inside survives, none outside moves; the partial
     tiles of a K split are all written and the workspace behind them stays untouched;
  4. bits: every call is made twice for identical bits; planned == unplanned; the same matrix
     under a second row order gives the same bits (a row is one chain of fmaf in storage order on
     the staged and on the gathered path alike, whichever workgroup, wave and wave-row holds it);
     the bias / ReLU entry equals max(product + bias, 0) of those bits (the epilogue is one add
     and one max behind the sum);
  5. the result is held to float64 at the suite's bound, rel_err < 1e-4.  A K split adds its
     partial tiles in another order than the unsplit walk: it is held to float64 only.

Small-integer operands must give exactly the integer products on every kernel body and on the
split; two runs go through torch.ops.torch_sputnik.spmm for the C entry's bits; one shape without
knobs checks the side-by-side tables of a plan made without the replica count."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import sddmm_cases as S
import spmm_cases as C
from torch_sputnik_amd import capi

pytestmark = pytest.mark.gpu

KNOB_NAMES = ("SPUTNIK_HIP_SPMM_KERNEL", "SPUTNIK_HIP_SPMM_SPARSE", "SPUTNIK_HIP_SPMM_MEDIUM",
              "SPUTNIK_HIP_SPMM_DEBUG")
PAD = 16        # elements between the replicas of the dense operand and of the output
RUNS = C.runs()
WORST = {"rel_err": 0.0, "run": None}


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
    fill = C.CANARY_INT if dtype == torch.int32 else float("nan")
    buf = torch.full((C.GUARD + numel + C.GUARD,), fill, dtype=dtype, device=dev())
    return buf, buf[C.GUARD:C.GUARD + numel]


def kept_canary(t):
    return t == C.CANARY_INT if t.dtype == torch.int32 else torch.isnan(t)


def guards_intact(buf, numel):
    return bool(kept_canary(buf[:C.GUARD]).all()) and bool(kept_canary(buf[C.GUARD + numel:]).all())


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def query(run, c=None):
    c = run.case if c is None else c
    return capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 4 if run.out_offset % 4 else 16)


class Problem:
    """A run's topology and operands on the device, its float64 reference, and its calls."""

    def __init__(self, run, integers=False, other_order=False):
        self.run, self.case, self.other = run, run.case, other_order
        c = self.case
        ri = c.other_order() if other_order else c.row_indices
        self.ri, self.ro, self.ci = (torch.from_numpy(np.ascontiguousarray(a)).to(dev())
                                     for a in (ri, c.row_offsets, c.column_indices))
        values, dense, bias = C.operands(run, integers=integers)
        self.host = (values, dense, bias)
        self.values = torch.from_numpy(values).to(dev())
        self.values_stride = 0 if run.shared else c.nnz
        self.dense_stride = c.k * run.n + PAD
        self.dense = torch.full((run.replicas * self.dense_stride,), float("nan"), device=dev())
        self.dense.view(run.replicas, self.dense_stride)[:, :c.k * run.n] = \
            torch.from_numpy(dense).to(dev()).reshape(run.replicas, -1)
        self.bias = torch.from_numpy(bias).to(dev())
        self.shape = query(run)
        self.model = C.plan_words(run.case_name, run.bk, other_order)

    def want(self):
        values, dense, _ = self.host
        return C.reference(self.case.row_offsets, self.case.column_indices, values, dense)

    def workspace(self):
        nbytes = self.shape["workspace_bytes"]
        assert nbytes > 0 and nbytes % 4 == 0
        return guarded(nbytes // 4, torch.int32)

    def tables(self, ws):
        first = self.shape["row_ok_offset"] // 4
        return ws[first:first + len(self.model[0])]

    def check_plan(self, buf, ws, product_ran):
        """The tables equal the model; what lies outside them is untouched -- but for the partial
        tiles of a K split once a product has run, which must then all be written."""
        words, defined = self.model
        got = self.tables(ws).cpu().numpy()
        wrong = np.nonzero((got != words) & defined)[0]
        assert wrong.size == 0, (self.run.id, "plan differs from the model at words", wrong[:8],
                                 got[wrong[:8]], words[wrong[:8]])
        assert self.shape["table_offset"] // 4 == self.shape["row_ok_offset"] // 4 + S.row_ok_ints(self.shape["slots"])
        assert guards_intact(buf, ws.numel()), (self.run.id, "a guard of the workspace moved")
        first = self.shape["row_ok_offset"] // 4
        end = first + len(words)
        assert bool(kept_canary(ws[:first]).all()), (self.run.id, "written in front of the tables")
        splits = self.shape["ksplits"]
        if product_ran and splits > 1:
            at = self.shape["partials_offset"] // 4
            count = splits * self.case.m * self.run.n
            assert bool(kept_canary(ws[end:at]).all()), (self.run.id, "written between tables and partial tiles")
            assert not bool(kept_canary(ws[at:at + count]).any()), (self.run.id, "a partial tile element is missing")
            end = at + count
        assert bool(kept_canary(ws[end:]).all()), (self.run.id, "written behind the tables / partial tiles")

    def plan(self):
        c = self.case
        buf, ws = self.workspace()
        status = capi.lib().sputnik_hip_spmm_plan(c.m, c.k, self.run.n, c.nnz, _p(self.ri), _p(self.ro), _p(self.ci),
                                                  _p(ws), ws.numel() * 4, _stream())
        assert status == 0, status
        self.check_plan(buf, ws, product_ran=False)
        return buf, ws

    def launch(self, entry, ws_pair=None, bias=None, relu=False):
        """One product into a fresh guarded output: float [R, m, n] of the bits written, after
        every canary check.  entry: "planned" (on ws_pair), "batched" or "bias" (plan for
        themselves into a fresh guarded workspace)."""
        c, run = self.case, self.run
        planned = entry == "planned"
        ws_buf, ws = ws_pair if planned else self.workspace()
        size = c.m * run.n
        stride = size + PAD
        obuf, view = guarded(run.out_offset + run.replicas * stride, torch.float32)
        out = view[run.out_offset:]
        assert out.data_ptr() % 16 == (4 * run.out_offset) % 16
        lib = capi.lib()
        head = (c.m, c.k, run.n, c.nnz, run.replicas, _p(self.ri), _p(self.values), self.values_stride,
                _p(self.ro), _p(self.ci), _p(self.dense), self.dense_stride)
        tail = (_p(out), stride, _p(ws), ws.numel() * 4, _stream())
        if entry == "bias":
            status = lib.sputnik_hip_spmm_bias_batched(*head, _p(bias), int(relu), *tail)
        elif planned:
            status = lib.sputnik_hip_spmm_batched_planned(*head, *tail)
        else:
            status = lib.sputnik_hip_spmm_batched(*head, *tail)
        assert status == 0, (run.id, entry, status)
        rows = out.view(run.replicas, stride)
        assert guards_intact(obuf, view.numel()), (run.id, entry, "a guard of out moved")
        assert bool(torch.isnan(view[:run.out_offset]).all()), (run.id, entry, "written in front of out")
        assert not bool(torch.isnan(rows[:, :size]).any()), (run.id, entry, "an output element was not written")
        assert bool(torch.isnan(rows[:, size:]).all()), (run.id, entry, "written between the replicas' outputs")
        self.check_plan(ws_buf, ws, product_ran=True)
        return rows[:, :size].reshape(run.replicas, c.m, run.n).clone()

    def twice(self, entry, ws_pair=None, **kw):
        first = self.launch(entry, ws_pair, **kw)
        assert same_bits(first, self.launch(entry, ws_pair, **kw)), (self.run.id, entry, "not repeatable")
        return first

    def error(self, got, want=None):
        want = self.want() if want is None else want
        return helpers.rel_err(got.cpu().numpy().astype(np.float64), want)


def assert_route(run):
    got = query(run)
    assert got == run.launch_shape(), (run.id, got)
    return got


@pytest.mark.parametrize("run", RUNS, ids=lambda run: run.id)
def test_instance_at_its_edges(run, knobs):
    # 1. the route, before anything is launched
    knobs(run.knobs())
    assert_route(run)
    problem = Problem(run)
    # 2. the plan against the model, in a guarded workspace
    plan = problem.plan()
    # 3. planned and unplanned, every canary checked; 4. identical bits
    planned = problem.twice("planned", plan)
    unplanned = problem.twice("batched")
    assert same_bits(planned, unplanned), (run.id, "planned and unplanned differ")
    # the bias entry: what the run asks for; every run that asks for none takes bias + ReLU
    bias, relu = (run.bias, run.relu) if run.form == "narrow_split" else (True, True)
    with_bias = problem.twice("bias", bias=problem.bias if bias else None, relu=relu)
    derived = planned + problem.bias[None, :, None] if bias else planned
    derived = torch.clamp_min(derived, 0.0) if relu else derived
    assert torch.equal(with_bias, derived), (run.id, "the epilogue is not max(product + bias, 0)")
    # the same matrix under a second row order
    other = Problem(run, other_order=True)
    assert other.shape == problem.shape
    reordered = other.launch("planned", other.plan())
    if run.ksplits() == 1:
        differ = (reordered != planned).nonzero()[:4].tolist()
        assert same_bits(reordered, planned), (run.id, "the row order changes the bits at", differ)
    # 5. float64
    want = problem.want()
    for name, got in (("planned", planned), ("reordered", reordered))[:2 if run.ksplits() > 1 else 1]:
        err = problem.error(got, want)
        if err > WORST["rel_err"]:
            WORST.update(rel_err=err, run=run.id)
        print(f"{run.id} {name}: error {err:.3e} of 1e-4 (worst so far {WORST['rel_err']:.3e})")
        assert err < 1e-4, (run.id, name, err)


def test_an_output_off_16_byte_alignment_takes_no_split(knobs):
    """The run whose `out` is off 16-byte alignment takes no split (asserted by the query) and
    must give the bits of the unsplit kernel on the same operands."""
    unaligned = [run for run in RUNS if run.out_offset]
    assert len(unaligned) == 1
    run = unaligned[0]
    aligned = C.Run("narrow_unsplit", run.case_name, run.n, 1, shared=False)
    knobs(run.knobs())
    assert assert_route(run)["ksplits"] == 1 and run.splits > 1
    got = Problem(run).launch("batched")
    knobs(aligned.knobs())
    assert same_bits(got, Problem(aligned).launch("batched"))


EXACT_IDS = ("large_short-edges_1283", "large_long-edges_1283", "medium_short-edges_523", "medium_long-pad_203",
             "small_short-edges_779", "small_long-edges_524", "wide512_short-edges_1283",
             "wide512half_short-edges_523", "narrow_unsplit-edges_1283", "narrow_unsplit-pad_197",
             "narrow_split-edges_523_permuted_last2-n64-r1-split2", "narrow_split-edges_523_permuted_last2-n72-r1-split4",
             "narrow_split-edges_779_identity_k276-n132-r1-split3", "narrow_split-pad_203_identity-n72-r1-split8")
EXACT_RUNS = [run for run in RUNS if run.id.startswith(EXACT_IDS)]


def test_exact_runs_are_all_there():
    assert len(EXACT_RUNS) == len(EXACT_IDS), [run.id for run in EXACT_RUNS]
    assert {run.form for run in EXACT_RUNS} == set(C.FORMS)


@pytest.mark.parametrize("run", EXACT_RUNS, ids=lambda run: run.id)
def test_small_integers_give_the_exact_products(run, knobs):
    """Values +-1..3, dense -4..4: every product and every partial sum is an integer that float32
    holds (at most 12 k), so the result must EQUAL the float64 reference in any order of
    summation -- an entry taken twice, left out, or taken with its neighbour's column shows as a
    whole number's difference.  The K split too."""
    knobs(run.knobs())
    assert_route(run)
    problem = Problem(run, integers=True)
    want = problem.want()
    assert np.abs(want).max() <= 12 * run.case.k < 2 ** 24
    got = problem.launch("batched").cpu().numpy().astype(np.float64)
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, (run.id, wrong[:8].tolist())


OPS_IDS = ("small_short-edges_523_permuted_last2", "narrow_split-edges_779_identity_k276-n132-r1-split3")
OPS_RUNS = [run for run in RUNS if run.id.startswith(OPS_IDS)]


@pytest.mark.parametrize("run", OPS_RUNS, ids=lambda run: run.id)
def test_torch_ops_entry(run, knobs):
    """torch.ops.torch_sputnik.spmm on contiguous operands under the run's knobs: the bits of the
    C entry point, within the float64 bound."""
    import torch_sputnik as ts
    assert len(OPS_RUNS) == 2 and not any(r.shared for r in OPS_RUNS)
    c = run.case
    knobs(run.knobs())
    assert_route(run)
    problem = Problem(run)
    values, dense, _ = problem.host
    v, d = torch.from_numpy(values).to(dev()), torch.from_numpy(dense).to(dev())
    if run.replicas == 1:
        v, d = v[0], d[0]
    got = ts.spmm(c.m, c.k, v, problem.ri, problem.ro, problem.ci, d).reshape(run.replicas, c.m, run.n)
    assert problem.error(got) < 1e-4
    assert same_bits(got.contiguous(), problem.launch("batched"))


def sorted_tables(c, bk, per, slots):
    """(row_ok, table) of a matrix whose rows are all sorted, vectorised."""
    rows = S.slot_rows(c.row_indices, c.m, per)
    ro = c.row_offsets.astype(np.int64)
    nchunks = C.ceil_div(c.k, bk)
    keys = np.repeat(np.arange(c.m), np.diff(ro)) * (nchunks + 1) + c.column_indices // bk
    # entries of row r in chunks < ch: searchsorted over (row, chunk) keys
    bounds = np.searchsorted(keys, np.arange(c.m)[:, None] * (nchunks + 1) + np.arange(nchunks + 1)[None, :])
    table = np.zeros((nchunks + 1, slots), dtype=np.int32)
    table[:, rows >= 0] = bounds[rows[rows >= 0]].T
    return np.ones(slots, dtype=np.int32), table


def test_a_plan_without_the_replica_count_carries_both_tables(knobs):
    """No knob: 2048 x 2048 x 256 at density 0.2 goes to the 64-column kernel with 4 replicas and
    to the 256-column kernel (128-row tile) with 16.  One plan made without the replica count must
    hold both kernels' tables at the offsets the query reports, and serve both calls."""
    knobs({})
    m = k = 2048
    n = 256
    dense_mask = np.random.default_rng(3).random((m, k)) < 0.2
    c = C.Case("auto_2048", dense_mask, None, "by_length")
    narrow, wide = (capi.spmm_launch_shape(m, k, n, c.nnz, r) for r in (4, 16))
    assert (narrow["family"], wide["family"], wide["tile_rows"], wide["sparse"]) == ("narrow64", "wide256", 128, True)
    assert wide["row_ok_offset"] == 0 < narrow["row_ok_offset"] and narrow["ksplits"] == 1
    ri, ro, ci = (torch.from_numpy(a).to(dev()) for a in c.csr)
    buf, ws = guarded(wide["workspace_bytes"] // 4, torch.int32)
    assert capi.lib().sputnik_hip_spmm_plan(m, k, n, c.nnz, _p(ri), _p(ro), _p(ci), _p(ws), ws.numel() * 4,
                                            _stream()) == 0
    for shape, bk, per in ((wide, 64, 256), (narrow, 128, 128)):
        row_ok, table = sorted_tables(c, bk, per, shape["slots"])
        got_ok = ws[shape["row_ok_offset"] // 4:shape["row_ok_offset"] // 4 + shape["slots"]].cpu().numpy()
        got = ws[shape["table_offset"] // 4:shape["table_offset"] // 4 + table.size].cpu().numpy()
        assert np.array_equal(got_ok, row_ok) and np.array_equal(got, table.reshape(-1)), shape["family"]
    assert guards_intact(buf, ws.numel())
    rng = np.random.default_rng(4)
    values = torch.from_numpy(rng.uniform(-1, 1, c.nnz).astype(np.float32)).to(dev())
    a = torch.zeros(m, k, dtype=torch.float64, device=dev())
    a[torch.from_numpy(dense_mask).to(dev())] = values.double()
    for replicas in (4, 16):
        b = torch.from_numpy(rng.uniform(-1, 1, (replicas, k, n)).astype(np.float32)).to(dev())
        obuf, out = guarded(replicas * m * n, torch.float32)
        status = capi.lib().sputnik_hip_spmm_batched_planned(
            m, k, n, c.nnz, replicas, _p(ri), _p(values), 0, _p(ro), _p(ci), _p(b), k * n, _p(out), m * n,
            _p(ws), ws.numel() * 4, _stream())
        assert status == 0 and guards_intact(obuf, out.numel()) and guards_intact(buf, ws.numel())
        err = helpers.rel_err_torch(out.view(replicas, m, n), a @ b.double())
        assert err < 1e-4, (replicas, err)
