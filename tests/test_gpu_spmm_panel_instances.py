"""GPU: every instance of the panel-resident SpMM kernels (csrc/spmm_panel.hip) -- the eight of
spmm_panel64_kernel<MULTI, PERM, TOUT>, the twelve of spmm_panel64_typed_kernel<MULTI, TV, TB>, the
four of spmm_panel64_group_kernel<PERM, TOUT, ACCUM> -- at its panel, window and cut edges, on the
run list of tests/spmm_panel_cases.py (tests/test_spmm_panel_cases_cpu.py proves what the list
reaches).  Per run:

  1. the route is asserted before any launch, under the run's knobs: capi.spmm_launch_shape and
     spmm_kernel_name for the float entries, spmm_typed_kernel_name for the typed one, the
     _supported queries for the permuted, transposing and group entries (which decline three
     panels, k = 1025, although the entries serve them: pinned here);
  2. `out` is a slice of a NaN-filled buffer with replica strides of m * n + 16 and 16 guard
     elements on each side, the dense operand has replica strides of k * n + 16 with NaN in the
     gaps: every element inside is written, nothing outside moves;
  3. small-integer operands (values +-1, +-2, dense -3 .. 3, exact in float16 and bfloat16 too)
     must give EXACTLY the integer product: an entry added twice, dropped, taken from the wrong
     panel, or a fallback that kept its first sums shows as a whole number's difference;
  4. random float operands are held to float64 at the suite's bound, rel_err < 1e-4;
  5. bit equalities.  All of them follow from one fact of the code: a row's sum is ONE chain of
     fmaf in the storage order of its entries, started from +0.  stream_pairs hands entry u of a
     window out in the order u = 0 .. 15, window after window; an entry past the row's end, or
     (CHECK) outside the panel, carries the value 0 and the offset 0, and fmaf(0, b, acc) = acc
     for finite b.  stream_masked does the same with the entries outside the resident panel, pass
     after pass.  So whichever workgroup, wave, quad and lane group holds a row, whether its
     partner rows are long or empty, whether it is cut (pass 0: the entries in front of the cut,
     pass 1: those behind it) or walked with a mask, the chain of a row whose entries are
     PARTITIONED at the boundary is the same; a row that is not goes through the masked walk on
     both paths (the fallback starts again from +0).  The panel holds B's own bits (half
     operands: widened exactly).  Hence:
       * every call made twice gives the same bits;
       * a second row order gives the same bits (the instances that take row_indices);
       * the cut path equals the same call under SPUTNIK_HIP_SPMM_DEBUG=16 (never cut), for
         sorted rows and for a workgroup that falls back alike;
       * permuted(values, perm) equals plain(values[perm]);
       * the transposed store equals the block transposes of the plain product, the bias + ReLU
         entries equal max(product + bias, 0) of those bits (one add and one max behind the sum);
       * the typed kernel on half operands equals the float kernel on the same operands widened;
       * a non-accumulating group equals its products run one by one.
     An accumulating group carries one chain through all its problems, another order than the
     sum of separate products: it is held to the integers and to float64 only.

On the device the cut search is covered only TOGETHER with its check: a wrong cut makes the cut
passes report an entry outside its panel and the workgroup falls back, so the result cannot show
it.  The search alone is proved by the CPU model (test_spmm_panel_cases_cpu.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers
import spmm_panel_cases as P
from torch_sputnik_amd import capi

pytestmark = pytest.mark.gpu

TOL = 1e-4
KNOB_NAMES = ("SPUTNIK_HIP_SPMM_KERNEL", "SPUTNIK_HIP_SPMM_SPARSE", "SPUTNIK_HIP_SPMM_MEDIUM",
              "SPUTNIK_HIP_SPMM_DEBUG")
PAD = 16        # elements between the replicas of the dense operand and of the output
UNSUPPORTED = -2
PANEL_KERNEL = "spmm_panel64_kernel"
RUNS = P.runs()
DTYPES = {P.F32: torch.float32, P.F16: torch.float16, P.BF16: torch.bfloat16}
GROUP_LDS = 512 * 64 * 4 + 64 * 65 * 4      # 144.25 KiB: the panel and the 64-row tile behind it


@pytest.fixture(scope="module", autouse=True)
def enough_lds():
    """The one skip of this file: a device (or partition) that offers a workgroup less LDS than
    the group kernel asks for serves none of these routes."""
    if not capi.lib().sputnik_hip_spmm_group_supported(256, 512, 64, 1, 0, 0):
        pytest.skip(f"the device offers less than the {GROUP_LDS} bytes of LDS the group kernel asks for")


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


def never_cut(run):
    return {**run.knobs(), "SPUTNIK_HIP_SPMM_DEBUG": str(P.DEBUG_NEVER_CUT)}


def dev():
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@functools.lru_cache(maxsize=None)
def topology(name, order):
    """(row_indices, row_offsets, column_indices) of a matrix on the device; order: "own",
    "other" (by length) or "none" (the instances that take contiguous rows)."""
    mat = MATRICES[name]
    ri = {"own": mat.row_indices, "other": mat.other_order(), "none": None}[order]
    return (None if ri is None else T(ri)), T(mat.row_offsets), T(mat.column_indices)


MATRICES = {}
for _run in RUNS:
    for _mat in _run.matrices():
        MATRICES.setdefault(_mat.name, _mat)


def padded_dense(dense, dtype=torch.float32, offset=0):
    """[R, k, n] -> (flat view, stride): replica strides of k * n + PAD elements, NaN in the gaps;
    `offset` elements in front (a pointer off 16-byte alignment)."""
    r, k, n = dense.shape
    stride = k * n + PAD
    buf = torch.full((offset + r * stride,), float("nan"), dtype=dtype, device=dev())
    view = buf[offset:]
    view.view(r, stride)[:, :k * n] = T(dense, dtype).reshape(r, -1)
    return view, stride


class Out:
    """`replicas` outputs of `size` elements in a NaN-filled buffer: strides of size + PAD, GUARD
    elements on each side."""

    def __init__(self, replicas, size):
        self.replicas, self.size, self.stride = replicas, size, size + PAD
        self.buf = torch.full((2 * P.GUARD + replicas * self.stride,), float("nan"), device=dev())
        self.view = self.buf[P.GUARD:P.GUARD + replicas * self.stride]
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def result(self, what):
        """[R, size] of the bits written, after every canary check."""
        rows = self.view.view(self.replicas, self.stride)
        assert bool(torch.isnan(self.buf[:P.GUARD]).all()) and bool(torch.isnan(self.buf[-P.GUARD:]).all()), \
            (what, "a guard of out moved")
        assert not bool(torch.isnan(rows[:, :self.size]).any()), (what, "an output element was not written")
        assert bool(torch.isnan(rows[:, self.size:]).all()), (what, "written between the replicas' outputs")
        return rows[:, :self.size].clone()


def plain(mat, n, replicas, values, values_stride, dense, dense_stride, order="own", bias=None, relu=False):
    """sputnik_hip_spmm_batched / _bias_batched (no workspace: the panel route plans nothing)
    -> [R, m, n]."""
    ri, ro, ci = topology(mat.name, order)
    out = Out(replicas, mat.m * n)
    head = (mat.m, mat.k, n, mat.nnz, replicas, _p(ri), _p(values), values_stride, _p(ro), _p(ci), _p(dense),
            dense_stride)
    if bias is None and not relu:
        status = capi.lib().sputnik_hip_spmm_batched(*head, _p(out.view), out.stride, None, 0, _stream())
    else:
        status = capi.lib().sputnik_hip_spmm_bias_batched(*head, _p(bias), int(relu), _p(out.view), out.stride,
                                                          None, 0, _stream())
    assert status == 0, (mat.name, status)
    return out.result(mat.name).view(replicas, mat.m, n)


def epilogue(product, bias, relu):
    """max(product + bias[row], 0) of a [R, m, n] tensor / array, as the kernels' epilogue."""
    if bias is not None:
        product = product + bias[None, :, None]
    if relu:
        product = torch.clamp_min(product, 0.0) if torch.is_tensor(product) else np.maximum(product, 0.0)
    return product


def stored(product, block_rows):
    """[R, m, n] in the layout the run stores: plain, or [R, m / hd, n, hd]."""
    if not block_rows:
        return product
    r, m, n = product.shape
    if torch.is_tensor(product):
        return product.view(r, m // block_rows, block_rows, n).transpose(2, 3).contiguous()
    return np.ascontiguousarray(P.transposed_layout(product, block_rows))


def unstored(t, block_rows, m, n):
    """Back to [R, m, n] (for the per-row error)."""
    if not block_rows:
        return t.reshape(-1, m, n)
    return t.reshape(-1, m // block_rows, n, block_rows).transpose(2, 3).reshape(-1, m, n)


def error(got, want):
    return helpers.rel_err(got.cpu().numpy().astype(np.float64), want)


def first_differences(got, want):
    return np.argwhere(got != want)[:6].tolist()


# ---------------------------------------------------------------------------
# one matrix: batched, permuted, transposed, typed
# ---------------------------------------------------------------------------
class Single:
    """A run of one matrix on the device: operands (rounded to the run's storage types first: the
    rounded numbers ARE the operands), float64 reference of what the call stores."""

    def __init__(self, run, integers):
        self.run, self.mat = run, run.case
        mat = self.mat
        values, dense, bias = P.operands(mat, run.n, run.replicas, run.shared, seed=len(run.id), integers=integers)
        tv, tb = (DTYPES[t] for t in run.types)
        self.values = T(values, tv)
        self.dense, self.dense_stride = padded_dense(dense, tb)
        self.values_stride = 0 if run.shared else mat.nnz
        self.bias = T(bias) if run.bias else None
        self.perm_host = P.permutation(mat) if run.perm else None
        self.perm = T(self.perm_host) if run.perm else None
        # what the kernel multiplies, widened
        self.values_f = self.values.float()
        self.dense_host = self.dense.view(run.replicas, -1)[:, :mat.k * run.n].float().cpu().numpy() \
            .reshape(run.replicas, mat.k, run.n)
        used = self.values_f.cpu().numpy()
        self.used_values = used[:, self.perm_host] if run.perm else used
        product = P.reference(mat, self.used_values.astype(np.float64), self.dense_host)
        self.want_product = epilogue(product, bias.astype(np.float64) if run.bias else None, run.relu)
        self.want = stored(self.want_product, run.block_rows)

    def route(self):
        run, mat, lib = self.run, self.mat, capi.lib()
        shape = (mat.m, mat.k, run.n, mat.nnz)
        if run.entry == "batched":
            assert capi.spmm_launch_shape(*shape, run.replicas)["family"] == "panel", run.id
            assert capi.spmm_kernel_name(*shape, run.replicas) == PANEL_KERNEL, run.id
        elif run.entry == "typed":
            name = capi.spmm_typed_kernel_name(*shape, run.replicas, DTYPES[run.types[0]], self.values_stride,
                                               DTYPES[run.types[1]])
            assert name == PANEL_KERNEL, (run.id, name)
        elif run.entry == "permuted":   # (three panels: declined by the query, served by the entry)
            assert lib.sputnik_hip_spmm_permuted_supported(*shape) == int(mat.k <= 2 * P.PANEL), run.id
        else:
            assert lib.sputnik_hip_spmm_transposed_out_supported(*shape, run.block_rows) == int(mat.k <= 2 * P.PANEL), run.id

    def launch(self, order="own"):
        """The run's own entry -> [R, ...] in the stored layout."""
        run, mat, lib = self.run, self.mat, capi.lib()
        ri, ro, ci = topology(mat.name, "none" if run.block_rows else order)
        out = Out(run.replicas, mat.m * run.n)
        shape = (mat.m, mat.k, run.n, mat.nnz, run.replicas)
        tail = (_p(ro), _p(ci), _p(self.dense))
        if run.entry == "batched":
            return plain(mat, run.n, run.replicas, self.values, self.values_stride, self.dense, self.dense_stride,
                         order, self.bias, run.relu)
        if run.entry == "permuted":
            status = lib.sputnik_hip_spmm_permuted_batched(*shape, _p(ri), _p(self.values), self.values_stride,
                                                           _p(self.perm), *tail, self.dense_stride, _p(out.view),
                                                           out.stride, _stream())
        elif run.entry == "transposed":
            status = lib.sputnik_hip_spmm_transposed_out_batched(*shape, _p(self.values), self.values_stride,
                                                                 _p(self.perm), *tail, self.dense_stride,
                                                                 _p(self.bias), int(run.relu), run.block_rows,
                                                                 _p(out.view), out.stride, _stream())
        else:
            tv, tb = (capi.TYPE_CODES[DTYPES[t]] for t in run.types)
            status = lib.sputnik_hip_spmm_typed(*shape, _p(ri), _p(self.values), tv, self.values_stride, _p(ro),
                                                _p(ci), _p(self.dense), tb, self.dense_stride, _p(self.bias),
                                                int(run.relu), _p(out.view), out.stride, None, 0, _stream())
        assert status == 0, (run.id, status)
        got = out.result(run.id)
        if run.block_rows:
            return got.view(run.replicas, mat.m // run.block_rows, run.n, run.block_rows)
        return got.view(run.replicas, mat.m, run.n)

    def float_plain(self, order="own", bias=None, relu=False):
        """The float kernel on the same numbers: values[perm] gathered on the host side, half
        operands widened; no epilogue unless asked."""
        run, mat = self.run, self.mat
        values = T(self.used_values)
        dense, stride = padded_dense(self.dense_host)
        return plain(mat, run.n, run.replicas, values, self.values_stride, dense, stride, order, bias, relu)


SINGLE_RUNS = [run for run in RUNS if run.entry in ("batched", "permuted", "transposed", "typed")]


@pytest.mark.parametrize("run", SINGLE_RUNS, ids=lambda run: run.id)
def test_instance_at_its_edges(run, knobs):
    knobs(run.knobs())
    mat = run.case
    # 3. small integers: exactly the integer product
    exact = Single(run, integers=True)
    exact.route()                                                   # 1. before any launch
    assert np.abs(exact.want).max() < 2 ** 24
    got = exact.launch().cpu().numpy().astype(np.float64)
    assert np.array_equal(got, exact.want), (run.id, "integers differ at", first_differences(got, exact.want))
    # 4. random floats against float64; 5. bits
    problem = Single(run, integers=False)
    first = problem.launch()
    assert same_bits(first, problem.launch()), (run.id, "not repeatable")
    err = error(unstored(first, run.block_rows, mat.m, run.n), problem.want_product)
    print(f"{run.id}: {run.label} {run.path()} error {err:.3e} of {TOL:.0e}")
    assert err < TOL, (run.id, err)
    if not run.block_rows:      # the instances that take row_indices: a second row order
        assert same_bits(first, problem.launch("other")), (run.id, "the row order changes the bits")
    if run.entry != "batched":
        # the float kernel on plain operands, then the layout and the epilogue on its bits
        base = problem.float_plain()
        derived = stored(epilogue(base, problem.bias, run.relu), run.block_rows)
        assert torch.equal(first, derived), (run.id, "differs from the plain product's bits")
    else:
        # the bias + ReLU entry on this run's operands
        bias = T(P.operands(mat, run.n, run.replicas, run.shared)[2])
        with_bias = problem.float_plain(bias=bias, relu=True)
        assert torch.equal(with_bias, epilogue(first, bias, True)), (run.id, "the epilogue is not max(product + bias, 0)")
    if run.path() == "cut":     # never cut: the masked walk for every row, the same chains
        knobs(never_cut(run))
        assert same_bits(first, problem.launch()), (run.id, "the cut path and the masked walk differ")


def test_320_row_blocks_are_declined_and_nothing_is_written(knobs):
    """(m, block_rows) = (320, 320): neither a divisor nor a multiple of the workgroup's 256 rows
    (block_rows_ok): the query says no, the entry answers UNSUPPORTED and leaves `out` alone."""
    knobs({"SPUTNIK_HIP_SPMM_KERNEL": "panel"})
    for m, hd in P.TRANSPOSED_DECLINED:
        mat = P.store_case(m)
        MATRICES.setdefault(mat.name, mat)
        n = 64
        assert capi.lib().sputnik_hip_spmm_transposed_out_supported(m, mat.k, n, mat.nnz, hd) == 0
        values, dense, _ = P.operands(mat, n, 1, False)
        _, ro, ci = topology(mat.name, "none")
        d, stride = padded_dense(dense)
        out = Out(1, m * n)
        status = capi.lib().sputnik_hip_spmm_transposed_out_batched(
            m, mat.k, n, mat.nnz, 1, _p(T(values)), mat.nnz, None, _p(ro), _p(ci), _p(d), stride, None, 0, hd,
            _p(out.view), out.stride, _stream())
        torch.cuda.synchronize()
        assert status == UNSUPPORTED and out.untouched()


# ---------------------------------------------------------------------------
# many masks
# ---------------------------------------------------------------------------
MANY_RUNS = [run for run in RUNS if run.entry == "many"]


class Many:
    def __init__(self, run, integers, order="own"):
        self.run, self.mats = run, run.matrices()
        mats, m, k, n = self.mats, run.case.m, run.case.k, run.n
        self.counts = [mat.nnz for mat in mats]
        width = max(self.counts)
        rng = np.random.default_rng(17)
        self.ri = T(np.concatenate([mat.other_order() if order == "other" else mat.row_indices for mat in mats]))
        self.ro = T(np.concatenate([mat.row_offsets for mat in mats]))
        self.ci = T(np.concatenate([mat.column_indices for mat in mats]))
        values = np.full((run.replicas, width), np.nan, dtype=np.float32)     # NaN behind a mask's own entries
        dense = np.zeros((run.replicas, k, n), dtype=np.float32)
        self.want = np.zeros((run.replicas, m, n))
        for r in range(run.replicas):
            mat = mats[r // run.heads]
            v, d, _ = P.operands(mat, n, 1, False, seed=int(rng.integers(1 << 20)), integers=integers)
            values[r, :mat.nnz], dense[r] = v[0], d[0]
            self.want[r] = P.reference(mat, v.astype(np.float64), d)[0]
        self.values, self.width = T(values), width
        self.dense, self.dense_stride = padded_dense(dense)

    def launch(self):
        run, m, k = self.run, self.run.case.m, self.run.case.k
        out = Out(run.replicas, m * run.n)
        counts = (ctypes.c_int * len(self.counts))(*self.counts)
        status = capi.lib().sputnik_hip_spmm_many_mask(
            len(self.mats), m, k, run.n, counts, run.replicas, _p(self.ri), _p(self.values), self.width, _p(self.ro),
            _p(self.ci), _p(self.dense), self.dense_stride, _p(out.view), out.stride, None, 0, _stream())
        assert status == 0, (run.id, status)
        return out.result(run.id).view(run.replicas, m, run.n)


@pytest.mark.parametrize("run", MANY_RUNS, ids=lambda run: run.id)
def test_many_masks_in_one_launch(run, knobs):
    """One launch for all masks (sputnik_hip_spmm_many_mask takes the panel kernel where the
    largest mask's shape is applicable: asserted through the kernel query under the knob)."""
    knobs(run.knobs())
    m, k = run.case.m, run.case.k
    assert len(run.matrices()) > 1 and capi.spmm_kernel_name(m, k, run.n, max(mat.nnz for mat in run.matrices()),
                                                             run.replicas) == PANEL_KERNEL
    exact = Many(run, integers=True)
    got = exact.launch().cpu().numpy().astype(np.float64)
    assert np.array_equal(got, exact.want), (run.id, first_differences(got, exact.want))
    problem = Many(run, integers=False)
    first = problem.launch()
    assert same_bits(first, problem.launch())
    assert same_bits(first, Many(run, integers=False, order="other").launch()), (run.id, "the row order changes the bits")
    err = error(first, problem.want)
    print(f"{run.id}: {run.label} error {err:.3e} of {TOL:.0e}")
    assert err < TOL
    # every replica equals its mask's product run alone
    for r in range(run.replicas):
        mat = problem.mats[r // run.heads]
        if mat.nnz:
            alone = plain(mat, run.n, 1, problem.values[r, :mat.nnz].contiguous(), mat.nnz,
                          *padded_dense(problem.dense.view(run.replicas, -1)[r:r + 1, :k * run.n].cpu().numpy()
                                        .reshape(1, k, run.n)))
            assert same_bits(first[r:r + 1], alone), (run.id, r)
        else:
            assert not bool(first[r].any())     # the empty mask: zeros, all written
    if run.path() == "cut":
        knobs(never_cut(run))
        assert same_bits(first, problem.launch())


# ---------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------
GROUP_RUNS = [run for run in RUNS if run.entry == "group"]


class Group:
    def __init__(self, run, integers, order="own"):
        self.run, self.mats = run, run.matrices()
        g, n, R = run.group, run.n, run.replicas
        self.order = "none" if run.identity else order
        self.values, self.perms, self.dense, self.products = [], [], [], []
        for j, mat in enumerate(self.mats):
            # values [1, nnz] shared by the replicas; a dense operand [R, k, n] per problem, or one for all
            v, d, _ = P.operands(mat, n, R, True, seed=j + 7, integers=integers)
            perm = P.permutation(mat, j) if run.perm else None
            self.values.append(T(v[0]))
            self.perms.append(None if perm is None else T(perm))
            if g["same_dense"] and j > 0:
                self.dense.append(self.dense[0])
            else:
                self.dense.append(padded_dense(d) + (d,))
            used = v[:, perm] if run.perm else v
            self.products.append(P.reference(mat, used.astype(np.float64), self.dense[j][2]))
        self.want = [sum(self.products)] if g["accumulate"] else [stored(p, run.block_rows) for p in self.products]

    def launch(self):
        run, m, k = self.run, self.mats[0].m, self.mats[0].k
        g = run.group
        outs = [Out(run.replicas, m * run.n) for _ in range(1 if g["accumulate"] else g["count"])]
        array = (capi.SpmmProblem * g["count"])()
        for j, (slot, mat) in enumerate(zip(array, self.mats)):
            ri, ro, ci = topology(mat.name, self.order)
            slot.row_indices, slot.row_offsets, slot.column_indices = (_p(x).value for x in (ri, ro, ci))
            slot.values, slot.value_permutation = _p(self.values[j]).value, _p(self.perms[j]).value
            slot.dense, slot.out = _p(self.dense[j][0]).value, _p(outs[0 if g["accumulate"] else j].view).value
            slot.nonzeros = mat.nnz
        assert len({d[1] for d in self.dense}) == 1 and len({o.stride for o in outs}) == 1
        status = capi.lib().sputnik_hip_spmm_group_batched(
            m, k, run.n, run.replicas, g["count"], ctypes.cast(array, ctypes.c_void_p), self.dense[0][1], outs[0].stride,
            run.block_rows, int(g["accumulate"]), _stream())
        assert status == 0, (run.id, status)
        shape = (run.replicas, m // run.block_rows, run.n, run.block_rows) if run.block_rows else (run.replicas, m, run.n)
        return [out.result(run.id).view(shape) for out in outs]

    def one_by_one(self):
        """Every problem as a product of its own (values[perm] gathered on the host side)."""
        run, out = self.run, []
        for j, mat in enumerate(self.mats):
            values = self.values[j] if self.perms[j] is None else self.values[j][self.perms[j].long()]
            MATRICES.setdefault(mat.name, mat)
            out.append(plain(mat, run.n, run.replicas, values.contiguous(), 0, self.dense[j][0], self.dense[j][1]))
        return out


@pytest.mark.parametrize("run", GROUP_RUNS, ids=lambda run: run.id)
def test_group_instance_at_its_edges(run, knobs):
    knobs(run.knobs())
    g, m, k = run.group, run.case.m, run.case.k
    assert capi.lib().sputnik_hip_spmm_group_supported(m, k, run.n, g["count"], run.block_rows, int(g["accumulate"])) == 1
    exact = Group(run, integers=True)
    for j, (got, want) in enumerate(zip(exact.launch(), exact.want)):
        got = got.cpu().numpy().astype(np.float64)
        assert np.abs(want).max() < 2 ** 24
        assert np.array_equal(got, want), (run.id, j, "integers differ at", first_differences(got, want))
    problem = Group(run, integers=False)
    first = problem.launch()
    assert all(same_bits(a, b) for a, b in zip(first, problem.launch())), (run.id, "not repeatable")
    wants = [sum(problem.products)] if g["accumulate"] else problem.products
    for j, (got, want) in enumerate(zip(first, wants)):
        err = error(unstored(got, run.block_rows, m, run.n), want)
        print(f"{run.id} problem {j}: {run.label} error {err:.3e} of {TOL:.0e}")
        assert err < TOL, (run.id, j, err)
    if not run.identity:
        other = Group(run, integers=False, order="other").launch()
        assert all(same_bits(a, b) for a, b in zip(first, other)), (run.id, "the row order changes the bits")
    if not g["accumulate"]:
        for j, (got, alone) in enumerate(zip(first, problem.one_by_one())):
            assert torch.equal(got, stored(alone, run.block_rows)), (run.id, j, "differs from the product run alone")


# ---------------------------------------------------------------------------
# off the route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.OFF_ROUTE))
def test_shapes_off_the_route_still_give_the_product(name, knobs):
    """Under the knob, a shape the panel kernel does not serve goes to another kernel, quietly
    and correctly."""
    knobs({"SPUTNIK_HIP_SPMM_KERNEL": "panel"})
    m, k, n, offset = P.OFF_ROUTE[name]
    mat = P.off_route_case(name)
    MATRICES.setdefault(mat.name, mat)
    if not offset:
        assert capi.spmm_kernel_name(m, k, n, mat.nnz, 3) != PANEL_KERNEL
        assert capi.spmm_launch_shape(m, k, n, mat.nnz, 3)["family"] != "panel"
    ws = torch.empty(max(capi.spmm_workspace_bytes(m, k, n, mat.nnz), 4), dtype=torch.uint8, device=dev())
    for integers in (True, False):
        values, dense, _ = P.operands(mat, n, 3, False, integers=integers)
        d, stride = padded_dense(dense, offset=offset)
        assert d.data_ptr() % 16 == (4 * offset) % 16
        ri, ro, ci = topology(mat.name, "own")
        out = Out(3, m * n)
        status = capi.lib().sputnik_hip_spmm_batched(m, k, n, mat.nnz, 3, _p(ri), _p(T(values)), mat.nnz, _p(ro),
                                                     _p(ci), _p(d), stride, _p(out.view), out.stride, _p(ws),
                                                     ws.numel(), _stream())
        assert status == 0, (name, status)
        got = out.result(name).view(3, m, n)
        want = P.reference(mat, values.astype(np.float64), dense)
        if integers:
            assert np.array_equal(got.cpu().numpy().astype(np.float64), want), name
        else:
            assert error(got, want) < TOL, name
