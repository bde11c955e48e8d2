"""GPU: every compiled instance of the fused attention kernels on the designed masks of
tests/attention_cases.py -- the 20 of the LDS-staged forward (csrc/attention.hip), the 2 of the
row-group forward (attention_rows.hip) and the 8 of the backward (attention_backward.hip) --
through the C ABI, against float64 dense references built here from the dense mask.

Every launch has its plan compared with the numpy model first (row_ok and chunk table bit for
bit, the gathered blocks the ones the case names), writes into canary-guarded allocations with
padded replica strides (float32) or packed [B, S, H * 64] head views (half), and reads operands
whose gaps hold NaN.  The backward runs on `out` and `lse` of the float64 reference rounded to
float32, so that a failure there cannot be the forward's.

Bounds: float32 rel_err < 1e-4 (the suite's); half storage the bounds of
test_gpu_half_attention.py (helpers.half_err < 1e-4 on the output, |lse - want| <
1e-4 (1 + max |want|)); with dropout the bounds of test_gpu_attention_dropout.py (TOL there)."""
import functools
import math

import numpy as np
import pytest
import torch

import attention_cases as A
import philox_ref as P
from helpers import half_err, rel_err_torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
DROP_TOL = {"float32": 1e-4, "float16": 5e-3, "bfloat16": 3e-2}   # test_gpu_attention_dropout.TOL
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16,
        torch.int32: torch.int32, torch.int64: torch.int64}
SEED, OFFSET = 0x1234567887654321, 4 * 1001
B, H = 2, 2            # the half instances' batch and heads
G = A.GUARD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def capi():
    from torch_sputnik_amd import capi
    return capi


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def canary_of(dtype):
    if dtype in (torch.int32, torch.int64):
        return A.CANARY_INT
    return A.CANARY_F32 if dtype == torch.float32 else A.CANARY_HALF


class Guarded:
    """A flat allocation filled with a canary, GUARD elements in front of and behind the
    strided `view` a kernel reads or writes; `flat` starts at the view's first element (what the
    C ABI takes).  intact(): every element outside the view still holds the canary, bitwise."""

    def __init__(self, dtype, shape, strides, dev, inside=None, outside=None):
        extent = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        self.canary = canary_of(dtype) if outside is None else outside
        self.buf = torch.full((extent + 2 * G,), self.canary, dtype=dtype, device=dev)
        self.view = self.buf.as_strided(shape, strides, G)
        covered = torch.zeros(extent + 2 * G, dtype=torch.bool, device=dev)
        covered.as_strided(shape, strides, G).fill_(True)
        self.outside = ~covered
        self.want = self.buf.clone().view(BITS[dtype])[self.outside]
        if inside is not None:
            self.view.fill_(inside)
        self.flat = self.buf[G:]

    def intact(self):
        return torch.equal(self.buf.view(BITS[self.buf.dtype])[self.outside], self.want)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def operand(values, strides, dev, dtype=torch.float32):
    """`values` (CPU) as a strided device view whose gaps and guards hold NaN."""
    g = Guarded(dtype, tuple(values.shape), strides, dev, outside=float("nan"))
    g.view.copy_(values.to(dtype))
    return g


@functools.lru_cache(maxsize=None)
def operands(m, n, d, replicas, tname):
    """q [R, m, d], k, v [R, n, d] and dO [R, m, d] as float32 CPU tensors that the storage type
    holds exactly (half: uniform(-2, 2) as in test_gpu_half_attention.py, rounded)."""
    g = torch.Generator().manual_seed(100000 * m + 100 * n + d)
    shapes = ((replicas, m, d), (replicas, n, d), (replicas, n, d), (replicas, m, d))
    if tname == "float32":
        return tuple(torch.randn(*s, generator=g) for s in shapes)
    return tuple(torch.empty(*s).uniform_(-2, 2, generator=g).to(DTYPES[tname]).float() for s in shapes)


def masks_of(name, many):
    return list(A.batch(name).cases) if many else [A.case(name)]


def dense_factor(cases, replicas, p):
    """([R, m, n] bool mask, [R, m, n] float64 keep(r, e) / (1 - p) at the mask), replica r under
    mask r // (R / masks); e = the entry's position inside its own mask's column_indices."""
    heads = replicas // len(cases)
    m, n = cases[0].m, cases[0].n
    mask = torch.from_numpy(np.stack([c.dense for c in cases])).repeat_interleave(heads, 0)
    factor = torch.ones(replicas, m, n, dtype=torch.float64)
    if p > 0:
        width = max(c.nnz for c in cases)
        keep = P.keep_mask(SEED, OFFSET, replicas, width, p) * float(P.keep_scale(p))
        factor = torch.zeros(replicas, m, n, dtype=torch.float64)
        for r in range(replicas):
            c = cases[r // heads]
            rows = np.repeat(np.arange(m), np.diff(c.row_offsets))
            factor[r, rows, c.column_indices.astype(np.int64)] = torch.from_numpy(keep[r, :c.nnz])
    return mask, factor


def reference(q, k, v, mask, factor, scale):
    """float64 dense (softmax(scale q k^T at mask) * factor) v and the rows' log-sum-exp of the
    undropped scores; rows without entries give 0 and -inf.  Differentiable."""
    s = (scale * q @ k.transpose(-1, -2)).masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    w = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])
    w = torch.where(mask, w, torch.zeros_like(w))
    return (w * factor) @ v, lse


@functools.lru_cache(maxsize=None)
def forward_reference(name, many, tname, replicas, d, p):
    cases = masks_of(name, many)
    q, k, v, _ = operands(cases[0].m, cases[0].n, d, replicas, tname)
    mask, factor = dense_factor(cases, replicas, p)
    out, lse = reference(q.double(), k.double(), v.double(), mask, factor, 1 / math.sqrt(d))
    return out, lse


def check_forward(out, lse, want, want_lse, tname, out_name, p, label):
    """The bounds named in the module docstring; rows without entries: exact zeros, -inf."""
    out, lse = out.cpu(), lse.cpu()
    finite = torch.isfinite(want_lse)
    assert torch.equal(torch.isneginf(lse), ~finite), label
    assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any(), label
    assert not out[~finite].any(), label
    errors = {}
    if p > 0:
        bound = DROP_TOL[tname]
        errors["out"] = rel_err_torch(out.float(), want)
        errors["lse"] = rel_err_torch(lse[finite], want_lse[finite])
    elif tname == "float32":
        bound = TOL
        errors["out"] = rel_err_torch(out, want)
        errors["lse"] = rel_err_torch(lse[finite], want_lse[finite])
    else:
        bound = TOL
        if out_name == "float32":
            errors["out"] = rel_err_torch(out, want)
        else:
            errors["out"] = half_err(out.float().numpy(), want.numpy(), DTYPES[out_name])
        errors["lse"] = float((lse.double() - want_lse)[finite].abs().max()
                              / (1 + want_lse[finite].abs().max()))
    print(label, {k: f"{v:.3e}" for k, v in errors.items()}, "bound", bound)
    assert max(errors.values()) < bound, (label, errors)


# ---------------------------------------------------------------------------
# the LDS-staged forward: 20 instances
# ---------------------------------------------------------------------------
def plan_words(capi, cases, many, topo, dev):
    """Runs the plan into a guarded workspace and holds it to the model: -> the workspace."""
    m, n = cases[0].m, cases[0].n
    nonzeros = [c.nnz for c in cases]
    if many:
        nbytes = capi.sparse_attention_many_mask_workspace_bytes(len(cases), m, n, 64, max(nonzeros))
    else:
        nbytes = capi.sparse_attention_workspace_bytes(m, n, 64, nonzeros[0])
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded(torch.int32, (nbytes // 4,), (1,), dev, inside=A.CANARY_INT)
    if many:
        assert capi.sparse_attention_many_mask_plan(len(cases), m, n, 64, nonzeros, *topo, ws.view) == 0
    else:
        capi.sparse_attention_plan(m, n, 64, *topo, ws.view)
    got = ws.view.cpu().numpy()
    slots = A.ceil_div(m, A.BM) * A.BM
    if many:
        want, defined = A.Batch("", cases).plan_model()
        ints = A.mask_plan_ints(slots, A.ceil_div(n, A.BK))
        assert len(want) * 4 == nbytes
        row_ok = [got[i * ints:i * ints + slots] for i in range(len(cases))]
    else:
        ok, table, table_defined = A.plan_model(*cases[0].csr, m, n)
        first = A.row_ok_ints(slots)
        assert (first + len(table)) * 4 == nbytes
        want = np.zeros(nbytes // 4, dtype=np.int32)
        defined = np.zeros(nbytes // 4, dtype=bool)
        want[:slots], defined[:slots] = ok, True
        want[first:], defined[first:] = table, table_defined
        row_ok = [got[:slots]]
    wrong = np.flatnonzero((got != want) & defined)
    assert len(wrong) == 0, f"plan differs from the model at words {wrong[:8]}: {got[wrong[:8]]} != {want[wrong[:8]]}"
    for c, ok in zip(cases, row_ok):    # the blocks the case means to gather are the ones that do
        gathers = ~ok.reshape(-1, A.BM).astype(bool).all(axis=1)
        assert np.array_equal(gathers, c.gathered), c.name
        if c.name.startswith("one_block_gathers"):
            assert list(gathers) == [True, False]
        elif c.name.startswith("every_block_gathers"):
            assert gathers.all()
        elif not c.unsorted_rows:
            assert not gathers.any()
    assert ws.intact()
    return ws


def forward_buffers(tname, out_name, m, n, replicas, dev):
    """Fresh guarded out and lse: float32 [R, m, 64] with replica stride m * 64 + 64, half
    [B, H, m, 64] views of a [B, m, H * 64 + 8] allocation; lse [R, m] with stride m + 3."""
    if tname == "float32":
        out = Guarded(torch.float32, (replicas, m, 64), (m * 64 + 64, 64, 1), dev)
    else:
        row = H * 64 + 8
        out = Guarded(DTYPES[out_name], (B, H, m, 64), (m * row, 64, row, 1), dev)
    return out, Guarded(torch.float32, (replicas, m), (m + 3, 1), dev)


def forward_inputs(tname, m, n, replicas, dev):
    q, k, v, _ = operands(m, n, 64, replicas, tname)
    if tname == "float32":
        return [operand(x, (rows * 64 + 64, 64, 1), dev) for x, rows in ((q, m), (k, n), (v, n))]
    dtype = DTYPES[tname]
    qg = operand(q.reshape(B, H, m, 64), (m * H * 64, 64, H * 64, 1), dev, dtype)
    # k and v as the two halves of one packed [B, n, 2 * H * 64] tensor
    kv = torch.cat([k.reshape(B, H, n, 64).transpose(1, 2).reshape(B, n, H * 64),
                    v.reshape(B, H, n, 64).transpose(1, 2).reshape(B, n, H * 64)], dim=-1)
    packed = operand(kv, (n * 2 * H * 64, 2 * H * 64, 1), dev, dtype)
    strides = (n * 2 * H * 64, 64, 2 * H * 64, 1)
    packed.k = packed.buf.as_strided((B, H, n, 64), strides, G)
    packed.v = packed.buf.as_strided((B, H, n, 64), strides, G + H * 64)
    return [qg, packed]


def call_forward(capi, inst, cases, topo, inputs, out, lse, ws, planned, p, state_out):
    t, to, many, drop = inst
    m, n = cases[0].m, cases[0].n
    nonzeros = [c.nnz for c in cases]
    kw = dict(lse_stride=m + 3)
    if drop:
        kw.update(p=p, rng=(SEED, OFFSET), rng_state_out=state_out)
    lse_arg = None if lse is None else lse.flat
    if t == "float32":
        qg, kg, vg = inputs
        replicas = out.view.shape[0]
        kw.update(q_stride=m * 64 + 64, k_stride=n * 64 + 64, v_stride=n * 64 + 64, out_stride=m * 64 + 64)
        if many:
            assert capi.sparse_attention_many_mask_forward(
                len(cases), m, n, 64, nonzeros, replicas, *topo, qg.flat, kg.flat, vg.flat, 0.125,
                out.flat, lse_arg, ws.view, planned, **kw) == 0
        elif planned:
            capi.sparse_attention_forward_planned(m, n, 64, replicas, *topo, qg.flat, kg.flat, vg.flat,
                                                  0.125, out.flat, lse_arg, ws.view, **kw)
        else:
            capi.sparse_attention_forward(m, n, 64, replicas, *topo, qg.flat, kg.flat, vg.flat, 0.125,
                                          out.flat, lse_arg, ws.view, **kw)
    else:
        qg, packed = inputs
        if many:
            assert capi.sparse_attention_heads_many_mask_forward(
                len(cases), m, n, 64, nonzeros, *topo, qg.view, packed.k, packed.v, 0.125, out.view,
                lse_arg, ws.view, planned, **kw) == 0
        else:
            capi.sparse_attention_heads_forward(m, n, 64, *topo, qg.view, packed.k, packed.v, 0.125,
                                                out.view, lse_arg, ws.view, planned, **kw)


def forward_id(run):
    (t, to, many, drop), name = run
    return f"{t}-{to}-{'many' if many else 'one'}-{'drop' if drop else 'plain'}-{name}"


@pytest.mark.parametrize("run", A.forward_runs(), ids=forward_id)
def test_staged_forward_instance(dev, capi, run):
    inst, name = run
    t, to, many, drop = inst
    cases = masks_of(name, many)
    m, n = cases[0].m, cases[0].n
    replicas = B * H if t != "float32" else (len(cases) if many else 3)
    p = A.DROP_P if drop else 0.0
    src = A.batch(name) if many else cases[0]
    topo = [T(x, dev) for x in (src.row_indices, src.row_offsets, src.column_indices)]
    if t != "float32" and not many:
        q, k, v, o = (torch.empty(B, H, rows, 64, dtype=DTYPES[t], device=dev) for rows in (m, n, n, m))
        assert capi.sparse_attention_heads_supported(m, n, 64, cases[0].nnz, q, k, v, o.to(DTYPES[to]))

    ws = plan_words(capi, cases, many, topo, dev)              # before any attention launch
    inputs = forward_inputs(t, m, n, replicas, dev)
    state = Guarded(torch.int64, (2,), (1,), dev) if drop else None
    out, lse = forward_buffers(t, to, m, n, replicas, dev)
    call_forward(capi, inst, cases, topo, inputs, out, lse, ws, True, p, state and state.view)
    torch.cuda.synchronize()
    label = forward_id(run)
    assert out.intact() and lse.intact() and ws.intact(), label
    if drop:
        assert state.view.tolist() == [SEED, OFFSET] and state.intact(), label

    # the unplanned form (its own pre-pass, into a fresh workspace), and the form without lse
    ws2 = Guarded(torch.int32, tuple(ws.view.shape), (1,), dev, inside=A.CANARY_INT)
    out2, lse2 = forward_buffers(t, to, m, n, replicas, dev)
    call_forward(capi, inst, cases, topo, inputs, out2, lse2, ws2, False, p, None)
    assert same_bits(out2.view, out.view) and same_bits(lse2.view, lse.view), label
    assert out2.intact() and lse2.intact() and ws2.intact(), label
    assert same_bits(ws2.view, ws.view), label
    out3, _ = forward_buffers(t, to, m, n, replicas, dev)
    call_forward(capi, inst, cases, topo, inputs, out3, None, ws, True, p, None)
    assert same_bits(out3.view, out.view) and out3.intact(), label

    want, want_lse = forward_reference(name, many, t, replicas, 64, p)
    got = out.view if t == "float32" else out.view.reshape(replicas, m, 64)
    check_forward(got, lse.view, want, want_lse, t, to, p, label)


# ---------------------------------------------------------------------------
# the row-group forward, d = 128: 2 instances
# ---------------------------------------------------------------------------
def rowgroup_id(run):
    (kernel, d, drop), name = run
    return f"{kernel}-d{d}-{'drop' if drop else 'plain'}-{name}"


ROWS_FORWARD_RUNS = [r for r in A.rowgroup_runs() if r[0][0] == "rows_forward"]
BACKWARD_RUNS = [r for r in A.rowgroup_runs() if r[0][0] == "backward_rows"]   # (one call runs both kernels)


def padded(rows, d):
    return (rows * d + d, d, 1)


@pytest.mark.parametrize("run", ROWS_FORWARD_RUNS, ids=rowgroup_id)
def test_rows_forward_instance(dev, capi, run):
    (_, d, drop), name = run
    c = A.case(name)
    m, n, R = c.m, c.n, 3
    p = A.DROP_P if drop else 0.0
    assert capi.sparse_attention_rows_supported(m, n, d, c.nnz)
    q, k, v, _ = operands(m, n, d, R, "float32")
    qg, kg, vg = (operand(x, padded(rows, d), dev) for x, rows in ((q, m), (k, n), (v, n)))
    strides = dict(q_stride=m * d + d, k_stride=n * d + d, v_stride=n * d + d, out_stride=m * d + d,
                   lse_stride=m + 3)
    want, want_lse = forward_reference(name, False, "float32", R, d, p)
    results = []
    for order in A.T_ORDERS:     # any row_indices order: the same bits
        ri = {"by_length": np.argsort(-np.diff(c.row_offsets), kind="stable"), "identity": np.arange(m),
              "permuted": np.random.default_rng(5).permutation(m)}[order].astype(np.int32)
        topo = [T(x, dev) for x in (ri, c.row_offsets, c.column_indices)]
        out = Guarded(torch.float32, (R, m, d), padded(m, d), dev)
        lse = Guarded(torch.float32, (R, m), (m + 3, 1), dev)
        state = Guarded(torch.int64, (2,), (1,), dev)
        kw = dict(p=p, rng=(SEED, OFFSET), rng_state_out=state.view) if drop else {}
        assert capi.sparse_attention_rows_forward(m, n, d, R, *topo, qg.flat, kg.flat, vg.flat,
                                                  1 / math.sqrt(d), out.flat, lse.flat, **strides, **kw) == 0
        torch.cuda.synchronize()
        assert out.intact() and lse.intact() and state.intact(), (name, order)
        if drop:
            assert state.view.tolist() == [SEED, OFFSET]
        results.append((out, lse))
    for out, lse in results[1:]:
        assert same_bits(out.view, results[0][0].view) and same_bits(lse.view, results[0][1].view)
    out3 = Guarded(torch.float32, (R, m, d), padded(m, d), dev)
    kw = dict(p=p, rng=(SEED, OFFSET)) if drop else {}
    assert capi.sparse_attention_rows_forward(m, n, d, R, *topo, qg.flat, kg.flat, vg.flat,
                                              1 / math.sqrt(d), out3.flat, None, **strides, **kw) == 0
    assert same_bits(out3.view, results[0][0].view) and out3.intact()
    check_forward(results[0][0].view, results[0][1].view, want, want_lse, "float32", "float32", p,
                  rowgroup_id(run))


# ---------------------------------------------------------------------------
# the backward: 8 instances (rows and columns kernels x d x dropout)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backward_reference(name, d, p):
    """float64: (out, lse, dq, dk, dv) of the dense reference and its autograd, and the float32
    floors of dq and dk (conditioned_error)."""
    c = A.case(name)
    R = 2
    q, k, v, go = operands(c.m, c.n, d, R, "float32")
    mask, factor = dense_factor([c], R, p)
    scale = 1 / math.sqrt(d)
    qd, kd, vd = (x.double().requires_grad_() for x in (q, k, v))
    out, lse = reference(qd, kd, vd, mask, factor, scale)
    out.backward(go.double())
    with torch.no_grad():
        weights = torch.exp((scale * qd @ kd.transpose(-1, -2)).masked_fill(~mask, float("-inf"))
                            - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])
        products = (go.double().abs() @ vd.abs().transpose(-1, -2)) * factor       # sum_c |dO_ic v_jc| f
        products = products + (go.double().abs() * out.abs()).sum(-1)[..., None]    # + sum_c |dO_ic O_ic|
        spread = torch.where(mask, weights * products, torch.zeros_like(products)) * (2.0 ** -24 * scale)
        floors = spread @ kd.abs(), spread.transpose(-1, -2) @ qd.abs()
    return (out.detach(), lse.detach(), qd.grad, kd.grad, vd.grad) + floors


def conditioned_error(got, want, floor):
    """rel_err_torch with a float32 floor under both of its criteria: the test stays
    ``conditioned_error(...) < 1e-4``, and floor = 0 gives rel_err_torch itself.

    Why dQ and dK need one.  ds_ij = p_ij (dp_ij - D_i) scale with D_i = sum_j p_ij dp_ij: the
    dp_ij of a row cancel against their own weighted mean (sum_j ds_ij = 0 without dropout), so
    a row of few entries, or of one dominant weight, has ds -- and with it dQ_i = sum_j ds_ij k_j
    and its share of dK_j -- far below |dp| and |D|, by as much as the data decides (two entries:
    dp_1 - D = p_2 (dp_1 - dp_2)).  dp_ij and D_i are dot products of float32 numbers.  Rounding
    each PRODUCT of them once to float32, u = 2^-24, and adding exactly -- less than any float32
    evaluation does -- already moves
        ds_ij  by up to  u p_ij (sum_c |dO_ic v_jc| f_ij + sum_c |dO_ic O_ic|) scale,
    which no longer shrinks with the cancellation, and through  sum_j . |k_jc|  (dQ) and
    sum_i . |q_ic|  (dK) is the floor passed here (backward_reference).  The float64 reference is
    ill-conditioned exactly where that floor is not small against the row: the query rows of 2
    entries of rowgroup_100x100 miss 1e-4 in a plain float32 numpy evaluation of the formulas too
    (1.8e-4; 2.6e-5 with the floor).  On ordinary rows the floor adds about 2 % to the
    allowance (median over the rows of the cases here).  dV has no difference in it: no floor."""
    err, aw = (got.double() - want).abs(), want.abs()
    slack = floor / TOL
    rowmean = aw.mean(dim=-1, keepdim=True).clamp_min(1e-30)
    worst = float((err / (aw + rowmean + slack)).max())
    significant = aw > 1e-2 * aw.amax(dim=-1, keepdim=True)
    if bool(significant.any()):
        worst = max(worst, float((err / (aw + slack))[significant].max()))
    return worst


def zero_row_error(got, want, floor, zero_rows):
    """conditioned_error of a gradient [R, rows, d] whose rows `zero_rows` are EXACTLY 0 in
    float64 by cancellation, not by emptiness.

    dQ_i of a query row with ONE entry: its softmax is the single weight 1, so D_i =
    <dO_i, O_i> = <dO_i, f v_j> = dp (f the keep factor) and ds = p (dp - D_i) scale = 0.  In
    float32 dp and D_i are two roundings of one dot product (three once `out` is the rounded
    reference), so dQ_i = (a few ulp of dp) * scale * k_j: small against the other rows, not
    against itself.  dK_j of a key row that only such query rows see is a sum of those terms
    times q_i: the same.  A zero row is no scale for a relative bound; such rows take the
    replica's mean magnitude, the rule helpers.rel_err has for short rows (and dq_error of
    test_gpu_attention_d128.py for dQ)."""
    zero_rows = torch.as_tensor(zero_rows)
    worst = conditioned_error(got[:, ~zero_rows], want[:, ~zero_rows], floor[:, ~zero_rows])
    if bool(zero_rows.any()):
        scale = want.abs().mean(dim=(1, 2), keepdim=True)
        assert float((want[:, zero_rows].abs() / scale).max()) < 1e-12    # (0 up to float64 rounding)
        err = (got[:, zero_rows].double() - want[:, zero_rows]).abs()
        worst = max(worst, float((err / (want[:, zero_rows].abs() + scale)).max()))
    return worst


def run_backward(capi, c, d, p, dev, t_order, wanted=(True, True, True), device_state=False):
    """One C ABI call on padded operands -> the three guarded gradients (None: not asked for)."""
    m, n, R = c.m, c.n, 2
    q, k, v, go = operands(m, n, d, R, "float32")
    out_ref, lse_ref = backward_reference(c.name, d, p)[:2]
    ins = [operand(x, padded(rows, d), dev) for x, rows in
           ((q, m), (k, n), (v, n), (out_ref.float(), m), (go, m))]
    lse = operand(lse_ref.float(), (m + 3, 1), dev)
    topo = [T(x, dev) for x in c.csr]
    t_topo = [T(x, dev) for x in c.transposed(t_order, seed=3)]
    nbytes = capi.sparse_attention_backward_workspace_bytes(m, n, d, c.nnz, R)
    assert nbytes >= 4 * R * m
    ws = Guarded(torch.float32, (nbytes // 4,), (1,), dev, inside=float("nan"))
    grads = [Guarded(torch.float32, (R, rows, d), padded(rows, d), dev, inside=float("nan")) if w else None
             for rows, w in zip((m, n, n), wanted)]
    kw = {}
    if p > 0:
        if device_state:   # an rng_state_out as the forward publishes it
            holder = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=dev)
            kw = dict(p=p, rng=capi.PhiloxState(seed_ptr=holder.data_ptr(),
                                                offset_ptr=holder.data_ptr() + 8))
        else:
            kw = dict(p=p, rng=(SEED, OFFSET))
    st = capi.sparse_attention_backward(
        m, n, d, R, *topo, *t_topo, ins[0].flat, ins[1].flat, ins[2].flat, 1 / math.sqrt(d),
        ins[3].flat, ins[4].flat, lse.flat, *(None if g is None else g.flat for g in grads), ws.view,
        q_stride=m * d + d, k_stride=n * d + d, v_stride=n * d + d, out_stride=m * d + d,
        grad_out_stride=m * d + d, lse_stride=m + 3, grad_q_stride=m * d + d, grad_k_stride=n * d + d,
        grad_v_stride=n * d + d, **kw)
    assert st == 0
    torch.cuda.synchronize()
    assert ws.intact(), (c.name, "workspace")       # the canary past workspace_bytes
    for g, label in zip(grads, ("dq", "dk", "dv")):
        if g is not None:
            assert g.intact(), (c.name, label)
            assert not torch.isnan(g.view).any(), (c.name, label, "a word was not written")
    return grads


@pytest.mark.parametrize("run", BACKWARD_RUNS, ids=lambda r: rowgroup_id(r).replace("backward_rows", "backward"))
def test_backward_instances(dev, capi, run):
    (_, d, drop), name = run
    c = A.case(name)
    p = A.DROP_P if drop else 0.0
    assert capi.sparse_attention_backward_supported(c.m, c.n, d, c.nnz)
    _, _, want_dq, want_dk, want_dv, floor_dq, floor_dk = backward_reference(name, d, p)
    orders = A.T_ORDERS if name in A.ROWGROUP_CASES else (A.T_ORDERS[len(name) % 3],)
    first = None
    for order in orders:          # whichever row group takes a key row: the same sums
        grads = run_backward(capi, c, d, p, dev, order)
        if first is None:
            first = grads
        for a, b in zip(grads, first):
            assert same_bits(a.view, b.view), (name, order)
    if drop:                      # replayed from a device state: the same bits
        for a, b in zip(run_backward(capi, c, d, p, dev, orders[0], device_state=True), first):
            assert same_bits(a.view, b.view), name
    dq, dk, dv = (g.view.cpu() for g in first)
    single = c.dense.sum(1) == 1
    seen_only_by_single = c.dense.any(0) & ~c.dense[~single].any(0)
    errors = {"dq": zero_row_error(dq, want_dq, floor_dq, single),
              "dk": zero_row_error(dk, want_dk, floor_dk, seen_only_by_single),
              "dv": rel_err_torch(dv, want_dv)}
    print(rowgroup_id(run), {k: f"{v:.3e}" for k, v in errors.items()})
    assert max(errors.values()) < TOL, errors
    empty_rows, empty_cols = ~c.dense.any(1), ~c.dense.any(0)
    assert not dq[:, empty_rows].any() and not dk[:, empty_cols].any() and not dv[:, empty_cols].any()
    if name in A.ROWGROUP_CASES:
        assert empty_rows.any() and empty_cols.any() and single.any()


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
@pytest.mark.parametrize("d", [64, 128])
def test_backward_partial_outputs(dev, capi, d, drop):
    """Each non-empty subset of {dQ, dK, dV}: the bits of the full run, nothing else written."""
    c = A.case("rowgroup_90x77")
    p = A.DROP_P if drop else 0.0
    full = run_backward(capi, c, d, p, dev, "by_length")
    for bits in range(1, 8):
        wanted = tuple(bool(bits >> i & 1) for i in range(3))
        part = run_backward(capi, c, d, p, dev, "by_length", wanted=wanted)
        for got, want, asked in zip(part, full, wanted):
            assert (got is not None) == asked
            if asked:
                assert same_bits(got.view, want.view), (wanted,)
