"""GPU: seeded random batches of masks for the many-mask family -- the five operators through
the C ABI against the numpy oracle, the fused attention (float32 and the float16 / bfloat16
heads kernel, unplanned and planned) against float64, the fused kernels against the
single-mask kernels bit for bit, and the autograd forms against float64 autograd.

Query and key counts m and n are drawn independently around the tile edges (128 query rows,
128-key chunks, 16-entry windows), masks of mixed kinds in one batch (empty first, in the
middle or last; single entries; bands; global tokens; one full row; empty rows), columns out
of order in some masks, and scores from narrow to far past float32's exp range."""
import os

import numpy as np
import pytest
import torch

from oracle import sputnik_oracle as O
from helpers import (MASK_KINDS, many_mask_entries, mask_of_kind, ref_attention_many_mask,
                     ref_sddmm_many_mask, ref_softmax_many_mask, ref_spmm_many_mask, rel_err,
                     rel_err_torch, shuffle_columns)

pytestmark = pytest.mark.gpu

# SPUTNIK_FUZZ_SCALE=10 runs ten times the cases from a different seed (soak run)
SCALE = int(os.environ.get("SPUTNIK_FUZZ_SCALE", "1"))
SEED_SHIFT = 0 if SCALE == 1 else 1000003

D = 64
TOL = 1e-4
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}   # (test_gpu_half_attention.py)
SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 300, 520)
SCALES = (0.125, 1.0, 0.01)
RANGES = ("narrow", "wide", "very_wide")
EMPTY_AT = ("first", "middle", "last", None)
# bound of the fused outputs against float64: at +-300 float32 resolves the exponent of a
# weight only to ~3e-5 (its ulp at 300), which a weighted mean of v can amplify several times
OUT_TOL = {"narrow": TOL, "wide": TOL, "very_wide": 1e-3}
SENTINEL = -7.0   # (the transpose's padding; the other CSR outputs are filled with NaN)
# served entries x replicas of one case: keeps the numpy oracle at the existing fuzz's sizes
ORACLE_BUDGET = 400_000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def capi():
    from torch_sputnik_amd import capi
    return capi


@pytest.fixture
def plan_cache_default():
    """Tests that switch the plan cache on leave the default behind them."""
    from torch_sputnik_amd import functional as F
    yield F
    F.enable_plan_cache(F.PLAN_CACHE_DEFAULT)


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _sizes(rng, choices=SIZES):
    """m and n drawn independently; equal in about a fifth of the cases."""
    m = int(rng.choice(choices))
    if rng.random() < 0.2:
        return m, m
    n = int(rng.choice(choices))
    while n == m:
        n = int(rng.choice(choices))
    return m, n


def _masks(rng, b, m, n, empty_at):
    """[b, m, n] masks of mixed kinds with an empty one at `empty_at`, at least one not empty."""
    kinds = [MASK_KINDS[int(rng.integers(1, len(MASK_KINDS)))] for _ in range(b)]
    if empty_at is not None and b > 1:
        kinds[{"first": 0, "middle": b // 2, "last": b - 1}[empty_at]] = "empty"
    dense = np.stack([mask_of_kind(kind, m, n, rng) for kind in kinds])
    if not dense.any():   # (a batch without any entry has a test of its own)
        kinds[-1 if kinds[0] == "empty" else 0] = "heavy_row"
        i = kinds.index("heavy_row")
        dense[i] = mask_of_kind("heavy_row", m, n, rng)
    return dense, kinds


def _draw_case(rng, it):
    """(b, heads, m, n, dense masks, kinds): a batch of 1..9 masks with 1..8 heads, or (one
    case in six) 40..70 small masks; redrawn until the oracle work fits the budget."""
    while True:
        if it % 6 == 5:
            b, heads, (m, n) = int(rng.integers(40, 71)), int(rng.integers(1, 3)), (64, 48)
        else:
            b, heads = int(rng.integers(1, 10)), int(rng.integers(1, 9))
            m, n = _sizes(rng)
        dense, kinds = _masks(rng, b, m, n, EMPTY_AT[it % len(EMPTY_AT)])
        entries = int(dense.sum())
        while heads > 1 and entries * heads > ORACLE_BUDGET:
            heads -= 1
        if entries * heads <= ORACLE_BUDGET:
            return b, heads, m, n, dense, kinds


def _topology(rng, dense, m):
    """Flat many-mask layout (oracle.dense_to_csr_many_mask); in about a third of the masks
    the columns of every third row are shuffled.  -> ri, ro, ci, nonzeros, shuffled masks."""
    ri, ro, ci, nn = O.dense_to_csr_many_mask(dense.astype(np.int32))
    ci = ci.copy()
    shuffled, first = [], 0
    for i, count in enumerate(nn):
        if rng.random() < 0.35 and count > 1:
            shuffle_columns(ci, ro, i, m, first, rng)
            shuffled.append(i)
        first += int(count)
    return ri, ro, ci, [int(c) for c in nn], shuffled


def _qkv(rng, replicas, m, n, score_range, scale):
    """float32 q [R, m, 64], k and v [R, n, 64] in [-2, 2] ("narrow": q and k scaled so
    that the scores spread as at scale 1/8, ~+-1).  "wide" / "very_wide": query
    dimension 0 is 1 and key dimension 0 a ramp, so that scale * q . k rises along every row
    over ~+-30 / ~+-300 (every window rescales; at +-300 most weights underflow).  There q and
    k are multiples of 1/8: every partial sum of q . k is exact in float32 in any order (at
    |q . k| ~ 2400 rounded partial sums alone would move the weights by ~1e-3), so what is
    measured is the kernel's softmax, not the conditioning of its inputs."""
    q = rng.uniform(-2, 2, (replicas, m, D)).astype(np.float32)
    k = rng.uniform(-2, 2, (replicas, n, D)).astype(np.float32)
    v = rng.uniform(-2, 2, (replicas, n, D)).astype(np.float32)
    if score_range == "narrow":   # scale * q . k spread as at scale 1/8 (about +-1)
        q, k = (x * np.float32(np.sqrt(0.125 / scale)) for x in (q, k))
    else:
        span = 30.0 if score_range == "wide" else 300.0
        q, k = np.round(q * 8) / 8, np.round(k * 8) / 8
        q[:, :, 0] = 1.0
        k[:, :, 0] = np.round(np.linspace(-span, span, n) / scale * 8) / 8
    return q, k, v


def _per_mask(nn, heads):
    """(mask, replica slice, entry slice) of every mask."""
    first = 0
    for i, count in enumerate(nn):
        yield i, slice(i * heads, (i + 1) * heads), slice(first, first + count)
        first += count


def _flush(x):
    """Values below float32's smallest normal as 0: no relative bound holds for denormals (at
    the widest score range whole rows of the softmax gradient fall there), and a kernel may
    flush them."""
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < np.finfo(np.float32).tiny, 0.0, x)


def _check_csr(got, want, nn, heads, ro, m, tag, what):
    """rel_err per CSR row, mask by mask (denormals flushed); padding past a replica's own
    count still holds the NaN it was filled with (never written); no served entry does."""
    for i, rows, _ in _per_mask(nn, heads):
        count = nn[i]
        assert np.isnan(got[rows, count:]).all(), f"{tag}: {what} wrote padding of mask {i}"
        if count == 0:
            continue
        assert not np.isnan(got[rows, :count]).any(), f"{tag}: {what} left entries of mask {i}"
        err = rel_err(_flush(got[rows, :count]), _flush(want[rows, :count]),
                      ro[i * (m + 1):(i + 1) * (m + 1)])
        assert err < TOL, f"{tag}: {what} mask {i} rel_err {err:.3g}"


def _check_attention(out, lse, want, want_lse, tag, what, bound=TOL):
    assert not torch.isnan(out).any(), f"{tag}: {what} left outputs unwritten"
    err = rel_err_torch(out.float(), want)
    assert err < bound, f"{tag}: {what} rel_err {err:.3g}"
    if lse is None:
        return
    assert not torch.isnan(lse).any(), f"{tag}: {what} left lse unwritten"
    finite = torch.isfinite(want_lse)
    assert torch.equal(torch.isneginf(lse), ~finite), f"{tag}: {what} lse = -inf exactly at empty rows"
    if finite.any():
        err = float((lse.double() - want_lse)[finite].abs().max())
        assert err < TOL * (1 + float(want_lse[finite].abs().max())), f"{tag}: {what} lse err {err:.3g}"


def _operators(capi, dev, rng, case, q, k, v):
    """The five operators through the C ABI against the numpy oracle."""
    b, heads, m, n, nn, (ri, ro, ci), topo, scale, tag = case
    R, width = b * heads, max(nn)
    oracle_topo = (ri, ro, ci)

    # SDDMM at inner dimension 64 (the attention's q, k) and one other, with and without the
    # per-mask plans in the workspace
    scores = None
    for inner in (D, int(rng.choice([8, 72]))):
        if inner == D:
            lhs, rhs = q, k
        else:
            lhs = rng.uniform(-1, 1, (R, m, inner)).astype(np.float32)
            rhs = rng.uniform(-1, 1, (R, n, inner)).astype(np.float32)
        pad = int(rng.integers(0, 5))
        out = torch.full((R, width + pad), float("nan"), device=dev)
        ws = None
        if rng.random() < 0.7:
            ws = torch.empty(max(capi.sddmm_many_mask_workspace_bytes(b, m, inner, n, width), 1),
                             dtype=torch.uint8, device=dev)
        capi.sddmm_many_mask(b, m, inner, n, nn, R, *topo, T(lhs, dev), T(rhs, dev), out, ws)
        got = out.cpu().numpy()
        want = O.sddmm_many_mask(b, m, n, nn, *oracle_topo, lhs, rhs)
        _check_csr(got, want, nn, heads, ro, m, tag, f"sddmm k={inner} ws={ws is not None}")
        if inner == D:
            scores = out

    # softmax (scaled) of those scores, and its backward
    probs = torch.full((R, scores.size(1)), float("nan"), device=dev)
    capi.sparse_softmax_many_mask(b, m, nn, R, scores, topo[0], topo[1], topo[2], scale, probs)
    got_p = probs.cpu().numpy()
    want_p = O.sparse_softmax_many_mask(b, m, nn, scores.cpu().numpy(), *oracle_topo, scale)
    _check_csr(got_p, want_p, nn, heads, ro, m, tag, "softmax")
    # (the backward takes well-conditioned weights: with a score spread of ~+-30 -- already
    # the narrow range at scale 1 -- a row's largest weight is ~1 and its gradient
    # g - sum(y g) cancels below float32's resolution of g)
    y = torch.full(probs.shape, float("nan"), device=dev)
    capi.sparse_softmax_many_mask(b, m, nn, R, T(rng.uniform(-3, 3, probs.shape).astype(np.float32), dev),
                                  topo[0], topo[1], topo[2], 1.0, y)
    grad = rng.uniform(-1, 1, probs.shape).astype(np.float32)
    grad_in = torch.full(probs.shape, float("nan"), device=dev)
    capi.sparse_softmax_backward_many_mask(b, m, nn, R, y, T(grad, dev), topo[1], scale, grad_in)
    want_g = O.sparse_softmax_backward_many_mask(b, m, nn, y.cpu().numpy(), grad, ro, scale)
    _check_csr(grad_in.cpu().numpy(), want_g, nn, heads, ro, m, tag, "softmax backward")

    # SpMM of the weights: width 64 (the panel kernel, all masks in one launch) and a width
    # that takes one launch per mask
    for cols in (D, int(rng.choice([1, 7, 72, 200]))):
        dense = v if cols == D else rng.uniform(-1, 1, (R, n, cols)).astype(np.float32)
        out = torch.full((R, m, cols), float("nan"), device=dev)
        ws = torch.empty(max(capi.spmm_workspace_bytes(m, n, cols, width), 1), dtype=torch.uint8,
                         device=dev)
        capi.spmm_many_mask(b, m, n, cols, nn, R, topo[0], probs, topo[1], topo[2], T(dense, dev),
                            out, ws)
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"{tag}: spmm width {cols} left outputs unwritten"
        want = O.spmm_many_mask(b, m, n, nn, got_p[:, :width], *oracle_topo, dense)
        err = rel_err(got, want)
        assert err < TOL, f"{tag}: spmm width {cols} rel_err {err:.3g}"

    # transpose of the weights' topology, bit for bit
    values = rng.uniform(-1, 1, (R, width + int(rng.integers(0, 5)))).astype(np.float32)
    regions = bool(rng.integers(0, 2))
    nbytes = (capi.csr_transpose_many_mask_workspace_bytes(b, m, n, width) if regions
              else capi.csr_transpose_workspace_bytes(m, n, width))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    vt = torch.full(values.shape, SENTINEL, device=dev)
    rot = torch.full((b, n + 1), -1, dtype=torch.int32, device=dev)
    cit = torch.full((len(ci),), -1, dtype=torch.int32, device=dev)
    perm = torch.full((len(ci),), -1, dtype=torch.int32, device=dev)
    capi.csr_transpose_many_mask(b, m, n, nn, R, T(values, dev), topo[1], topo[2], vt, rot, cit, perm, ws)
    w_vt, w_rot, w_cit = O.csr_transpose_many_mask(b, m, n, nn, values[:, :width], ro, ci)
    ttag = f"{tag} transpose regions={regions}"
    assert np.array_equal(rot.cpu().numpy(), w_rot), ttag
    assert np.array_equal(cit.cpu().numpy(), w_cit), ttag
    got, p = vt.cpu().numpy(), perm.cpu().numpy()
    for i, rows, span in _per_mask(nn, heads):
        assert np.array_equal(got[rows, :nn[i]], w_vt[rows, :nn[i]]), f"{ttag}: mask {i}"
        assert (got[rows, nn[i]:] == SENTINEL).all(), f"{ttag}: padding of mask {i}"
        assert np.array_equal(values[rows][:, p[span]], w_vt[rows, :nn[i]]), f"{ttag}: mask {i} perm"


def _single_mask_f32(capi, dev, case, q, k, v, out, lse):
    """Each mask and its heads alone on the single-mask kernel: the same bits (lse included);
    a mask without entries (refused there): zeros and -inf."""
    b, heads, m, n, nn, _, topo, scale, tag = case
    ri, ro, ci = topo
    for i, rows, span in _per_mask(nn, heads):
        if nn[i] == 0:
            assert not out[rows].any() and torch.isneginf(lse[rows]).all(), f"{tag}: empty mask {i}"
            continue
        one = (ri[i * m:(i + 1) * m], ro[i * (m + 1):(i + 1) * (m + 1)], ci[span])
        ws = torch.empty(capi.sparse_attention_workspace_bytes(m, n, D, nn[i]), dtype=torch.uint8,
                         device=dev)
        want = torch.full((heads, m, D), float("nan"), device=dev)
        want_lse = torch.full((heads, m), float("nan"), device=dev)
        capi.sparse_attention_forward(m, n, D, heads, *one, q[rows], k[rows], v[rows], scale, want,
                                      want_lse, ws)
        assert torch.equal(out[rows], want), f"{tag}: mask {i} differs from the single-mask kernel"
        assert torch.equal(lse[rows], want_lse), f"{tag}: mask {i} lse differs from the single-mask kernel"


def _single_mask_heads(capi, dev, case, qh, kh, vh, out, lse):
    b, heads, m, n, nn, _, topo, scale, tag = case
    ri, ro, ci = topo
    for i, rows, span in _per_mask(nn, heads):
        if nn[i] == 0:
            assert not out[i].any() and torch.isneginf(lse[rows]).all(), f"{tag}: empty mask {i}"
            continue
        one = (ri[i * m:(i + 1) * m], ro[i * (m + 1):(i + 1) * (m + 1)], ci[span])
        ws = torch.empty(capi.sparse_attention_heads_workspace_bytes(m, n, D, nn[i]), dtype=torch.uint8,
                         device=dev)
        want = torch.full((1, m, heads, D), float("nan"), device=dev, dtype=out.dtype).transpose(1, 2)
        want_lse = torch.full((heads, m), float("nan"), device=dev)
        capi.sparse_attention_heads_forward(m, n, D, *one, qh[i:i + 1], kh[i:i + 1], vh[i:i + 1], scale,
                                            want, want_lse, ws)
        assert torch.equal(out[i:i + 1], want), f"{tag}: mask {i} differs from the single-mask heads kernel"
        assert torch.equal(lse[rows], want_lse), f"{tag}: mask {i} lse differs from the single-mask heads kernel"


def _head_views(x, kind, b, heads, m, n):
    """[R, S, D] float32 q, k, v -> [B, H, S, D] views of [B, S, ...] storage: separate
    [B, S, H, D] tensors, one packed [B, S, 3*H*D] tensor (m == n), or q alone and one
    packed [B, n, H, 2*D] key / value tensor."""
    q, k, v = (t.reshape(b, heads, -1, D).transpose(1, 2) for t in x)   # [B, S, H, D]
    if kind == "packed" and m == n:
        packed = torch.cat([t.reshape(b, m, heads * D) for t in (q, k, v)], -1)
        views = [packed[..., j * heads * D:(j + 1) * heads * D].unflatten(-1, (heads, D)) for j in range(3)]
    elif kind == "packed":
        kv = torch.cat([k, v], -1)
        views = [q.contiguous(), kv[..., :D], kv[..., D:]]
    else:
        views = [t.contiguous() for t in (q, k, v)]
    return [t.transpose(1, 2) for t in views]


def test_fuzz_many_mask_operators_and_attention(capi, dev):
    rng = np.random.default_rng(20261016 + SEED_SHIFT)
    for it in range(24 * SCALE):
        b, heads, m, n, dense, kinds = _draw_case(rng, it)
        ri, ro, ci, nn, shuffled = _topology(rng, dense, m)
        # (the dense reference sees the same sets of entries in any column order)
        R = b * heads
        scale = float(rng.choice(SCALES))
        score_range = RANGES[int(rng.integers(0, len(RANGES)))]
        dtype = (torch.float16, torch.bfloat16)[it % 2]
        out_f32 = bool(rng.integers(0, 2))
        layout = ("packed", "separate")[int(rng.integers(0, 2))]
        tag = (f"case {it}: b={b} heads={heads} m={m} n={n} nnz={nn} kinds={kinds} "
               f"shuffled={shuffled} range={score_range} scale={scale} dtype={dtype} "
               f"out_f32={out_f32} layout={layout}")
        topo = tuple(T(x, dev) for x in (ri, ro, ci))
        case = (b, heads, m, n, nn, (ri, ro, ci), topo, scale, tag)
        q, k, v = _qkv(rng, R, m, n, score_range, scale)

        _operators(capi, dev, rng, case, q, k, v)

        # the fused float32 kernel, unplanned
        masks_d = torch.from_numpy(dense).to(dev)
        qd, kd, vd = (T(x, dev) for x in (q, k, v))
        nbytes = capi.sparse_attention_many_mask_workspace_bytes(b, m, n, D, max(nn))
        assert nbytes > 0, tag
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.full((R, m, D), float("nan"), device=dev)
        lse = torch.full((R, m), float("nan"), device=dev)
        st = capi.sparse_attention_many_mask_forward(b, m, n, D, nn, R, *topo, qd, kd, vd, scale, out,
                                                     lse, ws)
        assert st == 0, f"{tag}: status {st}"
        want, want_lse = ref_attention_many_mask(qd, kd, vd, masks_d, scale)
        _check_attention(out, lse, want, want_lse, tag, "fused f32", OUT_TOL[score_range])
        _single_mask_f32(capi, dev, case, qd, kd, vd, out, lse)

        # planned: one plan, two draws of q, k, v
        plan = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert capi.sparse_attention_many_mask_plan(b, m, n, D, nn, *topo, plan) == 0, tag
        for draw in range(2):
            if draw:
                qd, kd, vd = (T(x, dev) for x in _qkv(rng, R, m, n, score_range, scale))
                want, want_lse = ref_attention_many_mask(qd, kd, vd, masks_d, scale)
            got = torch.full((R, m, D), float("nan"), device=dev)
            got_lse = torch.full((R, m), float("nan"), device=dev)
            st = capi.sparse_attention_many_mask_forward(b, m, n, D, nn, R, *topo, qd, kd, vd, scale, got,
                                                         got_lse, plan, planned=True)
            assert st == 0, f"{tag}: planned status {st}"
            if draw == 0:
                assert torch.equal(got, out) and torch.equal(got_lse, lse), f"{tag}: planned != unplanned"
            else:
                _check_attention(got, got_lse, want, want_lse, tag, "fused f32 planned, second draw",
                                 OUT_TOL[score_range])

        # the heads kernel on float16 / bfloat16 views
        qh, kh, vh = _head_views([x.to(dtype) for x in (qd, kd, vd)], layout, b, heads, m, n)
        out_dtype = torch.float32 if out_f32 else dtype
        outh = torch.full((b, m, heads, D), float("nan"), device=dev, dtype=out_dtype).transpose(1, 2)
        lseh = torch.full((R, m), float("nan"), device=dev)
        planned = bool(rng.integers(0, 2))
        st = capi.sparse_attention_heads_many_mask_forward(b, m, n, D, nn, *topo, qh, kh, vh, scale, outh,
                                                           lseh, plan if planned else ws, planned=planned)
        assert st == 0, f"{tag}: heads status {st} (planned={planned})"
        flat = [x.reshape(R, -1, D) for x in (qh, kh, vh)]
        want, want_lse = ref_attention_many_mask(*flat, masks_d, scale)
        bound = OUT_TOL[score_range] + (0.0 if out_f32 else ULP[dtype])
        _check_attention(outh.reshape(R, m, D), lseh, want, want_lse, tag, "heads", bound)
        _single_mask_heads(capi, dev, case, qh, kh, vh, outh, lseh)


def _autograd_case(rng, it):
    """m != n, 1..4 masks with 1..4 heads, an empty mask first / in the middle / last."""
    m, n = _sizes(rng, (15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 255, 257))
    if m == n:
        n = m + 1 if m < 257 else m - 1
    b, heads = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    dense, kinds = _masks(rng, b, m, n, EMPTY_AT[it % len(EMPTY_AT)])
    return b, heads, m, n, dense, kinds


def _grad_check(got, want, tol, tag, what):
    """rel_err_torch; values below the smallest normal of got's type count as 0 on both sides
    (a float16 gradient row of a key that only near-zero weights reach lies there whole)."""
    assert got is not None, f"{tag}: no gradient for {what}"
    tiny = torch.finfo(got.dtype).tiny
    flush = lambda x: x.masked_fill(x.abs() < tiny, 0.0)
    err = rel_err_torch(flush(got.detach().double()), flush(want.double()))
    assert err < tol, f"{tag}: {what} rel_err {err:.3g}"


def test_fuzz_many_mask_attention_autograd(dev, plan_cache_default):
    """functional.sparse_attention_many_mask and _heads_many_mask at m != n: forward and the
    three gradients against float64 dense autograd, float32 / float16 / bfloat16; the
    plan cache on for every other case (a planned topology at m != n through its key)."""
    from torch_sputnik_amd import dense_to_sparse_3d
    F = plan_cache_default
    rng = np.random.default_rng(4242 + SEED_SHIFT)
    for it in range(9 * SCALE):
        b, heads, m, n, dense, kinds = _autograd_case(rng, it)
        dtype = (torch.float32, torch.float16, torch.bfloat16)[it % 3]
        cached = it % 2 == 1
        F.enable_plan_cache(True if cached else F.PLAN_CACHE_DEFAULT)
        # (test_autograd_both_forms's bounds; float32 at 5e-4: the recomputed softmax gradient
        # of full rows and single-entry rows cancels, and the composed backward does not sum
        # in one fixed order -- 1.1e-4 to 2.3e-4 measured on the same inputs)
        tol = {torch.float32: 5e-4, torch.float16: 5e-3, torch.bfloat16: 3e-2}[dtype]
        masks_d = torch.from_numpy(dense).to(dev)
        ri, ro, ci, nnz = (x.to(dev) if torch.is_tensor(x) else x for x in dense_to_sparse_3d(masks_d))
        R, scale = b * heads, 0.125
        tag = f"autograd case {it}: b={b} heads={heads} m={m} n={n} nnz={nnz} kinds={kinds} dtype={dtype} cache={cached}"
        q, k, v = (T(x, dev).to(dtype) for x in _qkv(rng, R, m, n, "narrow", scale))
        g = torch.randn(R, m, D, device=dev).to(dtype).float()   # (rounded as autograd hands it over)
        xd = [x.detach().double().requires_grad_(True) for x in (q, k, v)]
        want = ref_attention_many_mask(*xd, masks_d, scale)[0]
        (want * g.double()).sum().backward()
        # [R, S, D] form (twice with the cache on: the second call takes the cached plan)
        for _ in range(2 if cached else 1):
            xs = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
            out = F.sparse_attention_many_mask(b, m, n, nnz, ri, ro, ci, *xs, scale)
            assert out.dtype == dtype and out.shape == (R, m, D), tag
            _grad_check(out, want.detach(), tol, tag, "forward")
            (out.float() * g).sum().backward()
            for name, x, w in zip("qkv", xs, xd):
                assert x.grad.dtype == dtype, tag
                _grad_check(x.grad, w.grad, tol, tag, f"[R, S, D] grad {name}")
        # [B, S, H, D] form: query alone, key and value views of one [B, n, H, 2D] tensor
        q4 = q.detach().reshape(b, heads, m, D).transpose(1, 2).contiguous().requires_grad_(True)
        kv = torch.cat([x.detach().reshape(b, heads, n, D).transpose(1, 2) for x in (k, v)], -1)
        kv.requires_grad_(True)
        out4 = F.sparse_attention_heads_many_mask(q4, kv[..., :D], kv[..., D:], nnz, ri, ro, ci, scale)
        assert out4.shape == (b, m, heads, D) and out4.dtype == dtype, tag
        _grad_check(out4.transpose(1, 2).reshape(R, m, D), want.detach(), tol, tag, "heads forward")
        (out4.float() * g.reshape(b, heads, m, D).transpose(1, 2)).sum().backward()
        per_head = lambda t: t.transpose(1, 2).reshape(R, -1, D)
        _grad_check(per_head(q4.grad), xd[0].grad, tol, tag, "heads grad q")
        _grad_check(per_head(kv.grad[..., :D]), xd[1].grad, tol, tag, "heads grad k")
        _grad_check(per_head(kv.grad[..., D:]), xd[2].grad, tol, tag, "heads grad v")


def test_fuzz_many_mask_dropin_functions_autograd(dev):
    """SpmmManyMask, SddmmManyMask and CsrSoftmaxManyMask (the reference's drop-in functions)
    at m != n: outputs and the gradients of values / dense, lhs / rhs and scores against
    float64 autograd."""
    from torch_sputnik_amd import dense_to_sparse_3d
    from torch_sputnik_amd.functional import CsrSoftmaxManyMask, SddmmManyMask, SpmmManyMask
    rng = np.random.default_rng(777 + SEED_SHIFT)
    for it in range(9 * SCALE):
        b, heads, m, n, dense, kinds = _autograd_case(rng, it)
        R = b * heads
        masks_d = torch.from_numpy(dense).to(dev)
        ri, ro, ci, nnz = (x.to(dev) if torch.is_tensor(x) else x for x in dense_to_sparse_3d(masks_d))
        width = max(nnz)
        entries = many_mask_entries(nnz, ro, ci, m, heads, dev)
        tag = f"drop-in case {it}: b={b} heads={heads} m={m} n={n} nnz={nnz} kinds={kinds}"
        rnd = lambda *s: torch.from_numpy(rng.uniform(-1, 1, s).astype(np.float32)).to(dev)

        # SpMM: values [R, width + pad] (padding: gradient 0), dense [R, n, cols]
        cols = int(rng.choice([7, 64, 72]))
        values = rnd(R, width + int(rng.integers(0, 3))).requires_grad_(True)
        dns = rnd(R, n, cols).requires_grad_(True)
        out = SpmmManyMask.apply(b, m, n, nnz, values, ri, ro, ci, dns)
        vd, dd = (x.detach().double().requires_grad_(True) for x in (values, dns))
        want = ref_spmm_many_mask(entries, m, vd, dd)
        _grad_check(out, want.detach(), TOL, tag, f"spmm forward cols={cols}")
        g = rnd(R, m, cols)
        out.backward(g)
        want.backward(g.double())
        _grad_check(values.grad, vd.grad, TOL, tag, "spmm grad values")
        _grad_check(dns.grad, dd.grad, TOL, tag, "spmm grad dense")

        # SDDMM: lhs [R, m, inner], rhs [R, n, inner] -> [R, width]
        inner = int(rng.choice([8, 64, 72]))
        lhs, rhs = rnd(R, m, inner).requires_grad_(True), rnd(R, n, inner).requires_grad_(True)
        out = SddmmManyMask.apply(b, m, n, nnz, ri, ro, ci, lhs, rhs)
        ld, rd = (x.detach().double().requires_grad_(True) for x in (lhs, rhs))
        want = ref_sddmm_many_mask(entries, width, ld, rd)
        _grad_check(out, want.detach(), TOL, tag, f"sddmm forward inner={inner}")
        g = rnd(R, width)
        out.backward(g)
        want.backward(g.double())
        _grad_check(lhs.grad, ld.grad, TOL, tag, "sddmm grad lhs")
        _grad_check(rhs.grad, rd.grad, TOL, tag, "sddmm grad rhs")

        # softmax (scaled) of the scores
        scale = float(rng.choice([1.0, 0.125]))
        scores = (3 * rnd(R, width)).requires_grad_(True)
        out = CsrSoftmaxManyMask.apply(b, m, nnz, scores, ri, ro, ci, scale)
        sd = scores.detach().double().requires_grad_(True)
        want = ref_softmax_many_mask(entries, m, n, sd, scale)
        _grad_check(out, want.detach(), TOL, tag, f"softmax forward scale={scale}")
        g = rnd(R, width)
        out.backward(g)
        want.backward(g.double())
        _grad_check(scores.grad, sd.grad, TOL, tag, "softmax grad scores")
