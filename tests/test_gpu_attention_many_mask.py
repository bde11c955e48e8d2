"""GPU: the fused attention with one mask per batch element (C ABI
sputnik_hip_sparse_attention_many_mask_* / heads_many_mask_*, the torch ops, the autograd
forms and SparseCoreAttention) against the dense float64 masked softmax."""
import math

import numpy as np
import pytest
import torch

from helpers import rel_err_torch

pytestmark = pytest.mark.gpu

D = 64
UNSUPPORTED = -2
DENSITIES = (0.1, 0.5, 0.05, 0.2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def capi():
    from torch_sputnik_amd import capi
    return capi


def _dense_masks(masks, s, seed, empty_mask=None, empty_rows=True):
    rng = np.random.default_rng(seed)
    dense = np.zeros((masks, s, s), dtype=bool)
    for i in range(masks):
        dense[i] = rng.random((s, s)) < DENSITIES[i % len(DENSITIES)]
        if empty_rows:
            dense[i, rng.choice(s, size=max(1, s // 16), replace=False)] = False
    if empty_mask is not None:
        dense[empty_mask] = False
    return dense


def _topology(dense, dev, unsorted_mask=None, seed=0):
    """Many-mask layout of the [b, s, s] masks (topology.dense_to_sparse_3d); the rows of
    `unsorted_mask` with more than one entry get their columns in reversed / shuffled order."""
    from torch_sputnik_amd import dense_to_sparse_3d
    ri, ro, ci, nnz = dense_to_sparse_3d(torch.from_numpy(dense))
    if unsorted_mask is not None:
        rng = np.random.default_rng(seed)
        ci = ci.clone()
        first = sum(nnz[:unsorted_mask])
        offs = ro[unsorted_mask]
        for r in range(0, offs.numel() - 1, 3):
            a, b = first + int(offs[r]), first + int(offs[r + 1])
            if b - a > 1:
                ci[a:b] = ci[a:b][torch.from_numpy(rng.permutation(b - a))]
    return ri.to(dev), ro.to(dev), ci.to(dev), nnz


def _reference(q, k, v, dense, scale):
    """float64 dense masked softmax per replica (replica r under mask r // heads) -> out, lse."""
    q, k, v = (x.to(torch.float64) for x in (q, k, v))
    R, b = q.size(0), dense.shape[0]
    heads = R // b
    mask = torch.from_numpy(dense).to(q.device)
    out = torch.empty_like(q)
    lse = torch.empty(q.shape[:2], dtype=torch.float64, device=q.device)
    for r in range(R):
        m = mask[r // heads]
        s = (scale * q[r] @ k[r].T).masked_fill(~m, float("-inf"))
        lse[r] = torch.logsumexp(s, dim=-1)
        w = torch.softmax(s, dim=-1).nan_to_num(0.0)
        out[r] = w @ v[r]
    return out, lse


def _qkv(R, s, dev, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.empty(R, s, D).uniform_(-2, 2, generator=g).to(dev, dtype) for _ in range(3)]


def _check(out, lse, want, want_lse):
    assert not torch.isnan(out).any(), "some output elements were never written"
    assert rel_err_torch(out, want) < 1e-4
    finite = torch.isfinite(want_lse)
    assert torch.equal(torch.isneginf(lse), ~finite)
    if finite.any():
        err = (lse.double() - want_lse)[finite].abs().max()
        assert float(err) < 1e-4 * (1 + float(want_lse[finite].abs().max()))


def _run_f32(capi, dev, masks, topo, q, k, v, scale, planned=False, ws=None):
    ri, ro, ci, nnz = topo
    R, s = q.shape[:2]
    if ws is None:
        ws = torch.empty(capi.sparse_attention_many_mask_workspace_bytes(masks, s, s, D, max(nnz)),
                         dtype=torch.uint8, device=dev)
    out = torch.full((R, s, D), float("nan"), device=dev)
    lse = torch.full((R, s), float("nan"), device=dev)
    st = capi.sparse_attention_many_mask_forward(masks, s, s, D, nnz, R, ri, ro, ci, q, k, v, scale,
                                                 out, lse, ws, planned=planned)
    assert st == 0
    return out, lse


@pytest.mark.parametrize("s", [64, 130, 1024])
@pytest.mark.parametrize("heads", [1, 2, 8])
@pytest.mark.parametrize("masks", [1, 2, 3, 8])
def test_capi_vs_float64(capi, dev, masks, heads, s):
    empty = 1 if masks > 1 else None
    dense = _dense_masks(masks, s, seed=masks * 100 + heads * 10 + s, empty_mask=empty)
    topo = _topology(dense, dev, unsorted_mask=masks - 1 if masks != 2 else 0, seed=s)
    R = masks * heads
    q, k, v = _qkv(R, s, dev, seed=s + R)
    scale = 1.0 / math.sqrt(D)
    out, lse = _run_f32(capi, dev, masks, topo, q, k, v, scale)
    want, want_lse = _reference(q, k, v, dense, scale)
    _check(out, lse, want, want_lse)
    if empty is not None:
        assert not out[empty * heads:(empty + 1) * heads].any()


def test_capi_every_mask_empty(capi, dev):
    masks, heads, s = 3, 2, 64
    dense = np.zeros((masks, s, s), dtype=bool)
    topo = _topology(dense, dev)
    q, k, v = _qkv(masks * heads, s, dev, seed=5)
    out, lse = _run_f32(capi, dev, masks, topo, q, k, v, 0.125)
    assert not out.any() and torch.isneginf(lse).all()


def test_identical_masks_match_single_mask_kernel_bitwise(capi, dev):
    from helpers import make_csr
    s, masks, heads = 130, 3, 2
    _, _, ri, ro, ci = make_csr(s, s, 0.8, seed=7, empty_rows=(3,))
    ri_t, ro_t, ci_t = (torch.from_numpy(x).to(dev) for x in (ri, ro, ci))
    topo = (ri_t.repeat(masks), ro_t.repeat(masks), ci_t.repeat(masks), [len(ci)] * masks)
    R = masks * heads
    q, k, v = _qkv(R, s, dev, seed=11)
    out, lse = _run_f32(capi, dev, masks, topo, q, k, v, 0.125)
    ws = torch.empty(capi.sparse_attention_workspace_bytes(s, s, D, len(ci)), dtype=torch.uint8, device=dev)
    want = torch.empty_like(out)
    want_lse = torch.empty_like(lse)
    capi.sparse_attention_forward(s, s, D, R, ri_t, ro_t, ci_t, q, k, v, 0.125, want, want_lse, ws)
    assert torch.equal(out, want) and torch.equal(lse, want_lse)
    # the heads form against the single-mask heads kernel
    for dtype in (torch.float16, torch.bfloat16):
        qh, kh, vh = (x.to(dtype).reshape(masks, heads, s, D) for x in (q, k, v))
        got = torch.empty(masks, heads, s, D, dtype=dtype, device=dev)
        st = capi.sparse_attention_heads_many_mask_forward(masks, s, s, D, topo[3], *topo[:3], qh, kh, vh,
                                                           0.125, got, None, ws_many(capi, dev, masks, s, topo[3]))
        assert st == 0
        ref = torch.empty_like(got)
        capi.sparse_attention_heads_forward(s, s, D, ri_t, ro_t, ci_t, qh, kh, vh, 0.125, ref, None, ws)
        assert torch.equal(got, ref)


def ws_many(capi, dev, masks, s, nnz):
    return torch.empty(capi.sparse_attention_many_mask_workspace_bytes(masks, s, s, D, max(nnz)),
                       dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_mask_order_does_not_matter(capi, dev, order):
    masks, heads, s = 4, 2, 130
    dense = _dense_masks(masks, s, seed=21)
    counts = dense.reshape(masks, -1).sum(1)
    perm = np.argsort(counts if order == "ascending" else -counts, kind="stable")
    topo = _topology(dense, dev)
    topo_p = _topology(dense[perm], dev)
    q, k, v = _qkv(masks * heads, s, dev, seed=22)
    out, lse = _run_f32(capi, dev, masks, topo, q, k, v, 0.125)
    rperm = torch.from_numpy(np.repeat(perm * heads, heads) + np.tile(np.arange(heads), masks)).to(dev)
    out_p, lse_p = _run_f32(capi, dev, masks, topo_p, q[rperm], k[rperm], v[rperm], 0.125)
    assert torch.equal(out_p, out[rperm]) and torch.equal(lse_p, lse[rperm])


def test_planned_equals_unplanned(capi, dev):
    masks, heads, s = 3, 2, 130
    dense = _dense_masks(masks, s, seed=31)
    topo = _topology(dense, dev, unsorted_mask=1)
    ws = ws_many(capi, dev, masks, s, topo[3])
    assert capi.sparse_attention_many_mask_plan(masks, s, s, D, topo[3], *topo[:3], ws) == 0
    for seed in (1, 2):
        q, k, v = _qkv(masks * heads, s, dev, seed=seed)
        got = _run_f32(capi, dev, masks, topo, q, k, v, 0.125, planned=True, ws=ws)
        want = _run_f32(capi, dev, masks, topo, q, k, v, 0.125)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_heads_views_from_qkv(capi, dev, dtype, out_f32):
    masks, heads, s = 3, 4, 130
    dense = _dense_masks(masks, s, seed=41, empty_mask=2)
    topo = _topology(dense, dev, unsorted_mask=0)
    g = torch.Generator(device="cpu").manual_seed(42)
    qkv = torch.empty(masks, s, heads, 3 * D).uniform_(-2, 2, generator=g).to(dev, dtype)
    q, k, v = (qkv[..., i * D:(i + 1) * D].transpose(1, 2) for i in range(3))   # [B, H, S, D] views
    out = torch.full((masks, s, heads, D), float("nan"), device=dev,
                     dtype=torch.float32 if out_f32 else dtype).transpose(1, 2)
    lse = torch.full((masks * heads, s), float("nan"), device=dev)
    st = capi.sparse_attention_heads_many_mask_forward(masks, s, s, D, topo[3], *topo[:3], q, k, v, 0.125,
                                                       out, lse, ws_many(capi, dev, masks, s, topo[3]))
    assert st == 0
    flat = [x.reshape(masks * heads, s, D) for x in (q, k, v)]
    want, want_lse = _reference(*flat, dense, 0.125)
    got = out.reshape(masks * heads, s, D).float()
    assert not torch.isnan(got).any()
    if out_f32:
        _check(got, lse, want, want_lse)
    else:
        assert rel_err_torch(got, want) < (4e-3 if dtype == torch.float16 else 2e-2)
    # through the op: same bits as the C ABI
    from torch_sputnik_amd import ops
    via_op = ops.sparse_attention_heads_many_mask(masks, topo[3], *topo[:3], q, k, v, 0.125,
                                                  out_dtype=out.dtype)
    assert torch.equal(via_op, out)


def _dense_reference_autograd(q, k, v, dense, scale):
    out, _ = _reference(q, k, v, dense, scale)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_autograd_both_forms(dev, dtype):
    from torch_sputnik_amd import functional as F
    masks, heads, s = 2, 2, 130
    dense = _dense_masks(masks, s, seed=51)
    ri, ro, ci, nnz = _topology(dense, dev)
    scale = 1.0 / math.sqrt(D)
    q, k, v = (x.to(dtype) for x in _qkv(masks * heads, s, dev, seed=52))
    tol = {torch.float32: 1e-4, torch.float16: 5e-3, torch.bfloat16: 3e-2}[dtype]
    # (the gradient reaches a half output rounded to its type: the reference takes it so)
    g = torch.randn(masks * heads, s, D, device=dev).to(dtype).float()
    xd = [x.detach().double().requires_grad_(True) for x in (q, k, v)]
    want = _dense_reference_autograd(*xd, dense, scale)
    (want * g.double()).sum().backward()
    # [R, S, D] form
    xs = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
    out = F.sparse_attention_many_mask(masks, s, s, nnz, ri, ro, ci, *xs, scale)
    assert out.dtype == dtype
    assert rel_err_torch(out.float(), want.detach()) < tol
    (out.float() * g).sum().backward()
    for x, w in zip(xs, xd):
        assert x.grad.dtype == dtype
        assert rel_err_torch(x.grad.float(), w.grad) < tol
    # [B, S, H, D] form (views of one [B, S, H, 3D] tensor)
    qkv = torch.cat([x.detach().reshape(masks, heads, s, D).transpose(1, 2) for x in (q, k, v)], -1)
    qkv.requires_grad_(True)
    views = [qkv[..., i * D:(i + 1) * D] for i in range(3)]
    out4 = F.sparse_attention_heads_many_mask(*views, nnz, ri, ro, ci, scale)
    g4 = g.reshape(masks, heads, s, D).transpose(1, 2)
    assert rel_err_torch(out4.float().transpose(1, 2).reshape(-1, s, D), want.detach()) < tol
    (out4.float() * g4).sum().backward()
    for i, w in enumerate(xd):
        got = qkv.grad[..., i * D:(i + 1) * D].transpose(1, 2).reshape(-1, s, D)
        assert rel_err_torch(got.float(), w.grad) < tol


def test_autograd_d32_takes_the_composition(capi, dev):
    from torch_sputnik_amd import functional as F
    masks, heads, s, d = 2, 2, 64, 32
    dense = _dense_masks(masks, s, seed=61)
    ri, ro, ci, nnz = _topology(dense, dev)
    assert capi.sparse_attention_many_mask_workspace_bytes(masks, s, s, d, max(nnz)) == 0
    g = torch.Generator(device="cpu").manual_seed(62)
    q, k, v = (torch.empty(masks * heads, s, d).uniform_(-2, 2, generator=g).to(dev).requires_grad_(True)
               for _ in range(3))
    out = F.sparse_attention_many_mask(masks, s, s, nnz, ri, ro, ci, q, k, v, 0.2)
    xd = [x.detach().double().requires_grad_(True) for x in (q, k, v)]
    want = _dense_reference_autograd(*xd, dense, 0.2)
    assert rel_err_torch(out, want.detach()) < 1e-4
    out.sum().backward()
    want.sum().backward()
    for x, w in zip((q, k, v), xd):
        assert rel_err_torch(x.grad, w.grad) < 1e-4


def _module_reference(query, key, value, dense, hn):
    """float64 restatement of the reference module's forward (tests/transformer/modules.py:24-81)."""
    b, s, n, _ = query.shape
    q, k, v = (x.double().permute(0, 2, 1, 3).reshape(b * n, s, hn) for x in (query, key, value))
    out = _dense_reference_autograd(q, k, v, dense, 1.0 / math.sqrt(hn))
    return out.permute(1, 0, 2).reshape(s, b, n * hn)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_core_attention_module_small(dev, dtype):
    from torch_sputnik_amd import SparseCoreAttention
    b, n, s, hn = 2, 2, 128, 64
    dense = _dense_masks(b, s, seed=71)
    mask = torch.from_numpy(dense).to(dev).unsqueeze(1).to(torch.int64)
    g = torch.Generator(device="cpu").manual_seed(72)
    qkv = torch.empty(b, s, n, 3 * hn).uniform_(-2, 2, generator=g).to(dev, dtype).requires_grad_(True)
    q, k, v = torch.split(qkv, hn, dim=-1)
    mod = SparseCoreAttention(s, n * hn, n)
    out = mod(q, k, v, mask)
    assert out.shape == (s, b, n * hn) and out.dtype == dtype
    qd = qkv.detach().double().requires_grad_(True)
    want = _module_reference(*torch.split(qd, hn, dim=-1), dense, hn)
    tol = 1e-4 if dtype == torch.float32 else 5e-3
    assert rel_err_torch(out.float(), want.detach()) < tol
    grad = torch.randn(s, b, n * hn, device=dev).to(dtype).float()   # (rounded as autograd does)
    (out.float() * grad).sum().backward()
    (want * grad.double()).sum().backward()
    assert rel_err_torch(qkv.grad.float(), qd.grad) < tol


def test_core_attention_module_full_size(dev):
    from torch_sputnik_amd import SparseCoreAttention, dense_to_sparse_3d
    b, n, s, hn = 8, 8, 1024, 64
    dense = _dense_masks(b, s, seed=81, empty_rows=False)
    topology = dense_to_sparse_3d(torch.from_numpy(dense).to(dev).unsqueeze(1))
    g = torch.Generator(device="cpu").manual_seed(82)
    q, k, v = (torch.empty(b, s, n, hn).uniform_(-2, 2, generator=g).to(dev) for _ in range(3))
    with torch.no_grad():
        out = SparseCoreAttention(s, n * hn, n)(q, k, v, None, topology=topology)
    want = _module_reference(q, k, v, dense, hn)
    assert rel_err_torch(out, want) < 1e-4


def test_graph_replay_matches_eager(dev):
    from torch_sputnik_amd import ops
    masks, heads, s = 4, 2, 130
    dense = _dense_masks(masks, s, seed=91)
    ri, ro, ci, nnz = _topology(dense, dev)
    plan = ops.sparse_attention_many_mask_plan(masks, s, s, D, nnz, ri, ro, ci)
    q, k, v = _qkv(masks * heads, s, dev, seed=92)
    static = [x.clone() for x in (q, k, v)]
    ops.sparse_attention_many_mask_planned(masks, nnz, ri, ro, ci, *static, 0.125, plan)   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sparse_attention_many_mask_planned(masks, nnz, ri, ro, ci, *static, 0.125, plan)
    for seed in (93, 94):
        fresh = _qkv(masks * heads, s, dev, seed=seed)
        for dst, src in zip(static, fresh):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.sparse_attention_many_mask(masks, nnz, ri, ro, ci, *fresh, 0.125)
        assert torch.equal(out, eager)


def test_errors(capi, dev):
    from torch_sputnik_amd import functional as F
    masks, heads, s = 2, 2, 64
    dense = _dense_masks(masks, s, seed=101)
    ri, ro, ci, nnz = _topology(dense, dev)
    q, k, v = _qkv(masks * heads, s, dev, seed=102)
    out = torch.empty_like(q)
    ws = ws_many(capi, dev, masks, s, nnz)
    invalid = capi.sparse_attention_many_mask_forward(masks, s, s, D, nnz, 3, ri, ro, ci, q, k, v, 0.1, out,
                                                      None, ws)
    assert invalid not in (0, UNSUPPORTED)
    small = ws[:ws.numel() - 256]
    assert capi.sparse_attention_many_mask_forward(masks, s, s, D, nnz, 4, ri, ro, ci, q, k, v, 0.1, out,
                                                   None, small) == invalid
    # the heads form: batch must equal the number of masks
    qh, kh, vh, oh = (x.reshape(4, 1, s, D).half() for x in (q, k, v, out))
    assert capi.sparse_attention_heads_many_mask_forward(masks, s, s, D, nnz, ri, ro, ci, qh, kh, vh, 0.1,
                                                         oh, None, ws) == invalid
    d = 32
    q2, k2, v2 = (x[..., :d].contiguous() for x in (q, k, v))
    out2 = torch.empty_like(q2)
    assert capi.sparse_attention_many_mask_forward(masks, s, s, d, nnz, 4, ri, ro, ci, q2, k2, v2, 0.1,
                                                   out2, None, ws) == UNSUPPORTED
    got = F.sparse_attention_many_mask(masks, s, s, nnz, ri, ro, ci, q2, k2, v2, 0.1)
    want, _ = _reference(q2, k2, v2, dense, 0.1)
    assert rel_err_torch(got, want) < 1e-4
