"""GPU: attention on float16 / bfloat16 storage -- SparseAttention(half_storage=True).

  * the fused kernel on strided head views (ops.sparse_attention_heads, the C ABI's
    sputnik_hip_sparse_attention_heads_*) against float64 computed on the same half inputs:
    2-D / 3-D / 4-D views, slices of [B, S, E] and of one [B, S, 3E], out in float32 or
    in the storage type, planned and unplanned, lse, empty rows, a row block with
    shuffled columns (the order-independent path), m != n, unaligned views (fallback);
  * the row-orientation tile forward (ops.half_linear_rows) against float64;
  * the module: forward and forward + backward against dense float64 autograd with the
    rounding contract (the projections' outputs, the context and the output rounded to
    the storage type), no widening pass on served shapes, determinism and graph replay,
    and the flag leaving float32 inputs and the default mode alone.
"""
import math

import numpy as np
import pytest
import torch

from helpers import make_csr, rel_err_torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
# the module's norm-relative bounds (test_gpu_callers.py, C5)
MODULE_TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
HALF = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tsa():
    import torch_sputnik_amd
    from torch_sputnik_amd import capi, functional, graphs, ops  # noqa: F401  (attributes of the package)
    return torch_sputnik_amd


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def dense_mask(m, n, ro, ci, dev):
    mask = torch.zeros(m, n, dtype=torch.bool, device=dev)
    rows = torch.repeat_interleave(torch.arange(m, device=dev), T(np.diff(ro).astype(np.int64), dev))
    mask[rows, T(ci.astype(np.int64), dev)] = True
    return mask


def reference(q, k, v, mask, scale):
    """[.., m, d] x [.., n, d] -> (out, lse) in float64; rows without entries: 0, -inf."""
    scores = torch.matmul(q.double(), k.double().transpose(-1, -2)) * scale
    scores = scores.masked_fill(~mask, float("-inf"))
    out = torch.matmul(torch.nan_to_num(torch.softmax(scores, dim=-1)), v.double())
    return out, torch.logsumexp(scores, dim=-1)


def check_out(got, want, out_dtype, dtype):
    assert got.dtype == out_dtype
    assert not torch.isnan(got).any()
    bound = TOL if out_dtype == torch.float32 else TOL + ULP[dtype]
    assert rel_err_torch(got, want) < bound


def topology(m, n, sparsity, seed, dev, empty=(), order="ascending", shuffle_every=0):
    _, _, ri, ro, ci = make_csr(m, n, sparsity, seed=seed, empty_rows=empty, order=order)
    if shuffle_every:   # rows whose columns do not ascend: the order-independent path
        rng = np.random.default_rng(seed)
        ci = ci.copy()
        for r in range(0, m, shuffle_every):
            ci[ro[r]:ro[r + 1]] = ci[ro[r]:ro[r + 1]][rng.permutation(ro[r + 1] - ro[r])]
    return [T(x, dev) for x in (ri, ro, ci)], dense_mask(m, n, ro, ci, dev)


# ----------------------------------------------------------------------------
# the fused kernel on head views
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("planned", [False, True])
@pytest.mark.parametrize("layout", ["2d", "3d", "heads", "packed"])
def test_heads_kernel_vs_float64(tsa, dev, dtype, out_f32, planned, layout):
    ops, functional = tsa.ops, tsa.functional
    batch, heads, d = 2, 3, 64
    m, n = (200, 300) if layout != "packed" else (256, 256)   # (packed: one [B, S, 3E] tensor)
    topo, mask = topology(m, n, 0.85, seed=m + n, dev=dev, empty=(0, 17, m - 1))
    g = torch.Generator(device="cpu").manual_seed(m)
    rnd = lambda *s: torch.empty(*s).uniform_(-2, 2, generator=g).to(dtype).to(dev)
    if layout == "2d":
        q, k, v = rnd(m, d), rnd(n, d), rnd(n, d)
    elif layout == "3d":
        q, k, v = rnd(batch * heads, m, d), rnd(batch * heads, n, d), rnd(batch * heads, n, d)
    elif layout == "heads":   # [B, S, E] tensors, heads as strided views
        q, k, v = (functional._heads(rnd(batch, s, heads * d), heads) for s in (m, n, n))
    else:
        qkv = rnd(batch, m, 3 * heads * d)
        q, k, v = (functional._heads(qkv[..., i * heads * d:(i + 1) * heads * d], heads) for i in range(3))
        assert not q.is_contiguous()
    scale = 1.0 / math.sqrt(d)
    plan = ops.sparse_attention_plan(m, n, d, *topo) if planned else None
    out_dtype = torch.float32 if out_f32 else dtype
    out, lse = ops.sparse_attention_heads(q, k, v, *topo, scale, out_dtype=out_dtype, with_lse=True,
                                          plan=plan)
    assert out.shape == q.shape
    want, want_lse = reference(q, k, v, mask, scale)
    check_out(out, want, out_dtype, dtype)
    if layout in ("heads", "packed"):   # the context comes back as a view of [B, S, E]
        assert out.transpose(1, 2).is_contiguous()
    for r in (0, 17, m - 1):
        assert not out[..., r, :].any()
    finite = torch.isfinite(want_lse)
    assert torch.equal(torch.isneginf(lse), ~finite)
    assert torch.max(torch.abs(lse.double() - want_lse)[finite]) < 1e-4 * (1 + want_lse[finite].abs().max())


@pytest.mark.parametrize("dtype", HALF)
def test_heads_kernel_order_independent_path(tsa, dev, dtype):
    """Row blocks with shuffled columns: the kernel's order-independent path on half storage."""
    m, n, d, batch, heads = 256, 256, 64, 2, 2
    topo, mask = topology(m, n, 0.85, seed=77, dev=dev, shuffle_every=5)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = [torch.empty(batch, s, heads * d).uniform_(-1, 1, generator=g).to(dtype).to(dev) for s in (m, n, n)]
    q, k, v = (tsa.functional._heads(t, heads) for t in x)
    out = tsa.ops.sparse_attention_heads(q, k, v, *topo, 0.125)
    want, _ = reference(q, k, v, mask, 0.125)
    check_out(out, want, dtype, dtype)


@pytest.mark.parametrize("dtype", HALF)
def test_heads_kernel_c_abi(tsa, dev, dtype):
    """The C ABI directly: supported predicate, planned and unplanned forward, lse."""
    capi = tsa.capi
    m, n, d, batch, heads = 128, 384, 64, 2, 4
    topo, mask = topology(m, n, 0.9, seed=3, dev=dev, empty=(5,))
    g = torch.Generator(device="cpu").manual_seed(4)
    x = [torch.empty(batch, s, heads * d).uniform_(-2, 2, generator=g).to(dtype).to(dev) for s in (m, n, n)]
    q, k, v = (tsa.functional._heads(t, heads) for t in x)
    nnz = topo[2].numel()
    want, want_lse = reference(q, k, v, mask, 0.125)
    for out_dtype in (torch.float32, dtype):
        out = tsa.functional._heads(torch.full((batch, m, heads * d), float("nan"), dtype=out_dtype,
                                               device=dev), heads)
        assert capi.sparse_attention_heads_supported(m, n, d, nnz, q, k, v, out)
        ws = torch.empty(capi.sparse_attention_heads_workspace_bytes(m, n, d, nnz), dtype=torch.uint8,
                         device=dev)
        lse = torch.full((batch * heads, m), float("nan"), device=dev)
        capi.sparse_attention_heads_forward(m, n, d, *topo, q, k, v, 0.125, out, lse, ws)
        check_out(out, want, out_dtype, dtype)
        assert torch.isneginf(lse[:, 5]).all()
        planned = torch.full_like(out, float("nan"))
        capi.sparse_attention_plan(m, n, d, *topo, ws)
        capi.sparse_attention_heads_forward(m, n, d, *topo, q, k, v, 0.125, planned, None, ws, planned=True)
        assert torch.equal(planned, out)
        assert torch.allclose(lse.double().reshape(want_lse.shape)[torch.isfinite(want_lse)],
                              want_lse[torch.isfinite(want_lse)], atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("how", ["offset", "row_stride", "head_dim"])
def test_heads_kernel_unserved_views_fall_back(tsa, dev, dtype, how):
    """A view the kernel cannot serve never reaches it: _supported answers 0 and the op
    composes the typed operators -- still the right answer."""
    m = n = 128
    heads, d = 2, 64 if how != "head_dim" else 32
    topo, mask = topology(m, n, 0.8, seed=11, dev=dev, empty=(3,))
    g = torch.Generator(device="cpu").manual_seed(6)
    width = heads * d + (4 if how == "row_stride" else 0)       # row stride not a multiple of 8
    base = torch.empty(3, 2, m, width + 1).uniform_(-1, 1, generator=g).to(dtype).to(dev)
    start = 1 if how == "offset" else 0                          # storage offset of one element
    q, k, v = (tsa.functional._heads(base[i, :, :, start:start + heads * d], heads) for i in range(3))
    if how != "head_dim":
        out = torch.empty_like(q)
        assert not tsa.capi.sparse_attention_heads_supported(m, n, d, topo[2].numel(), q, k, v, out)
    got = tsa.ops.sparse_attention_heads(q, k, v, *topo, 0.2)
    want, _ = reference(q, k, v, mask, 0.2)
    check_out(got, want, dtype, dtype)
    ctx = tsa.functional.sparse_attention_heads(base[0, :, :, start:start + heads * d],
                                                base[1, :, :, start:start + heads * d],
                                                base[2, :, :, start:start + heads * d], heads, *topo, 0.2)
    assert ctx.shape == (2, m, heads * d)
    check_out(ctx, want.transpose(1, 2).reshape(2, m, heads * d), dtype, dtype)


# ----------------------------------------------------------------------------
# the row-orientation tile forward
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("values_half", [False, True])
@pytest.mark.parametrize("into_packed", [False, True])
def test_half_linear_rows_vs_float64(tsa, dev, dtype, values_half, into_packed):
    ops = tsa.ops
    out_f, in_f, seq, batch = 512, 512, 1024, 8
    _, vals, ri, ro, ci = make_csr(out_f, in_f, 0.8, seed=21)
    values = T(vals, dev)
    # a wide range: the float16 planes' shift must be undone exactly
    values = values * 1e3
    if values_half:
        values = values.to(dtype)
    ro_t, ci_t = T(ro, dev), T(ci, dev)
    assert ops.half_linear_rows_supported(out_f, in_f, seq, batch, ci_t.numel(), values.dtype, dtype)
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.empty(batch, seq, in_f).uniform_(-1, 1, generator=g).to(dtype).to(dev)
    image = ops.half_linear_image(out_f, in_f, values, ro_t, ci_t, dtype)
    w = torch.zeros(out_f, in_f, dtype=torch.float64, device=dev)
    rows = torch.repeat_interleave(torch.arange(out_f, device=dev), T(np.diff(ro).astype(np.int64), dev))
    w[rows, ci_t.long()] = values.double()
    want = torch.matmul(x.double(), w.t())
    y32 = ops.half_linear_rows(out_f, image, values.dtype, x, out_dtype=torch.float32)
    check_out(y32, want, torch.float32, dtype)
    if into_packed:
        packed = torch.full((batch, seq, 3 * out_f), float("nan"), dtype=dtype, device=dev)
        y = ops.half_linear_rows(out_f, image, values.dtype, x, out=packed[..., out_f:2 * out_f])
        assert y.data_ptr() == packed[..., out_f:].data_ptr()
        assert torch.isnan(packed[..., :out_f]).all() and torch.isnan(packed[..., 2 * out_f:]).all()
    else:
        y = ops.half_linear_rows(out_f, image, values.dtype, x)
    check_out(y, want, dtype, dtype)
    assert torch.equal(y, y32.to(dtype))


# ----------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------
def build_attention(tsa, dev, heads, embed, seq, seed, half_values=None, **flags):
    module = tsa.SparseAttention(heads, embed, max_sequence_length=seq, device=dev,
                                 mask_generator=np.random.default_rng(seed), **flags).to(dev)
    rng = np.random.default_rng(seed + 1)
    for layer in module.linears:
        w = rng.uniform(-1, 1, (embed, embed)) / math.sqrt(embed * 0.3)
        w = w * (rng.random((embed, embed)) < 0.3)
        with torch.no_grad():
            layer.weight.copy_(T(w.astype(np.float32), dev))
        layer.setup_sparse_tensors()
        if half_values is not None:
            layer.values = torch.nn.Parameter(layer.values.detach().to(half_values))
    return module


def dense_weights(module):
    out = []
    for layer in module.linears:
        w = torch.zeros(layer.output_features, layer.input_features, dtype=torch.float64,
                        device=layer.values.device)
        rows = torch.repeat_interleave(torch.arange(layer.output_features, device=w.device),
                                       (layer.row_offsets[1:] - layer.row_offsets[:-1]).long())
        w[rows, layer.column_indices.long()] = layer.values.detach().double()
        out.append(w.requires_grad_(True))
    return out


def dense_half_module(module, query, key, value, dtype, weights=None):
    """modules/sparse_attention.py:105-128 in float64 with the half mode's rounding points:
    q, k, v, the context and the output rounded to `dtype`."""
    heads, dim = module.num_heads, module.head_dim
    weights = dense_weights(module) if weights is None else weights
    rnd = lambda t: t + (t.to(dtype).double() - t).detach()   # rounding with a straight-through gradient
    batch, seq, _ = query.shape

    def project(x, w):
        return rnd(torch.matmul(x.double(), w.t()))

    q, k, v = (project(x, w).view(batch, seq, heads, dim).transpose(1, 2)
               for x, w in zip((query, key, value), weights))
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dim)
    scores = scores.masked_fill(module.mask2d.to(scores.device) == 0, float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1))
    context = rnd(torch.matmul(probs, v).transpose(1, 2).reshape(batch, seq, heads * dim))
    return project(context, weights[3])


def norm_rel(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


MODULE_SHAPES = [(4, 256, 256, 2), (8, 512, 1024, 2), (8, 512, 1024, 8)]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("heads,embed,seq,batch", MODULE_SHAPES)
def test_module_forward(tsa, dev, dtype, heads, embed, seq, batch):
    module = build_attention(tsa, dev, heads, embed, seq, seed=heads + seq, half_storage=True)
    g = torch.Generator(device="cpu").manual_seed(seq)
    q, k, v = (torch.empty(batch, seq, embed).uniform_(-1, 1, generator=g).to(dtype).to(dev) for _ in range(3))
    with torch.no_grad():
        out = module(q, k, v)
        want = dense_half_module(module, q, k, v, dtype)
    assert out.dtype == dtype and out.shape == (batch, seq, embed)
    assert norm_rel(out, want) < MODULE_TOL[dtype]


@pytest.mark.parametrize("dtype", HALF)
def test_module_forward_head_dim_32_falls_back(tsa, dev, dtype):
    module = build_attention(tsa, dev, 2, 64, 128, seed=5, half_storage=True)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.empty(2, 128, 64).uniform_(-1, 1, generator=g).to(dtype).to(dev)
    with torch.no_grad():
        out = module(x, x, x)
        want = dense_half_module(module, x, x, x, dtype)
    assert out.dtype == dtype
    assert norm_rel(out, want) < MODULE_TOL[dtype]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("values_half", [False, True])
@pytest.mark.parametrize("heads,embed,seq,batch", [(4, 256, 256, 2), (8, 512, 1024, 8)])
def test_module_backward(tsa, dev, dtype, shared, values_half, heads, embed, seq, batch):
    module = build_attention(tsa, dev, heads, embed, seq, seed=7, half_storage=True,
                             half_values=dtype if values_half else None)
    g = torch.Generator(device="cpu").manual_seed(2)
    mk = lambda: torch.empty(batch, seq, embed).uniform_(-1, 1, generator=g).to(dtype).to(dev).requires_grad_(True)
    if shared:
        x = mk()
        inputs = (x, x, x)
    else:
        inputs = (mk(), mk(), mk())
    go = torch.empty(batch, seq, embed).uniform_(-1, 1, generator=g).to(dtype).to(dev)
    out = module(*inputs)
    assert out.dtype == dtype
    out.backward(go)

    weights = dense_weights(module)
    dense_in = [t.detach().double().requires_grad_(True) for t in (inputs[:1] if shared else inputs)]
    dq, dk, dv = (dense_in * 3) if shared else dense_in
    want = dense_half_module(module, dq, dk, dv, dtype, weights)
    want.backward(go.double())
    tol = MODULE_TOL[dtype]
    assert norm_rel(out.detach(), want.detach()) < tol
    for t, td in zip(inputs[:1] if shared else inputs, dense_in):
        assert t.grad.dtype == dtype
        assert norm_rel(t.grad, td.grad) < tol
    for layer, w in zip(module.linears, weights):
        assert layer.values.grad.dtype == layer.values.dtype
        rows = torch.repeat_interleave(torch.arange(layer.output_features, device=dev),
                                       (layer.row_offsets[1:] - layer.row_offsets[:-1]).long())
        assert norm_rel(layer.values.grad, w.grad[rows, layer.column_indices.long()]) < tol


@pytest.mark.parametrize("dtype", HALF)
def test_module_no_widening_on_served_shapes(tsa, dev, dtype, monkeypatch):
    heads, embed, seq, batch = 8, 512, 1024, 8
    module = build_attention(tsa, dev, heads, embed, seq, seed=3, half_storage=True)
    lin = module.linears[0]
    assert tsa.ops.half_linear_rows_supported(embed, embed, seq, batch, lin.column_indices.numel(),
                                              lin.values.dtype, dtype)
    x = torch.empty(batch, seq, embed, device=dev).uniform_(-1, 1).to(dtype)
    with torch.no_grad():
        want = module(x, x, x)

    def refuse(*args, **kwargs):
        raise AssertionError("a layout pass ran on a served shape")

    monkeypatch.setattr(tsa.ops, "transpose_last2", refuse)
    monkeypatch.setattr(tsa.functional, "transpose_last2", refuse)
    with torch.no_grad():
        out = module(x, x, x)
    assert torch.equal(out, want)
    xg = x.clone().requires_grad_(True)
    assert torch.equal(module(xg, xg, xg).detach(), want)   # (the autograd forward too)


@pytest.mark.parametrize("dtype", HALF)
def test_module_deterministic_and_graph_replay(tsa, dev, dtype):
    heads, embed, seq, batch = 8, 512, 1024, 8
    module = build_attention(tsa, dev, heads, embed, seq, seed=9, half_storage=True)
    x = torch.empty(batch, seq, embed, device=dev).uniform_(-1, 1).to(dtype)
    with torch.no_grad():
        a, b = module(x, x, x), module(x, x, x)
    assert torch.equal(a, b)
    replay = tsa.graphs.capture_forward(module, x, x, x)
    assert torch.equal(replay(x, x, x), a)


def test_half_storage_flag_leaves_float32_and_default_alone(tsa, dev):
    heads, embed, seq, batch = 4, 256, 256, 2
    on = build_attention(tsa, dev, heads, embed, seq, seed=13, half_storage=True)
    off = build_attention(tsa, dev, heads, embed, seq, seed=13)
    x = torch.empty(batch, seq, embed, device=dev).uniform_(-1, 1)
    with torch.no_grad():
        assert torch.equal(on(x, x, x), off(x, x, x))
        for dtype in HALF:   # the default flag: half inputs still come back float32, as before
            xh = x.to(dtype)
            got = off(xh, xh, xh)
            assert got.dtype == torch.float32
            assert torch.equal(got, off(xh.float(), xh.float(), xh.float()))
        # mixed input types: the flag changes nothing
        xh = x.to(torch.float16)
        assert torch.equal(on(xh, x, x), off(xh, x, x))
