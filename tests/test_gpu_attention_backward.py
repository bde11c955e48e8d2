"""GPU: the fused sparse attention backward (csrc/attention_backward.hip,
functional.FusedBackwardAttentionFunction, SparseAttention(fused_backward=True)) against float64
dense autograd and against the composed backward, with and without dropout: partial
gradients, peak memory, determinism, the fallback for shapes it does not serve, the module's
training step and its captured replay."""
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from helpers import rel_err_torch
from oracle import sputnik_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def gen(dev):
    torch.cuda.init()   # (the default generators exist once CUDA is initialised)
    return torch.cuda.default_generators[dev.index or 0]


def make_mask(m, n, seed, density=0.2, shuffle_row=None, empty_cols=0):
    """[m, n] boolean mask and its CSR (row_offsets, column_indices): some rows without
    entries, `empty_cols` key columns without entries, row `shuffle_row` with its columns
    in descending order."""
    rng = np.random.default_rng(seed)
    dense = rng.random((m, n)) < density
    dense[rng.choice(m, size=max(1, m // 16), replace=False)] = False
    if empty_cols:
        dense[:, rng.choice(n, size=empty_cols, replace=False)] = False
    _, _, ro, ci = O.dense_to_csr(dense.astype(np.float32))
    ci = ci.copy()
    if shuffle_row is not None:
        a, b = ro[shuffle_row], ro[shuffle_row + 1]
        ci[a:b] = ci[a:b][::-1].copy()
    return dense, (ro, ci)


def topo_of(csr, dev):
    ro, ci = csr
    ri = np.argsort(-np.diff(ro), kind="stable").astype(np.int32)
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).int().to(dev) for t in (ri, ro, ci))


def dense_keep(csr, state, replicas, p, m, n):
    """[R, m, n] float64 factor keep(r, e) / (1 - p) at the mask (e = CSR position)."""
    ro, ci = csr
    out = np.zeros((replicas, m, n))
    if len(ci):
        keep = P.keep_mask_of(state, replicas, len(ci), p)
        rows = np.repeat(np.arange(m), np.diff(ro))
        out[:, rows, ci] = keep * float(P.keep_scale(p))
    return torch.from_numpy(out)


def reference(q, k, v, mask, factor, scale):
    """float64 dense (softmax(scale q k^T at mask) * factor) v; rows without entries give 0."""
    s = scale * q @ k.transpose(-1, -2)
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    w = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])
    w = torch.where(mask, w, torch.zeros_like(w))
    return (w * factor) @ v


def run(q, k, v, topo, scale, p, fused, go, needs=(True, True, True), offset=None, dev=None):
    """Forward at generator offset `offset` and backward -> (y, (dq, dk, dv), rng_state)."""
    from torch_sputnik_amd import functional
    xs = [t.detach().clone().requires_grad_(w) for t, w in zip((q, k, v), needs)]
    state = None
    if p > 0.0:
        gen(dev).set_offset(offset)
        state = torch.tensor([gen(dev).initial_seed(), offset])
    y = functional.sparse_attention(*xs, *topo, scale, dropout_p=p, fused_backward=fused)
    y.backward(go)
    return y.detach(), tuple(x.grad for x in xs), state


CASES = {
    "m!=n": dict(m=200, n=136, R=3),
    "non-ascending": dict(m=128, n=256, R=3, shuffle_row=5),
    "empty-rows-and-columns": dict(m=144, n=160, R=2, empty_cols=9),
    "S-not-128": dict(m=200, n=200, R=2),
    "long-rows": dict(m=160, n=512, R=2, density=0.9),
    "R1": dict(m=96, n=112, R=1),
    "R64": dict(m=128, n=128, R=64),
}


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_backward_matches_float64(dev, name, p):
    c = CASES[name]
    m, n, R, d = c["m"], c["n"], c["R"], 64
    dense, csr = make_mask(m, n, 11, density=c.get("density", 0.2),
                           shuffle_row=c.get("shuffle_row"), empty_cols=c.get("empty_cols", 0))
    topo = topo_of(csr, dev)
    torch.manual_seed(3)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    go = torch.randn(R, m, d, device=dev)
    scale = 1 / math.sqrt(d)
    y, grads, state = run(q, k, v, topo, scale, p, True, go, offset=800, dev=dev)
    factor = dense_keep(csr, state, R, p, m, n) if p > 0 else torch.ones(R, m, n, dtype=torch.float64)
    mask = torch.from_numpy(dense).expand(R, m, n)
    qd, kd, vd = (t.cpu().double().requires_grad_() for t in (q, k, v))
    want = reference(qd, kd, vd, mask, factor, scale)
    want.backward(go.cpu().double())
    assert rel_err_torch(y.cpu(), want.detach()) < TOL
    for got, ref in zip(grads, (qd.grad, kd.grad, vd.grad)):
        assert torch.isfinite(got).all()
        assert rel_err_torch(got.cpu(), ref) < TOL
    empty_rows = np.flatnonzero(~dense.any(1))
    empty_cols = np.flatnonzero(~dense.any(0))
    assert len(empty_rows) > 0
    assert not grads[0][:, empty_rows].any()
    if len(empty_cols):
        assert not grads[1][:, empty_cols].any() and not grads[2][:, empty_cols].any()


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_fused_backward_agrees_with_composed(dev, p):
    m, n, R, d = 256, 192, 4, 64
    _, csr = make_mask(m, n, 21, density=0.3, shuffle_row=3)
    topo = topo_of(csr, dev)
    torch.manual_seed(4)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    go = torch.randn(R, m, d, device=dev)
    y_f, fused, _ = run(q, k, v, topo, 0.125, p, True, go, offset=1200, dev=dev)
    y_c, composed, _ = run(q, k, v, topo, 0.125, p, False, go, offset=1200, dev=dev)
    assert torch.equal(y_f, y_c)   # (the same forward kernel)
    for a, b in zip(fused, composed):
        assert rel_err_torch(a, b) < TOL


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_partial_gradients(dev, p):
    m, n, R, d = 160, 176, 3, 64
    _, csr = make_mask(m, n, 31)
    topo = topo_of(csr, dev)
    torch.manual_seed(5)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    go = torch.randn(R, m, d, device=dev)
    _, full, _ = run(q, k, v, topo, 0.125, p, True, go, offset=40, dev=dev)
    for needs in ((False, False, True), (True, False, False), (False, True, False),
                  (True, False, True)):
        _, part, _ = run(q, k, v, topo, 0.125, p, True, go, needs=needs, offset=40, dev=dev)
        for want, got, asked in zip(full, part, needs):
            assert (got is not None) == asked
            if asked:
                assert torch.equal(got, want)


def test_fused_backward_peak_memory(dev):
    """R = 16, S = 2048, density 0.4: one [R, nnz] float32 array is ~107 MB, the three
    gradients ~25 MB.  With the transposed topology and the plan cached, the fused
    backward's peak stays below half of one [R, nnz] array; the composed one holds several."""
    from torch_sputnik_amd import functional
    R, S, d = 16, 2048, 64
    _, csr = make_mask(S, S, 41, density=0.4)
    topo = topo_of(csr, dev)
    nnz = topo[2].numel()
    row_array = R * nnz * 4
    functional.register_static_topology(*topo)
    try:
        torch.manual_seed(6)
        q, k, v = (torch.randn(R, S, d, device=dev).requires_grad_() for _ in range(3))
        go = torch.randn(R, S, d, device=dev)

        def backward_peak(fused):
            y = functional.sparse_attention(q, k, v, *topo, 0.125, fused_backward=fused)
            y.backward(go)   # warm-up: transposed topology and plans into the caches
            for t in (q, k, v):
                t.grad = None
            y = functional.sparse_attention(q, k, v, *topo, 0.125, fused_backward=fused)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y.backward(go)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
            grads = [t.grad for t in (q, k, v)]
            for t in (q, k, v):
                t.grad = None
            return peak, grads

        fused_peak, fused_grads = backward_peak(True)
        composed_peak, composed_grads = backward_peak(False)
        assert fused_peak < row_array / 2, (fused_peak, row_array)
        assert composed_peak > row_array, (composed_peak, row_array)
        for a, b in zip(fused_grads, composed_grads):
            assert rel_err_torch(a, b) < TOL
    finally:
        functional.unregister_static_topology(*topo)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_fused_backward_is_deterministic(dev, p):
    m, n, R, d = 512, 512, 8, 64
    _, csr = make_mask(m, n, 51, density=0.3)
    topo = topo_of(csr, dev)
    torch.manual_seed(7)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    go = torch.randn(R, m, d, device=dev)
    _, first, _ = run(q, k, v, topo, 0.125, p, True, go, offset=80, dev=dev)
    _, again, _ = run(q, k, v, topo, 0.125, p, True, go, offset=80, dev=dev)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_unserved_head_dimension_falls_back(dev):
    """d = 32: fused_backward=True trains on the composed backward, bit for bit."""
    from torch_sputnik_amd import ops
    m, n, R, d = 96, 96, 3, 32
    assert not ops.sparse_attention_backward_supported(m, n, d, 100)
    _, csr = make_mask(m, n, 61)
    topo = topo_of(csr, dev)
    torch.manual_seed(8)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    go = torch.randn(R, m, d, device=dev)
    for p in (0.0, 0.2):
        y_f, fused, _ = run(q, k, v, topo, 1 / math.sqrt(d), p, True, go, offset=160, dev=dev)
        y_c, composed, _ = run(q, k, v, topo, 1 / math.sqrt(d), p, False, go, offset=160, dev=dev)
        assert torch.equal(y_f, y_c)
        for a, b in zip(fused, composed):
            assert torch.equal(a, b)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_empty_mask_trains_as_without_the_flag(dev, p):
    """d = 64 with a mask without entries: the fused forward does not serve it, so
    fused_backward=True takes the composed route -- the same results, bit for bit, and
    zero gradients."""
    from torch_sputnik_amd import functional
    m, n, R, d = 64, 80, 2, 64
    assert not functional.fused_backward_served(torch.empty(R, m, d, device=dev),
                                                torch.empty(R, n, d, device=dev),
                                                torch.empty(0, dtype=torch.int32, device=dev))
    _, csr = make_mask(m, n, 81, density=0.0)
    topo = topo_of(csr, dev)
    assert topo[2].numel() == 0
    torch.manual_seed(9)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    go = torch.randn(R, m, d, device=dev)
    y_f, fused, _ = run(q, k, v, topo, 0.125, p, True, go, offset=240, dev=dev)
    y_c, composed, _ = run(q, k, v, topo, 0.125, p, False, go, offset=240, dev=dev)
    assert torch.equal(y_f, y_c) and not y_f.any()
    for a, b in zip(fused, composed):
        assert torch.equal(a, b) and not a.any()


def test_c_abi_empty_mask_writes_zero_gradients(dev):
    """The C ABI serves nonzeros = 0 itself: every wanted gradient row is zero."""
    import ctypes
    from torch_sputnik_amd import capi
    m, n, R, d = 48, 40, 3, 64
    ro = torch.zeros(m + 1, dtype=torch.int32, device=dev)
    ri = torch.arange(m, dtype=torch.int32, device=dev)
    ci = torch.zeros(1, dtype=torch.int32, device=dev)
    q, out, go = (torch.randn(R, m, d, device=dev) for _ in range(3))
    k, v = (torch.randn(R, n, d, device=dev) for _ in range(2))
    lse = torch.full((R, m), float("-inf"), device=dev)
    dq = torch.full((R, m, d), float("nan"), device=dev)
    dk, dv = (torch.full((R, n, d), float("nan"), device=dev) for _ in range(2))
    ws = torch.empty(max(16, capi.lib().sputnik_hip_sparse_attention_backward_workspace_bytes(
        m, n, d, 0, R)), dtype=torch.uint8, device=dev)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    status = capi.lib().sputnik_hip_sparse_attention_backward(
        m, n, d, 0, R, ptr(ri), ptr(ro), ptr(ci), ptr(ri), ptr(ro), ptr(ci), None,
        ptr(q), m * d, ptr(k), n * d, ptr(v), n * d, 0.125, ptr(out), m * d, ptr(go), m * d,
        ptr(lse), m, ptr(dq), m * d, ptr(dk), n * d, ptr(dv), n * d, 0.0, capi.PhiloxState(),
        ptr(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    for g in (dq, dk, dv):
        assert torch.equal(g, torch.zeros_like(g))


def test_backward_op_argument_checks(dev):
    from torch_sputnik_amd import ops
    m, n, R, d = 64, 64, 2, 64
    _, csr = make_mask(m, n, 71)
    topo = topo_of(csr, dev)
    q, k, v = (torch.randn(R, 64, d, device=dev) for _ in range(3))
    out, lse = ops.sparse_attention_with_lse(q, k, v, *topo, 0.125)
    with pytest.raises(RuntimeError):   # dK wanted without the transposed mask
        ops.sparse_attention_backward(q, k, v, out, out, lse, *topo, None, 0.125,
                                      needs=(False, True, False))
    with pytest.raises(RuntimeError):   # dropout without the forward's rng_state
        ops.sparse_attention_backward(q, k, v, out, out, lse, *topo, None, 0.125, p=0.2,
                                      needs=(True, False, False))
    dq, dk, dv = ops.sparse_attention_backward(q, k, v, out, out, lse, *topo, None, 0.125,
                                               needs=(True, False, False))
    assert dk is None and dv is None and dq.shape == q.shape


# ---------------------------------------------------------------------------
# SparseAttention(fused_backward=True)
# ---------------------------------------------------------------------------
def make_layer(dev, **kw):
    from torch_sputnik_amd import SparseAttention
    torch.manual_seed(0)
    layer = SparseAttention(num_heads=4, embedding_size=256, max_sequence_length=256, device=dev,
                            sparsity=0.9, mask_generator=np.random.default_rng(3), **kw).to(dev)
    g = torch.Generator().manual_seed(1)
    for lin in layer.linears:
        with torch.no_grad():
            w = torch.randn(256, 256, generator=g) * (torch.rand(256, 256, generator=g) < 0.3)
            lin.weight.copy_(w.to(dev) / 8)
        lin.setup_sparse_tensors()
    return layer


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_module_training_step_matches_float64(dev, p):
    B, S, E, H = 2, 256, 256, 4
    D = E // H
    layer = make_layer(dev, attention_dropout=p, fused_backward=True).train()
    torch.manual_seed(12)
    x = torch.randn(B, S, E, device=dev).requires_grad_()
    g, offset = gen(dev), 1000
    g.set_offset(offset)
    y = layer(x, x, x)
    assert g.get_offset() == (offset + 4 if p > 0 else offset)
    go = torch.randn_like(y)
    y.backward(go)

    csr = (layer.row_offsets.cpu().numpy(), layer.column_indices.cpu().numpy())
    mask = (layer.mask2d.cpu() != 0).expand(B * H, S, S)
    factor = (dense_keep(csr, torch.tensor([g.initial_seed(), offset]), B * H, p, S, S) if p > 0
              else torch.ones(B * H, S, S, dtype=torch.float64))
    weights = [lin.weight.detach().cpu().double().requires_grad_() for lin in layer.linears]
    xd = x.detach().cpu().double().requires_grad_()

    def heads(t):   # [B, S, E] -> [B*H, S, D]
        return t.reshape(B, S, H, D).transpose(1, 2).reshape(B * H, S, D)

    q, k, v = (heads(xd @ w.t()) for w in weights[:3])
    ctx = reference(q, k, v, mask, factor, 1 / math.sqrt(D))
    want = ctx.reshape(B, H, S, D).transpose(1, 2).reshape(B, S, E) @ weights[3].t()
    assert rel_err_torch(y.detach().cpu(), want.detach()) < TOL
    want.backward(go.cpu().double())
    assert rel_err_torch(x.grad.cpu(), xd.grad) < TOL
    for lin, w in zip(layer.linears, weights):
        want_values = w.grad[lin.weight.detach().cpu() != 0]
        assert rel_err_torch(lin.values.grad.cpu().reshape(1, -1),
                             want_values.reshape(1, -1)) < TOL


def test_module_captured_training_step_is_bitwise_eager(dev):
    from torch_sputnik_amd.graphs import capture_training_step
    layer = make_layer(dev, fused_backward=True).train()
    x = torch.randn(2, 256, 256, device=dev)
    go = torch.randn(2, 256, 256, device=dev)
    step = capture_training_step(layer, x, x, x, grad_output=go)
    out = step(x, x, x, grad_output=go).clone()
    grads = [None if g is None else g.clone() for g in step.param_grads]
    torch.cuda.synchronize()
    xe = x.clone().requires_grad_()
    y = layer(xe, xe, xe)
    eager = torch.autograd.grad(y, [xe] + step.params, go, allow_unused=True)
    assert torch.equal(y, out)
    assert torch.equal(step.input_grads[0], eager[0])
    for got, want in zip(grads, eager[1:]):
        assert (got is None) == (want is None)
        if got is not None:
            assert torch.equal(got, want)
