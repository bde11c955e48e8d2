"""GPU: fused sparse attention training at head dimension 128 -- the row-group forward
(csrc/attention_rows.hip, ops.sparse_attention_rows) and the D = 128 instances of the fused
backward (csrc/attention_backward.hip) -- against float64 dense autograd and the composed
route, with and without dropout: the kernel's edges (rows of 0 .. 33 entries, descending
columns, empty key columns, fewer rows than a workgroup), the dropout contract, partial
gradients, determinism, peak memory, and SparseAttention(fused_backward=True) with 128-wide
heads, eager and captured.

The op makes q, k and v contiguous (the C ABI takes a stride per replica, not per row), so
there is no case with operands that are column slices of a wider tensor."""
import functools
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from helpers import rel_err_torch
from oracle import sputnik_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the d = 64 fused backward's bound against float64
D = 128
SCALE = 1 / math.sqrt(D)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def gen(dev):
    torch.cuda.init()   # (the default generators exist once CUDA is initialised)
    return torch.cuda.default_generators[dev.index or 0]


def csr_of(dense, reversed_row=None):
    _, _, ro, ci = O.dense_to_csr(dense.astype(np.float32))
    ci = ci.copy()
    if reversed_row is not None:
        a, b = ro[reversed_row], ro[reversed_row + 1]
        ci[a:b] = ci[a:b][::-1].copy()
    return ro, ci


def make_mask(m, n, seed, density=0.2):
    """[m, n] boolean mask with some rows without entries, and its CSR."""
    rng = np.random.default_rng(seed)
    dense = rng.random((m, n)) < density
    dense[rng.choice(m, size=max(1, m // 16), replace=False)] = False
    return dense, csr_of(dense)


EDGE_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 32, 33)


def edge_mask():
    """m = 40 (not a multiple of the 16 rows of a workgroup), n = 48: rows 0..9 hold exactly
    EDGE_COUNTS entries -- a whole window of 16, more than one window, and every remainder of
    an unroll of 2 or 4 -- the others 1..20; key columns 5 and 30 are empty; row 8 (32
    entries) has descending columns."""
    m, n = 40, 48
    rng = np.random.default_rng(7)
    columns = np.array([c for c in range(n) if c not in (5, 30)])
    dense = np.zeros((m, n), dtype=bool)
    for i in range(m):
        count = EDGE_COUNTS[i] if i < len(EDGE_COUNTS) else int(rng.integers(1, 21))
        dense[i, rng.choice(columns, size=count, replace=False)] = True
    assert tuple(dense.sum(1)[:len(EDGE_COUNTS)]) == EDGE_COUNTS
    return dense, csr_of(dense, reversed_row=8)


CASES = {
    "edges": dict(R=2, mask=edge_mask),
    "m!=n": dict(R=3, mask=lambda: make_mask(200, 136, 11)),
    "one-partial-workgroup": dict(R=1, mask=lambda: make_mask(7, 5, 12, density=0.6)),
    "long-rows": dict(R=2, mask=lambda: make_mask(96, 512, 13, density=0.9)),
}


@functools.lru_cache(maxsize=None)
def case_mask(name):
    return CASES[name]["mask"]()


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
    """float64 dense (softmax(scale q k^T at mask) * factor) v and the rows' log-sum-exp;
    rows without entries give 0 and -inf."""
    s = scale * q @ k.transpose(-1, -2)
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    w = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])
    w = torch.where(mask, w, torch.zeros_like(w))
    return (w * factor) @ v, lse


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


def dq_error(got, want, dense):
    """rel_err_torch of dQ.  A query row with ONE entry has a softmax of one weight: its dQ is
    exactly 0 in float64, and in float32 the rounding of dp - D_i, two roundings of the same
    dot product once the keep scale is in it.  A zero row is no scale for a relative bound, so
    such rows take the replica's mean magnitude, the rule helpers.rel_err has for short rows."""
    single = torch.from_numpy(dense.sum(1) == 1)
    worst = rel_err_torch(got[:, ~single], want[:, ~single])
    if bool(single.any()):
        scale = want.abs().mean(dim=(1, 2), keepdim=True)
        err = (got[:, single].double() - want[:, single]).abs()
        worst = max(worst, float((err / (want[:, single].abs() + scale)).max()))
    return worst


def operands(R, m, n, seed, dev):
    torch.manual_seed(seed)
    q, k, v = (torch.randn(R, rows, D, device=dev) for rows in (m, n, n))
    return q, k, v, torch.randn(R, m, D, device=dev)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_match_float64(dev, name, p):
    from torch_sputnik_amd import functional, ops
    dense, csr = case_mask(name)
    (m, n), R = dense.shape, CASES[name]["R"]
    topo = topo_of(csr, dev)
    assert functional.fused_backward_served(torch.empty(R, m, D, device=dev),
                                            torch.empty(R, n, D, device=dev), topo[2])
    q, k, v, go = operands(R, m, n, 3, dev)
    y, grads, state = run(q, k, v, topo, SCALE, p, True, go, offset=800, dev=dev)

    # the op itself, at the same generator offset: out, lse and the published state
    g = gen(dev)
    g.set_offset(800)
    out, lse, rng_state = ops.sparse_attention_rows(q, k, v, *topo, SCALE, p)
    assert g.get_offset() == (804 if p > 0 else 800)
    if p > 0:
        assert torch.equal(rng_state.cpu(), state)
    else:
        assert rng_state is None
    assert torch.equal(out, y)

    factor = dense_keep(csr, state, R, p, m, n) if p > 0 else torch.ones(R, m, n, dtype=torch.float64)
    mask = torch.from_numpy(dense).expand(R, m, n)
    qd, kd, vd = (t.cpu().double().requires_grad_() for t in (q, k, v))
    want, want_lse = reference(qd, kd, vd, mask, factor, SCALE)
    want.backward(go.cpu().double())
    errors = {"out": rel_err_torch(y.cpu(), want.detach())}
    finite = torch.isfinite(want_lse)
    assert torch.equal(torch.isfinite(lse.cpu()), finite)
    assert bool((lse.cpu()[~finite] == float("-inf")).all())
    errors["lse"] = rel_err_torch(lse.cpu()[finite], want_lse.detach()[finite])
    for label, got, ref in zip(("dq", "dk", "dv"), grads, (qd.grad, kd.grad, vd.grad)):
        assert torch.isfinite(got).all()
        errors[label] = (dq_error(got.cpu(), ref, dense) if label == "dq"
                         else rel_err_torch(got.cpu(), ref))
    print(name, p, errors)
    assert max(errors.values()) < TOL, errors

    empty_rows = np.flatnonzero(~dense.any(1))
    empty_cols = np.flatnonzero(~dense.any(0))
    assert len(empty_rows) > 0
    assert not y[:, empty_rows].any() and not grads[0][:, empty_rows].any()
    if name == "edges":
        assert set(empty_cols) >= {5, 30}
    if len(empty_cols):
        assert not grads[1][:, empty_cols].any() and not grads[2][:, empty_cols].any()


def test_dropped_entries_are_those_of_the_published_state(dev):
    """v = the first n rows of the identity: out[r, i, j] is the weight of entry (i, j) times its
    keep factor, so the zeros of `out` at the mask are exactly the dropped entries."""
    from torch_sputnik_amd import ops
    dense, csr = case_mask("edges")
    (m, n), R, p = dense.shape, 2, 0.2
    topo = topo_of(csr, dev)
    q, k, _, _ = operands(R, m, n, 4, dev)
    v = torch.eye(n, D, device=dev).expand(R, n, D).contiguous()
    g = gen(dev)
    g.set_offset(2000)
    out, _, state = ops.sparse_attention_rows(q, k, v, *topo, SCALE, p)
    assert g.get_offset() == 2004
    assert state.tolist() == [g.initial_seed(), 2000]
    kept = dense_keep(csr, state.cpu(), R, p, m, n) != 0
    assert 0 < int(kept.sum()) < R * int(dense.sum())
    assert torch.equal(out[:, :, :n].cpu() != 0, kept)
    assert not out[:, :, n:].any()
    # p = 0 consumes nothing and publishes nothing
    plain, _, none = ops.sparse_attention_rows(q, k, v, *topo, SCALE, 0.0)
    assert none is None and g.get_offset() == 2004
    assert torch.equal(plain[:, :, :n].cpu() != 0, torch.from_numpy(dense).expand(R, m, n))


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_partial_gradients(dev, p):
    _, csr = make_mask(160, 176, 31)
    topo = topo_of(csr, dev)
    q, k, v, go = operands(3, 160, 176, 5, dev)
    _, full, _ = run(q, k, v, topo, SCALE, p, True, go, offset=40, dev=dev)
    for needs in ((False, False, True), (True, False, False), (False, True, False),
                  (True, False, True)):
        _, part, _ = run(q, k, v, topo, SCALE, p, True, go, needs=needs, offset=40, dev=dev)
        for want, got, asked in zip(full, part, needs):
            assert (got is not None) == asked
            if asked:
                assert torch.equal(got, want)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_deterministic(dev, p):
    _, csr = make_mask(512, 512, 51, density=0.3)
    topo = topo_of(csr, dev)
    q, k, v, go = operands(8, 512, 512, 7, dev)
    y1, first, _ = run(q, k, v, topo, SCALE, p, True, go, offset=80, dev=dev)
    y2, again, _ = run(q, k, v, topo, SCALE, p, True, go, offset=80, dev=dev)
    assert torch.equal(y1, y2)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_agrees_with_composed(dev, p):
    _, csr = make_mask(256, 192, 21, density=0.3)
    topo = topo_of(csr, dev)
    q, k, v, go = operands(4, 256, 192, 4, dev)
    y_f, fused, _ = run(q, k, v, topo, SCALE, p, True, go, offset=1200, dev=dev)
    y_c, composed, _ = run(q, k, v, topo, SCALE, p, False, go, offset=1200, dev=dev)
    assert rel_err_torch(y_f, y_c) < TOL
    for a, b in zip(fused, composed):
        assert rel_err_torch(a, b) < TOL


def test_served(dev):
    from torch_sputnik_amd import functional
    ci = torch.zeros(100, dtype=torch.int32, device=dev)

    def served(d, column_indices=ci):
        return functional.fused_backward_served(torch.empty(2, 64, d, device=dev),
                                                torch.empty(2, 80, d, device=dev), column_indices)

    assert served(128) and served(64)
    assert not served(32)
    assert not served(128, ci[:0])
    assert not functional.fused_backward_served(torch.empty(2, 64, 128), torch.empty(2, 80, 128),
                                                ci.cpu())


def test_peak_memory(dev):
    """R = 4, S = 2048, density 0.5: one [R, nnz] float32 array is ~31 MB, the three gradients
    and D ~12.6 MB, out and lse ~4.2 MB.  With the transposed topology cached, the fused
    forward and backward each peak below half of one [R, nnz] array; the composed backward
    holds more than a whole one."""
    from torch_sputnik_amd import functional
    R, S = 4, 2048
    _, csr = make_mask(S, S, 41, density=0.5)
    topo = topo_of(csr, dev)
    row_array = R * topo[2].numel() * 4
    functional.register_static_topology(*topo)
    try:
        torch.manual_seed(6)
        q, k, v = (torch.randn(R, S, D, device=dev).requires_grad_() for _ in range(3))
        go = torch.randn(R, S, D, device=dev)

        def peaks(fused):
            y = functional.sparse_attention(q, k, v, *topo, SCALE, fused_backward=fused)
            y.backward(go)   # warm-up: transposed topology and plans into the caches
            del y
            for t in (q, k, v):
                t.grad = None
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y = functional.sparse_attention(q, k, v, *topo, SCALE, fused_backward=fused)
            torch.cuda.synchronize()
            forward_peak = torch.cuda.max_memory_allocated() - before
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y.backward(go)
            torch.cuda.synchronize()
            backward_peak = torch.cuda.max_memory_allocated() - before
            grads = [t.grad for t in (q, k, v)]
            for t in (q, k, v):
                t.grad = None
            return forward_peak, backward_peak, grads

        fused_forward, fused_backward, fused_grads = peaks(True)
        _, composed_backward, composed_grads = peaks(False)
        print(dict(row_array=row_array, fused_forward=fused_forward, fused_backward=fused_backward,
                   composed_backward=composed_backward))
        assert fused_backward < row_array / 2, (fused_backward, row_array)
        assert fused_forward < row_array / 2, (fused_forward, row_array)
        assert composed_backward > row_array, (composed_backward, row_array)
        for a, b in zip(fused_grads, composed_grads):
            assert rel_err_torch(a, b) < TOL
    finally:
        functional.unregister_static_topology(*topo)


# ---------------------------------------------------------------------------
# SparseAttention(fused_backward=True) with 128-wide heads
# ---------------------------------------------------------------------------
B, S, E, H = 2, 128, 256, 2


def make_layer(dev, **kw):
    from torch_sputnik_amd import SparseAttention
    torch.manual_seed(0)
    layer = SparseAttention(num_heads=H, embedding_size=E, max_sequence_length=S, device=dev,
                            sparsity=0.9, mask_generator=np.random.default_rng(3),
                            fused_backward=True, **kw).to(dev)
    g = torch.Generator().manual_seed(1)
    for lin in layer.linears:
        with torch.no_grad():
            w = torch.randn(E, E, generator=g) * (torch.rand(E, E, generator=g) < 0.3)
            lin.weight.copy_(w.to(dev) / 8)
        lin.setup_sparse_tensors()
    return layer


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_module_training_step_matches_float64(dev, p):
    from torch_sputnik_amd import functional
    layer = make_layer(dev, attention_dropout=p).train()
    assert layer.head_dim == D
    assert functional.fused_backward_served(torch.empty(B * H, S, D, device=dev),
                                            torch.empty(B * H, S, D, device=dev),
                                            layer.column_indices)
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
    ctx, _ = reference(q, k, v, mask, factor, SCALE)
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
    layer = make_layer(dev).train()
    x = torch.randn(B, S, E, device=dev)
    go = torch.randn(B, S, E, device=dev)
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
        assert (got is not None) == (want is not None)
        if got is not None:
            assert torch.equal(got, want)
