"""GPU: attention dropout (csrc/philox.h, dropout.hip, the DROP attention kernels) against the
numpy restatement of the mask contract (tests/philox_ref.py) and float64 dense attention:
sparse_dropout bit for bit, the fused forms forward / lse / gradients, fused against
composed, the modules, and replay of a captured training step."""
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from helpers import rel_err_torch
from oracle import sputnik_oracle as O

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.float16: 5e-3, torch.bfloat16: 3e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def gen(dev):
    torch.cuda.init()   # (the default generators exist once CUDA is initialised)
    return torch.cuda.default_generators[dev.index or 0]


def expected_dropout(x, p, rng_state):
    """x * keep * scale in float32, rounded once to x's type ([nnz] or [R, width])."""
    x2 = x.reshape(1, -1) if x.dim() == 1 else x
    keep = torch.from_numpy(P.keep_mask_of(rng_state, x2.size(0), x2.size(1), p)).to(x.device)
    want = torch.where(keep, x2.float() * float(P.keep_scale(p)), torch.zeros((), device=x.device))
    return want.to(x.dtype).reshape(x.shape)


# ---------------------------------------------------------------------------
# 1, 2: sparse_dropout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_sparse_dropout_bitwise(dev, dtype, p):
    from torch_sputnik_amd import ops
    torch.manual_seed(1234)
    g = gen(dev)
    wide = torch.randn(5, 1031 + 9, device=dev).to(dtype)
    for x in (wide[0, :1031].contiguous(),       # [nnz]
              wide[:, :1024].contiguous(),       # [R, nnz], aligned
              wide[:, :1031].contiguous(),       # odd width: the tail entry by entry
              wide[:, 3:1030]):                  # strided, unaligned rows
        offset = g.get_offset()
        out, state = ops.sparse_dropout(x, p)
        assert g.get_offset() == offset + 4
        assert state.tolist() == [g.initial_seed(), offset]
        assert out.dtype == x.dtype and out.shape == x.shape
        want = expected_dropout(x, p, state)
        assert torch.equal(out, want)
        assert torch.equal((out != 0), (want != 0))
        replay, state2 = ops.sparse_dropout(x, p, state)      # replay: same mask, nothing drawn
        assert g.get_offset() == offset + 4
        assert torch.equal(replay, out) and torch.equal(state2, state)


def test_sparse_dropout_padding_and_seed(dev):
    from torch_sputnik_amd import ops
    x = torch.randn(6, 40, device=dev)
    x[:3, 25:] = 0   # many-mask padding of the shorter masks
    torch.manual_seed(7)
    a, sa = ops.sparse_dropout(x, 0.3)
    assert not a[:3, 25:].any()
    torch.manual_seed(7)
    b, sb = ops.sparse_dropout(x, 0.3)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert int(sa[0]) == 7


def test_state_of_calls_without_work(dev):
    from torch_sputnik_amd import ops
    g = gen(dev)
    x = torch.randn(4, 16, device=dev)
    offset = g.get_offset()
    out, state = ops.sparse_dropout(x, 0.0)          # p = 0: a copy that draws nothing
    assert state is None and torch.equal(out, x) and g.get_offset() == offset
    # a mask without entries: the generator advances, and rng_state holds what it drew
    _, csr = make_masks(1, 64, 64, 3, density=0.0)
    topo = topo_single(csr, dev)
    q = torch.randn(2, 64, 64, device=dev)
    offset = g.get_offset()
    out, _, state = ops.sparse_attention_dropout(q, q, q, *topo, 0.125, 0.3)
    assert g.get_offset() == offset + 4
    assert state.tolist() == [g.initial_seed(), offset]
    assert not out.any()


def test_keep_rate_and_fresh_masks(dev):
    from torch_sputnik_amd import ops
    p, n = 0.3, 16 * 65536
    x = torch.ones(16, 65536, device=dev)
    a, _ = ops.sparse_dropout(x, p)
    b, _ = ops.sparse_dropout(x, p)
    rate = (a != 0).double().mean().item()
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(rate - (1 - p)) < 5 * sigma
    assert not torch.equal(a != 0, b != 0)


# ---------------------------------------------------------------------------
# 3-5: the fused forms against float64
# ---------------------------------------------------------------------------
def dense_keep(csr_masks, state, replicas, p, m, n, per_mask, only=None):
    """[R, m, n] float64 factor keep * scale from the (r, e) layout: e is the CSR position of
    the replica's mask (per_mask: replicas // len(csr_masks) replicas per mask).  only: the
    replica numbers to build it for ([len(only), m, n]), all of them by default."""
    width = max(len(ci) for _, ci in csr_masks) if csr_masks else 0
    keep = P.keep_mask_of(state, replicas, max(width, 1), p)
    which = range(replicas) if only is None else only
    out = np.zeros((len(which), m, n))
    for at, r in enumerate(which):
        ro, ci = csr_masks[r // per_mask]
        for i in range(m):
            for e in range(ro[i], ro[i + 1]):
                out[at, i, ci[e]] = keep[r, e] * float(P.keep_scale(p))
    return torch.from_numpy(out)


def reference(q, k, v, mask, factor, scale, cut_softmax=False):
    """float64 dense: out = (softmax(scale q k^T at mask) * factor) v and lse; [R, m, n] mask.
    cut_softmax: no gradient through the weights to q and k (a softmax without a gradient)."""
    s = scale * q.double() @ k.double().transpose(-1, -2)
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    w = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])
    w = torch.where(mask, w, torch.zeros_like(w))
    if cut_softmax:
        w = w.detach()
    return (w * factor) @ v.double(), lse


def make_masks(masks, m, n, seed, density=0.2, empty_mask=None, shuffle_row=None):
    rng = np.random.default_rng(seed)
    dense = rng.random((masks, m, n)) < density
    dense[:, rng.choice(m, size=max(1, m // 16), replace=False)] = False   # rows without entries
    if empty_mask is not None:
        dense[empty_mask] = False
    csr = []
    for i in range(masks):
        _, _, ro, ci = O.dense_to_csr(dense[i].astype(np.float32))
        ci = ci.copy()
        if shuffle_row is not None:   # non-ascending columns: the order-independent path
            a, b = ro[shuffle_row], ro[shuffle_row + 1]
            ci[a:b] = ci[a:b][::-1].copy()
        csr.append((ro, ci))
    return dense, csr


def topo_single(csr, dev):
    ro, ci = csr[0]
    ri = np.argsort(-np.diff(ro), kind="stable").astype(np.int32)
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).int().to(dev) for t in (ri, ro, ci))


def topo_many(csr, m, dev):
    ri = np.concatenate([np.argsort(-np.diff(ro), kind="stable") for ro, _ in csr]).astype(np.int32)
    ro = np.concatenate([ro for ro, _ in csr]).astype(np.int32)
    ci = np.concatenate([ci for _, ci in csr]).astype(np.int32)
    nnz = torch.tensor([len(c) for _, c in csr])
    return nnz, tuple(torch.from_numpy(t).to(dev) for t in (ri, ro, ci))


SINGLE_CASES = [dict(m=200, n=136, d=64), dict(m=128, n=256, d=64, shuffle_row=5),
                dict(m=96, n=96, d=32)]


@pytest.mark.parametrize("case", SINGLE_CASES, ids=["m!=n", "non-ascending", "d32-composed"])
def test_single_mask_f32_forward_backward(dev, case):
    from torch_sputnik_amd import functional, ops
    m, n, d, R, p = case["m"], case["n"], case["d"], 3, 0.2
    dense, csr = make_masks(1, m, n, 11, shuffle_row=case.get("shuffle_row"))
    topo = topo_single(csr, dev)
    torch.manual_seed(3)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    scale = 1 / math.sqrt(d)
    out, lse, state = ops.sparse_attention_dropout(q, k, v, *topo, scale, p)
    factor = dense_keep(csr, state, R, p, m, n, R)
    mask = torch.from_numpy(dense[0]).expand(R, m, n)
    want, want_lse = reference(q.cpu(), k.cpu(), v.cpu(), mask, factor, scale)
    assert rel_err_torch(out.cpu(), want) < TOL[torch.float32]
    if d == 64:
        assert lse is not None
        fin = torch.isfinite(want_lse)
        assert torch.equal(torch.isfinite(lse.cpu()), fin)
        assert rel_err_torch(lse.cpu()[fin], want_lse[fin]) < TOL[torch.float32]
    # 4: the composed chain with the same rng_state drops the same entries
    w = ops.sparse_softmax_scaled(ops.sddmm(m, n, *topo, q, k), *topo, scale)
    composed = ops.spmm(m, n, ops.sparse_dropout(w, p, state)[0], *topo, v)
    assert rel_err_torch(composed, out) < 1e-4   # (a differing entry moves a row by ~1e-2)
    # 5: gradients
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    gen(dev).set_offset(int(state[1]))
    y = functional.sparse_attention(qg, kg, vg, *topo, scale, dropout_p=p)
    go = torch.randn_like(y)
    y.backward(go)
    qd, kd, vd = (t.detach().cpu().double().requires_grad_() for t in (q, k, v))
    want, _ = reference(qd, kd, vd, mask, factor, scale)
    want.backward(go.cpu().double())
    for got, ref in ((qg.grad, qd.grad), (kg.grad, kd.grad), (vg.grad, vd.grad)):
        assert rel_err_torch(got.cpu(), ref) < TOL[torch.float32]


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_replicas_beyond_one_grid_slice(dev, dtype, p):
    """R = 65537 replicas of a 4 x 4 mask: the forward runs in grid slices of 65535 replicas,
    and the second slice has to number its replicas from 65535 on -- for its operands, its
    lse rows and the (r, e) of the dropout mask.  float32 [R, 4, 64] and float16 [R, 4, 64]
    (one head per batch element).  The replicas on both sides of the slice boundary against
    float64, every replica against the composed chain with the same rng_state."""
    from torch_sputnik_amd import ops
    R, m, n, d = 65537, 4, 4, 64
    probes = [0, 65534, 65535, 65536]
    dense, csr = make_masks(1, m, n, 17, density=0.6)   # (make_masks leaves one row empty)
    assert 0 in np.diff(csr[0][0]) and len(csr[0][1]) >= 4
    topo = topo_single(csr, dev)
    torch.manual_seed(9)
    q, k, v = (torch.randn(R, m, d, device=dev).to(dtype) for _ in range(3))
    scale, state = 1 / math.sqrt(d), None
    if dtype == torch.float32:
        if p > 0.0:
            out, lse, state = ops.sparse_attention_dropout(q, k, v, *topo, scale, p)
        else:
            out, lse = ops.sparse_attention_with_lse(q, k, v, *topo, scale)
    elif p > 0.0:
        out, lse, state = ops.sparse_attention_heads_dropout(q, k, v, *topo, scale, p)
    else:
        out, lse = ops.sparse_attention_heads(q, k, v, *topo, scale, with_lse=True)
    assert out.shape == (R, m, d) and out.dtype == dtype and lse.shape == (R, m)
    factor = torch.ones(len(probes), m, n, dtype=torch.float64)
    if p > 0.0:
        factor = dense_keep(csr, state, R, p, m, n, R, only=probes)
    mask = torch.from_numpy(dense[0]).expand(len(probes), m, n)
    want, want_lse = reference(q[probes].cpu(), k[probes].cpu(), v[probes].cpu(), mask, factor, scale)
    assert rel_err_torch(out[probes].float().cpu(), want) < TOL[dtype]
    fin = torch.isfinite(want_lse)
    assert torch.equal(torch.isfinite(lse[probes].cpu()), fin)
    assert rel_err_torch(lse[probes].cpu()[fin], want_lse[fin]) < TOL[dtype]
    # every replica: the float32 chain (on widened inputs for float16)
    w = ops.sparse_softmax_scaled(ops.sddmm(m, n, *topo, q.float(), k.float()), *topo, scale)
    if p > 0.0:
        w = ops.sparse_dropout(w, p, state)[0]
    composed = ops.spmm(m, n, w, *topo, v.float())
    assert rel_err_torch(out.float(), composed) < (1e-4 if dtype == torch.float32 else TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("out_dtype", [torch.float32, None])
def test_heads_forward_backward(dev, dtype, out_dtype):
    from torch_sputnik_amd import functional, ops
    B, H, S, D, p = 2, 3, 160, 64, 0.15
    # (row 7 reversed: its row block takes the order-independent path, the other one windows)
    dense, csr = make_masks(1, S, S, 5, shuffle_row=7)
    topo = topo_single(csr, dev)
    torch.manual_seed(4)
    x = [torch.randn(B, S, H * D, device=dev).to(dtype) for _ in range(3)]
    heads = [t.unflatten(-1, (H, D)).transpose(1, 2) for t in x]
    scale = 1 / math.sqrt(D)
    out, lse, state = ops.sparse_attention_heads_dropout(*heads, *topo, scale, p, out_dtype=out_dtype)
    factor = dense_keep(csr, state, B * H, p, S, S, B * H)
    mask = torch.from_numpy(dense[0]).expand(B * H, S, S)
    flat = [h.reshape(B * H, S, D).cpu() for h in heads]
    want, want_lse = reference(*flat, mask, factor, scale)
    tol = TOL[dtype]   # (half inputs: the storage type's tolerance for either output type)
    assert rel_err_torch(out.reshape(B * H, S, D).float().cpu(), want) < tol
    fin = torch.isfinite(want_lse)
    assert rel_err_torch(lse.reshape(B * H, S).cpu()[fin], want_lse[fin]) < tol
    if out_dtype is not None:
        return
    xg = [t.clone().requires_grad_() for t in x]
    gen(dev).set_offset(int(state[1]))
    y = functional.sparse_attention_heads(*xg, H, *topo, scale, dropout_p=p)
    go = torch.randn_like(y)
    y.backward(go)
    xd = [h.double().requires_grad_() for h in flat]
    want, _ = reference(*xd, mask, factor, scale)
    want.backward(go.cpu().double().unflatten(-1, (H, D)).transpose(1, 2).reshape(B * H, S, D))
    for got, ref in zip(xg, xd):
        got = got.grad.unflatten(-1, (H, D)).transpose(1, 2).reshape(B * H, S, D).float().cpu()
        assert rel_err_torch(got, ref.grad) < TOL[dtype]


@pytest.mark.parametrize("d", [64, 32])
def test_many_mask_f32_forward_backward(dev, d):
    from torch_sputnik_amd import functional, ops
    b, heads, m, n, p = 3, 2, 144, 200, 0.25
    dense, csr = make_masks(b, m, n, 9, empty_mask=1)
    nnz, topo = topo_many(csr, m, dev)
    R = b * heads
    torch.manual_seed(5)
    q, k, v = (torch.randn(R, rows, d, device=dev) for rows in (m, n, n))
    scale = 1 / math.sqrt(d)
    out, lse, state = ops.sparse_attention_many_mask_dropout(b, nnz, *topo, q, k, v, scale, p)
    factor = dense_keep(csr, state, R, p, m, n, heads)
    mask = torch.from_numpy(dense).repeat_interleave(heads, 0)
    want, want_lse = reference(q.cpu(), k.cpu(), v.cpu(), mask, factor, scale)
    assert rel_err_torch(out.cpu(), want) < TOL[torch.float32]
    if d == 64:
        fin = torch.isfinite(want_lse)
        assert torch.equal(torch.isfinite(lse.cpu()), fin)
        assert rel_err_torch(lse.cpu()[fin], want_lse[fin]) < TOL[torch.float32]
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    gen(dev).set_offset(int(state[1]))
    y = functional.sparse_attention_many_mask(b, m, n, nnz, *topo, qg, kg, vg, scale, dropout_p=p)
    go = torch.randn_like(y)
    y.backward(go)
    qd, kd, vd = (t.detach().cpu().double().requires_grad_() for t in (q, k, v))
    want, _ = reference(qd, kd, vd, mask, factor, scale)
    want.backward(go.cpu().double())
    for got, ref in ((qg.grad, qd.grad), (kg.grad, kd.grad), (vg.grad, vd.grad)):
        assert rel_err_torch(got.cpu(), ref) < TOL[torch.float32]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_heads_many_mask_and_core_module(dev, dtype):
    from torch_sputnik_amd import SparseCoreAttention, ops
    from torch_sputnik_amd.topology import dense_to_sparse_3d
    b, heads, s, hn, p = 2, 4, 128, 64, 0.1
    dense, _ = make_masks(b, s, s, 13)
    mask = torch.from_numpy(dense[:, None]).to(dev)
    topology = dense_to_sparse_3d(mask)
    ro_all = topology[1].reshape(b, -1).cpu().numpy()
    ci_all = topology[2].cpu().numpy()
    counts = [int(c) for c in topology[3]]
    starts = np.cumsum([0] + counts)
    csr = [(ro_all[i], ci_all[starts[i]:starts[i + 1]]) for i in range(b)]
    torch.manual_seed(6)
    q, k, v = (torch.randn(b, s, heads, hn, device=dev).to(dtype).requires_grad_() for _ in range(3))
    layer = SparseCoreAttention(s, heads * hn, heads, attention_dropout=p).train()
    offset = gen(dev).get_offset()
    y = layer(q, k, v, mask, topology=topology)              # [s, b, heads * hn]
    state = torch.tensor([gen(dev).initial_seed(), offset])
    factor = dense_keep(csr, state, b * heads, p, s, s, heads)
    dmask = torch.from_numpy(dense).repeat_interleave(heads, 0)
    flat = [t.detach().cpu().double().transpose(1, 2).reshape(b * heads, s, hn).requires_grad_()
            for t in (q, k, v)]
    want, _ = reference(*flat, dmask, factor, 1 / math.sqrt(hn))
    want_y = want.reshape(b, heads, s, hn).permute(2, 0, 1, 3).reshape(s, b, -1)
    assert rel_err_torch(y.float().cpu(), want_y) < TOL[dtype]
    go = torch.randn_like(y)
    y.backward(go)
    want_y.backward(go.cpu().double())
    for got, ref in zip((q, k, v), flat):
        got = got.grad.transpose(1, 2).reshape(b * heads, s, hn).float().cpu()
        assert rel_err_torch(got, ref.grad) < TOL[dtype]
    if dtype != torch.float32:
        # the op itself, both output types: out and lse (of the undropped scores)
        views = [t.detach().transpose(1, 2) for t in (q, k, v)]      # [B, H, S, D]
        for out_dtype in (None, torch.float32):
            out, lse, st = ops.sparse_attention_heads_many_mask_dropout(
                b, topology[3], *topology[:3], *views, 1 / math.sqrt(hn), p, out_dtype=out_dtype)
            assert out.dtype == (dtype if out_dtype is None else torch.float32)
            f = dense_keep(csr, st, b * heads, p, s, s, heads)
            want, want_lse = reference(*(t.detach() for t in flat), dmask, f, 1 / math.sqrt(hn))
            assert rel_err_torch(out.reshape(b * heads, s, hn).float().cpu(), want) < TOL[dtype]
            fin = torch.isfinite(want_lse)
            assert torch.equal(torch.isfinite(lse.reshape(b * heads, s).cpu()), fin)
            assert rel_err_torch(lse.reshape(b * heads, s).cpu()[fin], want_lse[fin]) < TOL[dtype]
    # eval(): exactly the module without dropout
    layer.eval()
    plain = SparseCoreAttention(s, heads * hn, heads).eval()
    with torch.no_grad():
        assert torch.equal(layer(q, k, v, mask, topology=topology), plain(q, k, v, mask, topology=topology))


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("layout", ["single", "heads", "many_mask", "heads_many_mask"])
def test_recomputing_functions_partial_gradients(dev, layout, p):
    """The four recomputing Functions behind the public calls: all three gradients against
    float64, then q, k and v alone requiring grad -- the gradient asked for equals the full
    run's bit for bit, the others are None.  m = 72 x n = 136: one partial query block, two
    key chunks of the 128-row stage."""
    from torch_sputnik_amd import functional, ops
    B, H, m, n, d = 2, 2, 72, 136, 64
    many, views = "many_mask" in layout, layout.startswith("heads")
    dtype = torch.float16 if views else torch.float32
    R, scale = B * H, 1 / math.sqrt(d)
    dense, csr = make_masks(B if many else 1, m, n, 21)
    if many:
        nnz, topo = topo_many(csr, m, dev)
        assert nnz[0] != nnz[1]
        mask = torch.from_numpy(dense).repeat_interleave(H, 0)
    else:
        topo = topo_single(csr, dev)
        mask = torch.from_numpy(dense[0]).expand(R, m, n)

    def operand(x):   # [B, H, S, D] float32 -> the layout's operand
        if layout == "heads":
            return x.transpose(1, 2).reshape(B, x.size(2), H * d).to(dtype)
        if layout == "heads_many_mask":
            return x.transpose(1, 2).contiguous().to(dtype)
        return x.reshape(R, x.size(2), d)

    def head_views(t):   # operand -> [B, H, S, D] view
        return (t.unflatten(-1, (H, d)) if layout == "heads" else t).transpose(1, 2)

    def replicas(t):   # operand or gradient -> [R, S, D] on the CPU
        return (head_views(t).reshape(R, -1, d) if views else t).cpu()

    def call(q, k, v):
        if layout == "single":
            return functional.sparse_attention(q, k, v, *topo, scale, dropout_p=p)
        if layout == "heads":
            return functional.sparse_attention_heads(q, k, v, H, *topo, scale, dropout_p=p)
        if layout == "many_mask":
            return functional.sparse_attention_many_mask(B, m, n, nnz, *topo, q, k, v, scale, dropout_p=p)
        return functional.sparse_attention_heads_many_mask(q, k, v, nnz, *topo, scale, dropout_p=p)

    torch.manual_seed(8)
    q, k, v, go = (operand(torch.randn(B, H, rows, d, device=dev)) for rows in (m, n, n, m))
    factor, offset = torch.ones(R, m, n, dtype=torch.float64), gen(dev).get_offset()
    if p > 0.0:   # the state of one forward with dropout; every run below starts at its offset
        if layout == "single":
            state = ops.sparse_attention_dropout(q, k, v, *topo, scale, p)[2]
        elif layout == "heads":
            state = ops.sparse_attention_heads_dropout(*map(head_views, (q, k, v)), *topo, scale, p)[2]
        elif layout == "many_mask":
            state = ops.sparse_attention_many_mask_dropout(B, nnz, *topo, q, k, v, scale, p)[2]
        else:
            state = ops.sparse_attention_heads_many_mask_dropout(
                B, nnz, *topo, *map(head_views, (q, k, v)), scale, p)[2]
        factor, offset = dense_keep(csr, state, R, p, m, n, H if many else R), int(state[1])

    def run(needs):
        xs = [t.clone().requires_grad_(need) for t, need in zip((q, k, v), needs)]
        gen(dev).set_offset(offset)
        y = call(*xs)
        assert y.shape == go.shape and y.dtype == dtype
        y.backward(go)
        return [x.grad for x in xs]

    full = run((True, True, True))
    xd = [replicas(t).double().requires_grad_() for t in (q, k, v)]
    want, _ = reference(*xd, mask, factor, scale)
    want.backward(replicas(go).double())
    for name, got, ref in zip("qkv", full, xd):
        err = rel_err_torch(replicas(got).float(), ref.grad)
        print(f"{layout} p={p} d{name}: rel err {err:.3e} (bound {TOL[dtype]:g})")
        assert err < TOL[dtype]
    for alone in range(3):
        part = run(tuple(i == alone for i in range(3)))
        for i, (got, whole) in enumerate(zip(part, full)):
            if i == alone:
                assert torch.equal(got, whole)
            else:
                assert got is None


# ---------------------------------------------------------------------------
# 6, 7: SparseAttention and the captured training step
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


def test_sparse_attention_module_paths(dev):
    p = 0.1
    x = torch.randn(2, 256, 256, device=dev)
    layer = make_layer(dev, attention_dropout=p).train()
    plain = make_layer(dev).eval()
    with torch.no_grad():
        assert torch.equal(layer.eval()(x, x, x), plain(x, x, x))
    layer.train()
    results = {}
    for name, setup in (("fused", dict(fused_inference=True, low_memory_training=False)),
                        ("low_memory", dict(fused_inference=False, low_memory_training=True)),
                        ("separate", dict(fused_inference=False, low_memory_training=False))):
        for attr, val in setup.items():
            setattr(layer, attr, val)
        gen(dev).set_offset(400)
        with torch.no_grad():
            results[name] = layer(x, x, x)
        assert gen(dev).get_offset() == 404
    assert rel_err_torch(results["low_memory"], results["fused"]) < 1e-4
    assert rel_err_torch(results["separate"], results["fused"]) < 1e-4
    with torch.no_grad():
        gen(dev).set_offset(400)
        dropped = layer(x, x, x)
    assert not torch.equal(dropped, plain(x, x, x))
    # training (low_memory_training): two runs from one seed are bitwise equal
    layer.fused_inference, layer.low_memory_training = True, True
    torch.manual_seed(11)
    a = layer(x, x, x)
    torch.manual_seed(11)
    b = layer(x, x, x)
    assert torch.equal(a, b)
    a.sum().backward()
    for lin in layer.linears:
        assert torch.isfinite(lin.values.grad).all()


@pytest.mark.parametrize("path", ["low_memory", "separate", "separate_differentiable_softmax"])
def test_sparse_attention_training_step_matches_float64(dev, path):
    """One train-mode step of SparseAttention at a known offset, forward and backward, against
    the float64 module (projections, heads, masked softmax, the numpy mask, output projection).
    The separate-operator path drops with functional.sparse_dropout between the softmax and
    the SpMM; with differentiable_softmax its backward replays the mask on the gradient."""
    p, B, S, E, H = 0.1, 2, 256, 256, 4
    D = E // H
    layer = make_layer(dev, attention_dropout=p, low_memory_training=path == "low_memory",
                       differentiable_softmax=path == "separate_differentiable_softmax").train()
    torch.manual_seed(12)
    x = torch.randn(B, S, E, device=dev).requires_grad_()
    g, offset = gen(dev), 1000
    g.set_offset(offset)
    y = layer(x, x, x)
    assert g.get_offset() == offset + 4
    go = torch.randn_like(y)
    y.backward(go)

    state = torch.tensor([g.initial_seed(), offset])
    csr = [(layer.row_offsets.cpu().numpy(), layer.column_indices.cpu().numpy())]
    factor = dense_keep(csr, state, B * H, p, S, S, B * H)
    mask = (layer.mask2d.cpu() != 0).expand(B * H, S, S)
    weights = [lin.weight.detach().cpu().double().requires_grad_() for lin in layer.linears]
    xd = x.detach().cpu().double().requires_grad_()

    def heads(t):   # [B, S, E] -> [B*H, S, D]
        return t.reshape(B, S, H, D).transpose(1, 2).reshape(B * H, S, D)

    q, k, v = (heads(xd @ w.t()) for w in weights[:3])
    ctx, _ = reference(q, k, v, mask, factor, 1 / math.sqrt(D), cut_softmax=path == "separate")
    want = ctx.reshape(B, H, S, D).transpose(1, 2).reshape(B, S, E) @ weights[3].t()
    assert rel_err_torch(y.detach().cpu(), want.detach()) < TOL[torch.float32]
    want.backward(go.cpu().double())
    assert rel_err_torch(x.grad.cpu(), xd.grad) < TOL[torch.float32]
    for lin, w in zip(layer.linears, weights):
        if w.grad is None:   # (q and k projections behind a softmax without a gradient)
            assert lin.values.grad is None or not lin.values.grad.any()
            continue
        want_values = w.grad[lin.weight.detach().cpu() != 0]
        assert rel_err_torch(lin.values.grad.cpu().reshape(1, -1), want_values.reshape(1, -1)) < TOL[torch.float32]


def test_sparse_attention_half_storage_dropout(dev):
    x = torch.randn(2, 256, 256, device=dev).half()
    layer = make_layer(dev, attention_dropout=0.2, half_storage=True).train()
    torch.manual_seed(2)
    a = layer(x, x, x)
    torch.manual_seed(2)
    b = layer(x, x, x)
    assert torch.equal(a, b)
    with torch.no_grad():
        layer.eval()
        ev = layer(x, x, x)
        plain = make_layer(dev, half_storage=True).eval()
        assert torch.equal(ev, plain(x, x, x))
        assert not torch.equal(a, ev)


def test_captured_training_step_draws_new_masks(dev):
    from torch_sputnik_amd.graphs import capture_training_step
    layer = make_layer(dev, attention_dropout=0.1, low_memory_training=True).train()
    x = torch.randn(2, 256, 256, device=dev)
    go = torch.randn(2, 256, 256, device=dev)
    step = capture_training_step(layer, x, x, x, grad_output=go)
    outs, grads, offsets = [], [], []
    for _ in range(2):
        offsets.append(gen(dev).get_offset())
        outs.append(step(x, x, x, grad_output=go).clone())
        grads.append([None if g is None else g.clone() for g in step.param_grads])
    torch.cuda.synchronize()
    assert not torch.equal(outs[0], outs[1])
    for k in range(2):
        gen(dev).set_offset(offsets[k])
        xe = x.clone().requires_grad_()
        y = layer(xe, xe, xe)
        eager = torch.autograd.grad(y, step.params, go, allow_unused=True)
        assert rel_err_torch(y, outs[k]) < 1e-4
        for got, want in zip(grads[k], eager):
            assert (got is None) == (want is None)
            if got is not None:
                assert rel_err_torch(got, want) < 1e-4
