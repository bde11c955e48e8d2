"""CPU (host logic through the oracle backend): the many-mask topology helper, the autograd
forms of the many-mask attention on the composed operators, and SparseCoreAttention's
contract (tests/transformer/modules.py:9-81 of the reference)."""
import math

import numpy as np
import pytest
import torch


def _masks(b, s, seed):
    rng = np.random.default_rng(seed)
    dense = rng.random((b, s, s)) < np.array([0.3, 0.6, 0.1, 0.45])[np.arange(b) % 4, None, None]
    dense[0, 2] = False   # a row without entries
    return torch.from_numpy(dense)


def _reference_3d(mask):
    """tests/transformer/utils.py:17-38 restated (row_offsets and columns per mask)."""
    out = []
    for i in range(mask.size(0)):
        csr = mask[i].to_sparse_csr()
        out.append((csr.crow_indices().to(torch.int32), csr.col_indices().to(torch.int32), csr._nnz()))
    return out


def test_dense_to_sparse_3d_layout(cpu_ops):
    for b in (1, 3):
        mask = _masks(b, 12, seed=b).to(torch.int64).unsqueeze(1)   # [b, 1, s, s] as the module gets it
        ri, ro, ci, nnz = cpu_ops.dense_to_sparse_3d(mask)
        want = _reference_3d(mask.squeeze(1))
        assert ri.dtype == ro.dtype == ci.dtype == torch.int32
        assert ri.shape == (b, 12) and ro.shape == (b, 13)
        assert nnz == [w[2] for w in want] and isinstance(nnz, list)
        assert torch.equal(ci, torch.cat([w[1] for w in want]))
        for i in range(b):
            assert torch.equal(ro[i], want[i][0])
            lengths = (ro[i, 1:] - ro[i, :-1])[ri[i].long()]
            assert sorted(ri[i].tolist()) == list(range(12))
            assert torch.all(lengths[1:] >= lengths[:-1])   # rows by ascending length


def _dense_reference(q, k, v, mask, heads, scale):
    q, k, v = (x.double() for x in (q, k, v))
    m = mask.repeat_interleave(heads, 0)
    s = (scale * q @ k.transpose(1, 2)).masked_fill(~m, float("-inf"))
    return torch.softmax(s, -1).nan_to_num(0.0) @ v


def test_functional_forms_match_float64(cpu_ops):
    from torch_sputnik_amd import functional as F
    b, heads, s, d = 3, 2, 10, 8
    mask = _masks(b, s, seed=5)
    ri, ro, ci, nnz = cpu_ops.dense_to_sparse_3d(mask)
    torch.manual_seed(0)
    q, k, v = (torch.randn(b * heads, s, d, requires_grad=True) for _ in range(3))
    out = F.sparse_attention_many_mask(b, s, s, torch.tensor(nnz), ri, ro, ci, q, k, v, 0.4)
    xd = [x.detach().double().requires_grad_(True) for x in (q, k, v)]
    want = _dense_reference(*xd, mask, heads, 0.4)
    assert torch.allclose(out.double(), want, atol=1e-5)
    g = torch.randn_like(out)
    (out * g).sum().backward()
    (want * g.double()).sum().backward()
    for x, w in zip((q, k, v), xd):
        assert torch.allclose(x.grad.double(), w.grad, atol=1e-5)
    # [B, S, H, D] views of one [B, S, H, 3D] tensor
    qkv = torch.randn(b, s, heads, 3 * d, requires_grad=True)
    views = torch.split(qkv, d, dim=-1)
    out4 = F.sparse_attention_heads_many_mask(*views, nnz, ri, ro, ci, 0.4)
    assert out4.shape == (b, s, heads, d)
    per_head = [x.detach().double().transpose(1, 2).reshape(b * heads, s, d) for x in views]
    want4 = _dense_reference(*per_head, mask, heads, 0.4)
    assert torch.allclose(out4.double().transpose(1, 2).reshape(b * heads, s, d), want4, atol=1e-5)
    out4.sum().backward()
    assert qkv.grad.shape == qkv.shape and torch.isfinite(qkv.grad).all()


def test_core_attention_module_contract(cpu_ops):
    b, n, s, hn = 2, 3, 10, 4
    mod = cpu_ops.SparseCoreAttention(s, n * hn, n)
    mask = _masks(b, s, seed=9).unsqueeze(1).to(torch.int64)
    torch.manual_seed(1)
    qkv = torch.randn(b, s, n, 3 * hn, requires_grad=True)
    q, k, v = torch.split(qkv, hn, dim=-1)
    out = mod(q, k, v, mask)
    assert out.shape == (s, b, n * hn)
    # the reference's own computation, in float64
    qd, kd, vd = (x.detach().double().permute(0, 2, 1, 3).reshape(b * n, s, hn) for x in (q, k, v))
    want = _dense_reference(qd, kd, vd, mask.squeeze(1) != 0, n, 1 / math.sqrt(hn))
    want = want.permute(1, 0, 2).reshape(s, b, n * hn)
    assert torch.allclose(out.double(), want, atol=1e-5)
    out.sum().backward()
    assert qkv.grad is not None and torch.isfinite(qkv.grad).all()
    # a static topology gives the same result without the mask
    topology = cpu_ops.dense_to_sparse_3d(mask)
    with torch.no_grad():
        assert torch.equal(mod(q, k, v, None, topology=topology), out.detach())


# ---------------------------------------------------------------------------
# rectangular masks (m query rows != n key rows): the host-side m / n bookkeeping of the
# forward, the backward's transposed products and the drop-in functions
# ---------------------------------------------------------------------------
RECTANGLES = [(7, 13), (13, 5), (20, 9)]


def _rect_masks(b, m, n, seed, empty):
    """[b, m, n] masks of different densities, mask `empty` without entries, a row without
    entries in another one."""
    rng = np.random.default_rng(seed)
    dense = rng.random((b, m, n)) < np.array([0.5, 0.25, 0.8])[np.arange(b) % 3, None, None]
    dense[empty] = False
    dense[(empty + 1) % b, m // 2] = False
    dense[(empty + 2) % b, :, n - 1] = True   # a full last key column
    return torch.from_numpy(dense)


@pytest.mark.parametrize("m,n", RECTANGLES)
def test_dense_to_sparse_3d_rectangular(cpu_ops, m, n):
    for b, empty in ((1, None), (3, 0), (3, 2)):
        mask = _rect_masks(b, m, n, seed=m * n + b, empty=0 if empty is None else empty)
        if empty is None:
            mask[0, 0, 0] = True
        ri, ro, ci, nnz = cpu_ops.dense_to_sparse_3d(mask.unsqueeze(1).to(torch.int64))
        want = _reference_3d(mask)
        assert ri.shape == (b, m) and ro.shape == (b, m + 1)
        assert nnz == [w[2] for w in want]
        assert torch.equal(ci, torch.cat([w[1] for w in want]))
        assert ci.numel() == 0 or int(ci.max()) < n
        for i in range(b):
            assert torch.equal(ro[i], want[i][0])
            assert sorted(ri[i].tolist()) == list(range(m))


def _rect_reference(q, k, v, mask, heads, scale):
    from helpers import ref_attention_many_mask
    assert q.size(0) == mask.size(0) * heads
    return ref_attention_many_mask(q, k, v, mask, scale)[0]


@pytest.mark.parametrize("empty", [0, 2])
@pytest.mark.parametrize("m,n", RECTANGLES)
def test_functional_forms_rectangular(cpu_ops, m, n, empty):
    """Forward and all three gradients of both forms against float64, with the empty mask
    first or last."""
    from torch_sputnik_amd import functional as F
    b, heads, d, scale = 3, 2, 8, 0.4
    mask = _rect_masks(b, m, n, seed=m + 10 * n + empty, empty=empty)
    ri, ro, ci, nnz = cpu_ops.dense_to_sparse_3d(mask)
    g = torch.Generator().manual_seed(m * n + empty)
    q = torch.randn(b * heads, m, d, generator=g, requires_grad=True)
    k, v = (torch.randn(b * heads, n, d, generator=g, requires_grad=True) for _ in range(2))
    out = F.sparse_attention_many_mask(b, m, n, torch.tensor(nnz), ri, ro, ci, q, k, v, scale)
    assert out.shape == (b * heads, m, d)
    xd = [x.detach().double().requires_grad_(True) for x in (q, k, v)]
    want = _rect_reference(*xd, mask, heads, scale)
    assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)
    assert not out[empty * heads:(empty + 1) * heads].any()
    grad = torch.randn(out.shape, generator=g)
    (out * grad).sum().backward()
    (want * grad.double()).sum().backward()
    for name, x, w in zip("qkv", (q, k, v), xd):
        assert x.grad.shape == x.shape, name
        assert torch.allclose(x.grad.double(), w.grad, rtol=1e-5, atol=1e-5), name
    # [B, S, H, D]: query [B, m, H, D], key and value views of one [B, n, H, 2D] tensor
    q4 = q.detach().reshape(b, heads, m, d).transpose(1, 2).contiguous().requires_grad_(True)
    kv = torch.cat([x.detach().reshape(b, heads, n, d).transpose(1, 2) for x in (k, v)], -1)
    kv.requires_grad_(True)
    out4 = F.sparse_attention_heads_many_mask(q4, kv[..., :d], kv[..., d:], nnz, ri, ro, ci, scale)
    assert out4.shape == (b, m, heads, d)
    assert torch.allclose(out4.double().transpose(1, 2).reshape(b * heads, m, d), want, rtol=1e-5,
                          atol=1e-5)
    (out4 * grad.reshape(b, heads, m, d).transpose(1, 2)).sum().backward()
    per_head = lambda t: t.transpose(1, 2).reshape(b * heads, -1, d).double()
    assert torch.allclose(per_head(q4.grad), xd[0].grad, rtol=1e-5, atol=1e-5)
    assert torch.allclose(per_head(kv.grad[..., :d]), xd[1].grad, rtol=1e-5, atol=1e-5)
    assert torch.allclose(per_head(kv.grad[..., d:]), xd[2].grad, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("empty", [0, 2])
@pytest.mark.parametrize("m,n", RECTANGLES)
def test_dropin_functions_rectangular(cpu_ops, m, n, empty):
    """SpmmManyMask, SddmmManyMask and CsrSoftmaxManyMask: outputs and the gradients of
    values / dense, lhs / rhs and scores against float64 autograd."""
    from helpers import (many_mask_entries, ref_sddmm_many_mask, ref_softmax_many_mask,
                         ref_spmm_many_mask)
    from torch_sputnik_amd.functional import CsrSoftmaxManyMask, SddmmManyMask, SpmmManyMask
    b, heads = 3, 2
    R = b * heads
    mask = _rect_masks(b, m, n, seed=7 * m + n + empty, empty=empty)
    ri, ro, ci, nnz = cpu_ops.dense_to_sparse_3d(mask)
    width = max(nnz)
    entries = many_mask_entries(nnz, ro, ci, m, heads, "cpu")
    g = torch.Generator().manual_seed(m + n + empty)
    rnd = lambda *s: torch.randn(*s, generator=g)

    def check(got, want):
        assert got.shape == want.shape
        assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-5)

    # SpMM: [R, m, n] sparse x [R, n, 5]; values rows padded by 2 (their gradient: 0)
    values, dense = rnd(R, width + 2).requires_grad_(True), rnd(R, n, 5).requires_grad_(True)
    out = SpmmManyMask.apply(b, m, n, nnz, values, ri, ro, ci, dense)
    vd, dd = (x.detach().double().requires_grad_(True) for x in (values, dense))
    want = ref_spmm_many_mask(entries, m, vd, dd)
    check(out, want.detach())
    grad = rnd(R, m, 5)
    out.backward(grad)
    want.backward(grad.double())
    check(values.grad, vd.grad)
    check(dense.grad, dd.grad)

    # SDDMM: lhs [R, m, 6], rhs [R, n, 6] -> [R, width]
    lhs, rhs = rnd(R, m, 6).requires_grad_(True), rnd(R, n, 6).requires_grad_(True)
    out = SddmmManyMask.apply(b, m, n, nnz, ri, ro, ci, lhs, rhs)
    ld, rd = (x.detach().double().requires_grad_(True) for x in (lhs, rhs))
    want = ref_sddmm_many_mask(entries, width, ld, rd)
    check(out, want.detach())
    grad = rnd(R, width)
    out.backward(grad)
    want.backward(grad.double())
    check(lhs.grad, ld.grad)
    check(rhs.grad, rd.grad)

    # softmax of scale * scores over each row's entries
    scores = rnd(R, width).requires_grad_(True)
    out = CsrSoftmaxManyMask.apply(b, m, nnz, scores, ri, ro, ci, 0.5)
    sd = scores.detach().double().requires_grad_(True)
    want = ref_softmax_many_mask(entries, m, n, sd, 0.5)
    check(out, want.detach())
    grad = rnd(R, width)
    out.backward(grad)
    want.backward(grad.double())
    check(scores.grad, sd.grad)
