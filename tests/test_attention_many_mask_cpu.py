"""CPU (host logic through the oracle backend): the many-mask topology helper, the autograd
forms of the many-mask attention on the composed operators, and SparseCoreAttention's
contract (tests/transformer/modules.py:9-81 of the reference)."""
import math

import numpy as np
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
