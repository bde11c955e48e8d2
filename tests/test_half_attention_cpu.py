"""CPU (host logic through the oracle backend): SparseAttention's ``half_storage`` flag is
an opt-in for float16 / bfloat16 inputs only -- float32 inputs give bit for bit the
module's default result, and the flag is kept on the module."""
import numpy as np
import torch


def _module(cpu_ops, heads, emb, seq, **flags):
    torch.manual_seed(0)
    attn = cpu_ops.SparseAttention(heads, emb, max_sequence_length=seq, device="cpu", sparsity=0.5,
                                   mask_generator=np.random.default_rng(1), **flags)
    for lin in attn.linears:
        w = torch.randn(emb, emb) * (torch.rand(emb, emb) > 0.4)
        with torch.no_grad():
            lin.weight.copy_(w)
        lin.setup_sparse_tensors()
    return attn


def test_half_storage_with_float32_inputs_is_the_default_module(cpu_ops):
    heads, emb, seq, batch = 2, 8, 12, 2
    off = _module(cpu_ops, heads, emb, seq)
    on = _module(cpu_ops, heads, emb, seq, half_storage=True)
    assert off.half_storage is False and on.half_storage is True
    q, k, v = (torch.randn(batch, seq, emb) for _ in range(3))
    with torch.no_grad():
        assert torch.equal(on(q, k, v, None), off(q, k, v, None))
        assert torch.equal(on(q, q, q, None), off(q, q, q, None))
    # under autograd as well: same output, same gradients
    xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ys = [t.clone().requires_grad_(True) for t in (q, k, v)]
    a, b = on(*xs), off(*ys)
    assert torch.equal(a, b)
    a.sum().backward()
    b.sum().backward()
    for x, y in zip(xs, ys):
        assert torch.equal(x.grad, y.grad)
