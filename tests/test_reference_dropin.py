"""CPU: the drop-in claim against the reference's OWN Python layer
(modules/spmm.py, modules/sddmm.py, modules/sparse_linear.py and the many-mask
sketches of tests/transformer/functions.py).  What that layer returned --
forward values and the gradients autograd left on its inputs, run against this
repo's ``torch_sputnik`` -- is stored in tests/golden/reference_layer_*.npz
(oracle/make_golden.py ``reference_layer_cases``).  Here this package's own
layer, called the same way, must give the same results: same shapes and dtypes,
the dense float64 definition within the parity bound, and the reference layer's
values."""
import numpy as np
import torch

from helpers import make_csr, rel_err


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def same_inputs(g, **arrays):
    """The stored results belong to exactly these inputs."""
    for name, a in arrays.items():
        assert np.array_equal(g[name], a), f"golden {name} differs from the test's input"


def like_reference(got, want):
    """A result of this package's layer against the reference layer's."""
    got = got.detach()
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert rel_err(got.numpy(), want) < 2e-5


def test_reference_spmm_function(cpu_ops, golden):
    g = golden("reference_layer_spmm")
    dense_a, vals, ri, ro, ci = make_csr(18, 14, 0.6, seed=1, order="ascending")
    b = np.random.default_rng(2).uniform(-1, 1, (14, 9)).astype(np.float32)
    same_inputs(g, values=vals, row_indices=ri, row_offsets=ro, column_indices=ci, dense=b)
    v, d = T(vals).requires_grad_(True), T(b).requires_grad_(True)
    out = cpu_ops.Spmm.apply(18, 14, v, T(ri), T(ro), T(ci), d)
    out.square().sum().backward()
    ad = T(dense_a).double().requires_grad_(True)
    bd = T(b).double().requires_grad_(True)
    (ad @ bd).square().sum().backward()
    assert rel_err(out.detach().numpy(), (ad @ bd).detach().numpy()) < 2e-5
    assert rel_err(d.grad.numpy(), bd.grad.numpy()) < 2e-5
    assert rel_err(v.grad.numpy(), ad.grad.numpy()[dense_a != 0]) < 2e-5
    like_reference(out, g["out"])
    like_reference(v.grad, g["grad_values"])
    like_reference(d.grad, g["grad_dense"])


def test_reference_sddmm_function(cpu_ops, golden):
    g = golden("reference_layer_sddmm")
    mask, _, ri, ro, ci = make_csr(16, 20, 0.7, seed=3, round_to=1)
    rng = np.random.default_rng(4)
    lhs = rng.uniform(-1, 1, (16, 6)).astype(np.float32)
    rhs = rng.uniform(-1, 1, (20, 6)).astype(np.float32)
    same_inputs(g, row_indices=ri, row_offsets=ro, column_indices=ci, lhs=lhs, rhs=rhs)
    l, r = T(lhs).requires_grad_(True), T(rhs).requires_grad_(True)
    out = cpu_ops.Sddmm.apply(16, 20, T(ri), T(ro), T(ci), l, r)
    out.square().sum().backward()
    ld, rd = T(lhs).double().requires_grad_(True), T(rhs).double().requires_grad_(True)
    dense = (ld @ rd.t())[T(mask != 0)]
    dense.square().sum().backward()
    assert rel_err(out.detach().numpy(), dense.detach().numpy()) < 2e-5
    assert rel_err(l.grad.numpy(), ld.grad.numpy()) < 2e-5
    assert rel_err(r.grad.numpy(), rd.grad.numpy()) < 2e-5
    like_reference(out, g["out"])
    like_reference(l.grad, g["grad_lhs"])
    like_reference(r.grad, g["grad_rhs"])


def test_reference_sparse_linear_module(cpu_ops, golden):
    """The reference's module hands left_spmm an int64 row_indices in its
    backward (modules/sparse_linear.py:57-65); its stored
    gradients went through that path."""
    g = golden("reference_layer_sparse_linear")
    torch.manual_seed(0)
    out_f, in_f, seq, batch = 24, 16, 7, 3
    w = (torch.randn(out_f, in_f) * (torch.rand(out_f, in_f) > 0.7)).float()
    layer = cpu_ops.SparseLinear(in_f, out_f)
    with torch.no_grad():
        layer.weight.copy_(w)
    layer.setup_sparse_tensors()
    x = torch.randn(batch, seq, in_f, requires_grad=True)
    same_inputs(g, weight=w.numpy(), x=x.detach().numpy())
    y = layer(x)
    assert tuple(y.shape) == (batch, out_f, seq)
    y.square().sum().backward()
    wd = w.double().requires_grad_(True)
    xd = x.detach().double().requires_grad_(True)
    yd = torch.matmul(xd, wd.t()).transpose(1, 2)
    yd.square().sum().backward()
    assert rel_err(y.detach().numpy(), yd.detach().numpy()) < 2e-5
    assert rel_err(x.grad.numpy(), xd.grad.numpy()) < 2e-5
    assert rel_err(layer.values.grad.numpy(), wd.grad.numpy()[w.numpy() != 0]) < 2e-5
    like_reference(y, g["y"])
    like_reference(x.grad, g["grad_x"])
    like_reference(layer.values.grad, g["grad_values"])


def test_own_functions_agree_with_reference_functions(cpu_ops, golden):
    """Bit for bit: the gradients of this package's Spmm are the ones the
    reference's Spmm produced over the same ops."""
    g = golden("reference_layer_spmm_agree")
    dense_a, vals, ri, ro, ci = make_csr(20, 12, 0.5, seed=5)
    b = np.random.default_rng(6).uniform(-1, 1, (12, 5)).astype(np.float32)
    same_inputs(g, values=vals, row_indices=ri, row_offsets=ro, column_indices=ci, dense=b)
    v, d = T(vals).requires_grad_(True), T(b).requires_grad_(True)
    cpu_ops.Spmm.apply(20, 12, v, T(ri), T(ro), T(ci), d).square().sum().backward()
    assert torch.equal(v.grad, T(g["grad_values"])) and torch.equal(d.grad, T(g["grad_dense"]))


def test_reference_many_mask_sketches(cpu_ops, golden):
    """The many-mask autograd functions, with the topology the reference's
    tests/transformer/utils.py builds (stacked [b, s+1] offsets, int64 nnzs),
    forward and backward against the golden dense-autograd values and the
    reference sketches' results."""
    from torch_sputnik_amd.functional import SddmmManyMask, SpmmManyMask
    g = golden("many_mask_b3_h2_s24")
    r = golden("reference_layer_many_mask")
    b, s = int(g["b"]), int(g["s"])
    ri, ro, ci, nnzs = (T(r[n]) for n in ("row_indices", "row_offsets", "column_indices", "nnzs"))
    assert ro.shape == (b, s + 1) and np.array_equal(nnzs.numpy(), g["nnzs"])
    q, k = T(g["q"]).requires_grad_(True), T(g["k"]).requires_grad_(True)
    scores = SddmmManyMask.apply(b, s, s, nnzs, ri, ro, ci, q, k)
    scores.backward(T(g["grad_scores"]))
    assert rel_err(scores.detach().numpy(), g["scores"]) < 2e-5
    assert rel_err(q.grad.numpy(), g["grad_q"]) < 2e-5
    assert rel_err(k.grad.numpy(), g["grad_k"]) < 2e-5
    w, v = T(g["weights"]).requires_grad_(True), T(g["v"]).requires_grad_(True)
    ctx = SpmmManyMask.apply(b, s, s, nnzs, w, ri, ro, ci, v)
    ctx.backward(T(g["grad_context"]))
    assert rel_err(ctx.detach().numpy(), g["context"]) < 2e-5
    assert rel_err(w.grad.numpy(), g["grad_weights"]) < 2e-5
    assert rel_err(v.grad.numpy(), g["grad_v"]) < 2e-5
    for name, got in (("scores", scores), ("grad_q", q.grad), ("grad_k", k.grad),
                      ("context", ctx), ("grad_weights", w.grad), ("grad_v", v.grad)):
        like_reference(got, r[name])
