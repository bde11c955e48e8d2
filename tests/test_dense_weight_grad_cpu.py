"""CPU: the host logic around the dense weight gradient -- ops.dense_weight_grad's torch
path (what a call the kernel does not serve computes), the SparseLinear flow
(collect_dense_grad / dense_grad / zero_dense_grad / rigl_update) on a float32 CPU module,
and the host-only `supported` query of the C ABI.  No kernel runs here."""
import numpy as np
import pytest
import torch

from tests.helpers import rel_err

TOL = 1e-4
OUT, IN, SEQ, BATCH = 24, 16, 12, 3


def _operands(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(BATCH, OUT, SEQ, generator=gen), torch.randn(BATCH, SEQ, IN, generator=gen)


def _ref(g, x):
    return np.einsum("bos,bsi->oi", g.double().numpy(), x.double().numpy())


@pytest.mark.parametrize("layout", ["bsi", "bis"])
def test_dense_weight_grad_on_cpu_tensors(cpu_ops, layout):
    ops = cpu_ops.ops
    g, x = _operands()
    operand = x if layout == "bsi" else x.transpose(1, 2).contiguous()
    dense = ops.dense_weight_grad(g, operand, layout)
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (OUT, IN)
    assert rel_err(dense.numpy(), _ref(g, x)) < TOL
    # 2-D operands count as B = 1
    dense = ops.dense_weight_grad(g[0], operand[0], layout)
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (OUT, IN)
    assert rel_err(dense.numpy(), _ref(g[:1], x[:1])) < TOL
    # half operands of two types: float32 copies, float32 result
    dense = ops.dense_weight_grad(g.half(), operand.bfloat16(), layout)
    assert dense.dtype == torch.float32
    assert rel_err(dense.numpy(), _ref(g.half(), x.bfloat16())) < TOL


def test_dense_weight_grad_argument_errors(cpu_ops):
    ops = cpu_ops.ops
    g, x = _operands()
    with pytest.raises(ValueError):
        ops.dense_weight_grad(g, x, "sbi")
    with pytest.raises(ValueError):
        ops.dense_weight_grad(g, x, "bis")                    # [B, S, in] handed over as [B, in, S]
    with pytest.raises(ValueError):
        ops.dense_weight_grad(g, x[:2])
    with pytest.raises(ValueError):
        ops.dense_weight_grad(g[None], x[None])


def _layer(cpu_ops, seed, per_row=True):
    gen = torch.Generator().manual_seed(seed)
    return cpu_ops.SparseLinear.from_dense(torch.randn(OUT, IN, generator=gen), density=0.25, per_row=per_row)


def _backward(layer, x, upstream):
    layer.values.grad = None
    layer(x).backward(upstream)
    return layer.values.grad.clone()


def test_sparse_linear_collects_the_dense_gradient(cpu_ops):
    layer = _layer(cpu_ops, seed=1)
    upstream, x = _operands(seed=2)
    want = _ref(upstream, x)
    assert layer.dense_grad is None
    disarmed = _backward(layer, x, upstream)
    assert layer.dense_grad is None                           # disarmed: nothing collected
    assert layer.collect_dense_grad() is layer
    armed = _backward(layer, x, upstream)
    assert torch.equal(armed, disarmed)
    first = layer.dense_grad
    assert first.dtype == torch.float32 and tuple(first.shape) == (OUT, IN)
    assert not isinstance(first, torch.nn.Parameter)
    assert "dense_grad" not in layer.state_dict() and "dense_grad" not in dict(layer.named_buffers())
    assert rel_err(first.numpy(), want) < TOL
    # the sparse gradient is the dense one under the mask
    rows = torch.repeat_interleave(torch.arange(OUT), (layer.row_offsets[1:] - layer.row_offsets[:-1]).long())
    sampled = first[rows, layer.column_indices.long()].numpy()
    assert rel_err(armed.numpy()[None, :], sampled.astype(np.float64)[None, :]) < TOL
    _backward(layer, x, upstream)
    assert layer.dense_grad is first                          # added in place, as .grad
    assert rel_err(layer.dense_grad.numpy(), 2.0 * want) < TOL
    layer.zero_dense_grad()
    assert layer.dense_grad is None
    (layer(x) + layer(x)).backward(upstream)                  # a layer used twice in one graph
    assert rel_err(layer.dense_grad.numpy(), 2.0 * want) < TOL
    layer.zero_dense_grad()
    layer.collect_dense_grad(False)
    _backward(layer, x, upstream)
    assert layer.dense_grad is None


def test_arming_is_looked_at_when_the_backward_runs(cpu_ops):
    layer = _layer(cpu_ops, seed=9)
    upstream, x = _operands(seed=10)
    y = layer(x)
    layer.collect_dense_grad()                                # armed after the forward pass
    y.backward(upstream, retain_graph=True)
    assert rel_err(layer.dense_grad.numpy(), _ref(upstream, x)) < TOL
    layer.zero_dense_grad()
    layer.collect_dense_grad(False)
    y.backward(upstream)
    assert layer.dense_grad is None


def test_project_collects_through_split_rows_and_dense_blocks(cpu_ops):
    layer = _layer(cpu_ops, seed=3).collect_dense_grad()
    upstream, x = _operands(seed=4)
    want = _ref(upstream, x)
    d = 8
    dense = x.transpose(1, 2).contiguous()                    # [B, in, S]
    y = layer.project(dense, split_rows=d)                    # [B * out/d, S, d]
    y.backward(upstream.reshape(BATCH * OUT // d, d, SEQ).transpose(1, 2).contiguous())
    assert rel_err(layer.dense_grad.numpy(), want) < TOL
    layer.zero_dense_grad()
    blocks = dense.reshape(BATCH * IN // d, d, SEQ).clone().requires_grad_(True)
    layer.project(blocks, dense_blocks=d).backward(upstream)
    assert rel_err(layer.dense_grad.numpy(), want) < TOL
    assert blocks.grad is not None and blocks.grad.shape == blocks.shape


def test_function_call_sites_with_the_old_argument_counts(cpu_ops):
    """The sink is one trailing optional argument: apply() with the arguments of before."""
    layer = _layer(cpu_ops, seed=5)
    upstream, x = _operands(seed=6)
    dense = x.transpose(1, 2).contiguous()
    topo = (layer.row_indices, layer.row_offsets, layer.column_indices)
    y7 = cpu_ops.SparseLinearFunction.apply(OUT, IN, layer.values, *topo, dense)
    y9 = cpu_ops.SparseLinearFunction.apply(OUT, IN, layer.values, *topo, dense, 0, 0)
    assert torch.equal(y7, y9)
    y7.backward(upstream)
    assert layer.values.grad is not None and layer.dense_grad is None


@pytest.mark.parametrize("per_row", [True, False])
def test_rigl_update_twins(cpu_ops, per_row):
    twins = [_layer(cpu_ops, seed=7).collect_dense_grad() for _ in range(2)]
    upstream, x = _operands(seed=8)
    with pytest.raises(RuntimeError):
        twins[0].rigl_update(0.3, per_row=per_row)            # nothing collected
    for layer in twins:
        layer(x).backward(upstream)
    assert torch.equal(twins[0].dense_grad, twins[1].dense_grad)
    source = twins[0].rigl_update(0.3, per_row=per_row)
    want = twins[1].update_topology(0.3, grow_scores=twins[1].dense_grad.clone(), per_row=per_row)
    assert torch.equal(source, want) and int((source < 0).sum()) > 0
    for name in ("column_indices", "row_offsets"):
        assert torch.equal(getattr(twins[0], name), getattr(twins[1], name))
    assert torch.equal(twins[0].values.detach(), twins[1].values.detach())
    assert twins[0].dense_grad is None                        # cleared; the layer stays armed
    with pytest.raises(RuntimeError):
        twins[0].rigl_update(0.3, per_row=per_row)
    twins[0](x).backward(upstream)                            # forward and backward on the new pattern
    assert rel_err(twins[0].dense_grad.numpy(), _ref(upstream, x)) < TOL


def test_supported_query_is_host_only():
    from torch_sputnik_amd import capi, ops
    query = capi.lib().sputnik_hip_sparse_linear_dense_weight_gradient_supported
    F32, F16, BF16, BSI, BIS = 0, 1, 2, 0, 1
    assert query(2048, 2048, 512, 8, F16, F16, BSI, F16) == 1
    assert query(192, 320, 192, 3, F32, BF16, BIS, BF16) == 1          # no density or size floor
    assert query(2048, 2048, 512, 8, F32, F32, BSI, F16) == 1          # float16: 2 x 2 planes
    assert query(2048, 2048, 512, 8, F32, F32, BSI, BF16) == 0         # bfloat16: 3 x 3 is not built
    assert query(2048, 2048, 520, 8, F16, F16, BSI, F16) == 0          # seq % 64 != 0
    assert query(2048, 2044, 512, 8, F16, F16, BSI, F16) == 0          # in % 8 != 0
    assert query(2048, 2048, 512, 8, F16, BF16, BSI, F16) == 0         # two half types
    assert query(2048, 2048, 512, 8, F16, F16, 2, F16) == 0
    assert query(1 << 16, 1 << 15, 64, 1, F16, F16, BSI, F16) == 0     # out * in reaches 2^30
    assert ops.dense_weight_grad_supported(2048, 2048, 512, 8, torch.float32, torch.float16, "bis", torch.float16)
    assert not ops.dense_weight_grad_supported(2048, 2048, 512, 8, torch.float64, torch.float16, "bsi",
                                               torch.float16)
