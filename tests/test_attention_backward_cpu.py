"""CPU: the surface of the fused attention backward -- SparseAttention's fused_backward flag,
the C ABI's host-side rules (served shapes, workspace size, argument checks that return before
any launch) and the op's registration."""
import numpy as np
import pytest
import torch


def attention(**kw):
    from torch_sputnik_amd.modules import SparseAttention
    return SparseAttention(num_heads=2, embedding_size=16, max_sequence_length=24,
                           device=torch.device("cpu"), sparsity=0.6,
                           mask_generator=np.random.default_rng(5), **kw)


def test_module_rejects_half_storage_with_fused_backward():
    with pytest.raises(ValueError):
        attention(half_storage=True, fused_backward=True)


def test_module_accepts_fused_backward():
    assert attention(fused_backward=True).fused_backward
    assert not attention().fused_backward
    layer = attention(fused_backward=True, low_memory_training=True, attention_dropout=0.1)
    assert layer.fused_backward and layer.low_memory_training
    assert attention(half_storage=True).half_storage


def test_supported_shapes():
    from torch_sputnik_amd import capi, ops
    sup = capi.lib().sputnik_hip_sparse_attention_backward_supported
    assert sup(1024, 1024, 64, 104858) == 1
    assert sup(200, 136, 64, 0) == 1            # (a mask without entries: zero gradients)
    assert sup(1024, 1024, 32, 104858) == 0     # head dimension other than 64
    assert sup(1 << 24, 1024, 64, 100) == 0     # m * 64 * 4 reaches 2^32
    assert sup(1024, 1 << 24, 64, 100) == 0     # n * 64 * 4 reaches 2^32
    assert sup((1 << 24) - 1, (1 << 24) - 1, 64, 100) == 1
    assert ops.sparse_attention_backward_supported(64, 64, 64, 10)


def test_workspace_is_one_float_per_row():
    from torch_sputnik_amd import capi
    ws = capi.lib().sputnik_hip_sparse_attention_backward_workspace_bytes
    assert ws(1024, 1024, 64, 104858, 64) == 64 * 1024 * 4
    assert ws(3, 5, 64, 7, 1) == 16             # (rounded up to 16 bytes)
    assert ws(1024, 1024, 32, 104858, 64) == 0


def test_host_checks_return_before_any_launch():
    from torch_sputnik_amd import capi
    fn = capi.lib().sputnik_hip_sparse_attention_backward
    null = [None] * 7
    operands = [None, 0] * 3

    def call(m=64, n=64, d=64, nnz=10, replicas=2, p=0.0, grads=(None, 0) * 3, ws=None, wsb=0):
        return fn(m, n, d, nnz, replicas, *null, *operands, 0.125, None, 0, None, 0, None, 0,
                  *grads, p, capi.PhiloxState(), ws, wsb, None)

    assert call(p=1.0) == -1             # p outside [0, 1)
    assert call(p=float("nan")) == -1
    assert call(m=-1) == -1
    assert call() == 0                   # no gradient wanted: nothing to do
    fake = (16, 0) + (None, 0) * 2       # (a pointer value that is never dereferenced)
    assert call(d=32, grads=fake) == -2  # not served
    assert call(grads=(8, 0) + (None, 0) * 2) == -2   # misaligned output
    assert call(grads=fake) == -1        # missing operands


def test_ops_registered():
    from torch_sputnik_amd import ops  # noqa: F401  (loads the library)
    for name in ("sparse_attention_backward", "sparse_attention_with_lse_planned"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"torch_sputnik::{name}", "CUDA")
