"""CPU: the host-side rules of fused sparse attention training at head dimension 128 -- the
backward's served shapes and workspace at d = 128, the row-group forward's served shapes and
its argument checks (which return before any launch), and the op's registration."""
import torch


def test_backward_supported_at_128():
    from torch_sputnik_amd import capi
    sup = capi.lib().sputnik_hip_sparse_attention_backward_supported
    assert sup(1024, 1024, 128, 104858) == 1
    assert sup((1 << 23) - 1, (1 << 23) - 1, 128, 100) == 1
    assert sup(1 << 23, 1024, 128, 100) == 0     # m * 128 * 4 reaches 2^32
    assert sup(1024, 1 << 23, 128, 100) == 0     # n * 128 * 4 reaches 2^32
    assert sup(1024, 1024, 96, 104858) == 0
    assert sup(1024, 1024, 256, 104858) == 0


def test_backward_workspace_is_one_float_per_row_at_128():
    from torch_sputnik_amd import capi
    ws = capi.lib().sputnik_hip_sparse_attention_backward_workspace_bytes
    assert ws(1024, 1024, 128, 104858, 64) == 64 * 1024 * 4


def test_rows_supported():
    from torch_sputnik_amd import capi, ops
    sup = capi.lib().sputnik_hip_sparse_attention_rows_supported
    assert sup(1024, 1024, 128, 104858) == 1
    assert sup((1 << 23) - 1, (1 << 23) - 1, 128, 1) == 1
    assert sup(1024, 1024, 64, 104858) == 0      # the LDS-staged forward's head dimension
    assert sup(1024, 1024, 32, 104858) == 0
    assert sup(1024, 1024, 128, 0) == 0          # a mask without entries
    assert sup(1 << 23, 1024, 128, 100) == 0
    assert sup(1024, 1 << 23, 128, 100) == 0
    assert ops.sparse_attention_rows_supported(64, 64, 128, 10)
    assert not ops.sparse_attention_rows_supported(64, 64, 64, 10)


def test_rows_forward_host_checks_return_before_any_launch():
    from torch_sputnik_amd import capi
    fn = capi.lib().sputnik_hip_sparse_attention_rows_forward
    fake = 16   # (a pointer value that is never dereferenced)

    def call(m=64, n=64, d=128, nnz=10, replicas=2, p=0.0, topology=(None,) * 3,
             operands=(None, 0) * 3, out=(None, 0), lse=(None, 0)):
        return fn(m, n, d, nnz, replicas, *topology, *operands, 0.125, *out, *lse, p,
                  capi.PhiloxState(), None, None)

    assert call(p=1.0) == -1             # p outside [0, 1)
    assert call(p=float("nan")) == -1
    assert call(p=-0.5) == -1
    for name in ("m", "n", "d", "nnz", "replicas"):
        assert call(**{name: -1}) == -1
    assert call(replicas=0) == 0         # nothing to do
    assert call(d=64) == -2              # not served
    assert call(nnz=0) == -2
    assert call(m=1 << 23) == -2
    assert call(out=(8, 0)) == -2        # misaligned output
    assert call(operands=(fake, 2) + (None, 0) * 2) == -2   # stride not a multiple of 4
    assert call(operands=(fake, -4) + (None, 0) * 2) == -2  # negative stride
    assert call() == -1                  # missing operands
    assert call(operands=(fake, 0) * 3, out=(fake, 0)) == -1   # missing topology
    assert call(topology=(fake,) * 3, operands=(fake, 0) * 3) == -1   # missing out


def test_rows_op_registered():
    from torch_sputnik_amd import ops  # noqa: F401  (loads the library)
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torch_sputnik::sparse_attention_rows",
                                                          "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(
        "torch_sputnik::sparse_attention_rows", "CPU")
