"""GPU: attention patterns built straight to CSR on the device (csrc/topology.hip,
ops.attention_pattern_csr, topology.AttentionPattern.build) against the torch path of the same
rule on the CPU -- held to a plain-Python double loop in tests/test_attention_pattern_cpu.py --,
bit for bit in row_indices, row_offsets and column_indices; the generator contract of the random
blocks; that no dense image is allocated; and SparseAttention(pattern=...) against dense float64
masked-softmax attention under pattern.dense_mask."""
import math

import numpy as np
import pytest
import torch

from helpers import rel_err, rel_err_torch
from tests import attention_pattern_cases as C
from torch_sputnik_amd import SparseAttention, capi, ops, topology
from torch_sputnik_amd.topology import AttentionPattern

pytestmark = pytest.mark.gpu

TOL = 1e-4     # the module's bound in tests/test_gpu_callers.py (5 * TOL for gradients)
NAMES = ("row_indices", "row_offsets", "column_indices")


def state_on(device):
    return torch.tensor(C.RNG_STATE, dtype=torch.int64, device=device)


def assert_device_equals_torch(arguments, m, n, offset):
    pattern = AttentionPattern(**arguments)
    assert capi.attention_pattern_launch_shape(m, n, offset)["served"]
    got = pattern.build(m, n, offset=offset, device="cuda", rng_state=state_on("cuda"), return_rng_state=True)
    want = pattern.build(m, n, offset=offset, device="cpu", rng_state=state_on("cpu"))
    what = f"{arguments} at {m} x {n}, offset {offset}"
    for name, a, b in zip(NAMES, got, want):
        assert a.is_cuda and a.dtype == torch.int32 and a.shape == b.shape, f"{name} of {what}"
        assert torch.equal(a.cpu(), b), f"{name} of {what}"
    assert tuple(got[1].shape) == (m + 1,) and int(got[1][m]) == got[2].numel()   # the buffers, whole
    if pattern.random:
        assert got[3].tolist() == list(C.RNG_STATE)
    else:
        assert got[3] is None
    return got


@pytest.mark.parametrize("n", C.WIDTHS)
def test_device_equals_torch_path(n):
    """every rule at every (m, offset) of this width: each component alone and all together,
    dilation 1 and 3, flags at {0, n - 1} and as a count, random blocks of 1, 4 and 64"""
    for m in C.ROWS:
        if m == n:
            continue
        for offset in C.offsets(m, n):
            for arguments in C.rules(n).values():
                assert_device_equals_torch(arguments, m, n, offset)


def test_square_and_empty_shapes():
    for arguments in C.rules(128).values():
        assert_device_equals_torch(arguments, 128, 128, 0)
    for m, n in ((0, 17), (17, 0), (0, 0)):
        got = assert_device_equals_torch(dict(window=2, global_tokens=min(n, 1)), m, n, 0)
        assert got[2].numel() == 0
        assert_device_equals_torch(dict(random_blocks=(4, 0.5)), m, n, 0)


def test_counted_example():
    """(203, 300, offset -5, window (7, 0), causal): 5 empty rows and 1556 entries"""
    row_indices, row_offsets, column_indices, _ = assert_device_equals_torch(
        dict(window=(7, 0), causal=True), 203, 300, -5)
    lengths = row_offsets[1:] - row_offsets[:-1]
    assert int((lengths == 0).sum()) == 5 and column_indices.numel() == 1556


def test_global_row_is_a_full_row():
    m, n = 129, 300
    row_indices, row_offsets, column_indices, _ = assert_device_equals_torch(
        dict(window=1, global_tokens=[70]), m, n, 0)
    lengths = (row_offsets[1:] - row_offsets[:-1]).tolist()
    assert lengths[70] == n and int(row_indices[-1]) == 70
    begin = int(row_offsets[70])
    assert column_indices[begin:begin + n].tolist() == list(range(n))
    # (column 70 joins the windows that do not hold it already)
    assert lengths[0] == 3 and lengths[1] == 4 and lengths[68] == 4 and lengths[69] == 3 and lengths[71] == 3
    # the causal form of the same row stops at its position
    _, causal_offsets, _, _ = assert_device_equals_torch(dict(window=1, global_tokens=[70], causal=True), m, n, 0)
    assert int(causal_offsets[71] - causal_offsets[70]) == 71


def test_wide_products_are_clamped():
    """window * dilation, block, stride and rb far beyond the matrix: the host clamps them"""
    big = 2 ** 40
    for arguments in (dict(window=(big, 3), dilation=1), dict(window=(2, 5), dilation=big), dict(block=big),
                      dict(summary=(big, big - 7)), dict(summary=(big, 1)), dict(random_blocks=(big, 0.5)),
                      dict(window=(big, big), dilation=7, causal=True)):
        assert_device_equals_torch(arguments, 129, 65, -5)


def test_generator_contract():
    """without rng_state: torch.manual_seed makes two builds equal, the second build of a run
    differs, the returned state reproduces the build on the CPU path, and 4 of the generator
    are consumed -- none without random blocks"""
    pattern = AttentionPattern(window=2, random_blocks=(4, 0.25))
    generator = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(11)
    before = generator.get_offset()
    first = pattern.build(127, 300, device="cuda", return_rng_state=True)
    assert generator.get_offset() == before + 4
    second = pattern.build(127, 300, device="cuda", return_rng_state=True)
    torch.manual_seed(11)
    again = pattern.build(127, 300, device="cuda", return_rng_state=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[2], second[2]) and int(second[3][1]) == int(first[3][1]) + 4
    assert int(first[3][0]) == 11 and int(first[3][1]) % 4 == 0
    replay = pattern.build(127, 300, device="cpu", rng_state=first[3].cpu())
    for name, a, b in zip(NAMES, first, replay):
        assert torch.equal(a.cpu(), b), name
    # the torch path on the GPU draws as the device path does
    torch.manual_seed(11)
    topology.enable_device_build(False)
    try:
        fallback = pattern.build(127, 300, device="cuda", return_rng_state=True)
    finally:
        topology.enable_device_build(True)
    assert all(torch.equal(a, b) for a, b in zip(first, fallback))
    offset = generator.get_offset()
    row_indices, row_offsets, column_indices, state = ops.attention_pattern_csr(127, 300, window=2, device="cuda")
    assert state is None and generator.get_offset() == offset


def test_ops_contract_on_the_device():
    with pytest.raises(ValueError, match="attention_pattern_csr.*global_tokens"):
        ops.attention_pattern_csr(8, 8, global_tokens=[8], device="cuda")
    with pytest.raises(ValueError, match="attention_pattern_csr.*rng_state"):
        ops.attention_pattern_csr(8, 8, random_blocks=(2, 0.5), device="cuda", rng_state=torch.zeros(3))
    with pytest.raises(RuntimeError, match="beyond what the kernels serve"):
        ops.attention_pattern_csr(16385, 8, window=1, device="cuda")
    with pytest.raises(RuntimeError, match="beyond what the kernels serve"):
        ops.attention_pattern_csr(8, 8, offset=2 ** 30, window=1, device="cuda")
    # ... which AttentionPattern.build serves in torch, on the GPU
    row_indices, row_offsets, column_indices = AttentionPattern(window=1).build(8, 8, offset=2 ** 30, device="cuda")
    assert row_offsets.is_cuda and column_indices.numel() == 0


def test_no_dense_image():
    """2048 x 2048, window (64, 64): the outputs are 1 056 516 bytes; one bool image alone is
    4 194 304"""
    size = 2048
    pattern = AttentionPattern(window=(64, 64))
    pattern.build(size, device="cuda")                           # (warm-up)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    row_indices, row_offsets, column_indices = pattern.build(size, device="cuda")
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - before
    outputs = sum(t.numel() * t.element_size() for t in (row_indices, row_offsets, column_indices))
    print(f"peak over build: {raised} bytes; outputs {outputs} bytes; one bool image {size * size} bytes")
    assert outputs == 1056516
    assert raised < size * size


# ---- the module ----
def scatter_dense(layer):
    rows = torch.repeat_interleave(torch.arange(layer.output_features, device=layer.row_offsets.device),
                                   (layer.row_offsets[1:] - layer.row_offsets[:-1]).long())
    w = torch.zeros(layer.output_features, layer.input_features, dtype=torch.float64, device=layer.values.device)
    w[rows, layer.column_indices.long()] = layer.values.detach().double()
    return w, rows


def build_module(pattern, **flags):
    heads, embed, seq = 2, 128, 128
    module = SparseAttention(heads, embed, max_sequence_length=seq, device=torch.device("cuda"), pattern=pattern,
                             **flags).cuda()
    rng = np.random.default_rng(5)
    for layer in module.linears:
        w = rng.uniform(-1, 1, (embed, embed)) / math.sqrt(embed * 0.3)
        w = w * (rng.random((embed, embed)) < 0.3)
        with torch.no_grad():
            layer.weight.copy_(torch.from_numpy(w.astype(np.float32)).cuda())
        layer.setup_sparse_tensors()
    return module


def dense_module(module, mask, q, k, v, weights):
    """the module densely in float64: masked-weight projections, masked softmax under `mask`
    (a row without an entry gives zeros), context, output projection"""
    heads, dim = module.num_heads, module.head_dim
    batch, seq, embed = q.shape

    def project(x, w):
        return torch.matmul(x, w.t()).view(batch, seq, heads, dim).transpose(1, 2)

    pq, pk, pv = (project(x, w) for x, w in zip((q, k, v), weights))
    scores = torch.matmul(pq, pk.transpose(-1, -2)) / math.sqrt(dim)
    scores = scores.masked_fill(~mask.to(scores.device), float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1))
    context = torch.matmul(probs, pv).transpose(1, 2).reshape(batch, seq, embed)
    return torch.matmul(context, weights[3].t())


def inputs(batch, seq, embed, seed, grad):
    rng = np.random.default_rng(seed)
    return tuple(torch.from_numpy(rng.uniform(-1, 1, (batch, seq, embed)).astype(np.float32)).cuda()
                 .requires_grad_(grad) for _ in range(4))


PATTERN = dict(window=(16, 0), global_tokens=4, causal=True)


@pytest.mark.parametrize("flags", [dict(), dict(fused_backward=True)], ids=["default", "fused_backward"])
def test_module_forward_vs_dense(flags):
    pattern = AttentionPattern(**PATTERN)
    module = build_module(pattern, **flags)
    assert module.mask2d is None and module.pattern is pattern and module.pattern_rng_state is None
    want_topology = pattern.build(128, device="cpu")
    for got, want in zip((module.row_indices, module.row_offsets, module.column_indices), want_topology):
        assert got.is_cuda and torch.equal(got.cpu(), want)
    q, k, v, _ = inputs(2, 128, 128, 7, False)
    weights = [scatter_dense(layer)[0] for layer in module.linears]
    want = dense_module(module, pattern.dense_mask(128), q.double(), k.double(), v.double(), weights)
    with torch.no_grad():
        fused = module(q, k, v)
    err = rel_err_torch(fused, want)
    print(f"forward (fused inference): {err:.3e}")
    assert err < TOL
    module.fused_inference = False
    with torch.no_grad():
        composed = module(q, k, v)
    err = rel_err_torch(composed, want)
    print(f"forward (separate operators): {err:.3e}")
    assert err < TOL

    # set_pattern: the output follows the second pattern
    second = AttentionPattern(block=32, window=(4, 4), random_blocks=(8, 0.2))
    old = module.row_offsets
    module.fused_inference = True
    module.set_pattern(second, rng_state=state_on("cuda"))
    assert module.pattern is second and module.pattern_rng_state.tolist() == list(C.RNG_STATE)
    assert module.row_offsets is not old
    mask = second.dense_mask(128, rng_state=state_on("cpu"))
    assert not torch.equal(mask, pattern.dense_mask(128))
    assert int(module.row_offsets[-1]) == int(mask.sum())
    want_second = dense_module(module, mask, q.double(), k.double(), v.double(), weights)
    with torch.no_grad():
        swapped = module(q, k, v)
    err, stale = rel_err_torch(swapped, want_second), rel_err_torch(swapped, want)
    print(f"after set_pattern: {err:.3e} against the second pattern, {stale:.3e} against the first")
    assert err < TOL and stale > 100 * TOL


@pytest.mark.parametrize("flags", [dict(), dict(differentiable_softmax=True), dict(fused_backward=True)],
                         ids=["default", "differentiable_softmax", "fused_backward"])
def test_module_backward_vs_dense(flags):
    """forward + backward: gradients of the inputs and of every projection's values against
    dense float64 autograd.  Under the default flags the module calls the raw softmax op as the
    reference does, which cuts the gradient to Q and K (tests/test_gpu_callers.py): there the
    gradients that do not pass through the softmax -- v, and the values of the value and output
    projections -- are held to the bound; `differentiable_softmax` (how that file trains the
    module) and `fused_backward` give every gradient."""
    through_softmax = bool(flags)
    pattern = AttentionPattern(**PATTERN)
    module = build_module(pattern, **flags)
    q, k, v, go = inputs(2, 128, 128, 8, True)
    out = module(q, k, v)
    out.backward(go.detach())
    leaves = []
    for layer in module.linears:
        w, rows = scatter_dense(layer)
        leaves.append((w.requires_grad_(True), rows, layer))
    qd, kd, vd = (x.detach().double().requires_grad_(True) for x in (q, k, v))
    want = dense_module(module, pattern.dense_mask(128), qd, kd, vd, [leaf[0] for leaf in leaves])
    want.backward(go.detach().double())
    err = rel_err_torch(out.detach(), want.detach())
    print(f"forward under autograd: {err:.3e}")
    assert err < TOL
    for name, got, ref in (("q", q, qd), ("k", k, kd), ("v", v, vd)) if through_softmax else (("v", v, vd),):
        err = rel_err_torch(got.grad, ref.grad)
        print(f"grad {name}: {err:.3e}")
        assert err < 5 * TOL
    for i, (w, rows, layer) in enumerate(leaves):
        if i < 2 and not through_softmax:
            continue
        err = rel_err(layer.values.grad.cpu().numpy(), w.grad[rows, layer.column_indices.long()].cpu().numpy(),
                      layer.row_offsets.cpu().numpy())
        print(f"grad values[{i}]: {err:.3e}")
        assert err < 5 * TOL
