"""The fused attention forward on the matrix cores (ops.sparse_attention_tiles, the C ABI's
sputnik_hip_sparse_attention_tiles_*) against float64 computed on the same half inputs, at the
smallest shapes that reach the kernel's edges, and the flag that routes
functional.sparse_attention_heads and SparseAttention(half_storage=True) through it.

Bound on `out`, elementwise, with u = 2^-11 (float16) / 2^-8 (bfloat16) and P the float64 softmax:
    |out - want| <= 2 u (P @ |v|) + 1e-4 max|want| + (u |want| if out is stored as the half type)
-- the one rounding of the weights (times 2 for the normalisation), the float32 slack the half
attention tests allow, the output rounding."""
import functools

import numpy as np
import pytest
import torch

from helpers import make_csr

gpu = pytest.mark.gpu
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
HALF = [torch.float16, torch.bfloat16]
D = 64


@pytest.fixture(scope="module")
def tsa():
    import torch_sputnik_amd
    from torch_sputnik_amd import functional, ops, topology  # noqa: F401  (attributes of the package)
    return torch_sputnik_amd


def dev():
    return torch.device("cuda:0")


def dense_mask(m, n, row_offsets, column_indices):
    mask = torch.zeros(m, n, dtype=torch.bool, device=dev())
    counts = (row_offsets[1:] - row_offsets[:-1]).long()
    mask[torch.repeat_interleave(torch.arange(m, device=dev()), counts), column_indices.long()] = True
    return mask


@functools.lru_cache(maxsize=None)
def topology(case):
    """-> (m, n, [row_indices, row_offsets, column_indices] on the GPU, dense mask)."""
    if case == "pattern":   # row blocks reach tile 0 and the diagonal tiles, nothing between
        from torch_sputnik_amd.topology import AttentionPattern
        m = n = 328
        topo = list(AttentionPattern(window=(40, 0), global_tokens=3, causal=True).build(m, device=dev()))
        return m, n, topo, dense_mask(m, n, topo[1], topo[2])
    if case == "random":    # partial last row block and key tile, five tiles, empty rows
        m, n = 200, 300
        _, _, ri, ro, ci = make_csr(m, n, 0.85, seed=m + n, empty_rows=(0, 17, m - 1), order="ascending")
    else:                   # "holes": an empty row block, an unoccupied tile column, shuffled rows
        m, n = 384, 256
        _, _, ri, ro, ci = make_csr(m, n, 0.85, seed=7, empty_rows=range(128, 256), order="ascending")
        rows = np.repeat(np.arange(m), np.diff(ro))
        keep = (ci < 64) | (ci >= 128)
        ci = ci[keep]
        ro = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32)
        rng = np.random.default_rng(3)
        for r in range(0, m, 5):
            ci[ro[r]:ro[r + 1]] = rng.permutation(ci[ro[r]:ro[r + 1]])
    topo = [torch.from_numpy(np.ascontiguousarray(x)).to(dev()) for x in (ri, ro, ci)]
    return m, n, topo, dense_mask(m, n, topo[1], topo[2])


@functools.lru_cache(maxsize=None)
def problem(case, dtype, scale, amplitude, two_d=False):
    """Operands (head views of [B, S, E] tensors, or [S, 64]) and the float64 reference."""
    m, n, topo, mask = topology(case)
    g = torch.Generator(device="cpu").manual_seed(m + n)
    rnd = lambda s: torch.empty(s, D) if two_d else torch.empty(2, s, 3 * D)
    q, k, v = (rnd(s).uniform_(-amplitude, amplitude, generator=g).to(dtype).to(dev()) for s in (m, n, n))
    if not two_d:
        from torch_sputnik_amd.functional import _heads
        q, k, v = (_heads(t, 3) for t in (q, k, v))
    scores = (torch.matmul(q.double(), k.double().transpose(-1, -2)) * scale).masked_fill(~mask, float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1))
    return (q, k, v), topo, mask, (torch.matmul(probs, v.double()), torch.logsumexp(scores, dim=-1),
                                   torch.matmul(probs, v.double().abs()))


def check(out, lse, reference, mask, dtype, out_dtype):
    want, want_lse, weight_of_v = reference
    assert out.dtype == out_dtype and out.shape == want.shape
    assert not torch.isnan(out).any()
    bound = 2 * U[dtype] * weight_of_v + 1e-4 * want.abs().max()
    if out_dtype != torch.float32:
        bound = bound + U[dtype] * want.abs()
    excess = ((out.double() - want).abs() - bound).max()
    print(f"worst |out - want| - bound: {float(excess):.3e}")
    assert excess <= 0
    empty = ~mask.any(dim=-1)
    assert not out[..., empty, :].any()                     # exactly zero
    if lse is None:
        return
    assert not torch.isnan(lse).any()
    assert torch.equal(torch.isneginf(lse), empty.expand_as(lse))
    err = (lse.double() - want_lse)[..., ~empty].abs().max()
    print(f"worst |lse - want|: {float(err):.3e}")
    assert err < 1e-4 * (1 + want_lse[..., ~empty].abs().max())


CASES = [("random", 0.125, 1.0, False),   # 1. tails everywhere
         ("pattern", 0.125, 1.0, False),  # 2. skipped tiles, rows with no entry in a walked tile
         ("holes", 0.125, 1.0, False),    # 3. an empty row block, an unoccupied tile column
         ("random", 1.0, 2.0, False),     # 4. logits of several tens: maxima move from tile to tile
         ("random", 1.0, 2.0, True)]      #    ... and the [S, 64] operand form


@gpu
@pytest.mark.parametrize("dtype", HALF)
def test_tiles_kernel_vs_float64(tsa, dtype):
    """Every case with out stored as the operands' type and as float32 (one test per storage type:
    the cases share its operands and references); case 1 also through a plan made beforehand."""
    for case, scale, amplitude, two_d in CASES:
        (q, k, v), topo, mask, reference = problem(case, dtype, scale, amplitude, two_d)
        plans = [None]
        if (case, scale) == CASES[0][:2]:
            plans.append(tsa.ops.sparse_attention_tiles_plan(q.size(-2), k.size(-2), topo[1], topo[2]))
            again = tsa.ops.sparse_attention_tiles_plan(q.size(-2), k.size(-2), topo[1], topo[2])
            assert torch.equal(plans[1], again)
        for out_dtype in (dtype, torch.float32):
            outs = []
            for plan in plans:
                print(f"{case} scale {scale} 2-D {two_d} out {out_dtype} plan given {plan is not None}")
                out, lse = tsa.ops.sparse_attention_tiles(q, k, v, *topo, scale, out_dtype=out_dtype,
                                                          with_lse=True, plan=plan)
                check(out, lse, reference, mask, dtype, out_dtype)
                if not two_d:   # the context comes back as a view of [B, S, E]
                    assert out.transpose(1, 2).is_contiguous()
                outs.append(out)
            assert all(torch.equal(outs[0], other) for other in outs)   # the op's own plan is the same plan


@gpu
@pytest.mark.parametrize("dtype", HALF)
def test_functional_flag_forward_and_backward(tsa, dtype):
    """The forward through the tile kernel within its bound; the backward is the shared
    recomputing one and reads nothing the forward wrote, so the gradients of the two routes
    differ by less than one rounding of the storage type."""
    (q, k, v), topo, mask, reference = problem("random", dtype, 0.125, 1.0)
    merged = [t.transpose(1, 2).reshape(t.size(0), t.size(2), -1) for t in (q, k, v)]   # [B, S, E]
    grads = {}
    for flag in (True, False):
        x = [t.clone().requires_grad_(True) for t in merged]
        out = tsa.functional.sparse_attention_heads(*x, 3, *topo, 0.125, matrix_cores=flag)
        if flag:
            check(tsa.functional._heads(out.detach(), 3), None, reference, mask, dtype, dtype)
        out.backward(torch.ones_like(out) * torch.linspace(-1, 1, out.size(-1), device=out.device).to(dtype))
        grads[flag] = [t.grad for t in x]
    for on, off in zip(grads[True], grads[False]):
        assert on.dtype == dtype
        assert (on.double() - off.double()).abs().max() <= U[dtype] * off.double().abs().max()


@gpu
@pytest.mark.parametrize("dtype", HALF)
def test_module_flag(tsa, dtype):
    from test_gpu_half_attention import MODULE_TOL, build_attention, norm_rel
    heads, embed, seq, batch = 4, 256, 256, 2
    on = build_attention(tsa, dev(), heads, embed, seq, seed=11, half_storage=True, attention_matrix_cores=True)
    off = build_attention(tsa, dev(), heads, embed, seq, seed=11, half_storage=True)
    assert on.attention_matrix_cores is True and off.attention_matrix_cores is False
    g = torch.Generator(device="cpu").manual_seed(seq)
    x = torch.empty(batch, seq, embed).uniform_(-1, 1, generator=g).to(dev())
    with torch.no_grad():
        assert norm_rel(on(x.to(dtype), x.to(dtype), x.to(dtype)),
                        off(x.to(dtype), x.to(dtype), x.to(dtype))) < MODULE_TOL[dtype]
        # float32 inputs never reach the half-storage forward
        assert torch.equal(on(x, x, x), off(x, x, x))
    # attention dropout in training mode: the vector route with the flag as without it
    on.attention_dropout = off.attention_dropout = 0.25
    outs = []
    for module in (on, off):
        torch.manual_seed(5)
        with torch.no_grad():
            outs.append(module.train()(x.to(dtype), x.to(dtype), x.to(dtype)))
    assert torch.equal(*outs)


def test_flag_on_cpu_tensors_is_the_default_module(cpu_ops):
    torch.manual_seed(0)
    modules = [cpu_ops.SparseAttention(2, 8, max_sequence_length=12, device="cpu", sparsity=0.5,
                                       mask_generator=np.random.default_rng(1), half_storage=True,
                                       attention_matrix_cores=flag) for flag in (True, False)]
    for module in modules:
        for lin in module.linears:
            with torch.no_grad():
                lin.weight.copy_(torch.eye(8))
            lin.setup_sparse_tensors()
    q, k, v = (torch.randn(2, 12, 8) for _ in range(3))
    with torch.no_grad():
        assert torch.equal(modules[0](q, k, v, None), modules[1](q, k, v, None))
