"""The matrix-core attention forward at head dimension 128 against float64 on the same half inputs, with the
operands, topologies, bound and lse tolerance of test_gpu_attention_tiles.py (none depends on the head dimension)."""
import functools

import pytest
import torch

import test_gpu_attention_tiles as d64
from test_gpu_attention_tiles import HALF, U, check, gpu, tsa  # noqa: F401  (tsa: fixture)

SCALE = 128 ** -0.5
CASES = [("random", SCALE, 1.0, False),   # partial last row block and key tile, empty rows
         ("pattern", SCALE, 1.0, False),  # skipped tiles, rows with no entry in a walked tile
         ("holes", SCALE, 1.0, False),    # an empty row block, an unoccupied tile column, shuffled columns
         ("random", 0.7, 2.0, False),     # logits of several tens: the maximum moves between tiles
         ("random", SCALE, 1.0, True)]    # the [S, 128] operand form


@functools.lru_cache(maxsize=None)
def problem(*args):
    """d64.problem with D = 128 (it reads its module's D when it is called); cached here, not there."""
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(d64, "D", 128)
        return d64.problem.__wrapped__(*args)


@gpu
@pytest.mark.parametrize("dtype", HALF)
def test_tiles_kernel_and_functional_flag_d128(tsa, dtype):
    """The kernel with out as the operands' type and as float32, with lse, the first case also through a plan
    made beforehand; then the functional flag.  (One test per storage type: they share operands and references.)"""
    for case in CASES:
        (q, k, v), topo, mask, reference = problem(case[0], dtype, *case[1:])
        assert q.size(-1) == 128
        plans = [None, tsa.ops.sparse_attention_tiles_plan(q.size(-2), k.size(-2), topo[1], topo[2])]
        for out_dtype in (dtype, torch.float32):
            outs = [tsa.ops.sparse_attention_tiles(q, k, v, *topo, case[1], out_dtype=out_dtype, with_lse=True,
                                                   plan=plan) for plan in plans[:2 if case == CASES[0] else 1]]
            for out, lse in outs:
                check(out, lse, reference, mask, dtype, out_dtype)
            assert all(torch.equal(outs[0][0], out) for out, _ in outs)   # the op's own plan is the same plan

    # functional.sparse_attention_heads(matrix_cores=True): the forward within the bound; the backward is the
    # shared recomputing one, so the gradients of the two routes are within one rounding of the largest
    (q, k, v), topo, mask, reference = problem("random", dtype, SCALE, 1.0)
    merged = [t.transpose(1, 2).reshape(t.size(0), t.size(2), -1) for t in (q, k, v)]   # [2, S, 384]
    grads = {}
    for flag in (True, False):
        x = [t.clone().requires_grad_(True) for t in merged]
        out = tsa.functional.sparse_attention_heads(*x, 3, *topo, SCALE, matrix_cores=flag)
        if flag:
            check(tsa.functional._heads(out.detach(), 3), None, reference, mask, dtype, dtype)
        out.backward(torch.ones_like(out) * torch.linspace(-1, 1, out.size(-1), device=out.device).to(dtype))
        grads[flag] = [t.grad for t in x]
    for on, off in zip(grads[True], grads[False]):
        assert on.dtype == dtype and (on.double() - off.double()).abs().max() <= U[dtype] * off.double().abs().max()


def test_tiles_supported_on_the_host():
    """The tile route's own view check reads addresses and strides only: made-up aligned ones do."""
    from torch_sputnik_amd import capi

    def served(d, row=None, entry="tiles", q_row=None, m=200, n=300, heads=3):
        row = row or heads * d
        view = lambda base, rows, r: (base, rows * r, d, r)   # base, batch, head and row strides
        return getattr(capi.lib(), f"sputnik_hip_sparse_attention_{entry}_supported")(
            m, n, d, 1000, 2, heads, capi.TYPE_CODES[torch.float16], 0, *view(1 << 20, m, q_row or row),
            *view(2 << 20, n, row), *view(3 << 20, n, row), *view(4 << 20, m, row))

    assert served(128) == 1 and served(64) == 1 and served(96) == 0 and served(128, entry="heads") == 0
    assert served(128, row=3 * 128 + 4) == 0            # a row stride that is no multiple of 8 elements
    # q's extent ((m - 1) * row + d) * 2 bytes at m = 2: 2^32 - 16 is served, 2^32 is not
    assert served(128, q_row=(1 << 31) - 136, m=2) == 1 and served(128, q_row=(1 << 31) - 128, m=2) == 0
