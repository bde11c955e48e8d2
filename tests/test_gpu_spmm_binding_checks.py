"""GPU: the operand contract and the route ladder of the SpMM ops of the binding itself
(csrc/torch_binding.cpp), reached through ``torch.ops.torch_sputnik.*`` directly.  Every bad input
is a host-side rejection before any launch: a RuntimeError.  Every fallback of the ladder equals,
bit for bit, the composition it is documented to be -- the same kernels run either way.

Rejections use a 4 x 8 pattern with 6 entries (row lengths 2, 0, 3, 1).  Routes use a 128 x 32
pattern of density about 0.25 with 3 replicas: at n = 64 the panel kernel serves the permuted and
the transposed-store form (block_rows a multiple of 64), at n = 60 or block_rows = 32 it does not;
a group of 5 weights is more than the group kernel takes.

The binding accepts everything the list of bad inputs names as bad: nothing is asserted as accepted.

Float16 / bfloat16 operands of a transposed-store call that the fused store does not serve go to
the typed kernels as they are (not widened first): asserted bit for bit against ``spmm`` on the
same half operands, and against a float64 dense product within 1e-5 of |A| |B| per element (a
float32 accumulation of at most 32 products of exactly widened halves is within 32 * 2^-24 = 1.9e-6;
float32 values against bfloat16 entering as half planes add 2^-22 per product)."""
import pytest
import torch

from torch_sputnik_amd import capi

pytestmark = pytest.mark.gpu

T = torch.ops.torch_sputnik
M, K, NNZ, N = 4, 8, 6, 5
RM, RK, RN, REPLICAS = 128, 32, 64, 3
_BITS = {2: torch.int16, 4: torch.int32}


def rejects(op, *args, what):
    with pytest.raises(RuntimeError):
        op(*args)
        pytest.fail(f"accepted {what}")


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bits = _BITS[want.element_size()]
    assert torch.equal(got.contiguous().view(bits), want.contiguous().view(bits)), what


def row_order(row_offsets):
    """rows by ascending length, as the modules build row_indices"""
    return torch.argsort(row_offsets[1:] - row_offsets[:-1], stable=True).to(torch.int32)


@pytest.fixture(scope="module")
def small():
    """The 4 x 8 pattern with values, a permutation of its entries, a bias and dense operands."""
    gen = torch.Generator().manual_seed(11)
    row_offsets = torch.tensor([0, 2, 2, 5, 6], dtype=torch.int32)
    host = dict(
        values=torch.tensor([0.5, -2.0, 1.5, -0.25, 3.0, -1.0]),
        row_indices=row_order(row_offsets), row_offsets=row_offsets,
        column_indices=torch.tensor([1, 5, 0, 3, 7, 4], dtype=torch.int32),
        permutation=torch.tensor([4, 0, 5, 2, 1, 3], dtype=torch.int32),
        bias=torch.tensor([1.0, -1.0, 0.5, 2.0]),
        dense=torch.rand(K, N, generator=gen) * 2 - 1,
        dense3=torch.rand(2, K, N, generator=gen) * 2 - 1)
    return {name: t.cuda() for name, t in host.items()}


@pytest.fixture(scope="module")
def routes():
    """The 128 x 32 pattern: values [3, nnz] in [-1, 1], a permutation, dense [3, 32, 64]; 4 more
    weights of the same shape for the groups; and the pattern's dense form on the CPU."""
    gen = torch.Generator().manual_seed(2024)

    def pattern():
        mask = torch.rand(RM, RK, generator=gen) < 0.25
        mask[5] = False                                   # an empty row
        row_offsets = torch.cat([torch.zeros(1, dtype=torch.int64), mask.sum(1).cumsum(0)]).to(torch.int32)
        return mask, row_order(row_offsets), row_offsets, mask.nonzero()[:, 1].to(torch.int32)

    mask, row_indices, row_offsets, column_indices = pattern()
    nnz = column_indices.numel()
    host = dict(row_indices=row_indices, row_offsets=row_offsets, column_indices=column_indices,
                values=torch.rand(REPLICAS, nnz, generator=gen) * 2 - 1,
                permutation=torch.randperm(nnz, generator=gen).to(torch.int32),
                dense=torch.rand(REPLICAS, RK, RN, generator=gen) * 2 - 1)
    out = {name: t.cuda() for name, t in host.items()}
    out["mask"], out["nnz"] = mask, nnz
    out["group"] = []
    for _ in range(5):
        _, ri, ro, ci = pattern()
        out["group"].append(dict(values=(torch.rand(ci.numel(), generator=gen) * 2 - 1).cuda(),
                                 permutation=torch.randperm(ci.numel(), generator=gen).to(torch.int32).cuda(),
                                 topo=(ri.cuda(), ro.cuda(), ci.cuda()),
                                 dense=(torch.rand(REPLICAS, RK, RN, generator=gen) * 2 - 1).cuda()))
    return out


def topo_of(d):
    return d["row_indices"], d["row_offsets"], d["column_indices"]


def product_cases(small, left):
    """The bad inputs spmm (2-D dense) and left_spmm (3-D dense) share, as (values, row_indices,
    row_offsets, column_indices, dense)"""
    v, (ri, ro, ci) = small["values"], topo_of(small)
    d = small["dense3"] if left else small["dense"]
    yield (v, ri.cpu(), ro, ci, d), "row_indices on the CPU"
    yield (v, ri, ro.cpu(), ci, d), "row_offsets on the CPU"
    yield (v, ri, ro, ci.cpu(), d), "column_indices on the CPU"
    yield (v, ri.reshape(1, M), ro, ci, d), "2-D row_indices"
    yield (v, ri, ro.reshape(1, M + 1), ci, d), "2-D row_offsets"
    yield (v, ri, ro, ci.reshape(1, NNZ), d), "2-D column_indices"
    yield (v, ri, ro[:-1], ci, d), "row_offsets one short"
    yield (v[:-1], ri, ro, ci, d), "values one short"
    yield (v.double(), ri, ro, ci, d), "float64 values"
    yield (v, ri, ro, ci, d.reshape(-1)), "1-D dense"
    yield (v, ri, ro, ci, d.reshape((1, 1, K, N) if not left else (1, 2, K, N))), "4-D dense"
    yield (v, ri, ro, ci, d[..., :-1, :]), "inner dimension k - 1"


@pytest.mark.parametrize("left", [False, True], ids=["spmm", "left_spmm"])
def test_product_rejections(small, left):
    op = T.left_spmm if left else T.spmm
    for args, what in product_cases(small, left):
        rejects(op, M, K, *args, what=what)
    v, topo = small["values"], topo_of(small)
    if left:
        rejects(op, M, K, v.reshape(1, NNZ), *topo, small["dense3"], what="2-D values")
        assert op(M, K, v, *topo, small["dense3"][:1]).shape == (1, M, N)     # one replica stays 3-D
    else:
        rejects(op, M, K, v.reshape(1, NNZ), *topo, small["dense"], what="2-D values against 2-D dense")
        rejects(op, M, K, v.repeat(3, 1), *topo, small["dense3"], what="3 value rows against 2 dense replicas")
        assert op(M, K, v, *topo, small["dense"]).shape == (M, N)


def test_operands_on_two_devices(small):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device only")
    v, topo = small["values"], topo_of(small)
    rejects(T.spmm, M, K, v, *topo, small["dense"].to("cuda:1"), what="dense on another device")
    rejects(T.left_spmm, M, K, v, *topo, small["dense3"].to("cuda:1"), what="dense on another device")


def test_bias(small):
    v, topo, d, bias = small["values"], topo_of(small), small["dense"], small["bias"]
    for op in (T.spmm_bias, T.spmm_bias_relu):
        rejects(op, M, K, v, *topo, bias[:-1], d, what="bias of length m - 1")
        rejects(op, M, K, v, *topo, bias.reshape(M, 1), d, what="2-D bias")
        rejects(op, M, K, v, *topo, bias.cpu(), d, what="bias on the CPU")
    plain = T.spmm(M, K, v, *topo, d)
    same(T.spmm_bias(M, K, v, *topo, torch.zeros_like(bias), d), plain, "zero bias")
    for got, want in ((T.spmm_bias(M, K, v, *topo, bias, d), plain + bias[:, None]),
                      (T.spmm_bias_relu(M, K, v, *topo, bias, d), (plain + bias[:, None]).relu())):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def bad_permutations(perm):
    yield perm.long(), "int64 permutation"
    yield perm[:-1], "permutation one short"
    yield torch.stack([perm, perm], 1)[:, 0], "non-contiguous permutation"
    yield perm.cpu(), "permutation on the CPU"


def test_permutation_rejections(small):
    v, topo, d, d3, perm = small["values"], topo_of(small), small["dense"], small["dense3"], small["permutation"]
    for bad, what in bad_permutations(perm):
        rejects(T.spmm_permuted, M, K, v, bad, *topo, d, None, what=what)
        rejects(T.left_spmm_permuted, M, K, v, bad, *topo, d3, None, what=what)
        rejects(T.spmm_transposed_out, M, K, v, bad, *topo, d, 2, False, None, what=what)
        rejects(T.spmm_transposed_out, M, K, v, bad, *topo, d3, 2, True, None, what=what)
        rejects(T.left_spmm_group_sum, M, K, [v, v], [perm, bad], *[[t, t] for t in topo], [d3, d3], what=what)
    rejects(T.spmm_transposed_out, M, K, v, None, *topo, d, 0, False, None, what="block_rows 0")
    rejects(T.spmm_transposed_out, M, K, v, None, *topo, d, 3, False, None, what="block_rows 3 for m = 4")


def test_plan_rejections(routes):
    v, topo, d = routes["values"], topo_of(routes), routes["dense"]
    nnz = routes["nnz"]
    assert capi.spmm_workspace_bytes(RM, RK, RN, nnz) > 4 and capi.sddmm_workspace_bytes(RM, 64, RK, nnz) > 4
    lhs = torch.linspace(-1, 1, REPLICAS * RM * 64, device=d.device).reshape(REPLICAS, RM, 64)
    rhs = torch.linspace(1, -1, REPLICAS * RK * 64, device=d.device).reshape(REPLICAS, RK, 64)
    plan, sddmm_plan = T.spmm_plan(RM, RK, RN, *topo), T.sddmm_plan(RM, RK, 64, *topo)
    for make_bad, what in ((lambda p: p[:4].clone(), "plan of 4 bytes"), (lambda p: p.view(torch.int8), "int8 plan")):
        rejects(T.spmm_planned, RM, RK, v, *topo, d, make_bad(plan), what=what)
        rejects(T.left_spmm_planned, RM, RK, v[0].contiguous(), *topo, d, make_bad(plan), what=what)
        rejects(T.sddmm_planned, RM, RK, *topo, lhs, rhs, make_bad(sddmm_plan), what=what)
    same(T.spmm_planned(RM, RK, v, *topo, d, plan), T.spmm(RM, RK, v, *topo, d), "spmm_planned")
    same(T.left_spmm_planned(RM, RK, v[0].contiguous(), *topo, d, plan),
         T.left_spmm(RM, RK, v[0].contiguous(), *topo, d), "left_spmm_planned")
    same(T.sddmm_planned(RM, RK, *topo, lhs, rhs, sddmm_plan), T.sddmm(RM, RK, *topo, lhs, rhs), "sddmm_planned")


def test_group_rejections(small):
    v, (ri, ro, ci), d, d3, perm = small["values"], topo_of(small), small["dense"], small["dense3"], small["permutation"]
    rejects(T.left_spmm_group, M, K, [], [], [], [], d3, 0, what="empty lists")
    rejects(T.left_spmm_group_sum, M, K, [], [], [], [], [], [], what="empty lists")
    rejects(T.left_spmm_group, M, K, [v, v], [ri], [ro, ro], [ci, ci], d3, 0, what="lists of unequal length")
    rejects(T.left_spmm_group_sum, M, K, [v, v], [], [ri, ri], [ro], [ci, ci], [d3, d3], what="lists of unequal length")
    rejects(T.left_spmm_group_sum, M, K, [v, v], [perm], [ri, ri], [ro, ro], [ci, ci], [d3, d3],
            what="one permutation for two matrices")
    rejects(T.left_spmm_group_sum, M, K, [v, v], [], [ri, ri], [ro, ro], [ci, ci], [d3], what="one dense for two matrices")
    rejects(T.left_spmm_group, M, K, [v, v], [ri, ri], [ro, ro], [ci, ci], d, 0, what="2-D dense")
    rejects(T.left_spmm_group_sum, M, K, [v, v], [], [ri, ri], [ro, ro], [ci, ci], [d, d], what="2-D dense")
    rejects(T.left_spmm_group_sum, M, K, [v, v], [], [ri, ri], [ro, ro], [ci, ci], [d3, d3[:1]],
            what="dense operands of two shapes")
    rejects(T.left_spmm_group_sum, M, K, [v, v], [], [ri, ri], [ro, ro], [ci, ci], [d3, d3[..., :-1]],
            what="dense operands of two widths")


def blocks_transposed(product, block_rows):
    """[R, m, n] / [m, n] -> [R * m / block_rows, n, block_rows]: what spmm_transposed_out stores"""
    return T.transpose_last2(product.reshape(-1, block_rows, product.size(-1)))


def dense_product(routes, values, dense):
    """(A B in float64, |A| |B|) on the CPU from the operands widened exactly"""
    a = torch.zeros(values.size(0), RM, RK, dtype=torch.float64)
    a[:, routes["mask"]] = values.cpu().double()
    b = dense.cpu().double()
    return a @ b, a.abs() @ b.abs()


def close(got, want, scale, what):
    assert got.shape == want.shape, what
    assert bool(((got.cpu().double() - want).abs() <= 1e-5 * scale).all()), what


def test_the_shapes_branch_the_ladder_as_assumed(routes):
    lib, nnz = capi.lib(), routes["nnz"]
    assert lib.sputnik_hip_spmm_permuted_supported(RM, RK, RN, nnz) and not lib.sputnik_hip_spmm_permuted_supported(RM, RK, 60, nnz)
    assert lib.sputnik_hip_spmm_transposed_out_supported(RM, RK, RN, nnz, 64)
    assert lib.sputnik_hip_spmm_transposed_out_supported(RM, RK, RN, nnz, RM)
    assert not lib.sputnik_hip_spmm_transposed_out_supported(RM, RK, RN, nnz, 32)
    assert not lib.sputnik_hip_spmm_transposed_out_supported(RM, RK, 60, nnz, 64)
    assert lib.sputnik_hip_spmm_group_supported(RM, RK, RN, 3, 64, 0) and lib.sputnik_hip_spmm_group_supported(RM, RK, RN, 3, 0, 1)
    assert not lib.sputnik_hip_spmm_group_supported(RM, RK, RN, 5, 0, 0) and not lib.sputnik_hip_spmm_group_supported(RM, RK, RN, 5, 0, 1)


def test_fused_routes_against_float64(routes):
    v, topo, d, perm = routes["values"], topo_of(routes), routes["dense"], routes["permutation"]
    want, scale = dense_product(routes, v, d)
    close(T.spmm(RM, RK, v, *topo, d), want, scale, "spmm")
    close(T.spmm_permuted(RM, RK, v[:, torch.argsort(perm)].contiguous(), perm, *topo, d, None), want, scale, "spmm_permuted")
    for block_rows in (64, RM):
        stored = T.spmm_transposed_out(RM, RK, v, None, *topo, d, block_rows, False, None)
        assert stored.shape == (REPLICAS * RM // block_rows, RN, block_rows)
        close(stored, want.reshape(-1, block_rows, RN).transpose(1, 2), scale.reshape(-1, block_rows, RN).transpose(1, 2),
              f"spmm_transposed_out block_rows {block_rows}")
    inverse = v[:, torch.argsort(perm)].contiguous()
    stored = T.spmm_transposed_out(RM, RK, inverse, perm, *topo, d, 64, False, None)
    close(stored, want.reshape(-1, 64, RN).transpose(1, 2), scale.reshape(-1, 64, RN).transpose(1, 2),
          "spmm_transposed_out with a permutation")
    want0, scale0 = dense_product(routes, v[:1].expand(REPLICAS, -1), d)
    close(T.left_spmm(RM, RK, v[0].contiguous(), *topo, d), want0, scale0, "left_spmm")
    close(T.left_spmm_permuted(RM, RK, inverse[0].contiguous(), perm, *topo, d, None), want0, scale0, "left_spmm_permuted")


@pytest.mark.parametrize("left", [False, True], ids=["spmm", "left_spmm"])
def test_transposed_store_fallback_is_product_then_transpose(routes, left):
    topo, d, perm = topo_of(routes), routes["dense"], routes["permutation"]
    v = routes["values"][0].contiguous() if left else routes["values"]
    op, permuted = (T.left_spmm, T.left_spmm_permuted) if left else (T.spmm, T.spmm_permuted)
    plan = T.spmm_plan(RM, RK, RN, *topo)
    for dense, block_rows, what in ((d, 32, "block_rows 32"), (d[..., :60].contiguous(), 64, "n = 60")):
        product = op(RM, RK, v, *topo, dense)
        same(T.spmm_transposed_out(RM, RK, v, None, *topo, dense, block_rows, left, None),
             blocks_transposed(product, block_rows), what)
        same(T.spmm_transposed_out(RM, RK, v, perm, *topo, dense, block_rows, left, None),
             blocks_transposed(permuted(RM, RK, v, perm, *topo, dense, None), block_rows), what + ", permuted")
    same(T.spmm_transposed_out(RM, RK, v, None, *topo, d, 32, left, plan), blocks_transposed(op(RM, RK, v, *topo, d), 32),
         "block_rows 32, planned")
    if not left:        # 2-D operands: one replica
        same(T.spmm_transposed_out(RM, RK, v[0].contiguous(), None, *topo, d[0].contiguous(), 32, False, None),
             blocks_transposed(op(RM, RK, v[0].contiguous(), *topo, d[0].contiguous()), 32), "2-D operands")


def test_permuted_fallback_is_permute_then_product(routes):
    v, topo, perm = routes["values"], topo_of(routes), routes["permutation"]
    d60 = routes["dense"][..., :60].contiguous()
    same(T.spmm_permuted(RM, RK, v, perm, *topo, d60, None), T.spmm(RM, RK, T.permute_last(v, perm), *topo, d60), "spmm_permuted")
    v0 = v[0].contiguous()
    same(T.left_spmm_permuted(RM, RK, v0, perm, *topo, d60, None), T.left_spmm(RM, RK, T.permute_last(v0, perm), *topo, d60),
         "left_spmm_permuted")
    plan = T.spmm_plan(RM, RK, 60, *topo)
    same(T.spmm_permuted(RM, RK, v, perm, *topo, d60, plan), T.spmm(RM, RK, T.permute_last(v, perm), *topo, d60),
         "spmm_permuted, planned")


@pytest.mark.parametrize("values_dtype, dense_dtype", [(torch.float16, torch.float16), (torch.float32, torch.bfloat16),
                                                       (torch.bfloat16, torch.float32)])
def test_half_operands_of_an_unserved_transposed_store_stay_half(routes, values_dtype, dense_dtype):
    topo = topo_of(routes)
    v, d = routes["values"].to(values_dtype), routes["dense"].to(dense_dtype)
    want, scale = dense_product(routes, v.float(), d.float())
    for left in (False, True):
        values = v[0].contiguous() if left else v
        product = (T.left_spmm if left else T.spmm)(RM, RK, values, *topo, d)
        assert product.dtype == torch.float32
        same(T.spmm_transposed_out(RM, RK, values, None, *topo, d, 32, left, None), blocks_transposed(product, 32),
             f"left = {left}")
        if not left:
            close(product, want, scale, "the typed product against float64")


def test_a_half_mix_and_a_permutation_widen(routes):
    topo, perm = topo_of(routes), routes["permutation"]
    v, d = routes["values"].to(torch.float16), routes["dense"].to(torch.bfloat16)
    same(T.spmm(RM, RK, v, *topo, d), T.spmm(RM, RK, v.float(), *topo, d.float()), "float16 x bfloat16")
    h = routes["dense"].to(torch.float16)
    d60 = h[..., :60].contiguous()
    same(T.spmm_permuted(RM, RK, v, perm, *topo, d60, None),
         T.spmm(RM, RK, T.permute_last(v.float(), perm), *topo, d60.float()), "permuted half operands")
    same(T.spmm_transposed_out(RM, RK, v, perm, *topo, h, 32, False, None),
         blocks_transposed(T.spmm_permuted(RM, RK, v.float(), perm, *topo, h.float(), None), 32),
         "permuted half operands, transposed store")


def test_a_group_of_five_is_five_products(routes):
    group, d = routes["group"], routes["dense"]
    values, topos = [g["values"] for g in group], [g["topo"] for g in group]
    lists = [[t[i] for t in topos] for i in range(3)]
    singles = [T.left_spmm(RM, RK, v, *t, d) for v, t in zip(values, topos)]
    for got, want in zip(T.left_spmm_group(RM, RK, values, *lists, d, 0), singles):
        same(got, want, "left_spmm_group")
    for got, want in zip(T.left_spmm_group(RM, RK, values, *lists, d, 32), singles):
        same(got, blocks_transposed(want, 32), "left_spmm_group, block_rows 32")
    for got, v, t in zip(T.left_spmm_group(RM, RK, values, *lists, d, 64), values, topos):
        same(got, T.spmm_transposed_out(RM, RK, v, None, *t, d, 64, True, None), "left_spmm_group, block_rows 64")
    denses, perms = [g["dense"] for g in group], [g["permutation"] for g in group]
    total = None
    for v, t, dense in zip(values, topos, denses):
        part = T.left_spmm(RM, RK, v, *t, dense)
        total = part if total is None else total + part
    same(T.left_spmm_group_sum(RM, RK, values, [], *lists, denses), total, "left_spmm_group_sum")
    total = None
    for v, p, t, dense in zip(values, perms, topos, denses):
        part = T.left_spmm_permuted(RM, RK, v, p, *t, dense, None)
        total = part if total is None else total + part
    same(T.left_spmm_group_sum(RM, RK, values, perms, *lists, denses), total, "left_spmm_group_sum, permuted")


def test_a_group_the_kernel_takes_against_float64(routes):
    group, d = routes["group"][:3], routes["dense"]
    values, topos = [g["values"] for g in group], [g["topo"] for g in group]
    lists = [[t[i] for t in topos] for i in range(3)]
    singles = [T.left_spmm(RM, RK, v, *t, d).cpu().double() for v, t in zip(values, topos)]
    bound = 1e-5 * RK * float(d.abs().max())        # |A| |B| <= k max|B| for |values| <= 1
    for got, want in zip(T.left_spmm_group(RM, RK, values, *lists, d, 64), singles):
        assert bool(((got.cpu().double() - want.reshape(-1, 64, RN).transpose(1, 2)).abs() <= bound).all())
    denses = [g["dense"] for g in group]
    want = sum(T.left_spmm(RM, RK, v, *t, dense).cpu().double() for v, t, dense in zip(values, topos, denses))
    got = T.left_spmm_group_sum(RM, RK, values, [], *lists, denses)
    assert got.shape == (REPLICAS, RM, RN) and bool(((got.cpu().double() - want).abs() <= 3 * bound).all())
