"""The dense weight gradient of a sparse layer (RigL's grow scores) on the matrix cores:
the fused epilogue of the half layer's weight gradient (kSampledDense: the sampled entries
AND the whole float32 tile from one launch), the standalone op on either operand layout,
and the module flow (collect_dense_grad / dense_grad / rigl_update).

References are float64 einsums on the operands as stored (a half operand rounded, a
float32 operand with its full mantissa: it enters as half planes, not rounded); every
output is float32 and is held to the project's float32 bound, rel_err < 1e-4.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import make_csr, rel_err, rounded

pytestmark = pytest.mark.gpu

TOL = 1e-4
HALF_TYPES = [torch.float16, torch.bfloat16]
# (out, in, seq, batch, sparsity): one tile and one step; ragged in rows and columns
# (192 = 128 + 64, 320 = 2 x 128 + 64); very sparse, with a forced empty row
SHAPES = [(128, 64, 64, 1, 0.5), (192, 320, 192, 3, 0.8), (384, 256, 448, 2, 0.95)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=["tile_rows_128", "tile_rows_256"])
def mfma_tile(request, monkeypatch):
    """SPUTNIK_HIP_MFMA_TILE: the matrix-core kernels' tile has 128 rows (four waves, two LDS
    stages) or, where the output has 256 rows or more, 256 (eight waves, three stages)."""
    from torch_sputnik_amd import capi
    monkeypatch.setenv("SPUTNIK_HIP_MFMA_TILE", request.param.rsplit("_", 1)[1])
    capi.reload_options()
    yield request.param
    monkeypatch.delenv("SPUTNIK_HIP_MFMA_TILE", raising=False)
    capi.reload_options()


@pytest.fixture
def spmm_mfma(monkeypatch):
    """SPUTNIK_HIP_SPMM_KERNEL=mfma: the half layer takes the matrix-core route for every
    shape it serves -- small test shapes included."""
    from torch_sputnik_amd import capi
    monkeypatch.setenv("SPUTNIK_HIP_SPMM_KERNEL", "mfma")
    capi.reload_options()
    yield
    monkeypatch.delenv("SPUTNIK_HIP_SPMM_KERNEL", raising=False)
    capi.reload_options()


@pytest.fixture
def no_einsum(monkeypatch):
    """The served calls must run the kernel: the op's torch fallback is taken away."""
    def refuse(*args, **kwargs):
        raise AssertionError("dense_weight_grad fell back to torch.einsum on a served call")
    monkeypatch.setattr(torch, "einsum", refuse)


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def dense_ref(g, x, layout="bsi"):
    """float64 sum over (b, s) of dy[b, o, s] x[b, s, i]."""
    return np.einsum("bos,bsi->oi" if layout == "bsi" else "bos,bis->oi",
                     np.asarray(g, np.float64), np.asarray(x, np.float64), optimize=True)


@functools.lru_cache(maxsize=None)
def _raw_operands(out_f, in_f, seq, batch):
    """float32 dy [B, out, S] (rows over two decades of magnitude) and x [B, S, in]: drawn
    once per shape, shared by the tests, never written to."""
    rng = np.random.default_rng(out_f + in_f + seq)
    g = (rng.uniform(-1, 1, size=(batch, out_f, seq)) *
         10.0 ** rng.uniform(-2, 0, size=(batch, out_f, 1))).astype(np.float32)
    x = rng.uniform(-1, 1, size=(batch, seq, in_f)).astype(np.float32)
    g.setflags(write=False)
    x.setflags(write=False)
    return g, x


def _operand(x, kind, tile, dev):
    """(device tensor, the values it holds as float32 numpy)."""
    if kind == "half":
        return rounded(x, tile, dev)
    return T(x, dev), np.asarray(x, np.float32)


# ----------------------------------------------------------------------------
# the fused op: grad_values and the dense image from one launch
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("tile", HALF_TYPES)
@pytest.mark.parametrize("grad_kind", ["half", "float"])
@pytest.mark.parametrize("out_f,in_f,seq,batch,sparsity", SHAPES)
def test_fused_weight_gradient_dense(dev, tile, grad_kind, out_f, in_f, seq, batch, sparsity):
    from torch_sputnik_amd import ops
    _, _, _, ro, ci = make_csr(out_f, in_f, sparsity, seed=out_f + in_f + seq, round_to=1,
                               empty_rows=(out_f // 3,))
    g_raw, x_raw = _raw_operands(out_f, in_f, seq, batch)
    x, x32 = rounded(x_raw, tile, dev)
    g, g32 = _operand(g_raw, grad_kind, tile, dev)
    want = dense_ref(g32, x32)
    rows = np.repeat(np.arange(out_f), np.diff(ro))
    rod, cid = T(ro, dev), T(ci, dev)
    planes = grad_kind == "float"
    grad = ops.half_planes(g, tile) if planes else g
    at = (T(rows, dev).long(), cid.long())
    for plan in (None, ops.half_linear_plan(out_f, in_f, rod, cid)):
        dw, dense = ops.half_linear_weight_gradient_dense(out_f, rod, cid, grad, planes, x, plan)
        assert dense.dtype == torch.float32 and tuple(dense.shape) == (out_f, in_f)
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (len(ci),)
        assert rel_err(dense.cpu().numpy(), want) < TOL
        assert rel_err(dw.cpu().numpy()[None, :], want[rows, ci][None, :], ro) < TOL
        assert torch.equal(dw, dense[at])            # the same bits: both come from the tile in LDS


def _descending_row(ro, ci, row):
    """The pattern with `row`'s columns in descending order (a row whose columns do not
    ascend: the planned kernel must walk that tile row's entries flat)."""
    ci = ci.copy()
    ci[ro[row]:ro[row + 1]] = ci[ro[row]:ro[row + 1]][::-1]
    return ci


@pytest.mark.parametrize("pattern", ["ascending", "one_row_descending"])
def test_fused_exact_integers_inside_a_larger_buffer(mfma_tile, dev, pattern):
    """Small integers (every product and sum exact in float32): the image and the sampled
    entries must BE the integer matrices, at both tile heights, and the kernel must write
    the image's out * in floats and nothing around them."""
    from torch_sputnik_amd import capi, ops
    out_f, in_f, seq, batch = 320, 128, 384, 2     # (256-row tiles: one whole, one ragged)
    _, _, _, ro, ci = make_csr(out_f, in_f, 0.6, seed=23, round_to=1)
    if pattern == "one_row_descending":
        assert ro[142] - ro[141] > 1
        ci = _descending_row(ro, ci, 141)
    rng = np.random.default_rng(24)
    x32 = rng.integers(-4, 5, size=(batch, seq, in_f)).astype(np.float32)
    g32 = rng.integers(-4, 5, size=(batch, out_f, seq)).astype(np.float32)
    want = np.einsum("bos,bsi->oi", g32.astype(np.float64), x32.astype(np.float64), optimize=True)
    rows = np.repeat(np.arange(out_f), np.diff(ro))
    x, g = T(x32, dev).half(), T(g32, dev).half()
    rod, cid = T(ro, dev), T(ci, dev)
    guard = 256                                     # floats in front of and behind the image
    for plan in (None, ops.half_linear_plan(out_f, in_f, rod, cid)):
        buffer = torch.full((guard + out_f * in_f + guard,), 777.0, device=dev)
        image = buffer[guard:guard + out_f * in_f]
        dw = torch.full((len(ci),), float("nan"), device=dev)
        status = capi.lib().sputnik_hip_sparse_linear_half_weight_gradient_dense(
            out_f, in_f, seq, batch, len(ci), capi._ptr(rod), capi._ptr(cid), capi._ptr(g), 1, capi._ptr(x), 1,
            capi._ptr(dw), capi._ptr(plan), capi._ptr(image), in_f, capi._stream(x))
        assert status == 0
        got = buffer.cpu().numpy()
        assert np.array_equal(got[guard:-guard].reshape(out_f, in_f), want)
        assert np.array_equal(dw.cpu().numpy(), want[rows, ci])
        assert np.all(got[:guard] == 777.0) and np.all(got[-guard:] == 777.0)


def test_fused_argument_errors_return_before_a_launch(dev):
    from torch_sputnik_amd import capi
    out_f, in_f, seq, batch = 128, 64, 64, 1
    ro = torch.arange(0, out_f + 1, dtype=torch.int32, device=dev)
    ci = torch.zeros(out_f, dtype=torch.int32, device=dev)
    g = torch.zeros(batch, out_f, seq, dtype=torch.float16, device=dev)
    x = torch.zeros(batch, seq, in_f, dtype=torch.float16, device=dev)
    dw = torch.full((out_f,), 5.0, device=dev)
    image = torch.full((out_f * in_f + 4,), 5.0, device=dev)

    def call(image_t, ld, grad_type=1):
        return capi.lib().sputnik_hip_sparse_linear_half_weight_gradient_dense(
            out_f, in_f, seq, batch, out_f, capi._ptr(ro), capi._ptr(ci), capi._ptr(g), grad_type, capi._ptr(x),
            1, capi._ptr(dw), None, capi._ptr(image_t), ld, capi._stream(x))
    assert call(image[1:], in_f) != 0          # image not 16-byte aligned
    assert call(image, in_f + 2) != 0          # row stride not a multiple of 4
    assert call(image, in_f - 4) != 0          # rows would overlap
    assert call(image, in_f, grad_type=2) != 0  # dy neither float32 planes nor the tile type
    assert call(None, in_f) != 0
    torch.cuda.synchronize()
    assert bool((image == 5.0).all()) and bool((dw == 5.0).all())


# ----------------------------------------------------------------------------
# the standalone op
# ----------------------------------------------------------------------------
def _pairs():
    cases = []
    for tile in HALF_TYPES:
        for kinds in (("half", "half"), ("float", "half"), ("half", "float")):
            cases.append(pytest.param(tile, *kinds, id=f"{str(tile).split('.')[1]}-{kinds[0]}-{kinds[1]}"))
    # two float32 operands arrive as float16 2 x 2 planes
    cases.append(pytest.param(torch.float16, "float", "float", id="float-float"))
    return cases


@pytest.mark.parametrize("layout", ["bsi", "bis"])
@pytest.mark.parametrize("tile,grad_kind,x_kind", _pairs())
@pytest.mark.parametrize("out_f,in_f,seq,batch,sparsity", SHAPES)
def test_dense_weight_grad_op(no_einsum, dev, layout, tile, grad_kind, x_kind, out_f, in_f, seq, batch, sparsity):
    from torch_sputnik_amd import ops
    g_raw, x_raw = _raw_operands(out_f, in_f, seq, batch)
    if layout == "bis":
        x_raw = np.ascontiguousarray(x_raw.transpose(0, 2, 1))
    g, g32 = _operand(g_raw, grad_kind, tile, dev)
    x, x32 = _operand(x_raw, x_kind, tile, dev)
    assert ops.dense_weight_grad_supported(out_f, in_f, seq, batch, g.dtype, x.dtype, layout, tile)
    dense = ops.dense_weight_grad(g, x, layout)
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (out_f, in_f)
    assert rel_err(dense.cpu().numpy(), dense_ref(g32, x32, layout)) < TOL


def test_dense_weight_grad_op_2d_operands(no_einsum, dev):
    from torch_sputnik_amd import ops
    g_raw, x_raw = _raw_operands(128, 64, 64, 1)
    g, g32 = rounded(g_raw[0], torch.float16, dev)
    x, x32 = rounded(x_raw[0], torch.float16, dev)
    dense = ops.dense_weight_grad(g, x)
    assert rel_err(dense.cpu().numpy(), dense_ref(g32[None], x32[None])) < TOL


@pytest.mark.parametrize("case", ["seq_off_the_step", "in_off_the_chunk", "two_half_types", "bf16_two_float32",
                                  "float64"])
def test_dense_weight_grad_op_unserved_calls_equal_torch(dev, case):
    """What the kernel does not serve is torch's float32 einsum: same shape and dtype."""
    from torch_sputnik_amd import capi, ops
    out_f, in_f, seq, batch = 96, 64, 128, 2
    g_dtype = x_dtype = torch.float16
    if case == "seq_off_the_step":
        seq = 72
    elif case == "in_off_the_chunk":
        in_f = 60
    elif case == "two_half_types":
        x_dtype = torch.bfloat16
    elif case == "float64":
        g_dtype = torch.float64
    rng = np.random.default_rng(5)
    g = T(rng.uniform(-1, 1, size=(batch, out_f, seq)).astype(np.float32), dev).to(g_dtype)
    x = T(rng.uniform(-1, 1, size=(batch, seq, in_f)).astype(np.float32), dev).to(x_dtype)
    if case == "bf16_two_float32":   # (the op itself takes float16 tiles for two float32 operands)
        assert not capi.lib().sputnik_hip_sparse_linear_dense_weight_gradient_supported(
            out_f, in_f, seq, batch, 0, 0, 0, 2)
        return
    if case in ("seq_off_the_step", "in_off_the_chunk"):
        assert not ops.dense_weight_grad_supported(out_f, in_f, seq, batch, g_dtype, x_dtype, "bsi", torch.float16)
    dense = ops.dense_weight_grad(g, x)
    want = torch.einsum("bos,bsi->oi", g.float(), x.float())
    assert dense.dtype == want.dtype and dense.shape == want.shape
    assert torch.equal(dense, want)
    assert rel_err(dense.cpu().numpy(), dense_ref(g.double().cpu().numpy(), x.double().cpu().numpy())) < TOL


# ----------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------
def _layer(dev, out_f, in_f, density, seed, dtype=torch.float32, per_row=False):
    from torch_sputnik_amd import SparseLinear
    gen = torch.Generator().manual_seed(seed)
    weight = torch.randn(out_f, in_f, generator=gen).to(dev).to(dtype)
    return SparseLinear.from_dense(weight, density=density, per_row=per_row)


@pytest.mark.parametrize("route", ["tiles", "typed_operators"])
@pytest.mark.parametrize("tile", HALF_TYPES)
def test_module_half_activations(request, dev, tile, route):
    from torch_sputnik_amd import ops
    if route == "tiles":
        request.getfixturevalue("spmm_mfma")
    out_f, in_f, seq, batch = 256, 128, 128, 2
    layer = _layer(dev, out_f, in_f, 0.2, seed=1)
    assert ops.half_linear_supported(out_f, in_f, seq, batch, layer.values.numel(), torch.float32, tile) == \
        (route == "tiles")
    g_raw, x_raw = _raw_operands(out_f, in_f, seq, batch)
    x, x32 = rounded(x_raw, tile, dev)
    upstream = T(g_raw, dev)
    want = dense_ref(g_raw, x32)

    def backward():
        layer.values.grad = None
        layer(x).backward(upstream)
        return layer.values.grad.clone()

    disarmed = backward()
    assert layer.dense_grad is None
    assert layer.collect_dense_grad() is layer
    armed = backward()
    assert rel_err(armed.cpu().numpy()[None, :], disarmed.double().cpu().numpy()[None, :],
                   layer.row_offsets.cpu().numpy()) < TOL
    first = layer.dense_grad
    assert first.dtype == torch.float32 and tuple(first.shape) == (out_f, in_f)
    assert rel_err(first.cpu().numpy(), want) < TOL
    assert "dense_grad" not in layer.state_dict() and "dense_grad" not in dict(layer.named_buffers())
    backward()
    assert layer.dense_grad is first                                  # accumulated in place
    assert rel_err(layer.dense_grad.cpu().numpy(), 2.0 * want) < TOL
    layer.zero_dense_grad()
    assert layer.dense_grad is None
    layer.collect_dense_grad(False)
    backward()
    assert layer.dense_grad is None


def test_module_half_activations_frozen_values(spmm_mfma, dev):
    """Nothing is sampled when the values need no gradient: the standalone launch."""
    out_f, in_f, seq, batch = 256, 128, 128, 2
    layer = _layer(dev, out_f, in_f, 0.2, seed=1).collect_dense_grad()
    layer.values.requires_grad_(False)
    g_raw, x_raw = _raw_operands(out_f, in_f, seq, batch)
    x, x32 = rounded(x_raw, torch.float16, dev)
    x.requires_grad_(True)
    layer(x).backward(T(g_raw, dev))
    assert rel_err(layer.dense_grad.cpu().numpy(), dense_ref(g_raw, x32)) < TOL


@pytest.mark.parametrize("through", ["forward", "project_split_rows", "twice_in_one_graph"])
def test_module_float32_activations(no_einsum, dev, through):
    out_f, in_f, seq, batch = 256, 128, 128, 2
    layer = _layer(dev, out_f, in_f, 0.2, seed=2).collect_dense_grad()
    g_raw, x_raw = _raw_operands(out_f, in_f, seq, batch)
    x, upstream = T(x_raw, dev), T(g_raw, dev)
    want = dense_ref(g_raw, x_raw)
    if through == "forward":
        layer(x).backward(upstream)
    elif through == "twice_in_one_graph":
        (layer(x) + layer(x)).backward(upstream)
        want = 2.0 * want
    else:
        d = 64
        y = layer.project(x.transpose(1, 2).contiguous(), split_rows=d)      # [B * out/d, S, d]
        assert tuple(y.shape) == (batch * out_f // d, seq, d)
        y.backward(upstream.reshape(batch * out_f // d, d, seq).transpose(1, 2).contiguous())
    assert layer.dense_grad.dtype == torch.float32
    assert rel_err(layer.dense_grad.cpu().numpy(), want) < TOL


@pytest.mark.parametrize("per_row", [True, False])
def test_rigl_update_is_update_topology_on_the_collected_gradient(dev, per_row):
    out_f, in_f, seq, batch = 256, 128, 128, 2
    twins = [_layer(dev, out_f, in_f, 0.2, seed=3, per_row=True).collect_dense_grad() for _ in range(2)]
    g_raw, x_raw = _raw_operands(out_f, in_f, seq, batch)
    x, upstream = T(x_raw, dev), T(g_raw, dev)
    with pytest.raises(RuntimeError):
        twins[0].rigl_update(0.3, per_row=per_row)                    # nothing collected yet
    for layer in twins:
        layer(x).backward(upstream)
    assert torch.equal(twins[0].dense_grad, twins[1].dense_grad)
    old = twins[0].column_indices.clone()
    source = twins[0].rigl_update(0.3, per_row=per_row)
    want_source = twins[1].update_topology(0.3, grow_scores=twins[1].dense_grad.clone(), per_row=per_row)
    assert torch.equal(source, want_source)
    for name in ("column_indices", "row_offsets"):
        assert torch.equal(getattr(twins[0], name), getattr(twins[1], name))
    assert torch.equal(twins[0].values.detach(), twins[1].values.detach())
    assert int((source < 0).sum()) > 0 and not torch.equal(old, twins[0].column_indices)
    assert twins[0].dense_grad is None                                # cleared, still armed
    twins[0](x).backward(upstream)
    assert rel_err(twins[0].dense_grad.cpu().numpy(), dense_ref(g_raw, x_raw)) < TOL
    assert twins[0].values.grad is not None and bool(torch.isfinite(twins[0].values.grad).all())
