"""The five operators of the reference's ``torch_sputnik`` module
(src/sputnik.cpp:36-42), same names, positional signatures and return types,
backed by ``torch.ops.torch_sputnik.*`` (HIP kernels for gfx950), followed by
the extensions whose call sites exist only in the reference's tests
(``spmm_bias``, the ``*_many_mask`` family) or not at all (softmax gradient).

GPU only: a CPU tensor raises from the dispatcher; there is no fallback.  (One documented
exception: ``dense_weight_grad``, which the module flow calls on layers of any size, computes
what its kernel does not serve with ``torch.einsum``.)
"""
import numbers

import torch

from ._native import load_ops

_ops = load_ops()


def spmm(m, k, values, row_indices, row_offsets, column_indices, dense_matrix):
    """Sparse (CSR) x dense.  src/spmm_cuda.cu:9-60.

    values [nnz] with dense [k,n] -> [m,n]; values [R,nnz] with dense [R,k,n]
    -> [R,m,n] (2-D when R == 1, as the reference does).
    """
    return _ops.spmm(int(m), int(k), values, row_indices, row_offsets, column_indices,
                     dense_matrix)


def left_spmm(m, k, values, row_indices, row_offsets, column_indices, dense_matrix):
    """One sparse matrix x R dense matrices -> always [R,m,n].
    src/left_replicated_spmm.cu:8-44."""
    return _ops.left_spmm(int(m), int(k), values, row_indices, row_offsets, column_indices,
                          dense_matrix)


def left_spmm_half_tiles(m, k, values, row_offsets, column_indices, dense_matrix, tile_dtype):
    """left_spmm as a dense contraction on the matrix cores (the half-storage extension,
    csrc/spmm_mfma.hip): the densified weight against dense [R, k, n] on tiles of
    ``tile_dtype`` (float16 / bfloat16); `values` and `dense_matrix` float32 or of that
    type -- a float32 operand enters as half planes over its range.  -> [R, m, n] float32,
    or None where the route does not serve the call (take left_spmm then)."""
    import torch
    code = {torch.float16: 1, torch.bfloat16: 2}[tile_dtype]
    out = _ops.left_spmm_half_tiles(int(m), int(k), values, row_offsets, column_indices,
                                    dense_matrix, code)
    return out if out.numel() else None


# ---- a sparse layer on half-stored activations: the three products on the matrix cores with
# no layout pass (csrc/sparse_linear_half.hip; include/sputnik_hip.h: sparse_linear_half_*) ----
_HALF_CODES = None


def _half_code(dtype):
    global _HALF_CODES
    if _HALF_CODES is None:
        import torch
        _HALF_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    return _HALF_CODES[dtype]


def half_linear_supported(out_features, in_features, seq, batch, nonzeros, values_dtype, tile_dtype):
    """Whether forward, weight gradient and input gradient of a sparse layer with these
    sizes take the matrix-core route (they share the weight's image and dy's planes)."""
    from . import capi
    try:
        vt, tt = _half_code(values_dtype), _half_code(tile_dtype)
    except KeyError:
        return False
    if tt == 0:
        return False
    return bool(capi.lib().sputnik_hip_sparse_linear_half_supported(
        int(out_features), int(in_features), int(seq), int(batch), int(nonzeros), vt, tt))


def half_linear_image(out_features, in_features, values, row_offsets, column_indices, tile_dtype):
    """The weight as a zeroed [planes, out, in] image of `tile_dtype` with the CSR values
    scattered in (float32 values: half planes whose sum is the value)."""
    return _ops.half_linear_image(int(out_features), int(in_features), values, row_offsets,
                                  column_indices, _half_code(tile_dtype))


def half_planes(t, tile_dtype):
    """A float32 tensor as half planes whose (scaled) sum is the value."""
    return _ops.half_planes(t, _half_code(tile_dtype))


def half_linear_forward(out_features, image, values_dtype, x):
    """y [batch, out, seq] float32 from x [batch, seq, in] (float16 / bfloat16), no layout pass."""
    return _ops.half_linear_forward(int(out_features), image, _half_code(values_dtype), x)


def half_linear_plan(out_features, in_features, row_offsets, column_indices):
    return _ops.half_linear_plan(int(out_features), int(in_features), row_offsets, column_indices)


def half_linear_weight_gradient(out_features, row_offsets, column_indices, grad, grad_is_planes, x,
                                plan=None):
    """dW [nnz] float32 = sum over the batch of dy x, sampled at the weight's mask; `grad` is
    dy [batch, out, seq] in x's type, or the planes of the float32 dy (`half_planes`)."""
    return _ops.half_linear_weight_gradient(int(out_features), row_offsets, column_indices, grad,
                                            bool(grad_is_planes), x, plan)


def half_linear_weight_gradient_dense(out_features, row_offsets, column_indices, grad, grad_is_planes, x,
                                      plan=None):
    """``half_linear_weight_gradient`` and, from the same launch, the DENSE weight gradient:
    -> ``(grad_values [nnz], dense [out, in])``, both float32.  The kernel has every float32
    tile of ``sum_b dy_b x_b`` in LDS to sample it at the mask; here it stores the tile as
    well, so ``grad_values`` equals ``dense[rows, columns]`` bit for bit.  One workgroup per
    tile (no splits, no scratch)."""
    return _ops.half_linear_weight_gradient_dense(int(out_features), row_offsets, column_indices, grad,
                                                  bool(grad_is_planes), x, plan)


_X_LAYOUTS = {"bsi": 0, "bis": 1}


def dense_weight_grad_supported(out_features, in_features, seq, batch, grad_dtype, x_dtype, x_layout,
                                tile_dtype):
    """Whether ``dense_weight_grad`` runs these sizes and operand types on the matrix cores
    (host only: sputnik_hip_sparse_linear_dense_weight_gradient_supported)."""
    from . import capi
    try:
        gt, xt, tt = _half_code(grad_dtype), _half_code(x_dtype), _half_code(tile_dtype)
    except KeyError:
        return False
    return bool(capi.lib().sputnik_hip_sparse_linear_dense_weight_gradient_supported(
        int(out_features), int(in_features), int(seq), int(batch), gt, xt, _X_LAYOUTS[x_layout], tt))


def dense_weight_grad(grad_output, x, x_layout="bsi"):
    """The dense weight gradient of a linear layer, ``[out, in]`` float32 =
    ``sum_b sum_s dy[b, o, s] x[b, s, i]`` -- RigL's grow scores -- from the operands as a
    layer has them: ``grad_output`` [B, out, S] and ``x`` [B, S, in] (``x_layout="bsi"``) or
    [B, in, S] (``"bis"``, the k-major operand of ``SparseLinear.project``); 2-D operands
    count as B = 1.  No transposed copy and no per-batch partial products: one tile launch on
    the matrix cores, float32 accumulation.  Operands are float16, bfloat16 or float32; a
    float32 operand is split into half planes whose sum is the value (``half_planes``), the
    tile type is the half operand's, float16 for two float32 operands.  No host
    synchronisation.

    Calls the kernel does not serve -- CPU tensors, two different half types, other dtypes,
    ``S % 64 != 0``, ``in % 8 != 0``, bfloat16 against two float32 planes... -- are computed
    by ``torch.einsum`` on float32 copies (same shape and dtype of the result)."""
    if x_layout not in _X_LAYOUTS:
        raise ValueError(f"dense_weight_grad: x_layout should be 'bsi' or 'bis', got {x_layout!r}")
    if grad_output.dim() == 2:
        grad_output = grad_output.unsqueeze(0)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if grad_output.dim() != 3 or x.dim() != 3:
        raise ValueError("dense_weight_grad: expected [B, out, S] and [B, S, in] / [B, in, S] operands")
    batch, out_f, seq = grad_output.shape
    in_f = x.size(2) if x_layout == "bsi" else x.size(1)
    if x.size(0) != batch or (x.size(1) if x_layout == "bsi" else x.size(2)) != seq:
        raise ValueError(f"dense_weight_grad: operands {tuple(grad_output.shape)} and {tuple(x.shape)} "
                         f"do not match in layout {x_layout!r}")
    halves = {t.dtype for t in (grad_output, x)} - {torch.float32}
    tile = next(iter(halves)) if len(halves) == 1 else torch.float16
    if len(halves) <= 1 and grad_output.is_cuda and x.is_cuda and grad_output.device == x.device and \
            dense_weight_grad_supported(out_f, in_f, seq, batch, grad_output.dtype, x.dtype, x_layout, tile):
        grad_output, x = grad_output.detach().contiguous(), x.detach().contiguous()
        g_planes, x_planes = grad_output.dtype == torch.float32, x.dtype == torch.float32
        if (grad_output.data_ptr() | x.data_ptr()) % 16 == 0:
            return _ops.dense_weight_gradient(
                half_planes(grad_output, tile) if g_planes else grad_output, g_planes,
                half_planes(x, tile) if x_planes else x, x_planes, _X_LAYOUTS[x_layout], _half_code(tile),
                out_f, in_f, seq, batch)
    return torch.einsum("bos,bsi->oi" if x_layout == "bsi" else "bos,bis->oi",
                        grad_output.detach().float(), x.detach().float())


def half_linear_input_gradient(out_features, in_features, grad, grad_is_planes, image, values_dtype,
                               like, batch, seq):
    """dx [batch, seq, in] in `like`'s type, or None where the route does not serve the call."""
    out = _ops.half_linear_input_gradient(int(out_features), int(in_features), grad, bool(grad_is_planes),
                                          image, _half_code(values_dtype), like, int(batch), int(seq))
    return out if out.numel() else None


# BASELINE.json names this op left_replicated_spmm; the binding exports left_spmm.
left_replicated_spmm = left_spmm


def sddmm(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix):
    """(lhs @ rhs^T) sampled at the CSR pattern -> [nnz] / [R,nnz].
    src/sddmm_cuda.cu:7-57."""
    return _ops.sddmm(int(m), int(n), row_indices, row_offsets, column_indices, lhs_matrix,
                      rhs_matrix)


def sddmm_narrow(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix):
    """sddmm whose result is stored in the operands' type: float16 / bfloat16 operands
    give float16 / bfloat16 scores (float32 sums, rounded once); float32 as sddmm."""
    return _ops.sddmm_narrow(int(m), int(n), row_indices, row_offsets, column_indices, lhs_matrix,
                             rhs_matrix)


def sparse_softmax(values, row_indices, row_offsets, column_indices):
    """Row-wise softmax over the stored entries.  src/softmax_cuda.cu:7-46."""
    return _ops.sparse_softmax(values, row_indices, row_offsets, column_indices)


def csr_transpose(m, n, values, row_offsets, column_indices):
    """CSR(m x n) -> [values_t, row_offsets_t, column_indices_t] of the transpose.
    src/transpose_cuda.cu:45-102.  values may also be [R,nnz] (extension)."""
    return _ops.csr_transpose(int(m), int(n), values, row_offsets, column_indices)


def csr_transpose_with_permutation(m, n, values, row_offsets, column_indices, checked=True):
    """Extension: as csr_transpose plus a 4th tensor,
    ``permutation`` with values_t == values[..., permutation], so a static
    topology's transpose can be cached by the caller.  ``checked`` (what a caller
    that KEEPS the result wants): wait for the stream and raise on a pattern the
    transpose is not defined for; ``checked=False`` is asynchronous like
    csr_transpose itself (no host round trip, legal inside a stream capture)."""
    return _ops.csr_transpose_with_permutation(int(m), int(n), values, row_offsets,
                                               column_indices, bool(checked))


# ---------------------------------------------------------------------------
# extensions
# ---------------------------------------------------------------------------
def spmm_bias(m, k, values, row_indices, row_offsets, column_indices, bias, dense_matrix):
    """spmm with ``bias[i]`` added to output row i in the kernel's epilogue.
    Call site tests/test_spmm_bias_relu.py:35-37."""
    return _ops.spmm_bias(int(m), int(k), values, row_indices, row_offsets, column_indices, bias,
                          dense_matrix)


def spmm_bias_relu(m, k, values, row_indices, row_offsets, column_indices, bias, dense_matrix):
    """``relu(spmm + bias)`` in one pass."""
    return _ops.spmm_bias_relu(int(m), int(k), values, row_indices, row_offsets, column_indices,
                               bias, dense_matrix)


def sparse_softmax_scaled(values, row_indices, row_offsets, column_indices, scale):
    """softmax(scale * values): the 1/sqrt(d) of modules/sparse_attention.py:72 folded in."""
    return _ops.sparse_softmax_scaled(values, row_indices, row_offsets, column_indices,
                                      float(scale))


def sparse_softmax_backward(softmax_out, grad_out, row_offsets, scale=1.0):
    """Gradient of softmax(scale * x) w.r.t. x given the forward output."""
    return _ops.sparse_softmax_backward(softmax_out, grad_out, row_offsets, float(scale))


def sparse_attention(query, key, value, row_indices, row_offsets, column_indices, scale):
    """softmax(scale * sddmm(query, key)) @ value over a fixed mask in ONE kernel
    (forward only): the chain of modules/sparse_attention.py:66-82 without the
    [replicas, nnz] intermediates.  query [R,S,D], key/value [R,S',D] -> [R,S,D]."""
    return _ops.sparse_attention(query, key, value, row_indices, row_offsets, column_indices,
                                 float(scale))


def sparse_attention_with_lse(query, key, value, row_indices, row_offsets, column_indices, scale):
    """As sparse_attention, returning [out, lse]: lse[r, i] = log-sum-exp of row i's
    scaled scores (-inf for rows without entries).  Head dimension 64 only."""
    return _ops.sparse_attention_with_lse(query, key, value, row_indices, row_offsets,
                                          column_indices, float(scale))


def _counts(nonzeros):
    import torch
    return nonzeros if torch.is_tensor(nonzeros) else torch.tensor(list(nonzeros),
                                                                    dtype=torch.int64)


def spmm_many_mask(b, m, k, nonzeros, values, row_indices, row_offsets, column_indices,
                   dense_matrix):
    """One mask per batch element, shared by its heads: replica r of
    values [R, max nnz] / dense [R,k,n] uses mask r // (R // b).
    tests/transformer/functions.py:20; layout tests/transformer/utils.py:17-38."""
    return _ops.spmm_many_mask(int(b), int(m), int(k), _counts(nonzeros), values, row_indices,
                               row_offsets, column_indices, dense_matrix)


def sddmm_many_mask(b, m, n, nonzeros, row_indices, row_offsets, column_indices, lhs_matrix,
                    rhs_matrix):
    """-> [R, max(nonzeros)], zero past a replica's own count.
    tests/transformer/functions.py:135; tests/test_attention_many_masks.py:120-127."""
    return _ops.sddmm_many_mask(int(b), int(m), int(n), _counts(nonzeros), row_indices,
                                row_offsets, column_indices, lhs_matrix, rhs_matrix)


def sparse_softmax_many_mask(b, m, nonzeros, values, row_indices, row_offsets, column_indices,
                             scale=None):
    """tests/transformer/functions.py:81; tests/test_attention_many_masks.py:132-138."""
    if scale is None:
        return _ops.sparse_softmax_many_mask(int(b), int(m), _counts(nonzeros), values,
                                             row_indices, row_offsets, column_indices)
    return _ops.sparse_softmax_many_mask_scaled(int(b), int(m), _counts(nonzeros), values,
                                                row_indices, row_offsets, column_indices,
                                                float(scale))


def sparse_softmax_backward_many_mask(b, m, nonzeros, softmax_out, grad_out, row_offsets,
                                      scale=1.0):
    return _ops.sparse_softmax_backward_many_mask(int(b), int(m), _counts(nonzeros), softmax_out,
                                                  grad_out, row_offsets, float(scale))


def csr_transpose_many_mask(b, m, n, nonzeros, values, row_offsets, column_indices):
    """-> [values_t [R, max nnz], row_offsets_t [b, n+1], column_indices_t [sum nnz]].
    tests/transformer/functions.py:50,165."""
    return _ops.csr_transpose_many_mask(int(b), int(m), int(n), _counts(nonzeros), values,
                                        row_offsets, column_indices)


def dense_to_csr(dense, with_values=False):
    """CSR topology of a dense mask or matrix, built on the device (csrc/topology.hip):
    dense [m, n], [b, m, n] or [b, 1, m, n] of any real dtype, an element is an entry where
    ``x != 0``.  -> [row_indices, row_offsets, column_indices, nonzeros] in the many-mask layout
    (row_indices [b, m], row_offsets [b, m + 1], no batch dimension for 2-D input; `nonzeros`
    an int64 host tensor, the form ``_counts`` passes through), plus ``values`` (the entries in
    the input's dtype, 2-D input only) ``with_values``.  A fixed number of launches and one
    synchronisation for any b; views with a dense last dimension are read in place."""
    return _ops.dense_to_csr(dense, bool(with_values))


def row_order(row_offsets):
    """row_offsets [m + 1] or [b, m + 1] (int32) -> row_indices [m] / [b, m]: every mask's rows
    by ascending length, ties by row -- ``topology.diffsort`` per mask in one launch, no
    synchronisation.  Raises beyond the rows ``capi.csr_row_order_route`` serves."""
    return _ops.row_order(row_offsets)


# ---- the argument contract of the topology ops below (topology.py checks with the same
# functions): a ValueError names the op and the argument, the binding never sees such a call ----
_TOPK_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _resolve_count(op, per_row, total, per_row_most, total_most):
    """ValueError unless exactly one of per_row / total is given and lies within 0 .. its bound
    (``None``: unbounded).  -> the count."""
    if (per_row is None) == (total is None):
        raise ValueError(f"{op}: give exactly one of per_row / total")
    name, count, most = ("total", int(total), total_most) if per_row is None else ("per_row", int(per_row), per_row_most)
    if count < 0 or (most is not None and count > most):
        raise ValueError(f"{op}: {name} = {count} is outside 0 .. {'n' if most is None else most}")
    return count


def _binding_counts(per_row, count):
    """(per_row, total) as the binding takes them: the count and -1 for the other one"""
    return (-1, count) if per_row is None else (count, -1)


def _device_floats(op, fallback, **tensors):
    """The guard of a device op, after its other checks: ValueError unless every tensor given by
    name is float32 / float16 / bfloat16, RuntimeError unless the first one is on a GPU."""
    for name, t in tensors.items():
        if t.dtype not in _TOPK_DTYPES:
            raise ValueError(f"{op}: {name} must be float32, float16 or bfloat16, got {t.dtype}")
    if not next(iter(tensors.values())).is_cuda:
        raise RuntimeError(f"{op}: GPU tensors only ({fallback} serves CPU tensors)")


def _check_csr_pattern(op, values, row_offsets, column_indices, scores=None, drop_counts=None):
    """ValueError unless values [nnz], row_offsets [m + 1] and column_indices [nnz] (int32) are
    one CSR pattern with its values on one device; with dense ``scores`` they are [m, n] on that
    device, and ``drop_counts`` is int32 [m] there.  Dtypes of values and scores are the caller's
    matter."""
    if scores is not None and scores.dim() != 2:
        raise ValueError(f"{op}: expected [m, n] scores, got {tuple(scores.shape)}")
    if values.dim() != 1:
        raise ValueError(f"{op}: values should be [nnz], got {tuple(values.shape)}")
    indices = [("row_offsets", row_offsets, None if scores is None else scores.size(0) + 1),
               ("column_indices", column_indices, values.numel())]
    if drop_counts is not None:
        indices.append(("drop_counts", drop_counts, scores.size(0)))
    for name, t, size in indices:
        if t.dtype != torch.int32 or t.dim() != 1 or (t.numel() < 1 if size is None else t.numel() != size):
            raise ValueError(f"{op}: {name} should be int32 [{'m + 1' if size is None else size}], got {t.dtype} "
                             f"{tuple(t.shape)}")
    for name, t in [entry[:2] for entry in indices] + [("scores", scores)] * (scores is not None):
        if t.device != values.device:
            raise ValueError(f"{op}: {name} is on {t.device}, values on {values.device}")


def _check_topk_arguments(op, scores, per_row, total, values_from):
    """ValueError unless scores are [m, n], exactly one of per_row / total is a count in range and
    ``values_from`` (if any) has the scores' shape and device.  -> the count."""
    if scores.dim() != 2:
        raise ValueError(f"{op}: expected [m, n] scores, got {tuple(scores.shape)}")
    count = _resolve_count(op, per_row, total, scores.size(1), scores.numel())
    if values_from is not None and (values_from.shape != scores.shape or values_from.device != scores.device):
        raise ValueError(f"{op}: values_from must have the scores' shape and device, got "
                         f"{tuple(values_from.shape)} on {values_from.device}")
    return count


def topk_to_csr(scores, per_row=None, total=None, values_from=None):
    """The CSR topology of the largest ``|scores|`` of a dense [m, n] float32 / float16 /
    bfloat16 matrix, selected and written out on the device (csrc/topology.hip): ``per_row = k``
    keeps the k largest of every row (ties to the lowest column), ``total = K`` the K largest of
    the matrix (ties to the lowest flat index) -- exactly one of the two.  Magnitudes rank by
    the bit pattern without the sign: NaN above inf above every finite value, -0.0 with 0.0.
    -> (row_indices, row_offsets, column_indices, values); ``values`` are the elements of
    ``values_from`` (same shape, any 2- or 4-byte dtype; default: the scores) at the kept
    positions, bit for bit.  No host synchronisation.  Raises for CPU tensors and for shapes
    ``capi.topk_to_csr_launch_shape`` does not serve (total mode above 16384 rows)."""
    count = _check_topk_arguments("topk_to_csr", scores, per_row, total, values_from)
    if values_from is not None and values_from.element_size() not in (2, 4):
        raise ValueError(f"topk_to_csr: values_from must have 2- or 4-byte elements, got {values_from.dtype}")
    _device_floats("topk_to_csr", "topology.magnitude_prune", scores=scores)
    return tuple(_ops.topk_to_csr(scores, *_binding_counts(per_row, count), values_from))


RANDOM_KEY_MASK = 0x7fffffff


def random_value_scale(bound):
    """``float32(bound / 2**23)`` as a Python float: the step between two values of a random
    topology, computed in double and rounded once."""
    bound = float(bound)
    if not (0.0 <= bound < float("inf")):
        raise ValueError(f"random_csr: bound {bound} should be a finite number >= 0")
    return float(torch.tensor(bound / 2.0 ** 23, dtype=torch.float64).to(torch.float32))


def check_random_arguments(m, n, per_row, total, dtype, key_mask):
    """ValueError unless the arguments describe a random ``m x n`` topology; -> the count."""
    m, n = int(m), int(n)
    if m < 0 or n < 0:
        raise ValueError(f"random_csr: expected sizes >= 0, got {m} x {n}")
    if dtype not in _TOPK_DTYPES:
        raise ValueError(f"random_csr: dtype must be float32, float16 or bfloat16, got {dtype}")
    count = _resolve_count("random_csr", per_row, total, n, m * n)
    if not 0 <= int(key_mask) <= RANDOM_KEY_MASK:
        raise ValueError(f"random_csr: key_mask {key_mask} is outside 0 .. 0x7fffffff")
    return count


def random_csr(m, n, per_row=None, total=None, dtype=torch.float32, bound=1.0, device=None, rng_state=None,
               key_mask=RANDOM_KEY_MASK):
    """A uniformly random ``m x n`` CSR topology with its initial values, drawn on the device
    (csrc/topology.hip): ``per_row = k`` keeps k positions of every row, ``total = K`` K positions
    of the matrix -- exactly one of the two; exactly that many, every position equally likely.
    It is ``topk_to_csr`` over Philox keys that are computed where a score would be loaded
    (include/sputnik_hip.h states the rule), so no ``[m, n]`` array exists.  ``values``
    (float32 / float16 / bfloat16) are uniform on ``[-bound, bound)``.
    -> (row_indices, row_offsets, column_indices, values, rng_state); ``rng_state`` (int64 [2],
    {seed, offset}) is what the call drew from the device's default generator
    (``torch.manual_seed`` makes runs repeat; a captured call draws a new pattern per replay), or
    the ``rng_state`` given, which reproduces the call that returned it.  ``key_mask`` below
    0x7fffffff forces ties between keys (tests).  One launch per row, nine in total mode, no host
    synchronisation.  Raises for a CPU device and for shapes ``capi.random_csr_launch_shape``
    does not serve (total mode above 16384 rows)."""
    count = check_random_arguments(m, n, per_row, total, dtype, key_mask)
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("random_csr: GPU devices only (topology.random_csr serves the CPU)")
    if rng_state is not None and (rng_state.dtype != torch.int64 or rng_state.numel() != 2):
        raise ValueError("random_csr: rng_state must be an int64 [2] tensor {seed, offset}")
    if rng_state is not None:
        rng_state = rng_state.to(device).contiguous()
    return tuple(_ops.random_csr(int(m), int(n), *_binding_counts(per_row, count), dtype, random_value_scale(bound),
                                 device, rng_state, int(key_mask)))


PATTERN_REACH = 2 ** 33          # beyond every |c - p| the device path serves
PATTERN_MAX_OFFSET = 2 ** 30     # |offset| below it on the device path
_INT_MAX = 2 ** 31 - 1


def _pattern_int(op, name, value, least):
    """``value`` as a Python int >= ``least``; ValueError otherwise (bools and floats included)"""
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise ValueError(f"{op}: {name} must be an integer, got {value!r}")
    if int(value) < least:
        raise ValueError(f"{op}: {name} = {int(value)} is below {least}")
    return int(value)


def _pattern_pair(op, name, value, what):
    if not isinstance(value, (tuple, list)) or len(value) != 2:
        raise ValueError(f"{op}: {name} must be {what}, got {value!r}")
    return value


def check_pattern_arguments(op, window=None, dilation=1, block=0, global_tokens=None, global_rows=True, summary=None,
                            random_blocks=None, causal=False):
    """The argument contract of an attention pattern (``attention_pattern_csr`` states the rule):
    ValueError, naming ``op`` and the argument, unless ``window`` is None, an int w >= 0 or a pair
    (left, right) of such, ``dilation`` an int >= 1, ``block`` an int >= 0, ``summary`` None or
    (stride, width) with 0 < width <= stride, ``global_tokens`` None, an int >= 0 or a 1-D
    integer tensor / list of positions (checked against n by ``pattern_global_flags``),
    ``random_blocks`` None or (rb, probability) with rb >= 1 and 0 <= probability <= 1, and at
    least one component is given.  -> a dict of Python values: window (left, right) or None,
    dilation, block, summary (stride, width) or None, global_tokens, global_rows,
    random_blocks (rb, threshold) or None with threshold = round(probability * 2**31), causal."""
    if window is not None:
        if isinstance(window, (tuple, list)):
            left, right = _pattern_pair(op, "window", window, "an int or (left, right)")
        else:
            left = right = window
        window = (_pattern_int(op, "window", left, 0), _pattern_int(op, "window", right, 0))
    dilation = _pattern_int(op, "dilation", dilation, 1)
    block = _pattern_int(op, "block", block, 0)
    if summary is not None:
        stride, width = _pattern_pair(op, "summary", summary, "(stride, width)")
        stride, width = _pattern_int(op, "summary", stride, 1), _pattern_int(op, "summary", width, 1)
        if width > stride:
            raise ValueError(f"{op}: summary needs 0 < width <= stride, got stride {stride}, width {width}")
        summary = (stride, width)
    if global_tokens is not None:
        if torch.is_tensor(global_tokens):
            if global_tokens.dim() != 1 or global_tokens.dtype.is_floating_point or global_tokens.dtype.is_complex \
                    or global_tokens.dtype == torch.bool:
                raise ValueError(f"{op}: global_tokens must be an int or a 1-D integer tensor / list of positions, "
                                 f"got {global_tokens.dtype} {tuple(global_tokens.shape)}")
        elif isinstance(global_tokens, (tuple, list)):
            global_tokens = [_pattern_int(op, "global_tokens", g, 0) for g in global_tokens]
        else:
            global_tokens = _pattern_int(op, "global_tokens", global_tokens, 0)
    if random_blocks is not None:
        rb, probability = _pattern_pair(op, "random_blocks", random_blocks, "(rb, probability)")
        rb = _pattern_int(op, "random_blocks", rb, 1)
        if isinstance(probability, bool) or not isinstance(probability, (int, float)) or not 0.0 <= probability <= 1.0:
            raise ValueError(f"{op}: the probability of random_blocks must lie in 0 .. 1, got {probability!r}")
        random_blocks = (rb, round(probability * 2 ** 31))
    if window is None and block == 0 and summary is None and global_tokens is None and random_blocks is None:
        raise ValueError(f"{op}: a pattern needs at least one of window / block / summary / global_tokens / "
                         f"random_blocks")
    return dict(window=window, dilation=dilation, block=block, summary=summary, global_tokens=global_tokens,
                global_rows=bool(global_rows), random_blocks=random_blocks, causal=bool(causal))


def pattern_global_flags(op, global_tokens, n, device):
    """bool [n] on ``device``: True at the first ``g`` positions (int ``g``) or at the listed
    ones; None for None.  ValueError for a position outside 0 .. n - 1 (a count outside 0 .. n)."""
    if global_tokens is None:
        return None
    flags = torch.zeros(n, dtype=torch.bool, device=device)
    if isinstance(global_tokens, int):
        if global_tokens > n:
            raise ValueError(f"{op}: global_tokens = {global_tokens} is outside 0 .. {n}")
        flags[:global_tokens] = True
        return flags
    positions = torch.as_tensor(global_tokens, dtype=torch.int64).reshape(-1)
    if positions.numel() > 0:
        low, high = int(positions.min()), int(positions.max())
        if low < 0 or high >= n:
            raise ValueError(f"{op}: global_tokens holds position {low if low < 0 else high}, outside 0 .. {n - 1}")
        flags[positions.to(device)] = True
    return flags


def check_pattern_sizes(op, m, n, offset):
    """ValueError unless m, n >= 0 and offset are integers.  -> (m, n, offset) as Python ints"""
    return _pattern_int(op, "m", m, 0), _pattern_int(op, "n", n, 0), _pattern_int(op, "offset", offset, -2 ** 62)


def pattern_rng_state(op, rng_state):
    """ValueError unless ``rng_state`` is an int64 [2] tensor {seed, offset}, offset a multiple of 4"""
    if not torch.is_tensor(rng_state) or rng_state.dtype != torch.int64 or rng_state.numel() != 2:
        raise ValueError(f"{op}: rng_state must be an int64 [2] tensor {{seed, offset}}")
    return rng_state


def attention_pattern_csr(m, n, offset=0, window=None, dilation=1, block=0, global_tokens=None, global_rows=True,
                          summary=None, random_blocks=None, causal=False, device=None, rng_state=None):
    """The CSR topology of a structured attention pattern over ``m`` query rows and ``n`` key
    columns, built on the device from its rule with no dense mask (csrc/topology.hip).

    The rule: row r sits at position ``p = r + offset`` and ``d = c - p``; entry (r, c) is kept
    iff (not ``causal`` or d <= 0) and at least one component keeps it --
    ``window=(left, right)`` (an int w: (w, w)) with ``dilation``: ``-left * dilation <= d <=
    right * dilation`` and ``d % dilation == 0``; ``block=b``: ``c // b == p // b``;
    ``summary=(stride, width)``: ``c % stride >= stride - width``; ``global_tokens`` (an int g:
    the first g positions; or a 1-D integer tensor / list of positions): ``flag[c]``, or, with
    ``global_rows``, ``0 <= p < n and flag[p]``; ``random_blocks=(rb, probability)``:
    ``key(r // rb, c // rb) < round(probability * 2**31)`` with ``random_csr``'s key stream,
    ``key(R, C) = Philox(seed, (offset_rng / 4, C >> 2, R))[C & 3] & 0x7fffffff``.  Columns ascend
    inside a row, an entry appears once, a row may be empty.

    -> (row_indices, row_offsets, column_indices, rng_state).  Without ``random_blocks`` no
    generator state is consumed and ``rng_state`` is None; with them it is the int64 [2]
    {seed, offset} the call drew from the device's default generator (4, as ``random_csr``), or
    the ``rng_state`` given, which reproduces the call that returned it.  Four launches and one
    synchronisation; nothing of size ``m * n`` is allocated.  Raises ValueError for an argument
    outside the contract, RuntimeError for a CPU device and for sizes
    ``capi.attention_pattern_launch_shape`` does not serve (more than 16384 rows, ``m * n``
    above INT_MAX, ``|offset| >= 2**30``): ``topology.AttentionPattern.build`` serves those."""
    op = "attention_pattern_csr"
    m, n, offset = check_pattern_sizes(op, m, n, offset)
    rule = check_pattern_arguments(op, window, dilation, block, global_tokens, global_rows, summary, random_blocks,
                                   causal)
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"{op}: GPU devices only (topology.AttentionPattern.build serves the CPU)")
    if m > _INT_MAX or n > _INT_MAX or abs(offset) >= PATTERN_MAX_OFFSET:
        raise RuntimeError(f"{op}: the sizes are beyond what the kernels serve (capi.attention_pattern_launch_shape "
                           f"states the limits); take topology.AttentionPattern.build")
    flags = pattern_global_flags(op, rule["global_tokens"], n, device)
    if rule["random_blocks"] is None:
        rng_state = None
    elif rng_state is not None:
        rng_state = pattern_rng_state(op, rng_state).to(device).contiguous()
    # the products the kernel compares with, clamped beyond every |c - p| it can meet
    reach = PATTERN_REACH
    left, right = (-1, 0) if rule["window"] is None else (min(w * rule["dilation"], reach) for w in rule["window"])
    stride, width = (0, 0) if rule["summary"] is None else rule["summary"]
    rb, threshold = (0, 0) if rule["random_blocks"] is None else rule["random_blocks"]
    out = _ops.attention_pattern_csr(
        m, n, offset, left, right, min(rule["dilation"], reach), min(rule["block"], _INT_MAX),
        min(stride, _INT_MAX), min(stride - width, _INT_MAX), min(rb, _INT_MAX), threshold, rule["causal"],
        rule["global_rows"], None if flags is None else flags.view(torch.uint8), device, rng_state)
    return tuple(out) + ((None,) if len(out) == 3 else ())


def check_regrow_arguments(values, row_offsets, column_indices, drop_counts, scores):
    """ValueError unless the five tensors are one CSR pattern with its values, drop counts and
    dense scores (shapes, int32 indices, one device).  Dtypes of values and scores are the
    caller's matter."""
    _check_csr_pattern("csr_regrow", values, row_offsets, column_indices, scores, drop_counts)


def csr_regrow(values, row_offsets, column_indices, drop_counts, scores):
    """One per-row drop-and-grow step of a CSR pattern on the device (csrc/topology.hip): row r
    of ``len_r`` entries drops ``d_r = clamp(drop_counts[r], 0, len_r)`` of them and grows as
    many.  Kept: the ``len_r - d_r`` entries of largest ``|values|``, ties to the lower column.
    Grown: the ``d_r`` columns outside the kept ones of largest ``|scores[r]|``, ties to the
    lowest column; NaN and inf scores count as the dtype's largest finite value; columns dropped
    in this call are eligible.  Magnitudes rank by the bit pattern without the sign
    (``topology.magnitude_keys``).  values [nnz] and scores [m, n] are float32 / float16 /
    bfloat16, each of its own dtype; row_offsets [m + 1], column_indices [nnz] (ascending inside
    a row) and drop_counts [m] are int32.  -> (column_indices, values, source) of the new
    pattern in the same slots, ascending inside a row: a kept entry carries its value bit for
    bit and its old index in ``source`` (int64), a grown one is +0.0 and -1.  One launch, no
    host synchronisation.  Raises for CPU tensors and for ``n`` beyond
    ``capi.csr_regrow_launch_shape(...)["max_n"]``."""
    check_regrow_arguments(values, row_offsets, column_indices, drop_counts, scores)
    _device_floats("csr_regrow", "topology.regrow_per_row", values=values, scores=scores)
    return tuple(_ops.csr_regrow(values, row_offsets, column_indices, drop_counts, scores))


def check_regrow_total_arguments(values, row_offsets, column_indices, drop, scores):
    """ValueError unless the four tensors are one CSR pattern with its values and dense scores
    (shapes, int32 indices, one device) and ``drop`` is a count within 0 .. nnz.  -> the count.
    Dtypes of values and scores are the caller's matter."""
    _check_csr_pattern("csr_regrow_total", values, row_offsets, column_indices, scores)
    count = int(drop)
    if not 0 <= count <= values.numel():
        raise ValueError(f"csr_regrow_total: drop = {count} is outside 0 .. {values.numel()}")
    return count


def csr_regrow_total(values, row_offsets, column_indices, drop, scores):
    """One matrix-wide drop-and-grow step of a CSR pattern on the device (csrc/topology.hip):
    ``drop = d`` (a host integer, ``0 <= d <= nnz``) entries go and as many come, ``nnz`` stays.
    Kept: the ``nnz - d`` entries of largest ``|values|``, ties to the lower entry index.  Grown:
    the ``d`` positions outside the kept ones of largest ``|scores|``, ties to the lower flat
    (row-major) index; NaN and inf scores count as the dtype's largest finite value; positions
    dropped in this call are eligible.  Magnitudes rank by the bit pattern without the sign
    (``topology.magnitude_keys``).  values [nnz] and scores [m, n] are float32 / float16 /
    bfloat16, each of its own dtype; row_offsets [m + 1] and column_indices [nnz] (ascending
    inside a row) are int32.  -> (row_indices, row_offsets, column_indices, values, source) of
    the new pattern, columns ascending inside a row: a kept entry carries its value bit for bit
    and its old index in ``source`` (int64), a grown one is +0.0 and -1.  A fixed number of
    launches, no host synchronisation: the call can be captured in a graph.  Raises for CPU
    tensors and beyond the rows and columns ``capi.csr_regrow_total_launch_shape`` serves."""
    count = check_regrow_total_arguments(values, row_offsets, column_indices, drop, scores)
    _device_floats("csr_regrow_total", "topology.regrow_total", values=values, scores=scores)
    return tuple(_ops.csr_regrow_total(values, row_offsets, column_indices, count, scores))


REGROW_KEY_MASK = 0x3fffffff


def _check_key_step(op, values, n, grow_bound, rng_state, key_mask):
    """ValueError unless ``n`` is a width, ``key_mask`` lies in 0 .. 0x3fffffff, ``grow_bound`` is
    None or a finite number >= 0 and ``rng_state`` is None or int64 [2].  -> (the grow scale the
    binding takes: ``random_value_scale(grow_bound)``, -1.0 for None; the state on the values'
    device)"""
    if int(n) < 0:
        raise ValueError(f"{op}: expected n >= 0, got {int(n)}")
    if not 0 <= int(key_mask) <= REGROW_KEY_MASK:
        raise ValueError(f"{op}: key_mask {key_mask} is outside 0 .. 0x3fffffff")
    if grow_bound is not None and not 0.0 <= float(grow_bound) < float("inf"):
        raise ValueError(f"{op}: grow_bound {grow_bound} should be None or a finite number >= 0")
    if rng_state is not None and (rng_state.dtype != torch.int64 or rng_state.numel() != 2):
        raise ValueError(f"{op}: rng_state must be an int64 [2] tensor {{seed, offset}}")
    if rng_state is not None:
        rng_state = rng_state.to(values.device).contiguous()
    return -1.0 if grow_bound is None else random_value_scale(grow_bound), rng_state


def check_regrow_random_arguments(values, row_offsets, column_indices, drop_counts, n, grow_bound=None,
                                  rng_state=None, key_mask=REGROW_KEY_MASK):
    """ValueError unless the four tensors are one CSR pattern of ``m = row_offsets.numel() - 1``
    rows with its values and drop counts (shapes, int32 indices, one device) and the other
    arguments are those of a step under generated scores.  -> (grow scale, rng_state)"""
    op = "csr_regrow_random"
    _check_csr_pattern(op, values, row_offsets, column_indices)
    m = row_offsets.numel() - 1
    if drop_counts.dtype != torch.int32 or drop_counts.dim() != 1 or drop_counts.numel() != m:
        raise ValueError(f"{op}: drop_counts should be int32 [{m}], got {drop_counts.dtype} {tuple(drop_counts.shape)}")
    if drop_counts.device != values.device:
        raise ValueError(f"{op}: drop_counts is on {drop_counts.device}, values on {values.device}")
    return _check_key_step(op, values, n, grow_bound, rng_state, key_mask)


def csr_regrow_random(values, row_offsets, column_indices, drop_counts, n, grow_bound=None, rng_state=None,
                      key_mask=REGROW_KEY_MASK):
    """One per-row drop-and-grow step of the CSR pattern of an ``m x n`` matrix under random grow
    scores that are never stored (csrc/topology.hip): SET's step.  For ``rng_state = {seed,
    offset}`` (offset a multiple of 4), with Philox4x32-10, ``key(r, c) = Philox(seed, (offset / 4,
    c >> 2, r))[c & 3] & key_mask`` -- the key stream of ``random_csr``, under a mask of at most
    30 bits (``REGROW_KEY_MASK``), so that a key read as float32 bits is finite and non-negative
    and the clamp of the regrow rule never acts.  The step is EXACTLY ``csr_regrow`` under dense
    float32 scores whose bits are the keys: kept entries, ties (lowest column), eligibility of
    dropped columns, ascending columns and ``source`` are its.  A grown entry is ``+0.0``
    (``grow_bound=None``; RigL's choice) or the value ``random_csr`` gives that position under
    ``bound = grow_bound``: ``float32((word' >> 8) - 2**23) * float32(grow_bound / 2**23)`` from
    the value stream, rounded to nearest even into the values' dtype (SET re-initialises what it
    grows); its ``source`` is -1 either way.
    -> (column_indices, values, source, rng_state); ``rng_state`` (int64 [2]) is what the call
    drew from the device's default generator (4 of its offset; ``torch.manual_seed`` makes runs
    repeat; a captured call draws new scores per replay), or the one given, which reproduces the
    call that returned it.  One launch, 5 Philox calls per four columns of a row, no ``[m, n]``
    array, no host synchronisation.  Raises for CPU tensors and for ``n`` beyond
    ``capi.csr_regrow_random_launch_shape(...)["max_n"]`` (61440)."""
    scale, rng_state = check_regrow_random_arguments(values, row_offsets, column_indices, drop_counts, n, grow_bound,
                                                     rng_state, key_mask)
    _device_floats("csr_regrow_random", "topology.regrow_per_row_random", values=values)
    return tuple(_ops.csr_regrow_random(values, row_offsets, column_indices, drop_counts, int(n), scale, rng_state,
                                        int(key_mask)))


def check_regrow_total_random_arguments(values, row_offsets, column_indices, drop, n, grow_bound=None,
                                        rng_state=None, key_mask=REGROW_KEY_MASK):
    """ValueError unless the three tensors are one CSR pattern with its values (shapes, int32
    indices, one device), ``drop`` is a count within 0 .. nnz and the other arguments are those
    of a step under generated scores.  -> (the count, grow scale, rng_state)"""
    op = "csr_regrow_total_random"
    _check_csr_pattern(op, values, row_offsets, column_indices)
    count = int(drop)
    if not 0 <= count <= values.numel():
        raise ValueError(f"{op}: drop = {count} is outside 0 .. {values.numel()}")
    return (count,) + _check_key_step(op, values, n, grow_bound, rng_state, key_mask)


def csr_regrow_total_random(values, row_offsets, column_indices, drop, n, grow_bound=None, rng_state=None,
                            key_mask=REGROW_KEY_MASK):
    """One matrix-wide drop-and-grow step of the CSR pattern of an ``m x n`` matrix under random
    grow scores that are never stored (csrc/topology.hip): the layer-wise step of SET.  The keys,
    the mask, ``grow_bound`` and ``rng_state`` are those of ``csr_regrow_random``; the step is
    EXACTLY ``csr_regrow_total`` under dense float32 scores whose bits are the keys (ties to the
    lowest flat index).  -> (row_indices, row_offsets, column_indices, values, source,
    rng_state).  8 + value digits + 4 launches, 6 Philox calls per four positions, no ``[m, n]``
    array, no host synchronisation: the call is captured in a graph whole.  Raises for CPU
    tensors and beyond the 16384 rows and 65536 columns ``capi.csr_regrow_random_launch_shape``
    serves."""
    count, scale, rng_state = check_regrow_total_random_arguments(values, row_offsets, column_indices, drop, n,
                                                                  grow_bound, rng_state, key_mask)
    _device_floats("csr_regrow_total_random", "topology.regrow_total_random", values=values)
    return tuple(_ops.csr_regrow_total_random(values, row_offsets, column_indices, count, int(n), scale, rng_state,
                                              int(key_mask)))


def check_csr_topk_arguments(values, row_offsets, column_indices, per_row, total):
    """ValueError unless the three tensors are one CSR pattern with its values (shapes, int32
    indices, one device) and exactly one of per_row / total is a count in range (``total`` at
    most nnz, ``per_row`` at least 0).  -> the count.  The dtype of values is the caller's
    matter."""
    _check_csr_pattern("csr_topk", values, row_offsets, column_indices)
    return _resolve_count("csr_topk", per_row, total, None, values.numel())


def csr_topk(values, row_offsets, column_indices, per_row=None, total=None):
    """The entries of largest ``|values|`` of a CSR pattern, written out as a smaller CSR pattern
    on the device (csrc/topology.hip): ``total = K`` keeps the K largest of all nnz entries,
    ``per_row = k`` the ``min(len_r, k)`` largest of every row -- exactly one of the two; among
    equal magnitudes the lower entry index wins.  Magnitudes rank by the bit pattern without the
    sign (``topology.magnitude_keys``).  values [nnz] is float32 / float16 / bfloat16,
    row_offsets [m + 1] and column_indices [nnz] (ascending inside a row) are int32.
    -> (row_indices, row_offsets, column_indices, values, source): a kept entry carries its
    column, its value bit for bit and, in ``source`` (int64, ascending), its index in the old
    arrays.  ``total`` never synchronises; ``per_row`` reads the new size back once.  Raises for
    CPU tensors and for more rows than ``capi.csr_topk_launch_shape`` serves (16384)."""
    count = check_csr_topk_arguments(values, row_offsets, column_indices, per_row, total)
    _device_floats("csr_topk", "topology.prune_csr", values=values)
    return tuple(_ops.csr_topk(values, row_offsets, column_indices, *_binding_counts(per_row, count)))


def check_csr_topk_global_arguments(values, row_offsets, column_indices, total):
    """ValueError unless the three are sequences of one length whose l-th elements are one CSR
    pattern with its values (``check_csr_topk_arguments``), every tensor is on one device and
    ``total`` is a count within 0 .. sum nnz_l.  -> the count.  The dtypes of the values are the
    caller's matter."""
    values, row_offsets, column_indices = list(values), list(row_offsets), list(column_indices)
    if not len(values) == len(row_offsets) == len(column_indices):
        raise ValueError(f"csr_topk_global: {len(values)} values, {len(row_offsets)} row_offsets and "
                         f"{len(column_indices)} column_indices")
    if total is None:
        raise ValueError("csr_topk_global: total is missing")
    for v, ro, ci in zip(values, row_offsets, column_indices):
        _check_csr_pattern("csr_topk_global", v, ro, ci)
        if v.device != values[0].device:
            raise ValueError(f"csr_topk_global: values are on {values[0].device} and on {v.device}")
    return _resolve_count("csr_topk_global", None, total, None, sum(v.numel() for v in values))


def csr_topk_global(values, row_offsets, column_indices, total):
    """ONE top-k across the entries of several CSR patterns on the device (csrc/topology.hip):
    three lists of equal length -- values[l] [nnz_l] (float32 / float16 / bfloat16, one dtype for
    all), row_offsets[l] [m_l + 1] and column_indices[l] [nnz_l] (int32) -- of which the
    ``total = K`` entries of largest ``|value|`` over ALL layers are kept
    (``topology.magnitude_keys``); among equal magnitudes the layer listed first wins, then the
    lower entry index.  -> a list of (row_indices, row_offsets, column_indices, values, source),
    one per layer, as ``csr_topk`` returns them; a layer may keep nothing.  The layers' new
    sizes are read back once, whatever their number.  Raises for CPU tensors, mixed dtypes, a
    layer of more rows than ``capi.csr_topk_global_launch_shape`` serves (16384) and more than
    2**31 - 1 entries in all."""
    count = check_csr_topk_global_arguments(values, row_offsets, column_indices, total)
    values, row_offsets, column_indices = list(values), list(row_offsets), list(column_indices)
    if not values:
        return []
    for v in values:
        if v.dtype != values[0].dtype:
            raise ValueError(f"csr_topk_global: values must be of one dtype, got {values[0].dtype} and {v.dtype}")
    _device_floats("csr_topk_global", "topology.prune_csr_global", values=values[0])
    flat = _ops.csr_topk_global(values, row_offsets, column_indices, count)
    return [tuple(flat[5 * l:5 * l + 5]) for l in range(len(values))]


def sparse_attention_many_mask(b, nonzeros, row_indices, row_offsets, column_indices, query, key,
                               value, scale, with_lse=False, plan=None):
    """softmax(scale * q k^T at the mask) v with one mask per batch element in ONE kernel:
    query [R,S,D], key/value [R,S',D] (float32; half storage is widened -- the heads form
    keeps it), replica r under mask r // (R // b); topology in the many-mask layout
    (tests/transformer/utils.py:17-38).  -> [R,S,D] float32, or [out, lse] ``with_lse``.
    What the kernel does not serve (head dimension other than 64, unaligned operands) is
    composed from the many-mask operators (no lse then)."""
    outs = _ops.sparse_attention_many_mask(int(b), _counts(nonzeros), query, key, value, row_indices,
                                           row_offsets, column_indices, float(scale), bool(with_lse),
                                           plan)
    return outs if with_lse else outs[0]


def sparse_attention_many_mask_with_lse(b, nonzeros, row_indices, row_offsets, column_indices, query,
                                        key, value, scale):
    return sparse_attention_many_mask(b, nonzeros, row_indices, row_offsets, column_indices, query,
                                      key, value, scale, with_lse=True)


def sparse_attention_many_mask_plan(b, m, n, d, nonzeros, row_indices, row_offsets, column_indices):
    """Pre-pass of both many-mask attention forms over b masks of m x n, head dimension d."""
    return _ops.sparse_attention_many_mask_plan(int(b), int(m), int(n), int(d), _counts(nonzeros),
                                                row_indices, row_offsets, column_indices)


def sparse_attention_many_mask_planned(b, nonzeros, row_indices, row_offsets, column_indices, query,
                                       key, value, scale, plan, with_lse=False):
    return sparse_attention_many_mask(b, nonzeros, row_indices, row_offsets, column_indices, query,
                                      key, value, scale, with_lse=with_lse, plan=plan)


def sparse_attention_heads_many_mask(b, nonzeros, row_indices, row_offsets, column_indices, query,
                                     key, value, scale, out_dtype=None, with_lse=False, plan=None):
    """The many-mask attention on float16 / bfloat16 head views [B, H, rows, 64] (any strides
    with a unit last one; batch element i under mask i, so B = b), as
    sparse_attention_heads: the result is stored as `out_dtype` (the operands' type by
    default, or float32) in a [B, rows, H, 64] buffer and returned as its [B, H, rows, 64]
    view; ``with_lse`` -> [out, lse [B, H, rows]]."""
    out_code = _half_code(query.dtype if out_dtype is None else out_dtype)
    outs = _ops.sparse_attention_heads_many_mask(int(b), _counts(nonzeros), query, key, value,
                                                 row_indices, row_offsets, column_indices,
                                                 float(scale), out_code, bool(with_lse), plan)
    return outs if with_lse else outs[0]


# ---------------------------------------------------------------------------
# static topologies: plan once, run many times (no counterpart in the reference,
# which re-derives everything per call, src/spmm_cuda.cu:48-57)
# ---------------------------------------------------------------------------
def spmm_plan(m, k, n, row_indices, row_offsets, column_indices):
    """Topology-only pre-pass for spmm / left_spmm with a dense operand of width
    `n`; returns the plan (a uint8 tensor) for spmm_planned / left_spmm_planned.
    Valid as long as the three index tensors, m, k and n do not change."""
    return _ops.spmm_plan(int(m), int(k), int(n), row_indices, row_offsets, column_indices)


def spmm_planned(m, k, values, row_indices, row_offsets, column_indices, dense_matrix, plan):
    return _ops.spmm_planned(int(m), int(k), values, row_indices, row_offsets, column_indices,
                             dense_matrix, plan)


def left_spmm_planned(m, k, values, row_indices, row_offsets, column_indices, dense_matrix, plan):
    return _ops.left_spmm_planned(int(m), int(k), values, row_indices, row_offsets,
                                  column_indices, dense_matrix, plan)


def sddmm_plan(m, n, k, row_indices, row_offsets, column_indices):
    """Pre-pass for sddmm over an m x n mask with inner dimension k."""
    return _ops.sddmm_plan(int(m), int(n), int(k), row_indices, row_offsets, column_indices)


def sddmm_planned(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix, plan):
    return _ops.sddmm_planned(int(m), int(n), row_indices, row_offsets, column_indices,
                              lhs_matrix, rhs_matrix, plan)


def permute_band_size():
    return _ops.permute_band_size()


def banded_lists(permutation):
    """(dest_list, source_in_band) of sputnik_hip_permute_banded_batched for a
    permutation (out[i] = in[permutation[i]]): the output positions grouped by the
    band of their source, ascending inside a band."""
    band = permute_band_size()
    perm = permutation.long()
    order = torch.argsort(torch.div(perm, band, rounding_mode="floor"), stable=True)
    return (order.to(torch.int32).contiguous(),
            torch.remainder(perm[order], band).to(torch.int32).contiguous())


def permute_last_banded(values, dest_list, source_in_band):
    """permute_last for many rows of values, through LDS (lists: banded_lists)."""
    return _ops.permute_last_banded(values, dest_list, source_in_band)


def spmm_permuted_fused(m, k, n, nonzeros):
    """True where spmm_permuted runs as one kernel (and that is the faster form)."""
    from . import capi
    return bool(capi.lib().sputnik_hip_spmm_permuted_supported(int(m), int(k), int(n), int(nonzeros)))


def spmm_permuted(m, k, values, permutation, row_indices, row_offsets, column_indices,
                  dense_matrix, plan=None, left=False):
    """spmm / left_spmm over a topology whose values are stored in another order of
    the same entries (entry p takes ``values[..., permutation[p]]``): the product
    with a transpose whose topology and permutation are cached.  One kernel where
    the panel kernel serves the shape, else permute_last + the planned product."""
    op = _ops.left_spmm_permuted if left else _ops.spmm_permuted
    return op(int(m), int(k), values, permutation, row_indices, row_offsets, column_indices,
              dense_matrix, plan)


def spmm_transposed_out(m, k, values, row_indices, row_offsets, column_indices, dense_matrix,
                        block_rows, permutation=None, plan=None, left=False):
    """spmm / left_spmm with the product stored as the transposes of its blocks of
    ``block_rows`` rows -> [replicas * m / block_rows, n, block_rows]: the head
    split behind a projection (block_rows = head_dim,
    modules/sparse_attention.py:38-45) or C^T (block_rows = m), written by the
    kernel's store phase where the panel kernel serves the shape."""
    return _ops.spmm_transposed_out(int(m), int(k), values, permutation, row_indices,
                                    row_offsets, column_indices, dense_matrix, int(block_rows),
                                    bool(left), plan)


def left_spmm_group(m, k, values, row_indices, row_offsets, column_indices, dense_matrix,
                    block_rows=0):
    """Several sparse weights of one shape times ONE batch of dense matrices in one
    launch (lists with one entry per weight) -> list of products, each head split
    as in spmm_transposed_out when ``block_rows`` > 0: the q, k and v projections of
    a self-attention block (modules/sparse_attention.py:108-110)."""
    return _ops.left_spmm_group(int(m), int(k), list(values), list(row_indices),
                                list(row_offsets), list(column_indices), dense_matrix,
                                int(block_rows))


def left_spmm_group_sum(m, k, values, permutations, row_indices, row_offsets, column_indices,
                        dense_matrices):
    """sum_p A_p @ dense_p in one launch, accumulated in registers (values gathered
    through ``permutations`` when the list is not empty): the input gradient of a
    group of projections."""
    return _ops.left_spmm_group_sum(int(m), int(k), list(values), list(permutations),
                                    list(row_indices), list(row_offsets), list(column_indices),
                                    list(dense_matrices))


def sddmm_sum(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix):
    """sum over the replicas of sddmm(...) -> [nnz]: the gradient of sparse values
    shared by a batch (what autograd makes of the [R, nnz] result of
    tests/test_linear_3d.py:64-69), summed inside the call in replica order."""
    return _ops.sddmm_sum(int(m), int(n), row_indices, row_offsets, column_indices, lhs_matrix,
                          rhs_matrix)


def sddmm_sum_plan(m, n, k, row_indices, row_offsets, column_indices):
    """Pre-pass for sddmm_sum_planned (its own: not interchangeable with sddmm_plan)."""
    return _ops.sddmm_sum_plan(int(m), int(n), int(k), row_indices, row_offsets, column_indices)


def sddmm_sum_planned(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix,
                      plan):
    return _ops.sddmm_sum_planned(int(m), int(n), row_indices, row_offsets, column_indices,
                                  lhs_matrix, rhs_matrix, plan)


def sddmm_sum_group_planned(m, n, row_indices, row_offsets, column_indices, lhs_matrices, rhs_matrix,
                            plans):
    """Up to four summed SDDMMs of one shape against ONE rhs in one call (lists with an entry
    per product; float32, [replicas, rows, k]): the weight gradients of a group of projections
    (modules/sparse_attention.py:108-110), whose partial sums one launch adds.  Bit-identical
    to sddmm_sum_planned product by product."""
    return _ops.sddmm_sum_group_planned(int(m), int(n), list(row_indices), list(row_offsets),
                                        list(column_indices), list(lhs_matrices), rhs_matrix,
                                        list(plans))


def sparse_attention_plan(m, n, d, row_indices, row_offsets, column_indices):
    """Pre-pass for the fused attention over an m x n mask with head dimension d."""
    return _ops.sparse_attention_plan(int(m), int(n), int(d), row_indices, row_offsets,
                                      column_indices)


def sparse_attention_planned(query, key, value, row_indices, row_offsets, column_indices, scale,
                             plan):
    return _ops.sparse_attention_planned(query, key, value, row_indices, row_offsets,
                                         column_indices, float(scale), plan)


def sparse_attention_with_lse_planned(query, key, value, row_indices, row_offsets, column_indices,
                                      scale, plan):
    """sparse_attention_with_lse through a plan of sparse_attention_plan -> [out, lse]."""
    return _ops.sparse_attention_with_lse_planned(query, key, value, row_indices, row_offsets,
                                                  column_indices, float(scale), plan)


def sparse_attention_supported(m, n, d, nonzeros):
    """True where the fused forward (sparse_attention*, with lse) serves the shape: head
    dimension 64 and a mask with entries."""
    from . import capi
    return bool(capi.lib().sputnik_hip_sparse_attention_supported(int(m), int(n), int(d),
                                                                  int(nonzeros)))


def sparse_attention_backward_supported(m, n, d, nonzeros):
    """True where sparse_attention_backward serves the shape (head dimension 64 or 128, 32-bit
    offsets)."""
    from . import capi
    return bool(capi.lib().sputnik_hip_sparse_attention_backward_supported(
        int(m), int(n), int(d), int(nonzeros)))


def sparse_attention_rows_supported(m, n, d, nonzeros):
    """True where the row-group forward (sparse_attention_rows) serves the shape: head
    dimension 128, a mask with entries, 32-bit offsets (m and n below 2^23)."""
    from . import capi
    return bool(capi.lib().sputnik_hip_sparse_attention_rows_supported(int(m), int(n), int(d),
                                                                       int(nonzeros)))


def sparse_attention_rows(query, key, value, row_indices, row_offsets, column_indices, scale, p=0.0):
    """The fused attention forward at head dimension 128, in the row-group form: one kernel,
    one 16-lane row group per query row that gathers K and V rows and keeps an online softmax
    in registers; no plan, nothing of size [R, nnz].  float32 [R, S, 128] (or [S, 128])
    operands, made contiguous.  -> (out, lse, rng_state): lse is the log-sum-exp of the
    undropped scores (-inf for rows without entries), what sparse_attention_backward needs;
    p > 0 is dropout on the weights (the sparse_attention_dropout contract: e = CSR position,
    the generator offset advances by 4), p = 0 draws nothing and rng_state is None.  Raises
    where sparse_attention_rows_supported is false."""
    p = check_dropout_p(p)
    outs = _ops.sparse_attention_rows(query, key, value, row_indices, row_offsets, column_indices,
                                      float(scale), p)
    return outs[0], outs[1], (outs[2] if p > 0.0 else None)


def sparse_attention_backward(query, key, value, out, grad_out, lse, row_indices, row_offsets,
                              column_indices, transposed, scale, p=0.0, rng_state=None,
                              needs=(True, True, True)):
    """Gradients (dQ, dK, dV) of the fused attention, two kernels and nothing of size
    [R, nnz]: `out` and `lse` from the forward (sparse_attention_with_lse or
    sparse_attention_dropout), `grad_out` the gradient of out.  `transposed` =
    (row_indices_t, row_offsets_t, column_indices_t, permutation) of the mask, as
    csr_transpose_with_permutation and diffsort give them; it may be None when neither dK nor
    dV is wanted.  p > 0: the forward's dropout, replayed from its rng_state.  `needs` picks
    which of the three are computed; the others come back as None."""
    t = transposed if transposed is not None else (None, None, None, None)
    grads = _ops.sparse_attention_backward(query, key, value, out, grad_out, lse, row_indices,
                                           row_offsets, column_indices, *t, float(scale),
                                           float(p), rng_state, *(bool(x) for x in needs))
    return tuple(g if want else None for g, want in zip(grads, needs))


def sparse_attention_heads(query, key, value, row_indices, row_offsets, column_indices, scale,
                           out_dtype=None, with_lse=False, plan=None):
    """The fused attention on float16 / bfloat16 storage, operands as strided head views:
    [B, H, rows, 64] (e.g. ``x.unflatten(-1, (H, 64)).transpose(1, 2)`` of a [B, S, E]
    tensor -- no copy), [R, rows, 64] or [rows, 64].  Scores, weights and sums are float32;
    the result is stored as `out_dtype` (float32, or the operands' type by default) in a
    buffer laid out [B, rows, H, 64] for 4-D operands (the returned [B, H, rows, 64] view
    of it is a [B, S, E] context).  A call the kernel does not serve (head dimension other
    than 64, views not 16-byte aligned) is composed from the typed operators; ``with_lse``
    ([out, lse], lse float32 [.., rows]) needs a served call."""
    out_code = _half_code(query.dtype if out_dtype is None else out_dtype)
    outs = _ops.sparse_attention_heads(query, key, value, row_indices, row_offsets, column_indices,
                                       float(scale), out_code, bool(with_lse), plan)
    return outs if with_lse else outs[0]


def half_linear_rows_supported(out_features, in_features, seq, batch, nonzeros, values_dtype, tile_dtype):
    """Whether y [B, S, out] = x W^T (half_linear_rows) takes the matrix-core route."""
    from . import capi
    try:
        vt, tt = _half_code(values_dtype), _half_code(tile_dtype)
    except KeyError:
        return False
    if tt == 0:
        return False
    return bool(capi.lib().sputnik_hip_sparse_linear_half_rows_supported(
        int(out_features), int(in_features), int(seq), int(batch), int(nonzeros), vt, tt))


def half_linear_rows(out_features, image, values_dtype, x, out=None, out_dtype=None):
    """y [B, S, out] = x W^T from W's image (half_linear_image) and x [B, S, in] half, in row
    orientation (no layout pass), stored as `out_dtype` (x's type by default, or float32) --
    into `out` when given (a [B, S, out] view with a unit last stride, e.g. a column slice
    of a wider buffer).  None where the route does not serve the call (unaligned x)."""
    code = _half_code(x.dtype if out_dtype is None else out_dtype)
    y = _ops.half_linear_rows(int(out_features), image, _half_code(values_dtype), x, out, code)
    return None if y.numel() == 0 else y


_TYPE_CODES = None


def transpose_last2(x, dtype=None):
    """``x.transpose(-1, -2).contiguous()`` as one tiled HIP kernel: the layout
    pass in front of / behind every SparseLinear (modules/sparse_linear.py:89,
    modules/sparse_attention.py:108-126).  ``dtype`` (float32 / float16 /
    bfloat16) changes the storage type inside the same pass."""
    global _TYPE_CODES
    if dtype is None or dtype == x.dtype:
        return _ops.transpose_last2(x)
    if _TYPE_CODES is None:
        import torch
        _TYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    return _ops.transpose_last2_as(x, _TYPE_CODES[dtype])


def permute_last(values, permutation):
    """``values[..., permutation]`` for value arrays [nnz] / [R, nnz] sharing one
    int32 permutation (a static pattern's transposed order): one kernel, the
    permutation read once for all rows.  float32 out."""
    return _ops.permute_last(values, permutation)


# ---------------------------------------------------------------------------
# attention dropout (csrc/philox.h, sputnik_hip.h "Attention dropout"): entry e of replica r
# is kept iff Philox4x32-10 word e & 3 of counter (offset/4, e >> 2, r) under key seed is below
# floor((1 - p) 2^32); kept values are scaled by 1 / (1 - p).  Fresh draws come from the
# device's default generator (offset + 4 per call, as torch.nn.functional.dropout); every
# result carries the int64 [2] device tensor rng_state = {seed, offset} that replays it.
# ---------------------------------------------------------------------------
def check_dropout_p(p):
    """0 <= p < 1 as a float, else ValueError."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must lie in [0, 1), got {p}")
    return p


def sparse_dropout(values, p, rng_state=None):
    """out = values * keep * 1/(1-p) for a values array [nnz] or [R, width] (row r = replica
    r; rows may be strided; many-mask arrays at their full [R, max(nonzeros)] width) of
    float32 / float16 / bfloat16, in values' type.  -> (out, rng_state).  With `rng_state`
    given the mask is replayed from it and no generator state is consumed.  p = 0 is a copy
    that draws nothing: rng_state is then None (or the one given)."""
    p = check_dropout_p(p)
    out, state = _ops.sparse_dropout(values, p, rng_state)
    return out, state


def _lse(lse):
    return lse if lse is not None and lse.numel() > 0 else None


def sparse_attention_dropout(query, key, value, row_indices, row_offsets, column_indices, scale, p,
                             plan=None):
    """sparse_attention with dropout p (0 < p < 1) on the attention weights, one kernel.
    -> (out, lse, rng_state); lse (of the undropped scores) is None where the call is composed
    from the operators (SDDMM, scaled softmax, sparse_dropout, SpMM: head dimension other than
    64)."""
    out, lse, state = _ops.sparse_attention_dropout(query, key, value, row_indices, row_offsets,
                                                    column_indices, float(scale), float(p), plan)
    return out, _lse(lse), state


def sparse_attention_heads_dropout(query, key, value, row_indices, row_offsets, column_indices, scale,
                                   p, out_dtype=None, plan=None):
    """sparse_attention_heads with dropout p on the weights: r = b * heads + h.
    -> (out, lse, rng_state) as sparse_attention_dropout."""
    out_code = _half_code(query.dtype if out_dtype is None else out_dtype)
    out, lse, state = _ops.sparse_attention_heads_dropout(query, key, value, row_indices, row_offsets,
                                                          column_indices, float(scale), out_code,
                                                          float(p), plan)
    return out, _lse(lse), state


def sparse_attention_many_mask_dropout(b, nonzeros, row_indices, row_offsets, column_indices, query,
                                       key, value, scale, p, plan=None):
    """sparse_attention_many_mask with dropout p on the weights (e = position inside the mask).
    -> (out, lse, rng_state) as sparse_attention_dropout."""
    out, lse, state = _ops.sparse_attention_many_mask_dropout(int(b), _counts(nonzeros), query, key,
                                                              value, row_indices, row_offsets,
                                                              column_indices, float(scale), float(p),
                                                              plan)
    return out, _lse(lse), state


def sparse_attention_heads_many_mask_dropout(b, nonzeros, row_indices, row_offsets, column_indices,
                                             query, key, value, scale, p, out_dtype=None, plan=None):
    """sparse_attention_heads_many_mask with dropout p on the weights (r = b * heads + h).
    -> (out, lse, rng_state) as sparse_attention_dropout."""
    out_code = _half_code(query.dtype if out_dtype is None else out_dtype)
    out, lse, state = _ops.sparse_attention_heads_many_mask_dropout(
        int(b), _counts(nonzeros), query, key, value, row_indices, row_offsets, column_indices,
        float(scale), out_code, float(p), plan)
    return out, _lse(lse), state
