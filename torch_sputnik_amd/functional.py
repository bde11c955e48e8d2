"""autograd.Functions over the five ops, mirroring the reference's Python
layer: ``Spmm`` (modules/spmm.py:8-74), ``Sddmm`` (modules/sddmm.py:9-74),
``SparseLinearFunction`` (modules/sparse_linear.py:18-67).  Same ``apply``
signatures, same gradients returned in the same positions.

Beyond the reference:
  * 3-D (batched) backward works, because csr_transpose here accepts [R,nnz]
    values (the reference's is 1-D only, src/transpose_cuda.cu:50);
  * ``SparseSoftmax`` gives sparse_softmax a backward (the reference calls the
    raw op, modules/sparse_attention.py:76, which cuts the gradient);
  * the transposed topology of a static mask can be cached
    (``TransposeCache``), so a backward is one gather instead of a transpose.
"""
import collections

import torch

from . import ops
from .topology import diffsort, diffsort_many


def _identity(*tensors):
    """Key part naming these tensors' storage and contents: address, version
    counter (bumped by every in-place write through autograd-visible ops), size,
    dtype, device."""
    return tuple((t.data_ptr(), t._version, t.numel(), t.dtype, str(t.device)) for t in tensors)


def _storage_key(t):
    return (t.data_ptr(), t.numel(), t.dtype, str(t.device))


def _tensor_bytes(obj):
    if isinstance(obj, torch.Tensor):
        return obj.numel() * obj.element_size()
    if isinstance(obj, (tuple, list)):
        return sum(_tensor_bytes(o) for o in obj)
    return 0


# ---------------------------------------------------------------------------
# Static topologies.
#
# The caches below serve, by default, only index tensors that their OWNER has
# declared static (`register_static_topology`: SparseLinear.setup_sparse_tensors
# and SparseAttention do, for the patterns they create and never write to).  An
# arbitrary tensor handed to Spmm / Sddmm gets the reference's per-call behaviour
# (modules/spmm.py:59-64): nothing is remembered about it.
#
# A registration lives as long as the registered tensor object (weakref): when
# the owner drops it, the registration and every cache entry made for it go too,
# so a recycled address can never hit an old entry and no topology is pinned in
# memory by the cache alone.
#
# What the key cannot see: writes that bypass the version counter --
# `index.data.copy_(...)`, `set_`, a kernel or C-ABI call writing through the raw
# pointer.  Whoever does that to a registered topology calls
# `unregister_static_topology` / `clear_caches()` (or simply builds new tensors).
# ---------------------------------------------------------------------------
_static = {}        # storage key -> number of live registrations
_listeners = []     # caches to tell when a registration dies


def _drop_registration(key):
    left = _static.get(key, 0) - 1
    if left > 0:
        _static[key] = left
        return
    _static.pop(key, None)
    for cache in list(_listeners):
        cache.forget(key)


def register_static_topology(*tensors):
    """Declares index tensors (row_indices / row_offsets / column_indices) as
    static: transposed topologies and kernel plans derived from them are cached
    until the tensors are written to (in place) or die."""
    import weakref
    for t in tensors:
        key = _storage_key(t)
        _static[key] = _static.get(key, 0) + 1
        weakref.finalize(t, _drop_registration, key)
    return tensors


def unregister_static_topology(*tensors):
    for t in tensors:
        key = _storage_key(t)
        _static.pop(key, None)
        for cache in list(_listeners):
            cache.forget(key)


def _is_static(*tensors):
    return all(_storage_key(t) in _static for t in tensors)


class _Lru:
    """Bounded map: at most `capacity` entries and `max_bytes` of device memory
    (static topologies are few -- a model's layers and masks -- but a 4096^2
    pattern at density 0.1 comes to 27 MB of transposed indices and plan)."""

    def __init__(self, capacity, max_bytes=1 << 30):
        self.capacity = capacity
        self.max_bytes = max_bytes
        self.bytes = 0
        self._entries = collections.OrderedDict()   # key -> (entry, bytes, storage keys it was made for)

    def get(self, key):
        slot = self._entries.get(key)
        if slot is None:
            return None
        self._entries.move_to_end(key)
        return slot[0]

    def put(self, key, entry, made_for=()):
        size = _tensor_bytes(entry)
        old = self._entries.pop(key, None)
        if old is not None:
            self.bytes -= old[1]
        self._entries[key] = (entry, size, tuple(made_for))
        self.bytes += size
        while len(self._entries) > 1 and (len(self._entries) > self.capacity or self.bytes > self.max_bytes):
            _, (_, dropped, _) = self._entries.popitem(last=False)
            self.bytes -= dropped
        return entry

    def forget(self, storage_key):
        for key in [k for k, (_, _, made_for) in self._entries.items() if storage_key in made_for]:
            self.bytes -= self._entries.pop(key)[1]

    def clear(self):
        self._entries.clear()
        self.bytes = 0

    def __len__(self):
        return len(self._entries)


class _TopologyCache:
    """Common part of the two caches: whom they serve.  scope "static": index
    tensors registered with `register_static_topology` only (entries hold no
    reference to them: they die with their owner); scope "all": any tensor --
    the caller's promise that the index tensors it passes are not written to
    behind the version counter; entries then keep the tensors alive so that an
    address cannot be recycled under a live entry."""

    def __init__(self, capacity, scope):
        self.scope = scope
        self._entries = _Lru(capacity)
        _listeners.append(self)

    def serves(self, *tensors):
        return self.scope == "all" or _is_static(*tensors)

    def _keep(self, *tensors):
        return tensors if self.scope == "all" else ()

    def forget(self, storage_key):
        self._entries.forget(storage_key)

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)


class TransposeCache(_TopologyCache):
    """Memoises the transposed topology (and the value permutation) of static
    CSR patterns.  The reference re-runs csr_transpose + diffsort in every
    backward although the topology never changes (modules/spmm.py:59-64,
    modules/sddmm.py:60-65, modules/sparse_linear.py:52-57); with the cache a
    backward is one gather of the values through the stored permutation."""

    def __init__(self, capacity=128, scope="static"):
        super().__init__(capacity, scope)

    def lookup(self, m, n, row_offsets, column_indices, probe_values):
        """(row_indices_t, row_offsets_t, column_indices_t, permutation), cached
        when this cache serves the pattern, computed for this call otherwise."""
        cached = self.serves(row_offsets, column_indices)
        key = (m, n) + _identity(row_offsets, column_indices)
        entry = self._entries.get(key) if cached else None
        if entry is None:
            _, row_offsets_t, column_indices_t, permutation = ops.csr_transpose_with_permutation(
                m, n, probe_values.detach().reshape(-1, probe_values.shape[-1])[0].contiguous(),
                row_offsets, column_indices, checked=cached)   # the wait only for a result that is kept
            entry = (diffsort(row_offsets_t), row_offsets_t, column_indices_t,
                     permutation.contiguous()) + self._keep(row_offsets, column_indices)
            if cached:
                # the derived pattern is as static as the one it was made from: plans
                # for it (the transposed products of every backward) are cached too,
                # for as long as this entry holds its tensors
                register_static_topology(*entry[:3])
                self._entries.put(key, entry, (_storage_key(row_offsets), _storage_key(column_indices)))
        return entry[:4]


class PlanCache(_TopologyCache):
    """Memoises the topology-only pre-pass of the LDS-tiled kernels
    (ops.spmm_plan / ops.sddmm_plan) per static topology and operand width, so
    that training steps launch kernels only.  Every method returns None for a
    pattern this cache does not serve (the caller then takes the per-call op)."""

    def __init__(self, capacity=256, scope="static"):
        super().__init__(capacity, scope)

    def _plan(self, kind, shape, make, *index):
        if not self.serves(*index):
            return None
        key = (kind,) + shape + _identity(*index)
        entry = self._entries.get(key)
        if entry is None:
            entry = self._entries.put(key, (make(),) + self._keep(*index),
                                      tuple(_storage_key(t) for t in index))
        return entry[0]

    def spmm(self, m, k, n, row_indices, row_offsets, column_indices):
        return self._plan("spmm", (m, k, n),
                          lambda: ops.spmm_plan(m, k, n, row_indices, row_offsets, column_indices),
                          row_indices, row_offsets, column_indices)

    def sddmm(self, m, n, k, row_indices, row_offsets, column_indices, summed=False):
        return self._plan("sddmm_sum" if summed else "sddmm", (m, n, k),
                          lambda: (ops.sddmm_sum_plan if summed else ops.sddmm_plan)(
                              m, n, k, row_indices, row_offsets, column_indices),
                          row_indices, row_offsets, column_indices)

    def half_linear(self, m, k, row_offsets, column_indices):
        """Plan of the half-storage layer's weight gradient (ops.half_linear_plan)."""
        return self._plan("half_linear", (m, k),
                          lambda: ops.half_linear_plan(m, k, row_offsets, column_indices),
                          row_offsets, column_indices)

    def attention(self, m, n, d, row_indices, row_offsets, column_indices):
        return self._plan("attention", (m, n, d),
                          lambda: ops.sparse_attention_plan(m, n, d, row_indices, row_offsets,
                                                            column_indices),
                          row_indices, row_offsets, column_indices)

    def attention_many_mask(self, b, m, n, d, nonzeros, row_indices, row_offsets, column_indices):
        """Plan of the many-mask attention (ops.sparse_attention_many_mask_plan); `nonzeros` a
        host list / tensor, part of the key."""
        counts = tuple(int(c) for c in (nonzeros.tolist() if torch.is_tensor(nonzeros) else nonzeros))
        return self._plan("attention_many_mask", (b, m, n, d, counts),
                          lambda: ops.sparse_attention_many_mask_plan(b, m, n, d, counts, row_indices,
                                                                      row_offsets, column_indices),
                          row_indices, row_offsets, column_indices)


# Both caches exist by default with scope "static": they serve the patterns that
# modules register (see above) and nothing else.  `enable_*_cache(True)` widens
# a cache to every tensor (scope "all": the caller vouches for the tensors),
# `enable_*_cache(False)` gives the reference's per-call behaviour everywhere.
TRANSPOSE_CACHE_DEFAULT = "static"
PLAN_CACHE_DEFAULT = "static"


def _make_cache(cls, enabled):
    if not enabled:
        return None
    return cls(scope="all" if enabled is True or enabled == "all" else "static")


_cache = _make_cache(TransposeCache, TRANSPOSE_CACHE_DEFAULT)
_plans = _make_cache(PlanCache, PLAN_CACHE_DEFAULT)


def enable_transpose_cache(enabled=True):
    """False: off; "static" (the default): registered topologies only; True: all tensors."""
    global _cache
    if _cache is not None and _cache in _listeners:
        _listeners.remove(_cache)
    _cache = _make_cache(TransposeCache, enabled)
    return _cache


def enable_plan_cache(enabled=True):
    """False: off; "static" (the default): registered topologies only; True: all tensors."""
    global _plans
    if _plans is not None and _plans in _listeners:
        _listeners.remove(_plans)
    _plans = _make_cache(PlanCache, enabled)
    return _plans


def clear_caches():
    for cache in (_cache, _plans):
        if cache is not None:
            cache.clear()


def _contiguous(x):
    """``x.contiguous()``; a transposed view of a contiguous tensor (the gradient
    that reaches a module which returned ``out.transpose(1, 2)``,
    modules/sparse_attention.py:126) goes through the tiled transpose kernel
    instead of a strided elementwise copy (7 vs 23 us at config 3)."""
    if x.is_contiguous():
        return x
    if x.is_cuda and x.dim() >= 2 and x.dtype == torch.float32:
        view = x.transpose(-1, -2)
        if view.is_contiguous():
            return ops.transpose_last2(view)
    return x.contiguous()


def _as_transposed(x):
    """``x.transpose(-1, -2)`` as a contiguous tensor.  Free when `x` is itself the
    transposed view of a contiguous tensor -- how the Functions below hand each
    other gradients that a kernel's store phase already wrote in the layout the
    receiver needs (`transposed_grads`) -- and one tiled-transpose launch otherwise."""
    view = x.transpose(-1, -2)
    if view.is_contiguous():
        return view
    return ops.transpose_last2(_contiguous(x))


# From this many values on (several rows of them) a cached permutation goes
# through the LDS-banded kernel; its two index lists are made once per cached
# permutation and kept on the permutation tensor (the cache entry owns it).
BANDED_PERMUTE_FROM = 1 << 21


def _permute_cached(values, perm):
    """values[..., perm] for a permutation held by the transpose cache."""
    if values.dim() == 2 and values.size(0) > 1 and values.numel() >= BANDED_PERMUTE_FROM \
            and values.is_cuda:
        lists = getattr(perm, "_sputnik_banded_lists", None)
        if lists is None:
            lists = ops.banded_lists(perm)
            perm._sputnik_banded_lists = lists
        return ops.permute_last_banded(values, *lists)
    return ops.permute_last(values, perm)


def _spmm(m, k, values, row_indices, row_offsets, column_indices, dense, left=False, block_rows=0,
          permutation=None, blocks=0):
    """THE sparse x dense product of this layer: spmm, or left_spmm with ``left``;
    ``block_rows = d``: stored head split, [R * m/d, n, d] (ops.spmm_transposed_out);
    ``blocks = d``: the same buffer handed back as its transposed VIEW, [R * m/d, d, n];
    ``permutation``: the values are in another order of the entries (ops.spmm_permuted).
    The plan of a static topology is looked up here and nowhere else; which kernel serves the
    call, and every fallback, is the binding's business."""
    plan = None if _plans is None else _plans.spmm(m, k, dense.size(-1), row_indices, row_offsets,
                                                   column_indices)
    if block_rows or blocks:
        out = ops.spmm_transposed_out(m, k, values, row_indices, row_offsets, column_indices, dense,
                                      block_rows or blocks, permutation=permutation, plan=plan, left=left)
        return out.transpose(1, 2) if blocks else out
    if permutation is not None:
        return ops.spmm_permuted(m, k, values, permutation, row_indices, row_offsets,
                                 column_indices, dense, plan, left=left)
    if plan is None:
        return (ops.left_spmm if left else ops.spmm)(m, k, values, row_indices, row_offsets,
                                                     column_indices, dense)
    return (ops.left_spmm_planned if left else ops.spmm_planned)(
        m, k, values, row_indices, row_offsets, column_indices, dense, plan)


def _linear(m, k, values, row_indices, row_offsets, column_indices, dense, split_rows=0):
    """left_spmm, optionally with the head-split store."""
    return _spmm(m, k, values, row_indices, row_offsets, column_indices, dense, left=True,
                 block_rows=split_rows)


def _transposed(m, n, values, row_offsets, column_indices, width=None):
    """The transposed topology of the m x n pattern and the values that go with it:
    (values, permutation, row_indices_t, row_offsets_t, column_indices_t).  Where the transpose
    cache serves the pattern the transpose is the cached one and the values are gathered
    through its permutation -- inside the product's kernel where that serves a dense operand
    of ``width`` columns (ops.spmm_permuted_fused: the values come back in A's order WITH the
    permutation), else here (permutation None).  A pattern no cache serves takes the
    reference's per-call csr_transpose (modules/spmm.py:59-62; asynchronous, one pass).
    (The attention backwards and the group's input gradient ask another question -- "is the
    cache ON": they need the permutation itself, served pattern or not -- `_transposed_topology`.)"""
    values = values.contiguous()
    if _cache is not None and _cache.serves(row_offsets, column_indices):
        row_indices_t, row_offsets_t, column_indices_t, perm = _cache.lookup(
            m, n, row_offsets, column_indices, values)
        if width is not None and ops.spmm_permuted_fused(n, m, width, perm.numel()):
            return values, perm, row_indices_t, row_offsets_t, column_indices_t
        return _permute_cached(values, perm), None, row_indices_t, row_offsets_t, column_indices_t
    values_t, row_offsets_t, column_indices_t = ops.csr_transpose(
        m, n, values, row_offsets, column_indices)
    return values_t, None, diffsort(row_offsets_t), row_offsets_t, column_indices_t


def _spmm_transposed(m, n, values, row_offsets, column_indices, dense, left=False, blocks=0):
    """(A^T) @ dense for the m x n CSR matrix A, [R, n, width]; ``blocks = d``: as the
    transposed view of the head-split buffer the kernel wrote (`_spmm`), [R * n/d, d, width]."""
    values_t, perm, *topology_t = _transposed(m, n, values, row_offsets, column_indices,
                                              width=dense.size(-1))
    return _spmm(n, m, values_t, *topology_t, dense, left=left, permutation=perm, blocks=blocks)


def _incoming(grad_output, m=0, split_rows=0):
    """The gradient of a product as the backward products read it: contiguous [..., m, n]; with
    ``split_rows`` from the head-split [B * m/d, n, d] form (free where it arrives as the
    transposed view of a buffer a kernel wrote that way)."""
    if split_rows:
        return _as_transposed(grad_output).reshape(-1, m, grad_output.size(-2))
    return _contiguous(grad_output)


def _sddmm(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix,
           sum_replicas=False):
    plan = None if _plans is None else _plans.sddmm(m, n, lhs_matrix.size(-1), row_indices,
                                                    row_offsets, column_indices, summed=sum_replicas)
    if plan is None:
        return (ops.sddmm_sum if sum_replicas else ops.sddmm)(
            m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix)
    return (ops.sddmm_sum_planned if sum_replicas else ops.sddmm_planned)(
        m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix, plan)


def _attention_forward(query, key, value, row_indices, row_offsets, column_indices, scale, p=0.0,
                       want_lse=False):
    """Fused attention forward -> (out, lse or None, rng_state or None), as every private
    forward helper of the attention layouts below returns: `rng_state` is None at p == 0.
    `want_lse` (the fused backward) takes the row-group forward where it serves (head
    dimension 128, ops.sparse_attention_rows: no plan); without it that shape stays on the
    plain op.  Else through the cached plan of the mask when enabled: the dropout op for
    p > 0, the lse ops for `want_lse`, or the plain ones."""
    operands = (query, key, value, row_indices, row_offsets, column_indices, scale)
    if want_lse and ops.sparse_attention_rows_supported(query.size(-2), key.size(-2), query.size(-1),
                                                        column_indices.numel()):
        return ops.sparse_attention_rows(*operands, p)
    plan = None if _plans is None else _plans.attention(query.size(-2), key.size(-2), query.size(-1),
                                                        row_indices, row_offsets, column_indices)
    if p > 0.0:
        return ops.sparse_attention_dropout(*operands, p, plan)
    if want_lse:
        out, lse = (ops.sparse_attention_with_lse(*operands) if plan is None
                    else ops.sparse_attention_with_lse_planned(*operands, plan))
        return out, lse, None
    out = (ops.sparse_attention(*operands) if plan is None
           else ops.sparse_attention_planned(*operands, plan))
    return out, None, None


# ---------------------------------------------------------------------------
# Attention dropout (ops.sparse_dropout, csrc/philox.h): the keep decision of entry e of
# replica r is a function of (seed, offset, r, e) alone, so the fused forward, the composed
# chain and the backward's replay from the saved rng_state drop the same entries.
# ---------------------------------------------------------------------------
def _replay(values, p, rng_state):
    """values * keep * 1/(1-p) with the mask of `rng_state` (no generator state consumed)."""
    return ops.sparse_dropout(values, p, rng_state)[0]


class SparseDropout(torch.autograd.Function):
    """Dropout on a sparse values array ([nnz] or [R, width], row r = replica r) with the
    library's counter-based mask; the backward replays the mask from the saved rng_state:
    grad * keep * 1/(1-p).  ``apply(values, p)``."""

    @staticmethod
    def forward(ctx, values, p):
        out, rng_state = ops.sparse_dropout(values, p)
        ctx.p = float(p)
        ctx.save_for_backward(rng_state)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        rng_state, = ctx.saved_tensors
        return _replay(_contiguous(grad_output), ctx.p, rng_state), None


def sparse_dropout(values, p, training=True):
    """Differentiable dropout of a sparse values array (ops.sparse_dropout): identity when
    not `training` or p == 0 (nothing drawn then); ValueError for p outside [0, 1)."""
    p = ops.check_dropout_p(p)
    if not training or p == 0.0:
        return values
    if torch.is_grad_enabled() and values.requires_grad:
        return SparseDropout.apply(values, p)
    return ops.sparse_dropout(values, p)[0]


class TransposeLast2(torch.autograd.Function):
    """``x.transpose(-1, -2).contiguous()`` as one tiled kernel (ops.transpose_last2):
    the layout pass of modules/sparse_linear.py:89 and
    modules/sparse_attention.py:108-126, optionally widening half-precision
    storage to float32 on the way.  Its gradient is the same operation (narrowing
    back to the input's storage type inside the pass)."""

    @staticmethod
    def forward(ctx, x, dtype=None):
        ctx.in_dtype = x.dtype
        return ops.transpose_last2(x, dtype)

    @staticmethod
    def backward(ctx, grad_output):
        return ops.transpose_last2(grad_output, ctx.in_dtype), None


def transpose_last2(x, dtype=None):
    """Differentiable ``x.transpose(-1, -2).contiguous()`` (``.to(dtype)``)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return TransposeLast2.apply(x, dtype)
    return ops.transpose_last2(x, dtype)


def _to_operand(x):
    """[B, S, in] -> the k-major float32 operand [B, in, S] of left_spmm.  The
    operators compute and return float32 whatever the storage type
    (src/spmm_cuda.cu:42); half-precision activations are widened inside this
    pass instead of in one of their own."""
    return transpose_last2(x, torch.float32 if x.dtype in (torch.float16, torch.bfloat16) else None)


class Spmm(torch.autograd.Function):
    """sparse(values, CSR topology) @ dense.  ``apply(m, k, values, row_indices,
    row_offsets, column_indices, dense[, transposed_out[, transposed_grads]])``; with
    ``transposed_out`` the product comes back transposed, [R, n, m] (written in that
    order by the kernel's store phase, ops.spmm_transposed_out: SparseAttention's
    head merge).  ``transposed_grads``: the gradient of `dense` is handed back as
    the transposed VIEW of a buffer the kernel wrote transposed (same shape and
    values; free for a receiver that wants that layout, see `_as_transposed`)."""

    @staticmethod
    def forward(ctx, m, k, values, row_indices, row_offsets, column_indices, dense,
                transposed_out=False, transposed_grads=False):
        ctx.shape = (m, k)
        ctx.topology = (row_indices, row_offsets, column_indices)
        ctx.transposed_out = bool(transposed_out)
        ctx.transposed_grads = bool(transposed_grads)
        ctx.save_for_backward(values, dense)
        return _spmm(m, k, values, row_indices, row_offsets, column_indices, dense,
                     block_rows=m if transposed_out else 0)

    @staticmethod
    def backward(ctx, grad_output):
        m, k = ctx.shape
        row_indices, row_offsets, column_indices = ctx.topology
        values, dense = ctx.saved_tensors
        grad_output = _incoming(grad_output, m, ctx.transposed_out)   # [R, n, m] -> the product's own layout
        if ctx.transposed_out and dense.dim() == 2:
            grad_output = grad_output[0]
        grad_values = grad_dense = None
        if ctx.needs_input_grad[2]:
            # dL/dA sampled at the pattern: <dC[i,:], B[j,:]>
            grad_values = _sddmm(m, k, row_indices, row_offsets, column_indices, grad_output,
                                 dense.contiguous())
        if ctx.needs_input_grad[6]:
            # dL/dB = A^T @ dC
            grad_dense = _spmm_transposed(m, k, values, row_offsets, column_indices, grad_output,
                                          blocks=k if ctx.transposed_grads and dense.dim() == 3 else 0)
        return None, None, grad_values, None, None, None, grad_dense, None, None


class Sddmm(torch.autograd.Function):
    """(lhs @ rhs^T) sampled at a CSR mask.  ``apply(m, n, row_indices,
    row_offsets, column_indices, lhs_matrix, rhs_matrix[, transposed_grads])``;
    ``transposed_grads`` as in `Spmm` (both gradients, 3-D operands)."""

    @staticmethod
    def forward(ctx, m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix,
                transposed_grads=False):
        ctx.shape = (m, n)
        ctx.topology = (row_indices, row_offsets, column_indices)
        ctx.transposed_grads = bool(transposed_grads) and lhs_matrix.dim() == 3
        ctx.save_for_backward(lhs_matrix, rhs_matrix)
        return _sddmm(m, n, row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix)

    @staticmethod
    def backward(ctx, grad_output):
        m, n = ctx.shape
        row_indices, row_offsets, column_indices = ctx.topology
        lhs_matrix, rhs_matrix = ctx.saved_tensors
        grad_output = _contiguous(grad_output)
        grad_lhs = grad_rhs = None
        if ctx.needs_input_grad[5]:
            # dL/dlhs = dS @ rhs, dS sparse with the mask's pattern
            grad_lhs = _spmm(m, n, grad_output, row_indices, row_offsets, column_indices,
                             rhs_matrix.contiguous(), blocks=m if ctx.transposed_grads else 0)
        if ctx.needs_input_grad[6]:
            # dL/drhs = dS^T @ lhs
            grad_rhs = _spmm_transposed(m, n, grad_output, row_offsets, column_indices,
                                        lhs_matrix.contiguous(), blocks=n if ctx.transposed_grads else 0)
        return None, None, None, None, None, grad_lhs, grad_rhs, None


def _armed(sink):
    """The layer a Function was handed as ``dense_grad_sink`` if it collects the dense weight
    gradient NOW -- asked when the backward runs, so arming between forward and backward
    counts -- else None."""
    return sink if sink is not None and getattr(sink, "_collects_dense_grad", False) else None


def _collect_dense_grad(sink, dense):
    """Adds one backward's dense weight gradient [out, in] into ``sink.dense_grad`` the way
    autograd fills ``.grad``: the first one is kept as the kernel wrote it, later ones are
    added in place (micro-batches, a layer used twice in one graph)."""
    with torch.no_grad():
        if sink.dense_grad is None:
            sink.dense_grad = dense
        else:
            sink.dense_grad.add_(dense)


def _sink_dense(ctx, grad_output, operand, layout):
    """While the layer behind ``ctx.dense_grad_sink`` is armed: one ops.dense_weight_grad launch on
    dy [B, out, S] and the kept operand (``layout`` "bis" / "bsi"), added into its ``dense_grad``."""
    sink = _armed(ctx.dense_grad_sink)
    if sink is not None:
        _collect_dense_grad(sink, ops.dense_weight_grad(grad_output, operand, layout))


class SparseLinearFunction(torch.autograd.Function):
    """One sparse weight x a batch of dense matrices (left_spmm).  ``apply(m, k,
    values, row_indices, row_offsets, column_indices, dense[, split_rows[,
    dense_blocks[, dense_grad_sink]]])`` with dense [B,k,n] -> [B,m,n]; with ``split_rows = d`` the
    product comes back head split, [B * m/d, n, d] (every block of d output rows
    transposed, written by the kernel's store phase:
    modules/sparse_attention.py:38-45,108-126).  ``dense_blocks = d``: `dense` is
    given as [B * k/d, d, n] (the same memory: merged heads) and its gradient is
    handed back in that shape as the transposed view of a head-split buffer the
    kernel wrote (see `Spmm`, ``transposed_grads``).  ``dense_grad_sink`` (the
    ``SparseLinear``, or None): while it is armed the backward also adds the DENSE weight gradient
    ``sum_b dy_b dense_b^T`` [m, k] into ``sink.dense_grad`` (ops.dense_weight_grad on the
    normalised [B, m, n] / [B, k, n] forms: one tile launch, no layout copy)."""

    @staticmethod
    def forward(ctx, m, k, values, row_indices, row_offsets, column_indices, dense,
                split_rows=0, dense_blocks=0, dense_grad_sink=None):
        ctx.dense_grad_sink = dense_grad_sink
        ctx.shape = (m, k)
        ctx.topology = (row_indices, row_offsets, column_indices)
        ctx.split_rows = int(split_rows)
        ctx.dense_blocks = int(dense_blocks)
        if dense_blocks:
            dense = dense.reshape(-1, k, dense.size(-1))
        ctx.save_for_backward(values, dense)
        return _linear(m, k, values, row_indices, row_offsets, column_indices, dense, split_rows)

    @staticmethod
    def backward(ctx, grad_output):
        m, k = ctx.shape
        row_indices, row_offsets, column_indices = ctx.topology
        values, dense = ctx.saved_tensors
        grad_output = _incoming(grad_output, m, ctx.split_rows)   # [B * m/d, n, d] -> [B, m, n]
        grad_values = grad_dense = None
        _sink_dense(ctx, grad_output, dense, "bis")
        if ctx.needs_input_grad[2]:
            # the [B,nnz] products summed over B (what autograd makes of the
            # reference's result for the shared `values`), inside the call
            grad_values = _sddmm(m, k, row_indices, row_offsets, column_indices, grad_output,
                                 dense.contiguous(), sum_replicas=True)
        if ctx.needs_input_grad[6]:
            grad_dense = _spmm_transposed(m, k, values, row_offsets, column_indices, grad_output,
                                          left=True, blocks=ctx.dense_blocks)
            if not ctx.dense_blocks and dense.dim() == 2:
                grad_dense = grad_dense[0]
        return None, None, grad_values, None, None, None, grad_dense, None, None, None


def _half_input_gradient(m, k, values, row_offsets, column_indices, image, x, grad, planes, plain_grad):
    """dx [B, S, in] of the half layer's tile routes from dy [B, out, S] (``grad``: in x's type, or
    its half planes) and the weight's image; where that launch does not serve (bfloat16 tiles with
    float32 values AND a float32 dy) W^T dy on ``plain_grad`` and the layout pass back to x's type."""
    grad_x = ops.half_linear_input_gradient(m, k, grad, planes, image, values.dtype, x, x.size(0), x.size(1))
    if grad_x is None:
        grad_dense = _spmm_transposed(m, k, values, row_offsets, column_indices, plain_grad, left=True)
        grad_x = ops.transpose_last2(grad_dense, x.dtype)
    return grad_x


class HalfSparseLinearFunction(torch.autograd.Function):
    """``SparseLinear.forward`` for activations stored in float16 / bfloat16 (BASELINE
    config 5; the reference knows float32 only, src/left_replicated_spmm.cu:34-38):
    ``apply(m, k, values, row_indices, row_offsets, column_indices, x[, dense_grad_sink])``
    with x [B, S, in] -> [B, out, S] float32.

    At a layer's density and size all three products run on the matrix cores and read
    their operands as the caller has them -- NO layout pass (csrc/sparse_linear_half.hip):
    the weight as one densified image (made in the forward pass, kept for the backward),
    x [B, S, in], dy [B, out, S]; float32 values and the float32 dy enter as half planes
    whose sum is the value (float16: over the tensor's range, 22 bits down to 2^-28 of its
    largest finite magnitude; inf / NaN stay non-finite).  Elsewhere the typed operators with the layout passes of
    modules/sparse_linear.py:89 inside the Function (the half operand is what is kept).

    ``dense_grad_sink`` (the ``SparseLinear``, or None): while it is armed the backward also adds the dense
    weight gradient into ``sink.dense_grad``.  On the tile route it is the weight gradient's
    own launch that stores it (ops.half_linear_weight_gradient_dense: the tiles it samples,
    stored whole); elsewhere one ops.dense_weight_grad launch on dy and the kept operand."""

    @staticmethod
    def forward(ctx, m, k, values, row_indices, row_offsets, column_indices, x, dense_grad_sink=None):
        ctx.dense_grad_sink = dense_grad_sink
        ctx.shape = (m, k)
        ctx.topology = (row_indices, row_offsets, column_indices)
        ctx.in_dtype = x.dtype
        batch, seq = x.size(0), x.size(1)
        ctx.tiles = x.is_cuda and ops.half_linear_supported(m, k, seq, batch, column_indices.numel(),
                                                            values.dtype, x.dtype)
        if ctx.tiles:
            x = x.contiguous()
            image = ops.half_linear_image(m, k, values, row_offsets, column_indices, x.dtype)
            ctx.save_for_backward(values, x, image)
            return ops.half_linear_forward(m, image, values.dtype, x)
        dense = ops.transpose_last2(x)
        ctx.save_for_backward(values, dense)
        return _linear(m, k, values, row_indices, row_offsets, column_indices, dense)

    @staticmethod
    def backward(ctx, grad_output):
        m, k = ctx.shape
        row_indices, row_offsets, column_indices = ctx.topology
        grad_output = _incoming(grad_output)
        grad_values = grad_x = None
        if ctx.tiles:
            values, x, image = ctx.saved_tensors
            # dy as planes, once for both gradients (float32 dy), or as it is (dy in x's type)
            planes = grad_output.dtype == torch.float32
            grad = ops.half_planes(grad_output, x.dtype) if planes else grad_output.to(x.dtype)
            sink = _armed(ctx.dense_grad_sink)
            if ctx.needs_input_grad[2]:
                plan = None if _plans is None else _plans.half_linear(m, k, row_offsets, column_indices)
                if sink is None:
                    grad_values = ops.half_linear_weight_gradient(m, row_offsets, column_indices, grad,
                                                                  planes, x, plan)
                else:
                    grad_values, dense_grad = ops.half_linear_weight_gradient_dense(
                        m, row_offsets, column_indices, grad, planes, x, plan)
                    _collect_dense_grad(sink, dense_grad)
            else:   # (frozen values: nothing is sampled)
                _sink_dense(ctx, grad_output, x, "bsi")
            if ctx.needs_input_grad[6]:
                grad_x = _half_input_gradient(m, k, values, row_offsets, column_indices, image, x, grad,
                                              planes, grad_output)
            return None, None, grad_values, None, None, None, grad_x, None
        values, dense = ctx.saved_tensors
        _sink_dense(ctx, grad_output, dense, "bis")
        if ctx.needs_input_grad[2]:
            grad_values = _sddmm(m, k, row_indices, row_offsets, column_indices, grad_output, dense,
                                 sum_replicas=True)
        if ctx.needs_input_grad[6]:
            grad_dense = None
            if grad_output.dim() == 3:
                # W^T dy as a dense contraction on half tiles where that route serves the
                # shape (the float32 gradient enters as half planes over its range)
                values_t, _, _, row_offsets_t, column_indices_t = _transposed(
                    m, k, values, row_offsets, column_indices)
                grad_dense = ops.left_spmm_half_tiles(k, m, values_t, row_offsets_t, column_indices_t,
                                                      grad_output, ctx.in_dtype)
            if grad_dense is None:
                grad_dense = _spmm_transposed(m, k, values, row_offsets, column_indices, grad_output,
                                              left=True)
            grad_x = ops.transpose_last2(grad_dense, ctx.in_dtype)
        return None, None, grad_values, None, None, None, grad_x, None


class GroupProjectionFunction(torch.autograd.Function):
    """Several SparseLinear weights of one shape applied to ONE input in one launch
    (ops.left_spmm_group): the q, k and v projections of a self-attention block,
    which the reference runs one after the other (modules/sparse_attention.py:108-110).
    ``apply(m, k, split_rows, dense, values_0, row_indices_0, row_offsets_0,
    column_indices_0, values_1, ...)`` -> one product per weight ([B, m, n], or head
    split [B * m/d, n, d] with ``split_rows = d``).  The backward runs one summed
    SDDMM per weight and ONE launch for the input gradient  sum_w W_w^T dY_w
    (ops.left_spmm_group_sum: accumulated in registers, no partial results)."""

    @staticmethod
    def forward(ctx, m, k, split_rows, dense, *flat):
        values, ris, ros, cis = flat[0::4], flat[1::4], flat[2::4], flat[3::4]
        ctx.shape = (m, k, int(split_rows))
        ctx.topologies = list(zip(ris, ros, cis))
        ctx.save_for_backward(dense, *values)
        return tuple(ops.left_spmm_group(m, k, values, ris, ros, cis, dense, split_rows))

    @staticmethod
    def backward(ctx, *grads):
        m, k, split_rows = ctx.shape
        dense, *values = ctx.saved_tensors
        live, grad_ys = [], []
        for w, g in enumerate(grads):
            if g is None:
                continue
            live.append(w)
            grad_ys.append(_incoming(g, m, split_rows))   # [B * m/d, n, d] -> [B, m, n]
        grad_values = [None] * len(values)
        wanted = [(w, g) for w, g in zip(live, grad_ys) if ctx.needs_input_grad[4 + 4 * w]]
        grouped = (_plans is not None and 2 <= len(wanted) <= 4 and dense.dim() == 3 and dense.is_cuda
                   and dense.dtype == torch.float32 and all(g.dtype == torch.float32 for _, g in wanted))
        if grouped:   # one call: every weight's partial sums added by ONE launch
            topo = [ctx.topologies[w] for w, _ in wanted]
            plans = [_plans.sddmm(m, k, dense.size(-1), *t, summed=True) for t in topo]
            grouped = all(p is not None for p in plans)
        if grouped:
            outs = ops.sddmm_sum_group_planned(m, k, [t[0] for t in topo], [t[1] for t in topo],
                                               [t[2] for t in topo], [g for _, g in wanted], dense, plans)
            for (w, _), out in zip(wanted, outs):
                grad_values[w] = out
        else:
            for w, g in wanted:
                ri, ro, ci = ctx.topologies[w]
                grad_values[w] = _sddmm(m, k, ri, ro, ci, g, dense, sum_replicas=True)
        grad_dense = None
        if ctx.needs_input_grad[3] and live:
            if _cache is not None:
                vals, perms, ris_t, ros_t, cis_t = [], [], [], [], []
                for w in live:
                    _, ro, ci = ctx.topologies[w]
                    ri_t, ro_t, ci_t, perm = _cache.lookup(m, k, ro, ci, values[w])
                    vals.append(values[w]); perms.append(perm)
                    ris_t.append(ri_t); ros_t.append(ro_t); cis_t.append(ci_t)
                grad_dense = ops.left_spmm_group_sum(k, m, vals, perms, ris_t, ros_t, cis_t,
                                                     grad_ys)
            else:
                for w, g in zip(live, grad_ys):
                    _, ro, ci = ctx.topologies[w]
                    part = _spmm_transposed(m, k, values[w], ro, ci, g, left=True)
                    grad_dense = part if grad_dense is None else grad_dense + part
        flat = []
        for gv in grad_values:
            flat += [gv, None, None, None]
        return (None, None, None, grad_dense, *flat)


class SparseSoftmax(torch.autograd.Function):
    """sparse_softmax with a gradient: dX = scale * Y * (dY - rowsum(dY * Y)), the
    row sums taken over the stored entries (extension).
    ``apply(values, row_indices, row_offsets, column_indices[, scale])`` computes
    softmax(scale * values)."""

    @staticmethod
    def forward(ctx, values, row_indices, row_offsets, column_indices, scale=1.0):
        if scale == 1.0:
            out = ops.sparse_softmax(values, row_indices, row_offsets, column_indices)
        else:
            out = ops.sparse_softmax_scaled(values, row_indices, row_offsets, column_indices,
                                            scale)
        ctx.scale = float(scale)
        ctx.save_for_backward(out, row_offsets)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        out, row_offsets = ctx.saved_tensors
        grad_values = ops.sparse_softmax_backward(out, grad_output.contiguous(), row_offsets,
                                                  ctx.scale)
        return grad_values, None, None, None, None


def _transposed_topology(m, n, row_offsets, column_indices, probe_values):
    """(row_indices_t, row_offsets_t, column_indices_t, permutation) of the mask, for both
    attention backwards: from the transpose cache, or one csr_transpose_with_permutation when
    the cache is off.  `probe_values`: [..., nnz] values whose first row the transpose carries
    along when it runs (its result is not used).  A mask without entries has the empty
    transpose, built here (the transpose and the cache take a row of values, which an empty
    mask does not have)."""
    if column_indices.numel() == 0:
        index = dict(dtype=torch.int32, device=row_offsets.device)
        return (torch.arange(n, **index), torch.zeros(n + 1, **index),
                torch.empty(0, **index), torch.empty(0, **index))
    if _cache is not None:
        return _cache.lookup(m, n, row_offsets, column_indices, probe_values)
    _, row_offsets_t, column_indices_t, perm = ops.csr_transpose_with_permutation(
        m, n, probe_values.reshape(-1, probe_values.shape[-1])[0].contiguous(),
        row_offsets, column_indices, checked=False)
    return diffsort(row_offsets_t), row_offsets_t, column_indices_t, perm


# ---------------------------------------------------------------------------
# The recomputing backward.  Four Functions share it (SparseAttentionFunction, ...Heads...,
# ...ManyMask..., ...HeadsManyMask...): each saves (query, key, value, *topo, rng_state),
# brings its operands to contiguous [R, S, D] and runs `_attention_backward` on the operator
# family of its mask layout.
# ---------------------------------------------------------------------------
_Operators = collections.namedtuple(
    "_Operators", "sddmm softmax softmax_backward spmm transposed_products")


def _single_mask_operators(topo, m, n):
    """The operators of one m x n mask for `_attention_backward`: plan-cached sddmm / spmm,
    and the transposed products through the mask's transposed topology (one csr_transpose
    with permutation per call, or the cached one), gathered inside ops.spmm_permuted where
    that serves."""
    _, row_offsets, column_indices = topo

    def transposed_products(grad_scores, kept, query, grad_output, needs_key, needs_value):
        row_indices_t, row_offsets_t, column_indices_t, perm = _transposed_topology(
            m, n, row_offsets, column_indices, grad_scores)

        def product(values, dense):
            if ops.spmm_permuted_fused(n, m, dense.size(-1), perm.numel()):
                return ops.spmm_permuted(n, m, values, perm, row_indices_t, row_offsets_t,
                                         column_indices_t, dense)
            values_t = (_permute_cached(values, perm) if _cache is not None
                        else ops.permute_last(values, perm))
            return _spmm(n, m, values_t, row_indices_t, row_offsets_t, column_indices_t, dense)

        return (product(grad_scores, query) if needs_key else None,
                product(kept, grad_output) if needs_value else None)

    return _Operators(
        sddmm=lambda lhs, rhs: _sddmm(m, n, *topo, lhs, rhs),
        softmax=lambda scores, scale: ops.sparse_softmax_scaled(scores, *topo, scale),
        softmax_backward=lambda weights, grad, scale: ops.sparse_softmax_backward(
            weights, grad, row_offsets, scale),
        spmm=lambda values, dense: _spmm(m, n, values, *topo, dense),
        transposed_products=transposed_products)


def _attention_backward(operators, query, key, value, scale, grad_output, needs, dropout=None):
    """Gradients of softmax(scale * sddmm(q, k)) @ v for contiguous [R, S, D] operands on one
    operator family (`_single_mask_operators`: float32 or one half type, the typed operators
    with float32 scores, weights and gradients; `_many_mask_operators`: float32): the scores
    and weights are recomputed, then

        dV = P^T dO          dP = sddmm(dO, v)
        dS = softmax'(P, dP) (the softmax backward, carries the scale)
        dQ = dS k            dK = dS^T q

    on the mask and, when dK or dV is wanted, its transpose.  `needs`: which of (dQ, dK, dV)
    to compute.  `dropout` = (p, rng_state) of a forward with attention dropout: the mask is
    replayed, Pd = drop(P), dV = Pd^T dO, dP = drop(sddmm(dO, v)), and the rest is unchanged."""
    scores = operators.sddmm(query, key)
    weights = operators.softmax(scores, scale)
    grad_weights = operators.sddmm(grad_output, value)
    kept = weights
    if dropout is not None:
        kept = _replay(weights, *dropout)
        grad_weights = _replay(grad_weights, *dropout)
    grad_scores = operators.softmax_backward(weights, grad_weights, scale)
    grad_query = grad_key = grad_value = None
    if needs[0]:
        grad_query = operators.spmm(grad_scores, key)
    if needs[1] or needs[2]:
        grad_key, grad_value = operators.transposed_products(grad_scores, kept, query, grad_output,
                                                             needs[1], needs[2])
    return grad_query, grad_key, grad_value


def _saved(ctx):
    """(query, key, value, topo, dropout) of a recomputing Function's backward; `dropout` is
    (p, rng_state), or None for a forward without dropout (which saved rng_state = None)."""
    query, key, value, row_indices, row_offsets, column_indices, rng_state = ctx.saved_tensors
    dropout = (ctx.p, rng_state) if ctx.p > 0.0 else None
    return query, key, value, (row_indices, row_offsets, column_indices), dropout


class SparseAttentionFunction(torch.autograd.Function):
    """softmax(scale * sddmm(q, k)) @ v with the ONE-kernel forward
    (ops.sparse_attention) and a backward built from the separate operators
    (`_attention_backward`).  Nothing of size [R, nnz] is kept between the passes: the
    backward recomputes the weights (sddmm + scaled softmax) before it runs the chain.
    ``dropout_p`` > 0: dropout on the weights in the fused forward
    (ops.sparse_attention_dropout), replayed by the backward from the saved rng_state."""

    @staticmethod
    def forward(ctx, query, key, value, row_indices, row_offsets, column_indices, scale,
                dropout_p=0.0):
        ctx.scale, ctx.p = float(scale), float(dropout_p)
        out, _, rng_state = _attention_forward(query, key, value, row_indices, row_offsets,
                                               column_indices, scale, ctx.p)
        ctx.save_for_backward(query, key, value, row_indices, row_offsets, column_indices, rng_state)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        query, key, value, topo, dropout = _saved(ctx)
        grads = _attention_backward(
            _single_mask_operators(topo, query.size(-2), key.size(-2)), query, key, value,
            ctx.scale, _contiguous(grad_output), ctx.needs_input_grad[:3], dropout)
        return (*grads, None, None, None, None, None)


# ---------------------------------------------------------------------------
# Fused backward (ops.sparse_attention_backward): the forward keeps its output
# and row log-sum-exp, the backward runs two kernels over the mask and its cached transpose.
# ---------------------------------------------------------------------------
def fused_backward_served(query, key, column_indices):
    """Whether a fused forward and the fused backward both serve these operands: float32 on
    the GPU, a mask with entries, offsets within 32 bits, and head dimension 64 (the LDS-staged
    forward) or 128 (the row-group forward, ops.sparse_attention_rows).  Elsewhere
    ``fused_backward=True`` trains on SparseAttentionFunction, as without the flag."""
    m, n, d, nnz = query.size(-2), key.size(-2), query.size(-1), column_indices.numel()
    return (query.dtype == torch.float32 and key.dtype == torch.float32 and query.is_cuda
            and ops.sparse_attention_backward_supported(m, n, d, nnz)
            and (ops.sparse_attention_supported(m, n, d, nnz)
                 or ops.sparse_attention_rows_supported(m, n, d, nnz)))


class FusedBackwardAttentionFunction(torch.autograd.Function):
    """softmax(scale * sddmm(q, k)) @ v with a one-kernel forward (ops.sparse_attention* at
    head dimension 64, ops.sparse_attention_rows at 128; keeping its output O and row
    log-sum-exp) and the fused backward (ops.sparse_attention_backward): with
    D_i = dO_i . O_i, per entry p = exp(scale q_i.k_j - lse_i), ds = p (dp - D_i) scale,
    dQ += ds k, dK += ds q, dV += p dO -- two kernels over the mask and its (cached)
    transpose, nothing of size [R, nnz] at any time.  ``dropout_p`` > 0: the forward's
    dropout, replayed from the saved rng_state."""

    @staticmethod
    def forward(ctx, query, key, value, row_indices, row_offsets, column_indices, scale,
                dropout_p=0.0):
        ctx.scale, ctx.p = float(scale), float(dropout_p)
        out, lse, rng_state = _attention_forward(query, key, value, row_indices, row_offsets,
                                                 column_indices, scale, ctx.p, want_lse=True)
        ctx.save_for_backward(query, key, value, out, lse, row_indices, row_offsets,
                              column_indices, rng_state)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        query, key, value, out, lse, row_indices, row_offsets, column_indices, rng_state = \
            ctx.saved_tensors
        needs = tuple(ctx.needs_input_grad[:3])
        transposed = None
        if needs[1] or needs[2]:
            # (the probe row is a broadcast zero, materialised only when a transpose runs)
            probe = query.new_zeros(()).expand(1, column_indices.numel())
            transposed = _transposed_topology(query.size(-2), key.size(-2), row_offsets,
                                              column_indices, probe)
        grad_query, grad_key, grad_value = ops.sparse_attention_backward(
            query, key, value, out, _contiguous(grad_output), lse, row_indices, row_offsets,
            column_indices, transposed, ctx.scale, ctx.p, rng_state, needs)
        return grad_query, grad_key, grad_value, None, None, None, None, None


def sparse_attention(query, key, value, row_indices, row_offsets, column_indices, scale,
                     dropout_p=0.0, fused_backward=False):
    """softmax(scale * q k^T at the mask) v for float32 [R, S, D] (or [S, D]) operands, one
    fused kernel forward; differentiable (SparseAttentionFunction).  ``dropout_p``: dropout
    on the attention weights (0 <= p < 1; the caller decides when it is training).
    ``fused_backward``: the backward runs the two fused kernels
    (FusedBackwardAttentionFunction) where they serve the operands (head dimension 64 or
    128), and nothing of size [R, nnz] is allocated; elsewhere the composed backward runs as
    without the flag."""
    p = ops.check_dropout_p(dropout_p)
    topo = (row_indices, row_offsets, column_indices)
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        if fused_backward and fused_backward_served(query, key, column_indices):
            return FusedBackwardAttentionFunction.apply(query, key, value, *topo, scale, p)
        return SparseAttentionFunction.apply(query, key, value, *topo, scale, p)
    return _attention_forward(query, key, value, *topo, scale, p)[0]


# ---------------------------------------------------------------------------
# Half storage through attention (SparseAttention(half_storage=True)): q, k, v and the
# context stay [B, S, E] tensors in the input's half type, every head a strided view
# (element (b, h, s, c) at b*S*E + h*D + s*E + c).  Values are rounded to the storage type
# at the projection outputs, the context and the module output only; scores, weights and
# every sum are float32.
# ---------------------------------------------------------------------------
def _rows_route(m, k, values, column_indices, x):
    """Whether y = x W^T takes the row-orientation tile kernel (ops.half_linear_rows)."""
    return (x.is_cuda and x.dim() == 3 and x.stride(2) == 1 and x.data_ptr() % 16 == 0
            and x.stride(1) % 8 == 0 and x.stride(0) % 8 == 0
            and ops.half_linear_rows_supported(m, k, x.size(1), x.size(0), column_indices.numel(),
                                               values.dtype, x.dtype))


class HalfRowLinearFunction(torch.autograd.Function):
    """y [B, S, out] = x W^T in x's half type, on the matrix cores with no layout pass
    (ops.half_linear_rows: the weight's image against x as it is).  ``apply(m, k, values,
    row_indices, row_offsets, column_indices, x)``.  Backward: dy goes to [B, out, S] in one
    layout pass, then the half layer's weight and input gradients (HalfSparseLinearFunction)
    read it, the image and x."""

    @staticmethod
    def forward(ctx, m, k, values, row_indices, row_offsets, column_indices, x):
        ctx.shape = (m, k)
        ctx.topology = (row_indices, row_offsets, column_indices)
        image = ops.half_linear_image(m, k, values, row_offsets, column_indices, x.dtype)
        ctx.save_for_backward(values, x, image)
        return ops.half_linear_rows(m, image, values.dtype, x)

    @staticmethod
    def backward(ctx, grad_output):
        m, k = ctx.shape
        _, row_offsets, column_indices = ctx.topology
        values, x, image = ctx.saved_tensors
        x = x.contiguous()
        grad = ops.transpose_last2(_contiguous(grad_output).to(x.dtype))   # [B, out, S]
        grad_values = grad_x = None
        if ctx.needs_input_grad[2]:
            plan = None if _plans is None else _plans.half_linear(m, k, row_offsets, column_indices)
            grad_values = ops.half_linear_weight_gradient(m, row_offsets, column_indices, grad, False, x, plan)
        if ctx.needs_input_grad[6]:
            grad_x = _half_input_gradient(m, k, values, row_offsets, column_indices, image, x, grad, False, grad)
        return None, None, grad_values, None, None, None, grad_x


def half_linear_rows(m, k, values, row_indices, row_offsets, column_indices, x):
    """Differentiable y [B, S, m] = x W^T for x [B, S, k] in float16 / bfloat16, stored in
    x's type.  A shape the row-orientation kernel does not serve goes through the half
    layer in column orientation (HalfSparseLinearFunction) and a narrowing layout pass."""
    if _rows_route(m, k, values, column_indices, x):
        if torch.is_grad_enabled() and (x.requires_grad or values.requires_grad):
            return HalfRowLinearFunction.apply(m, k, values, row_indices, row_offsets, column_indices, x)
        values = values.detach()
        image = ops.half_linear_image(m, k, values, row_offsets, column_indices, x.dtype)
        y = ops.half_linear_rows(m, image, values.dtype, x)
        if y is not None:
            return y
    y = HalfSparseLinearFunction.apply(m, k, values, row_indices, row_offsets, column_indices, x)
    return transpose_last2(y, x.dtype)


def _heads(x, heads):
    """[B, S, E] -> the [B, H, S, E/H] view of its heads (no copy)."""
    return x.unflatten(-1, (heads, x.size(-1) // heads)).transpose(1, 2)


def _per_head(x, heads, dtype):
    """[B, S, E] -> [B*H, S, D] in `dtype` (one copy for more than one head)."""
    return _heads(x.to(dtype), heads).reshape(-1, x.size(1), x.size(2) // heads)


def _merge_heads(g, like, heads):
    """A gradient [B*H, S, D] (or None) -> [B, S, E] in the type of the input `like`."""
    if g is None:
        return None
    return g.reshape(like.size(0), heads, like.size(1), -1).transpose(1, 2).reshape(
        like.shape).to(like.dtype)


def _attention_heads(query, key, value, heads, row_indices, row_offsets, column_indices, scale, p=0.0):
    """-> (context [B, S, E], None, rng_state or None), as `_attention_forward`."""
    q, k, v = _heads(query, heads), _heads(key, heads), _heads(value, heads)
    plan = None if _plans is None else _plans.attention(q.size(-2), k.size(-2), q.size(-1), row_indices,
                                                        row_offsets, column_indices)
    operands = (q, k, v, row_indices, row_offsets, column_indices, scale)
    if p > 0.0:
        out, _, rng_state = ops.sparse_attention_heads_dropout(*operands, p, plan=plan)
    else:
        out, rng_state = ops.sparse_attention_heads(*operands, plan=plan), None
    # (the kernel's buffer is [B, S, H, D]: this is a view)
    return out.transpose(1, 2).reshape(query.size(0), query.size(1), -1), None, rng_state


class SparseAttentionHeadsFunction(torch.autograd.Function):
    """`sparse_attention_heads` under autograd: the fused forward on the head views, and
    the recomputing backward of SparseAttentionFunction (`_attention_backward`) on
    contiguous per-head copies in the storage type; the gradients come back as [B, S, E]
    in the inputs' type.  (Unlike the reference's raw softmax call, the gradient reaches
    q and k.)"""

    @staticmethod
    def forward(ctx, query, key, value, heads, row_indices, row_offsets, column_indices, scale,
                dropout_p=0.0):
        ctx.heads, ctx.scale, ctx.p = int(heads), float(scale), float(dropout_p)
        out, _, rng_state = _attention_heads(query, key, value, heads, row_indices, row_offsets,
                                             column_indices, scale, ctx.p)
        ctx.save_for_backward(query, key, value, row_indices, row_offsets, column_indices, rng_state)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        query, key, value, topo, dropout = _saved(ctx)
        q, k, v, grad = (_per_head(x, ctx.heads, query.dtype) for x in (query, key, value, grad_output))
        grads = _attention_backward(_single_mask_operators(topo, q.size(-2), k.size(-2)), q, k, v,
                                    ctx.scale, _contiguous(grad), ctx.needs_input_grad[:3], dropout)
        return (*(_merge_heads(g, x, ctx.heads) for g, x in zip(grads, (query, key, value))),
                None, None, None, None, None, None)


def sparse_attention_heads(query, key, value, heads, row_indices, row_offsets, column_indices, scale,
                           dropout_p=0.0):
    """softmax(scale * q k^T at the mask) v per head for [B, S, E] tensors in float16 /
    bfloat16 (query [B, m, E], key and value [B, n, E], any strides with a unit last one),
    E = heads * D: head h is columns h*D .. h*D+D-1 of every row -- read as strided views by
    the fused kernel (ops.sparse_attention_heads), no head split or merge pass.  Returns the
    context [B, m, E] in the inputs' type (rounded once); scores, weights and sums are
    float32.  Differentiable: the backward recomputes the weights (SparseAttentionHeadsFunction),
    and the gradient reaches q, k and v.  ``dropout_p``: dropout on the attention weights
    (replica r = b * heads + h of the library's mask contract)."""
    p = ops.check_dropout_p(dropout_p)
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        return SparseAttentionHeadsFunction.apply(query, key, value, heads, row_indices, row_offsets,
                                                  column_indices, scale, p)
    return _attention_heads(query, key, value, heads, row_indices, row_offsets, column_indices,
                            scale, p)[0]


# ---------------------------------------------------------------------------
# many-mask family: one mask per batch element, shared by its heads.  Same
# ``apply`` signatures and gradient positions as the reference's sketches in
# tests/transformer/functions.py (Spmm :5-69, CsrSoftmax :70-120, Sddmm :122-188).
# ---------------------------------------------------------------------------
def diffsort_many_mask(row_offsets, masks):
    """Per-mask ``diffsort`` of stacked / concatenated offsets
    (tests/transformer/utils.py:51-62) -> flat [masks * rows].  On the GPU one launch for
    all masks and no synchronisation (``topology.diffsort_many``)."""
    return diffsort_many(row_offsets, masks)


class SpmmManyMask(torch.autograd.Function):
    """tests/transformer/functions.py:5-69."""

    @staticmethod
    def forward(ctx, b, m, k, nonzeros, values, row_indices, row_offsets, column_indices, dense):
        ctx.dims = (b, m, k)
        ctx.nonzeros = nonzeros
        ctx.save_for_backward(values, row_indices, row_offsets, column_indices, dense)
        return ops.spmm_many_mask(b, m, k, nonzeros, values, row_indices, row_offsets,
                                  column_indices, dense)

    @staticmethod
    def backward(ctx, grad_output):
        b, m, k = ctx.dims
        nonzeros = ctx.nonzeros
        values, row_indices, row_offsets, column_indices, dense = ctx.saved_tensors
        grad_output = _contiguous(grad_output)
        grad_values = grad_dense = None
        if ctx.needs_input_grad[4]:
            grad_values = ops.sddmm_many_mask(b, m, k, nonzeros, row_indices, row_offsets,
                                              column_indices, grad_output, dense)
            if grad_values.shape[-1] != values.shape[-1]:  # values rows were padded
                grad_values = torch.nn.functional.pad(
                    grad_values, (0, values.shape[-1] - grad_values.shape[-1]))
        if ctx.needs_input_grad[8]:
            values_t, row_offsets_t, column_indices_t = ops.csr_transpose_many_mask(
                b, m, k, nonzeros, values.detach(), row_offsets, column_indices)
            row_indices_t = diffsort_many_mask(row_offsets_t, b)
            grad_dense = ops.spmm_many_mask(b, k, m, nonzeros, values_t, row_indices_t,
                                            row_offsets_t, column_indices_t, grad_output)
        return None, None, None, None, grad_values, None, None, None, grad_dense


class SddmmManyMask(torch.autograd.Function):
    """tests/transformer/functions.py:122-188."""

    @staticmethod
    def forward(ctx, b, m, n, nonzeros, row_indices, row_offsets, column_indices, lhs_matrix,
                rhs_matrix):
        ctx.dims = (b, m, n)
        ctx.nonzeros = nonzeros
        ctx.save_for_backward(row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix)
        return ops.sddmm_many_mask(b, m, n, nonzeros, row_indices, row_offsets, column_indices,
                                   lhs_matrix, rhs_matrix)

    @staticmethod
    def backward(ctx, grad_output):
        b, m, n = ctx.dims
        nonzeros = ctx.nonzeros
        row_indices, row_offsets, column_indices, lhs_matrix, rhs_matrix = ctx.saved_tensors
        grad_output = _contiguous(grad_output)
        grad_lhs = grad_rhs = None
        if ctx.needs_input_grad[7]:
            grad_lhs = ops.spmm_many_mask(b, m, n, nonzeros, grad_output, row_indices,
                                          row_offsets, column_indices, rhs_matrix)
        if ctx.needs_input_grad[8]:
            grad_t, row_offsets_t, column_indices_t = ops.csr_transpose_many_mask(
                b, m, n, nonzeros, grad_output, row_offsets, column_indices)
            row_indices_t = diffsort_many_mask(row_offsets_t, b)
            grad_rhs = ops.spmm_many_mask(b, n, m, nonzeros, grad_t, row_indices_t,
                                          row_offsets_t, column_indices_t, lhs_matrix)
        return None, None, None, None, None, None, None, grad_lhs, grad_rhs


class CsrSoftmaxManyMask(torch.autograd.Function):
    """tests/transformer/functions.py:70-120 with the softmax Jacobian in the
    backward (the sketch there returns ``s * (1 - s)`` of a dense softmax of the
    incoming gradient).  Optional trailing ``scale``."""

    @staticmethod
    def forward(ctx, b, m, nonzeros, scores, row_indices, row_offsets, column_indices,
                scale=1.0):
        out = ops.sparse_softmax_many_mask(b, m, nonzeros, scores, row_indices, row_offsets,
                                           column_indices, None if scale == 1.0 else scale)
        ctx.dims = (b, m, float(scale))
        ctx.nonzeros = nonzeros
        ctx.save_for_backward(out, row_offsets)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        b, m, scale = ctx.dims
        out, row_offsets = ctx.saved_tensors
        grad_scores = ops.sparse_softmax_backward_many_mask(
            b, m, ctx.nonzeros, out, grad_output.contiguous(), row_offsets, scale)
        return None, None, None, grad_scores, None, None, None, None


# ---------------------------------------------------------------------------
# Fused attention with one mask per batch element (the reference's SparseCoreAttention,
# tests/transformer/modules.py:9-81: sddmm_many_mask, sparse_softmax_many_mask, spmm_many_mask).
# The forward is one kernel (ops.sparse_attention_many_mask / _heads_many_mask); the backward
# is `_attention_backward` on the many-mask operators, which are float32 only: half inputs
# get float32 per-head copies there, and their gradients are returned in the input's type.
# ---------------------------------------------------------------------------
def _many_mask_plan(b, m, n, d, nonzeros, row_indices, row_offsets, column_indices):
    if _plans is None:
        return None
    return _plans.attention_many_mask(b, m, n, d, nonzeros, row_indices, row_offsets, column_indices)


def _many_mask_composed(b, nonzeros, topo, query, key, value, scale):
    """softmax(scale * sddmm) @ v from the separate many-mask operators, [R, S, D] float32
    (the path of tensors the kernels do not serve, CPU tensors among them)."""
    row_indices, row_offsets, column_indices = topo
    m, n = query.size(-2), key.size(-2)
    scores = ops.sddmm_many_mask(b, m, n, nonzeros, row_indices, row_offsets, column_indices,
                                 query, key)
    weights = ops.sparse_softmax_many_mask(b, m, nonzeros, scores, row_indices, row_offsets,
                                           column_indices, scale)
    return ops.spmm_many_mask(b, m, n, nonzeros, weights, row_indices, row_offsets,
                              column_indices, value)


def _many_mask_operators(b, nonzeros, topo, m, n):
    """The many-mask operators of b stacked m x n masks for `_attention_backward`; the
    transposed products run one csr_transpose_many_mask per values array they transpose."""
    _, row_offsets, column_indices = topo

    def transpose(values):
        return ops.csr_transpose_many_mask(b, m, n, nonzeros, values, row_offsets, column_indices)

    def transposed_products(grad_scores, kept, query, grad_output, needs_key, needs_value):
        grad_t, row_offsets_t, column_indices_t = transpose(grad_scores)
        topo_t = (diffsort_many_mask(row_offsets_t, b), row_offsets_t, column_indices_t)
        grad_key = grad_value = None
        if needs_key:
            grad_key = ops.spmm_many_mask(b, n, m, nonzeros, grad_t, *topo_t, query)
        if needs_value:
            grad_value = ops.spmm_many_mask(b, n, m, nonzeros, transpose(kept)[0], *topo_t,
                                            grad_output)
        return grad_key, grad_value

    return _Operators(
        sddmm=lambda lhs, rhs: ops.sddmm_many_mask(b, m, n, nonzeros, *topo, lhs, rhs),
        softmax=lambda scores, scale: ops.sparse_softmax_many_mask(b, m, nonzeros, scores, *topo,
                                                                   scale),
        softmax_backward=lambda weights, grad, scale: ops.sparse_softmax_backward_many_mask(
            b, m, nonzeros, weights, grad, row_offsets, scale),
        spmm=lambda values, dense: ops.spmm_many_mask(b, m, n, nonzeros, values, *topo, dense),
        transposed_products=transposed_products)


def _float_replicas(x):
    """[R, S, D], or a [B, S, H, D] view, -> contiguous [R, S, D] float32 (R = B * H)."""
    x = x.to(torch.float32)
    if x.dim() == 3:
        return x.contiguous()
    return x.transpose(1, 2).reshape(x.size(0) * x.size(2), x.size(1), x.size(3))


def _like_input(g, like):
    """A gradient [R, S, D] (or None) -> the shape and type of the input `like`."""
    if g is None:
        return None
    if like.dim() == 4:
        g = g.reshape(like.size(0), like.size(2), like.size(1), -1).transpose(1, 2)
    return g.to(like.dtype)


def _many_mask_forward(b, nonzeros, topo, query, key, value, scale, p=0.0):
    """[R, S, D] forward -> (out, None, rng_state or None), as `_attention_forward`: the fused
    kernel on GPU tensors (the heads kernel for half storage, whose [R, S, D] is a
    [b, R/b, S, D] head view), the composition elsewhere."""
    if p == 0.0 and not query.is_cuda:
        return _many_mask_composed(b, nonzeros, topo, query.float(), key.float(), value.float(),
                                   scale).to(query.dtype), None, None
    plan = _many_mask_plan(b, query.size(-2), key.size(-2), query.size(-1), nonzeros, *topo)
    half = query.dtype in (torch.float16, torch.bfloat16)
    if half:
        query, key, value = (x.unflatten(0, (b, x.size(0) // b)) for x in (query, key, value))
    operands = (b, nonzeros, *topo, query, key, value, scale)
    if p > 0.0:
        op = ops.sparse_attention_heads_many_mask_dropout if half else ops.sparse_attention_many_mask_dropout
        out, _, rng_state = op(*operands, p, plan=plan)
    else:
        op = ops.sparse_attention_heads_many_mask if half else ops.sparse_attention_many_mask
        out, rng_state = op(*operands, plan=plan), None
    if half:
        out = out.flatten(0, 1)   # ([b, H, S, D] view of a [b, S, H, D] buffer: one copy)
    return out, None, rng_state


def _heads_many_mask_forward(query, key, value, nonzeros, topo, scale, p=0.0):
    """[B, S, H, D] views -> ([B, m, H, D], None, rng_state or None), as `_attention_forward`."""
    b, heads = query.size(0), query.size(2)
    q, k, v = (x.transpose(1, 2) for x in (query, key, value))   # [B, H, S, D] views
    if query.dtype in (torch.float16, torch.bfloat16) and (p > 0.0 or query.is_cuda):
        plan = _many_mask_plan(b, q.size(-2), k.size(-2), q.size(-1), nonzeros, *topo)
        operands = (b, nonzeros, *topo, q, k, v, scale)
        if p > 0.0:
            out, _, rng_state = ops.sparse_attention_heads_many_mask_dropout(*operands, p, plan=plan)
        else:
            out, rng_state = ops.sparse_attention_heads_many_mask(*operands, plan=plan), None
        out = out.transpose(1, 2)   # the kernel's [B, S, H, D] buffer
    else:   # float32 views, CPU tensors: one copy to [B*H, S, D]
        per_head = [x.reshape(b * heads, x.size(2), x.size(3)) for x in (q, k, v)]
        out, _, rng_state = _many_mask_forward(b, nonzeros, topo, *per_head, scale, p)
        out = out.reshape(b, heads, query.size(1), -1).transpose(1, 2).to(query.dtype)
    return out, None, rng_state


class SparseAttentionManyMaskFunction(torch.autograd.Function):
    """sparse_attention_many_mask under autograd (apply(b, nonzeros, row_indices, row_offsets,
    column_indices, query, key, value, scale[, dropout_p])): [R, S, D] operands."""

    @staticmethod
    def forward(ctx, b, nonzeros, row_indices, row_offsets, column_indices, query, key, value, scale,
                dropout_p=0.0):
        ctx.b, ctx.nonzeros, ctx.scale, ctx.p = int(b), nonzeros, float(scale), float(dropout_p)
        topo = (row_indices, row_offsets, column_indices)
        out, _, rng_state = _many_mask_forward(ctx.b, nonzeros, topo, query, key, value, scale, ctx.p)
        ctx.save_for_backward(query, key, value, *topo, rng_state)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        query, key, value, topo, dropout = _saved(ctx)
        q, k, v, grad = (_float_replicas(x) for x in (query, key, value, grad_output))
        grads = _attention_backward(
            _many_mask_operators(ctx.b, ctx.nonzeros, topo, q.size(-2), k.size(-2)), q, k, v,
            ctx.scale, grad.contiguous(), ctx.needs_input_grad[5:8], dropout)
        return (None, None, None, None, None,
                *(_like_input(g, x) for g, x in zip(grads, (query, key, value))), None, None)


def sparse_attention_many_mask(b, m, n, nonzeros, row_indices, row_offsets, column_indices, query,
                               key, value, scale, dropout_p=0.0):
    """softmax(scale * q k^T at the mask) v with one mask per batch element, for [R, S, D]
    tensors (R = b * heads, replica r under mask r // heads), topology in the many-mask layout
    of tests/transformer/utils.py:17-38 (``topology.dense_to_sparse_3d``), `nonzeros` a host
    list or tensor.  float32, float16 or bfloat16: half inputs are read in their type by the
    fused kernel and the result keeps it (scores, weights and sums float32).  Differentiable:
    the backward recomputes the weights with the many-mask operators, which are float32 only
    (half inputs: float32 copies, gradients returned in the input's type).  Head dimensions
    other than 64, unaligned operands and CPU tensors take the composed operators.
    ``dropout_p``: dropout on the attention weights (entry e = position inside the mask)."""
    m, n = int(m), int(n)
    p = ops.check_dropout_p(dropout_p)
    if query.size(-2) != m or key.size(-2) != n:
        raise ValueError(f"expected query rows {m} and key rows {n}, got {query.size(-2)}, {key.size(-2)}")
    topo = (row_indices, row_offsets, column_indices)
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        return SparseAttentionManyMaskFunction.apply(b, nonzeros, *topo, query, key, value, scale, p)
    return _many_mask_forward(int(b), nonzeros, topo, query, key, value, scale, p)[0]


class SparseAttentionHeadsManyMaskFunction(torch.autograd.Function):
    """sparse_attention_heads_many_mask under autograd: [B, S, H, D] views, batch element i
    under mask i."""

    @staticmethod
    def forward(ctx, query, key, value, nonzeros, row_indices, row_offsets, column_indices, scale,
                dropout_p=0.0):
        ctx.nonzeros, ctx.scale, ctx.p = nonzeros, float(scale), float(dropout_p)
        topo = (row_indices, row_offsets, column_indices)
        out, _, rng_state = _heads_many_mask_forward(query, key, value, nonzeros, topo, scale, ctx.p)
        ctx.save_for_backward(query, key, value, *topo, rng_state)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        query, key, value, topo, dropout = _saved(ctx)
        q, k, v, grad = (_float_replicas(x) for x in (query, key, value, grad_output))
        grads = _attention_backward(
            _many_mask_operators(query.size(0), ctx.nonzeros, topo, q.size(-2), k.size(-2)), q, k, v,
            ctx.scale, grad.contiguous(), ctx.needs_input_grad[:3], dropout)
        return (*(_like_input(g, x) for g, x in zip(grads, (query, key, value))),
                None, None, None, None, None, None)


def sparse_attention_heads_many_mask(query, key, value, nonzeros, row_indices, row_offsets,
                                     column_indices, scale, dropout_p=0.0):
    """The many-mask attention for [B, S, H, D] views (query [B, m, H, D], key and value
    [B, n, H, D], any strides with a unit last one; batch element i under mask i): the layout
    split_tensor_along_last_dim gives (tests/transformer/modules.py:98-111, head stride 3 D),
    read in place by the fused kernel for float16 / bfloat16 -- no copy.  float32 views are
    copied once to [B*H, S, D].  Returns [B, m, H, D] in the inputs' type (a contiguous
    tensor).  Differentiable as sparse_attention_many_mask; ``dropout_p`` as there (replica
    r = b * heads + h)."""
    p = ops.check_dropout_p(dropout_p)
    topo = (row_indices, row_offsets, column_indices)
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        return SparseAttentionHeadsManyMaskFunction.apply(query, key, value, nonzeros, *topo, scale, p)
    return _heads_many_mask_forward(query, key, value, nonzeros, topo, scale, p)[0]
