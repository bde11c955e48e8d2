"""CSR topology helpers the reference duplicates in every module
(modules/spmm.py:4-6, modules/sparse_linear.py:5-16,
modules/sparse_attention.py:12-36).  CPU tensors take pure torch; GPU tensors are
built by the device kernels of csrc/topology.hip (``ops.dense_to_csr``,
``ops.row_order``) where their host queries serve the shape -- the same integers
either way (``enable_device_build``).  ``random_csr`` draws a uniformly random topology
with its initial values (``ops.random_csr`` on a GPU), ``erk_densities`` gives the layers of
a model their Erdos-Renyi-Kernel densities."""
import math

import numpy as np
import torch

from . import capi, ops
from .ops import _TOPK_DTYPES

_device_build = True

# element types ops.dense_to_csr reads: 1, 2, 4 and 8 bytes wide, every real dtype of torch
_BUILD_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64,
                 torch.float16, torch.bfloat16, torch.float32, torch.float64)


def enable_device_build(enabled=True):
    """True (the default): GPU tensors get their topologies from the device kernels
    (a fixed number of launches, one synchronisation per build, none per row order).
    False: the torch path for every tensor -- the same results, for comparison."""
    global _device_build
    _device_build = bool(enabled)
    return _device_build


def _served(where, query, *args):
    """Whether the device kernels take a call: the device build is on, ``where`` (a tensor or a
    device) is a GPU and the host query ``capi.<query>(*args)`` serves the sizes -- its "served"
    field, or, for a query without one, that it does not raise (it raises RuntimeError for sizes
    beyond int32).  The dtypes are the caller's matter."""
    device = where.device if torch.is_tensor(where) else where
    if not (_device_build and device.type == "cuda"):
        return False
    try:
        return getattr(capi, query)(*args).get("served", True)
    except RuntimeError:
        return False


def _row_order_served(masks, rows):
    """(the kernel's limit is on the rows alone; its 64-bit keys hold every length)"""
    return rows >= 0 and capi.csr_row_order_route(masks, rows, 0)["served"]


def _build_served(dense, masks, m, n):
    return (dense.dtype in _BUILD_DTYPES and _served(dense, "dense_to_csr_launch_shape", masks, m, n, dense.element_size())
            and _row_order_served(masks, m))


def diffsort(row_offsets):
    """``row_indices`` for a CSR matrix: rows ordered by ASCENDING length.

    Same order as the reference's ``argsort(offsets - roll(offsets, -1),
    descending=True)[:-1]`` (modules/spmm.py:4-6), always
    int32 (the reference forgets the cast in modules/sparse_linear.py:5-7).
    """
    if (_device_build and row_offsets.is_cuda and row_offsets.dtype == torch.int32
            and row_offsets.dim() == 1 and row_offsets.numel() >= 1
            and _row_order_served(1, row_offsets.numel() - 1)):
        return ops.row_order(row_offsets)
    lengths = row_offsets[1:] - row_offsets[:-1]
    return torch.argsort(lengths, stable=True).to(torch.int32)


def diffsort_many(row_offsets, masks):
    """Per-mask ``diffsort`` of stacked / concatenated offsets -> flat [masks * rows]
    (``functional.diffsort_many_mask``): one launch for all masks on the GPU."""
    per_mask = row_offsets.reshape(masks, -1)
    if (_device_build and per_mask.is_cuda and per_mask.dtype == torch.int32 and masks >= 1
            and per_mask.size(1) >= 1 and _row_order_served(masks, per_mask.size(1) - 1)):
        return ops.row_order(per_mask).reshape(-1)
    return torch.cat([diffsort(per_mask[i]) for i in range(masks)])


def dense_to_sparse(matrix):
    """2-D dense tensor -> (values, row_indices, row_offsets, column_indices),
    int32 indices, as modules/sparse_linear.py:9-16 builds them."""
    if matrix.dim() == 2 and _build_served(matrix, 1, matrix.size(0), matrix.size(1)):
        row_indices, row_offsets, column_indices, _, values = ops.dense_to_csr(matrix.detach(), True)
        return values, row_indices, row_offsets, column_indices
    csr = matrix.detach().to_sparse_csr()
    values = csr.values().clone()
    row_offsets = csr.crow_indices().to(torch.int32)
    column_indices = csr.col_indices().to(torch.int32)
    return values, diffsort(row_offsets), row_offsets, column_indices


def magnitude_keys(x):
    """The selection key of every element of a float32 / float16 / bfloat16 tensor, int64: its
    bit pattern with the sign bit cleared, read as an unsigned integer.  Ranking by key is
    ranking by ``|x|``; -0.0 ties with 0.0, denormals rank by their bits, inf ranks above every
    finite value and NaN above inf."""
    x = x.contiguous()
    if x.element_size() == 2:
        return x.view(torch.int16).to(torch.int64) & 0x7fff
    return x.view(torch.int32).to(torch.int64) & 0x7fffffff


_BIT_VIEWS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _take_bits(tensor, flat):
    """``tensor.reshape(-1)[flat]`` as a copy of bits (a NaN keeps its payload and sign)"""
    bits = tensor.contiguous().view(_BIT_VIEWS[tensor.element_size()]).reshape(-1)
    return bits[flat].view(tensor.dtype)


def _rankable(x):
    """``x`` itself where it is float32 / float16 / bfloat16, else ``x.float()``: what is ranked
    in its place"""
    return x if x.dtype in _TOPK_DTYPES else x.float()


def _entry_rows(row_offsets, nnz):
    """int64 [nnz]: the row of every entry of a CSR pattern (nnz is given: nothing is read back)"""
    lengths = (row_offsets[1:] - row_offsets[:-1]).to(torch.int64)
    rows = torch.arange(lengths.numel(), dtype=torch.int64, device=row_offsets.device)
    return torch.repeat_interleave(rows, lengths, output_size=nnz)


def _offsets_of(rows, m):
    """int32 row_offsets [m + 1] of a pattern of ``m`` rows whose entries lie in ``rows``"""
    row_offsets = torch.zeros(m + 1, dtype=torch.int32, device=rows.device)
    row_offsets[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0)
    return row_offsets


def _csr_from_source(values, rows, m, column_indices, source):
    """(row_indices, row_offsets, column_indices, values, source) of the entries ``source``
    (old entry indices, ascending) of a pattern of ``m`` rows whose entries lie in ``rows``"""
    row_offsets = _offsets_of(rows[source], m)
    return diffsort(row_offsets), row_offsets, column_indices[source], _take_bits(values, source), source


def _count_of(op, density, nonzeros, most):
    """The entries a ``density`` / ``nonzeros`` pair asks of ``most`` positions:
    ``round(density * most)``, or ``nonzeros`` itself.  ValueError unless exactly one of the two
    is given, the density lies within 0 .. 1 and the count within 0 .. most."""
    if (density is None) == (nonzeros is None):
        raise ValueError(f"{op}: give exactly one of density / nonzeros")
    if density is not None:
        if not 0.0 <= density <= 1.0:
            raise ValueError(f"{op}: density {density} is outside 0 .. 1")
        nonzeros = round(density * most)
    count = int(nonzeros)
    if not 0 <= count <= most:
        raise ValueError(f"{op}: nonzeros = {count} is outside 0 .. {most}")
    return count


def topk_to_csr(scores, per_row=None, total=None, values_from=None):
    """``ops.topk_to_csr`` for any tensor: the device build where it serves the call, else the
    same rule in torch -- a stable descending sort of the keys (``magnitude_keys``), so ties go
    to the lowest column (per row) or flat index (total).  Scores of another dtype are ranked
    as ``.float()``.  -> (row_indices, row_offsets, column_indices, values), the same integers
    and value bits on both paths."""
    count = ops._check_topk_arguments("topk_to_csr", scores, per_row, total, values_from)
    values_from = (scores if values_from is None else values_from).detach()
    scores = _rankable(scores.detach())
    if values_from.element_size() in (2, 4) and _served(scores, "topk_to_csr_launch_shape", scores.size(0),
                                                         scores.size(1), scores.element_size(), per_row is None):
        return ops.topk_to_csr(scores, per_row, total, values_from)
    return _topk_to_csr_torch(scores, None if per_row is None else count, None if total is None else count,
                              values_from)


def _topk_to_csr_torch(scores, per_row, total, values_from):
    """the torch path of ``topk_to_csr``: float32 / float16 / bfloat16 scores, checked arguments"""
    m, n = scores.shape
    count = total if per_row is None else per_row
    keys = magnitude_keys(scores)
    int32 = dict(dtype=torch.int32, device=scores.device)
    if per_row is not None:
        kept = torch.argsort(keys, dim=1, descending=True, stable=True)[:, :count]
        columns = torch.sort(kept, dim=1).values
        row_offsets = torch.arange(m + 1, **int32) * count
        flat = (columns + torch.arange(m, device=scores.device)[:, None] * n).reshape(-1)
        return (torch.arange(m, **int32), row_offsets, columns.reshape(-1).to(torch.int32),
                _take_bits(values_from, flat))
    kept = torch.argsort(keys.reshape(-1), descending=True, stable=True)[:count]
    flat = torch.sort(kept).values
    rows = torch.div(flat, max(n, 1), rounding_mode="floor")
    row_offsets = _offsets_of(rows, m)
    return (diffsort(row_offsets), row_offsets, (flat - rows * n).to(torch.int32),
            _take_bits(values_from, flat))


_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_LO32 = 0xffffffff


def _mulhilo32(multiplier, c):
    """(high, low) 32-bit words of ``multiplier * c`` for int64 tensors holding 32-bit words,
    through 16-bit halves so that no product leaves int64"""
    upper, lower = (c >> 16) * multiplier, (c & 0xffff) * multiplier   # below 2**48 each
    return (upper + (lower >> 16)) >> 16, (((upper & 0xffff) << 16) + lower) & _LO32


def _philox4x32_10(key, counter):
    """Philox4x32-10 (csrc/philox.h) on int64 tensors that hold 32-bit words: ``key`` two Python
    ints, ``counter`` four broadcastable tensors -> the four output words."""
    k0, k1 = key
    c0, c1, c2, c3 = torch.broadcast_tensors(*counter)
    for _ in range(10):
        hi0, lo0 = _mulhilo32(_PHILOX_M[0], c0)
        hi1, lo1 = _mulhilo32(_PHILOX_M[1], c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W[0]) & _LO32, (k1 + _PHILOX_W[1]) & _LO32
    return c0, c1, c2, c3


def _random_words(m, n, seed, offset, device, values):
    """int64 [m, n]: word ``c & 3`` of Philox(seed, counter (offset / 4, c >> 2, r)) for every
    position (r, c); ``values``: r | 2**31 in the counter (the stream of the values)"""
    seed, block = int(seed) & 0xffffffffffffffff, (int(offset) & 0xffffffffffffffff) // 4
    index = dict(dtype=torch.int64, device=device)
    quads = torch.arange((n + 3) // 4, **index)[None, :]
    rows = torch.arange(m, **index)[:, None] | (0x80000000 if values else 0)
    words = _philox4x32_10((seed & _LO32, seed >> 32),
                           (torch.full((1, 1), block & _LO32, **index), torch.full((1, 1), block >> 32, **index),
                            quads, rows))
    return torch.stack(words, dim=2).reshape(m, -1)[:, :n]


def _random_csr_torch(m, n, per_row, total, dtype, scale, seed, offset, device, key_mask=ops.RANDOM_KEY_MASK):
    """The rule of ``random_csr`` in torch: the keys and the values of every position as dense
    [m, n] images, through the torch path of ``topk_to_csr`` -- a key viewed as float32 bits ranks
    by exactly ``magnitude_keys``.  -> (row_indices, row_offsets, column_indices, values)"""
    keys = _random_words(m, n, seed, offset, device, False) & int(key_mask)
    q = (_random_words(m, n, seed, offset, device, True) >> 8) - 2 ** 23
    values = (q.to(torch.float32) * scale).to(dtype)      # one conversion, one float32 multiply, one rounding
    scores = keys.to(torch.int32).view(torch.float32)
    return _topk_to_csr_torch(scores, per_row, total, values)


def _draw_philox_state(device):
    """(seed, offset) for a call without an ``rng_state``: 4 of the device's default generator
    on a GPU, as the device path draws them; a seed from torch's CPU generator otherwise"""
    if device.type == "cuda":
        index = torch.cuda.current_device() if device.index is None else device.index
        generator = torch.cuda.default_generators[index]
        offset = generator.get_offset()
        generator.set_offset(offset + 4)
        return generator.initial_seed(), offset
    return int(torch.randint(0, 2 ** 62, (1,))), 0


def random_csr(m, n, density=None, nonzeros=None, per_row=False, dtype=torch.float32, bound=None, device=None,
               rng_state=None, return_rng_state=False):
    """A uniformly random ``m x n`` topology with its initial values -> (values, row_indices,
    row_offsets, column_indices), the tuple of ``dense_to_sparse``: how a layer of SET, RigL or
    any sparse-from-scratch method starts.  Counts are ``magnitude_prune``'s: ``density`` keeps
    ``round(density * m * n)`` positions of the matrix, or ``per_row`` ``round(density * n)`` of
    every row; ``nonzeros`` is that number itself.  Exactly that many positions are kept, every
    position with the same probability, columns ascending inside a row.

    The rule, for ``rng_state = {seed, offset}`` (offset a multiple of 4), with Philox4x32-10:
    ``key(r, c) = Philox(seed, (offset / 4, c >> 2, r))[c & 3] & 0x7fffffff``; the positions of
    largest key are kept, ties to the lowest flat index (column, ``per_row``) --
    ``topk_to_csr``'s selection.  A kept position's value is ``float32(q) * float32(bound /
    2**23)`` with ``q = (Philox(seed, (offset / 4, c >> 2, r | 2**31))[c & 3] >> 8) - 2**23``,
    rounded to nearest even into ``dtype``: uniform on ``[-bound, bound)``.  ``bound=None`` is
    ``1 / sqrt(max(1, count_per_row))`` with the (mean) entries of a row: kaiming-uniform on the
    effective fan-in.

    A GPU ``device`` takes the device kernels (``ops.random_csr``: the keys are computed where a
    score would be loaded, one launch per row or nine matrix-wide, no ``[m, n]`` array, no host
    synchronisation); the CPU, ``enable_device_build(False)`` and matrix-wide draws over more
    than 16384 rows take the same rule in torch.  Given the same ``rng_state`` (int64 [2]) both
    return the same integers and value bits.  Without one a GPU call draws 4 from the device's
    default generator (``torch.manual_seed`` makes runs repeat) and a CPU call a seed from
    torch's CPU generator with offset 0.  ``return_rng_state``: the state used is appended."""
    m, n = int(m), int(n)
    if m < 0 or n < 0:
        raise ValueError(f"random_csr: expected sizes >= 0, got {m} x {n}")
    count = _count_of("random_csr", density, nonzeros, n if per_row else m * n)
    per_row_count, total = (count, None) if per_row else (None, count)
    ops.check_random_arguments(m, n, per_row_count, total, dtype, ops.RANDOM_KEY_MASK)
    if bound is None:
        bound = 1.0 / math.sqrt(max(1.0, float(count) if per_row else count / max(m, 1)))
    device = torch.device("cpu" if device is None else device)
    if _served(device, "random_csr_launch_shape", m, n, not per_row):
        row_indices, row_offsets, column_indices, values, state = ops.random_csr(
            m, n, per_row=per_row_count, total=total, dtype=dtype, bound=bound, device=device, rng_state=rng_state)
    else:
        if rng_state is None:
            seed, offset = _draw_philox_state(device)
            state = torch.tensor([seed, offset], dtype=torch.int64, device=device)
        else:
            state = rng_state
            seed, offset = (int(v) for v in rng_state.tolist())
        if offset % 4 != 0:
            raise ValueError(f"random_csr: the offset of rng_state must be a multiple of 4, got {offset}")
        row_indices, row_offsets, column_indices, values = _random_csr_torch(
            m, n, per_row_count, total, dtype, ops.random_value_scale(bound), seed, offset, device)
    result = (values, row_indices, row_offsets, column_indices)
    return result + (state,) if return_rng_state else result


def erk_densities(shapes, density, power=1.0):
    """The Erdos-Renyi-Kernel densities of a list of layers (Evci et al., "Rigging the Lottery",
    2020): ``shapes`` a list of ``(out, in)``, layer l gets ``eps * ((out + in) / (out * in)) **
    power`` with eps such that the layers hold ``density`` of all positions together,
    ``sum density_l * out_l * in_l = density * sum out_l * in_l``.  While the layer of largest
    density would exceed 1 it is made dense and eps is solved again without it (RigL's
    procedure).  ``power = 0`` is the uniform distribution.  Host only -> a list of floats in
    (0, 1], to pass to ``SparseLinear.random(..., density=)``."""
    if not 0.0 < density <= 1.0:
        raise ValueError(f"erk_densities: density {density} is outside (0, 1]")
    shapes = [(int(out), int(inp)) for out, inp in shapes]
    if any(out <= 0 or inp <= 0 for out, inp in shapes):
        raise ValueError(f"erk_densities: every shape must be (out, in) with positive sizes, got {shapes}")
    if density == 1.0:
        return [1.0] * len(shapes)
    sizes = [out * inp for out, inp in shapes]
    raw = [((out + inp) / (out * inp)) ** power for out, inp in shapes]
    dense = set()
    while True:
        sparse = [l for l in range(len(shapes)) if l not in dense]
        if not sparse:
            break
        budget = density * sum(sizes) - sum(sizes[l] for l in dense)
        eps = budget / sum(raw[l] * sizes[l] for l in sparse)
        largest = max(raw[l] for l in sparse)
        if largest * eps <= 1.0:
            break
        dense.update(l for l in sparse if raw[l] == largest)
    return [1.0 if l in dense else min(1.0, eps * raw[l]) for l in range(len(shapes))]


def magnitude_prune(matrix, density=None, nonzeros=None, per_row=False):
    """Dense [m, n] matrix -> (values, row_indices, row_offsets, column_indices), the tuple of
    ``dense_to_sparse``, keeping its entries of largest magnitude.

    ``density``: keep ``round(density * m * n)`` entries of the matrix, or ``per_row``
    ``round(density * n)`` of every row.  ``nonzeros``: that number itself (of every row,
    ``per_row``).  Give one of the two.  Exactly that many entries are kept, ties to the lowest
    flat index (column, ``per_row``); zeros are kept as explicit entries where the count demands
    it.  The ranking is that of ``magnitude_keys``.

    GPU float32 / float16 / bfloat16 matrices are selected and written out by the device
    kernels (``ops.topk_to_csr``; no host synchronisation); CPU tensors, other dtypes (ranked as
    ``.float()``), ``enable_device_build(False)`` and matrix-wide selection over more than 16384
    rows take the same rule in torch.  Both give the same integers and value bits."""
    if matrix.dim() != 2:
        raise ValueError(f"magnitude_prune: expected a [m, n] matrix, got {tuple(matrix.shape)}")
    count = _count_of("magnitude_prune", density, nonzeros, matrix.size(1) if per_row else matrix.numel())
    row_indices, row_offsets, column_indices, values = topk_to_csr(
        matrix, per_row=count if per_row else None, total=None if per_row else count)
    return values, row_indices, row_offsets, column_indices


def _first_in_stable_order(keys, counts):
    """bool [m, n]: the counts[r] first columns of row r in the stable descending order of its
    keys (largest key first, lowest column among equals)"""
    m, n = keys.shape
    order = torch.argsort(keys, dim=1, descending=True, stable=True)
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(n, device=keys.device).expand(m, n))
    return rank < counts[:, None]


def regrow_per_row(values, row_offsets, column_indices, drop_counts, scores):
    """``ops.csr_regrow`` for any tensor: one per-row drop-and-grow step of the CSR pattern
    (row_offsets [m + 1], column_indices [nnz], int32, ascending inside a row) with ``values``
    [nnz] under dense ``scores`` [m, n].  Row r of ``len_r`` entries has
    ``d_r = clamp(drop_counts[r], 0, len_r)``:

    * Kept: its ``len_r - d_r`` entries of largest value key (``magnitude_keys``: NaN above inf,
      -0.0 with 0.0), ties to the lower column.
    * Grown: the ``d_r`` columns outside Kept of largest score key, ties to the lowest column; a
      score key is clamped to that of the dtype's largest finite value (NaN and inf count as
      it); the sign is ignored; columns dropped in this step are eligible.
    * The new row is Kept and Grown in ascending column order in the row's own slots.

    -> (column_indices int32 [nnz], values [nnz], source int64 [nnz]), new tensors: a kept entry
    carries its value bit for bit and its old entry index, a grown one is +0.0 and -1.
    ``row_offsets`` does not change.

    GPU float32 / float16 / bfloat16 values and scores take the device kernel where
    ``capi.csr_regrow_launch_shape`` serves ``n`` (one launch, no host synchronisation); CPU
    tensors, other dtypes (ranked as ``.float()``), wider rows and ``enable_device_build(False)``
    take the same rule in torch: per row a stable descending argsort of the keys, with the kept
    columns forced first.  Both give the same integers and value bits."""
    ops.check_regrow_arguments(values, row_offsets, column_indices, drop_counts, scores)
    values, scores = values.detach(), _rankable(scores.detach())
    m, n = scores.shape
    if values.dtype in _TOPK_DTYPES and _served(values, "csr_regrow_launch_shape", m, n, scores.element_size(),
                                                values.element_size()):
        return ops.csr_regrow(values, row_offsets, column_indices, drop_counts, scores)
    nnz = column_indices.numel()
    index = dict(dtype=torch.int64, device=values.device)
    lengths = (row_offsets[1:] - row_offsets[:-1]).to(torch.int64)
    flat = _entry_rows(row_offsets, nnz) * n + column_indices.to(torch.int64)
    drop = torch.minimum(drop_counts.to(torch.int64).clamp(min=0), lengths)
    # dense images of the old entries: their value keys (-1 elsewhere: behind every entry) and
    # their indices
    value_keys = torch.full((m * n,), -1, **index)
    value_keys[flat] = magnitude_keys(_rankable(values))
    entry = torch.full((m * n,), -1, **index)
    entry[flat] = torch.arange(nnz, **index)
    kept = _first_in_stable_order(value_keys.view(m, n), lengths - drop)
    limit = int(magnitude_keys(torch.tensor([torch.finfo(scores.dtype).max], dtype=scores.dtype))[0])
    score_keys = magnitude_keys(scores).clamp(max=limit)
    score_keys = torch.where(kept, limit + 1, score_keys)              # Kept comes first
    new = _first_in_stable_order(score_keys, lengths).view(-1)
    # the flat positions of the new entries, ascending; nnz of them, so nothing is read back
    slot = torch.where(new, torch.cumsum(new, 0) - 1, nnz)
    new_flat = torch.empty(nnz + 1, **index).scatter_(0, slot, torch.arange(m * n, **index))[:nnz]
    carried = kept.view(-1)[new_flat]
    source = torch.where(carried, entry[new_flat], -1)
    bits = values.contiguous().view(_BIT_VIEWS[values.element_size()])
    new_bits = torch.where(carried, bits[source.clamp(min=0)], torch.zeros(1, dtype=bits.dtype, device=bits.device))
    new_columns = new_flat - torch.div(new_flat, max(n, 1), rounding_mode="floor") * n
    return new_columns.to(torch.int32), new_bits.view(values.dtype), source


def regrow_total_composed(values, row_offsets, column_indices, drop, scores):
    """The rule of ``regrow_total`` composed from torch indexing and one ``topk_to_csr`` call
    (which itself picks the device build or torch): the kept entries are forced first in a dense
    image of the scores, their values travel in a second dense image, and ``source`` is looked up
    afterwards.  What ``regrow_total`` runs where the device step does not serve the call; under
    its own name so that the two can be compared on a GPU."""
    d = ops.check_regrow_total_arguments(values, row_offsets, column_indices, drop, scores)
    values, scores = values.detach(), scores.detach()
    m, n = scores.shape
    nnz = values.numel()
    device = values.device
    order = torch.argsort(magnitude_keys(_rankable(values)), descending=True, stable=True)
    kept = torch.sort(order[:nnz - d]).values                     # old entry indices, ascending
    flat = _entry_rows(row_offsets, nnz) * n + column_indices.to(torch.int64)   # ascending: CSR is row major
    kept_flat = flat[kept]

    scores = _rankable(scores)
    largest = torch.finfo(scores.dtype).max
    scores = torch.nan_to_num(scores.abs(), nan=largest, posinf=largest).contiguous()
    scores.view(-1)[kept_flat] = float("inf")                      # Kept comes first ...
    image = torch.zeros(m, n, dtype=values.dtype, device=device)
    bits = _BIT_VIEWS[values.element_size()]                         # ... and carries its values,
    image.view(bits).view(-1)[kept_flat] = values.contiguous().view(bits)[kept]   # bit for bit
    row_indices, new_offsets, new_columns, new_values = topk_to_csr(scores, total=nnz, values_from=image)

    new_flat = _entry_rows(new_offsets, nnz) * n + new_columns.to(torch.int64)
    at = torch.searchsorted(kept_flat, new_flat).clamp_(max=kept_flat.numel() - 1)
    if kept_flat.numel():
        source = torch.where(kept_flat[at] == new_flat, kept[at], torch.full_like(at, -1))
    else:
        source = torch.full_like(new_flat, -1)
    return row_indices, new_offsets, new_columns, new_values, source


def regrow_total(values, row_offsets, column_indices, drop, scores):
    """``ops.csr_regrow_total`` for any tensor: one matrix-wide drop-and-grow step of the CSR
    pattern (row_offsets [m + 1], column_indices [nnz], int32, ascending inside a row) with
    ``values`` [nnz] under dense ``scores`` [m, n]; ``drop = d`` is a host integer,
    ``0 <= d <= nnz``.  The layer-wise rule of SET and RigL:

    * Kept: the ``nnz - d`` entries of largest value key (``magnitude_keys``: NaN above inf,
      -0.0 with 0.0), ties to the lower entry index.
    * Grown: the ``d`` positions outside Kept of largest score key, ties to the lower flat
      (row-major) index; a score key is clamped to that of the dtype's largest finite value (NaN
      and inf count as it); the sign is ignored; positions dropped in this step are eligible.
    * The new pattern is Kept and Grown, ``nnz`` entries, columns ascending inside a row; the row
      lengths change.

    -> (row_indices, row_offsets, column_indices int32 [nnz], values [nnz], source int64 [nnz]),
    new tensors: a kept entry carries its value bit for bit and its old entry index, a grown one
    is +0.0 and -1.  ``d = 0`` reproduces the pattern (``source = arange(nnz)``).

    GPU float32 / float16 / bfloat16 values and scores take the device step where
    ``capi.csr_regrow_total_launch_shape`` serves the shape (up to 16384 rows and 65536 columns:
    a fixed number of launches, no dense temporary, no host synchronisation); CPU tensors, other
    dtypes (ranked as ``.float()``), larger shapes and ``enable_device_build(False)`` take
    ``regrow_total_composed``.  Both give the same integers and value bits."""
    d = ops.check_regrow_total_arguments(values, row_offsets, column_indices, drop, scores)
    values, scores = values.detach(), _rankable(scores.detach())
    if values.dtype in _TOPK_DTYPES and _served(values, "csr_regrow_total_launch_shape", scores.size(0), scores.size(1),
                                                values.numel(), scores.element_size(), values.element_size()):
        return ops.csr_regrow_total(values, row_offsets, column_indices, d, scores)
    return regrow_total_composed(values, row_offsets, column_indices, d, scores)


def _key_step_state(op, device, rng_state):
    """(seed, offset, state tensor) of a step under generated scores that takes the torch path:
    the ``rng_state`` given, or a fresh draw (``_draw_philox_state``)"""
    if rng_state is None:
        seed, offset = _draw_philox_state(device)
        state = torch.tensor([seed, offset], dtype=torch.int64, device=device)
    else:
        state = rng_state
        seed, offset = (int(v) for v in rng_state.tolist())
    if offset % 4 != 0:
        raise ValueError(f"{op}: the offset of rng_state must be a multiple of 4, got {offset}")
    return seed, offset, state


def _key_scores(m, n, seed, offset, device, key_mask):
    """float32 [m, n] whose bit patterns are the masked keys of every position: the dense scores
    the step under generated scores is defined by"""
    keys = _random_words(m, n, seed, offset, device, False) & int(key_mask)
    return keys.to(torch.int32).view(torch.float32)


def _write_grown_values(values, row_offsets, column_indices, source, n, seed, offset, grow_bound):
    """``values`` with the entries of ``source == -1`` replaced by the value stream of their
    positions under ``grow_bound``"""
    m = row_offsets.numel() - 1
    q = (_random_words(m, n, seed, offset, values.device, True) >> 8) - 2 ** 23
    image = (q.to(torch.float32) * ops.random_value_scale(grow_bound)).to(values.dtype)
    flat = _entry_rows(row_offsets, values.numel()) * n + column_indices.to(torch.int64)
    return torch.where(source < 0, image.reshape(-1)[flat], values) if values.numel() else values


def regrow_per_row_random(values, row_offsets, column_indices, drop_counts, n, grow_bound=None, rng_state=None,
                          return_rng_state=False, key_mask=ops.REGROW_KEY_MASK):
    """``ops.csr_regrow_random`` for any tensor: one per-row drop-and-grow step of the CSR pattern
    of an ``m x n`` matrix (row_offsets [m + 1], column_indices [nnz], int32, ascending inside a
    row) with ``values`` [nnz] under random grow scores that are never stored -- SET's step.

    The rule, for ``rng_state = {seed, offset}`` (offset a multiple of 4), with Philox4x32-10:
    ``key(r, c) = Philox(seed, (offset / 4, c >> 2, r))[c & 3] & 0x3fffffff``, the key stream of
    ``random_csr`` under a 30-bit mask.  Every such key read as float32 bits is a finite,
    non-negative number, so the step is EXACTLY ``regrow_per_row`` under dense float32 scores
    whose bits are ``key(r, c)``: Kept, Grown, the ties (lowest column), the eligibility of
    dropped columns, ascending columns and ``source`` are its.  A grown entry is ``+0.0``
    (``grow_bound=None``, as RigL initialises) or, for a finite ``grow_bound >= 0``, the value
    ``random_csr`` gives that position: ``float32((word' >> 8) - 2**23) * float32(grow_bound /
    2**23)`` with ``word'`` from the value stream (``r | 2**31`` in the counter), rounded to
    nearest even into the values' dtype (SET re-initialises what it grows).

    -> (column_indices, values, source), and the ``rng_state`` used (int64 [2]) with
    ``return_rng_state``.  GPU float32 / float16 / bfloat16 values take the device kernel where
    ``capi.csr_regrow_random_launch_shape`` serves ``n`` (up to 61440: one launch, no ``[m, n]``
    array, no host synchronisation); CPU tensors, other dtypes, wider rows and
    ``enable_device_build(False)`` take the rule as written: the keys as a dense image through
    ``regrow_per_row``.  Given the same ``rng_state`` both return the same integers and value
    bits.  Without one a GPU call draws 4 from the device's default generator
    (``torch.manual_seed`` makes runs repeat) and a CPU call a seed from torch's CPU generator
    with offset 0."""
    ops.check_regrow_random_arguments(values, row_offsets, column_indices, drop_counts, n, grow_bound, rng_state,
                                      key_mask)
    values, n = values.detach(), int(n)
    m = row_offsets.numel() - 1
    if values.dtype in _TOPK_DTYPES and _served(values, "csr_regrow_random_launch_shape", m, n, values.numel(),
                                                values.element_size(), False):
        new_columns, new_values, source, state = ops.csr_regrow_random(
            values, row_offsets, column_indices, drop_counts, n, grow_bound, rng_state, key_mask)
    else:
        seed, offset, state = _key_step_state("regrow_per_row_random", values.device, rng_state)
        new_columns, new_values, source = regrow_per_row(
            values, row_offsets, column_indices, drop_counts, _key_scores(m, n, seed, offset, values.device, key_mask))
        if grow_bound is not None:
            new_values = _write_grown_values(new_values, row_offsets, new_columns, source, n, seed, offset, grow_bound)
    result = (new_columns, new_values, source)
    return result + (state,) if return_rng_state else result


def regrow_total_random(values, row_offsets, column_indices, drop, n, grow_bound=None, rng_state=None,
                        return_rng_state=False, key_mask=ops.REGROW_KEY_MASK):
    """``ops.csr_regrow_total_random`` for any tensor: one matrix-wide drop-and-grow step of the CSR
    pattern of an ``m x n`` matrix under random grow scores that are never stored -- the layer-wise
    step of SET.  Keys, ``grow_bound``, ``rng_state`` and the fallback are those of
    ``regrow_per_row_random``; the step is EXACTLY ``regrow_total`` under dense float32 scores
    whose bits are ``key(r, c)`` (ties to the lowest flat index; the row lengths change).

    -> (row_indices, row_offsets, column_indices, values, source), and the ``rng_state`` used with
    ``return_rng_state``.  The device step serves up to 16384 rows and 65536 columns
    (``capi.csr_regrow_random_launch_shape``): a fixed number of launches, no ``[m, n]`` array, no
    host synchronisation."""
    d, _, _ = ops.check_regrow_total_random_arguments(values, row_offsets, column_indices, drop, n, grow_bound,
                                                      rng_state, key_mask)
    values, n = values.detach(), int(n)
    m = row_offsets.numel() - 1
    if values.dtype in _TOPK_DTYPES and _served(values, "csr_regrow_random_launch_shape", m, n, values.numel(),
                                                values.element_size(), True):
        row_indices, new_offsets, new_columns, new_values, source, state = ops.csr_regrow_total_random(
            values, row_offsets, column_indices, d, n, grow_bound, rng_state, key_mask)
    else:
        seed, offset, state = _key_step_state("regrow_total_random", values.device, rng_state)
        row_indices, new_offsets, new_columns, new_values, source = regrow_total(
            values, row_offsets, column_indices, d, _key_scores(m, n, seed, offset, values.device, key_mask))
        if grow_bound is not None:
            new_values = _write_grown_values(new_values, new_offsets, new_columns, source, n, seed, offset, grow_bound)
    result = (row_indices, new_offsets, new_columns, new_values, source)
    return result + (state,) if return_rng_state else result


def prune_csr(values, row_offsets, column_indices, n, per_row=None, total=None):
    """``ops.csr_topk`` for any tensor: the entries of largest magnitude of the CSR pattern
    (row_offsets [m + 1], column_indices [nnz], int32, ascending inside a row) of an ``m x n``
    matrix with ``values`` [nnz], as a smaller CSR pattern -- one step of gradual magnitude
    pruning, without a dense image.  ``total = K`` (``0 <= K <= nnz``) keeps the K entries of
    largest key (``magnitude_keys``: NaN above inf, -0.0 with 0.0); ``per_row = k``
    (``0 <= k <= n``) keeps the ``min(len_r, k)`` largest of every row.  Among equal keys the
    lower entry index wins: the lower column inside a row, the lower flat index across rows.

    -> (row_indices, row_offsets, column_indices, values, source), new tensors: a kept entry
    carries its column, its value bit for bit and, in ``source`` (int64, ascending), its index
    in the old arrays.

    GPU float32 / float16 / bfloat16 values take the device kernels up to 16384 rows
    (``capi.csr_topk_launch_shape``; ``total`` without a host synchronisation, ``per_row`` with
    the one read of the new size); CPU tensors, other dtypes (ranked as ``.float()``), more rows
    and ``enable_device_build(False)`` take the same rule in torch: a stable descending argsort
    of the keys.  Both give the same integers and value bits."""
    count = ops.check_csr_topk_arguments(values, row_offsets, column_indices, per_row, total)
    if per_row is not None and count > n:
        raise ValueError(f"prune_csr: per_row = {count} is outside 0 .. {n}")
    values = values.detach()
    m, nnz = row_offsets.numel() - 1, values.numel()
    if values.dtype in _TOPK_DTYPES and _served(values, "csr_topk_launch_shape", m, n, nnz, values.element_size(),
                                                per_row is None):
        return ops.csr_topk(values, row_offsets, column_indices, per_row=per_row, total=total)
    index = dict(dtype=torch.int64, device=values.device)
    # key descending, index ascending
    order = torch.argsort(magnitude_keys(_rankable(values)), descending=True, stable=True)
    rows = _entry_rows(row_offsets, nnz)
    if per_row is None:
        source = torch.sort(order[:count]).values
    else:
        # a stable sort by row keeps that order inside every row: an entry's rank in its row is
        # its position behind the row's start
        by_row = order[torch.argsort(rows[order], stable=True)]
        rank = torch.empty(nnz, **index)
        rank[by_row] = torch.arange(nnz, **index) - row_offsets[:-1].to(torch.int64)[rows[by_row]]
        source = torch.nonzero(rank < count).reshape(-1)
    return _csr_from_source(values, rows, m, column_indices, source)


_INT_MAX = 2 ** 31 - 1


def _csr_topk_global_served(values, row_offsets):
    first = values[0]
    if first.dtype not in _TOPK_DTYPES or any(v.device != first.device or v.dtype != first.dtype for v in values):
        return False
    rows, nonzeros = [ro.numel() - 1 for ro in row_offsets], [v.numel() for v in values]
    if max(rows) > _INT_MAX or sum(nonzeros) > _INT_MAX:   # (the query takes C ints)
        return False
    return _served(first, "csr_topk_global_launch_shape", rows, nonzeros, first.element_size())


def prune_csr_global(layers, total):
    """Global magnitude pruning: ONE top-k across the entries of several CSR patterns.
    ``layers`` is a sequence of ``(values, row_offsets, column_indices, n)`` -- the pattern of an
    ``m_l x n_l`` matrix as ``prune_csr`` takes it -- and ``total = K`` (``0 <= K <= sum nnz_l``)
    keeps the K entries of largest key over all layers (``magnitude_keys``: NaN above inf, -0.0
    with 0.0).  Among equal keys the entry of the layer listed first wins, then the lower entry
    index.

    -> a list with one ``(row_indices, row_offsets, column_indices, values, source)`` per layer,
    new tensors, as ``prune_csr`` returns them: a kept entry carries its column, its value bit
    for bit and, in ``source`` (int64, ascending), its index in the layer's old arrays.  A layer
    may end with no entry at all.  One layer gives ``prune_csr(..., total=K)``.

    Values on one GPU and of one dtype among float32 / float16 / bfloat16 take the device
    kernels (``ops.csr_topk_global``: the digit passes of a radix select walk all layers into one
    set of bins; the layers' new sizes are read back once) while every layer has at most 16384
    rows and the layers hold at most 2**31 - 1 entries together.  CPU tensors, other or mixed
    dtypes (every layer ranked as ``.float()`` then), more rows and
    ``enable_device_build(False)`` take the same rule in torch for the whole call: the keys of
    all layers in one array, one stable descending argsort, the first K split at the layer
    boundaries.  Both give the same integers and value bits."""
    layers = [tuple(layer) for layer in layers]
    for layer in layers:
        if len(layer) != 4:
            raise ValueError("prune_csr_global: a layer is (values, row_offsets, column_indices, n), got "
                             f"{len(layer)} elements")
    values = [layer[0].detach() for layer in layers]
    row_offsets, column_indices = [layer[1] for layer in layers], [layer[2] for layer in layers]
    count = ops.check_csr_topk_global_arguments(values, row_offsets, column_indices, total)
    if not layers:
        return []
    if _csr_topk_global_served(values, row_offsets):
        return ops.csr_topk_global(values, row_offsets, column_indices, count)
    native = values[0].dtype in _TOPK_DTYPES and all(v.dtype == values[0].dtype for v in values)
    keys = torch.cat([magnitude_keys(v if native else v.float()) for v in values])
    order = torch.argsort(keys, descending=True, stable=True)   # key descending, then layer, then index
    kept = torch.sort(order[:count]).values
    sizes = [v.numel() for v in values]
    bounds = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    cuts = torch.searchsorted(kept, bounds.to(kept.device)).tolist()   # the one read of the new sizes
    results = []
    for l, v in enumerate(values):
        source = kept[cuts[l]:cuts[l + 1]] - int(bounds[l])
        results.append(_csr_from_source(v, _entry_rows(row_offsets[l], sizes[l]), row_offsets[l].numel() - 1,
                                        column_indices[l], source))
    return results


def prune_layers_to(modules, density=None, nonzeros=None, optimizer=None):
    """One step of GLOBAL magnitude pruning over a list of ``SparseLinear``: the layers' values
    are ranked together and the K of largest ``|values|`` over all of them stay
    (``prune_csr_global``; ties to the layer listed first, then to the lower entry index).
    ``density`` is a share of all positions, ``K = round(density * sum out_l * in_l)``;
    ``nonzeros`` is K itself.  Give exactly one of the two.

    ``K`` at or above the current number of entries changes nothing: the same Parameters, every
    ``source = arange(nnz_l)``.  Otherwise EVERY listed layer gets a new, shorter ``values``
    ``nn.Parameter`` (the old one's ``requires_grad``, no ``.grad``), kept entries bit for bit,
    and new index tensors (the old ones are unregistered, never written to, the new ones
    registered as static) -- also a layer that happened to keep all its entries.
    Global pruning can EMPTY a layer: nothing keeps a layer of small weights from losing every
    entry; its forward pass then returns zeros.  ``dense_grad`` is left alone.

    A dense model enters the same way: ``SparseLinear.from_dense(weight, density=1.0)`` per
    layer, then this call -- there is no separate dense variant.

    Returns the list of ``source`` tensors, int64 ``[new nnz_l]``, ascending: for every new
    entry its index in the layer's old ``values``.  With ``optimizer=`` the state of every
    layer's old Parameter is handed to the new one (``remap_optimizer_state``)."""
    modules = list(modules)
    count = _count_of("prune_layers_to", density, nonzeros,
                      sum(module.output_features * module.input_features for module in modules))
    olds = [module.values for module in modules]
    if count >= sum(old.numel() for old in olds):
        return [torch.arange(old.numel(), dtype=torch.int64, device=old.device) for old in olds]
    with torch.no_grad():
        results = prune_csr_global(
            [(old.detach(), module.row_offsets, module.column_indices, module.input_features)
             for old, module in zip(olds, modules)], count)
        sources = []
        for module, old, (row_indices, row_offsets, column_indices, values, source) in zip(modules, olds, results):
            module._install_topology(values, row_indices, row_offsets, column_indices, into_parameter=False)
            if optimizer is not None:
                remap_optimizer_state(optimizer, old, module.values, source)
            sources.append(source)
    return sources


def gradual_density(step, begin_step, end_step, initial_density, final_density):
    """The density at ``step`` of the cubic schedule of gradual magnitude pruning (Zhu & Gupta,
    "To prune, or not to prune", 2017): ``d_f + (d_i - d_f) * (1 - (t - t0) / (t1 - t0)) ** 3``
    between ``begin_step`` t0 and ``end_step`` t1, ``initial_density`` d_i up to t0 and
    ``final_density`` d_f from t1 on.  A pure function of Python floats: pass the result to
    ``SparseLinear.prune_to(density=...)`` every few hundred steps."""
    if end_step < begin_step:
        raise ValueError(f"gradual_density: end_step {end_step} is before begin_step {begin_step}")
    if step <= begin_step:
        return float(initial_density)
    if step >= end_step:
        return float(final_density)
    left = 1.0 - (step - begin_step) / (end_step - begin_step)
    return float(final_density + (initial_density - final_density) * left ** 3)


def remap_optimizer_state(optimizer, old_parameter, new_parameter, source):
    """Hands an optimizer's state over a topology step.  ``source`` [new nnz] (int64) is what
    ``SparseLinear.prune_to`` / ``update_topology`` / ``rigl_update`` return: for every new
    entry its index in the old ``values``, or -1 for a grown one.

    Every tensor in ``optimizer.state[old_parameter]`` of ``old_parameter``'s shape (momentum
    buffer, Adam's moments) becomes ``where(source >= 0, state[source], 0)`` at
    ``new_parameter``'s length -- a copy of bits for carried entries, zero for grown ones; other
    entries (``step``) are kept.  The state moves to the key ``new_parameter`` and
    ``new_parameter`` takes ``old_parameter``'s slot in ``optimizer.param_groups``.  With
    ``old_parameter is new_parameter`` (after ``update_topology``, which writes into the
    Parameter) only the tensors are rewritten.  Plain torch indexing."""
    source = source.to(torch.int64)
    if source.dim() != 1 or source.numel() != new_parameter.numel():
        raise ValueError(f"remap_optimizer_state: source should be [{new_parameter.numel()}], got "
                         f"{tuple(source.shape)}")
    if old_parameter is not new_parameter:
        slots = [(group, i) for group in optimizer.param_groups
                 for i, p in enumerate(group["params"]) if p is old_parameter]
        if not slots:
            raise ValueError("remap_optimizer_state: old_parameter is not in optimizer.param_groups")
        for group, i in slots:
            group["params"][i] = new_parameter
    state = optimizer.state.pop(old_parameter, None)
    if state is None:      # (no step taken yet: nothing to carry)
        return
    carried = source >= 0
    at = source.clamp(min=0)
    for name, t in list(state.items()):
        if torch.is_tensor(t) and t.shape == old_parameter.shape and t.dim() == 1:
            where = carried.to(t.device)
            bits = t.contiguous().view(_BIT_VIEWS[t.element_size()])
            moved = torch.where(where, bits[at.to(t.device)], torch.zeros(1, dtype=bits.dtype, device=t.device))
            state[name] = moved.view(t.dtype).reshape(new_parameter.shape)
    optimizer.state[new_parameter] = state


def generate_mask(m, n, device="cpu", sparsity=0.9, round_to=4, generator=None):
    """Random 0/1 mask with the nonzero count of modules/sparse_attention.py:25-36:
    ``int(m*n*sparsity)`` zeros rounded DOWN to a multiple of ``round_to``.
    ``generator`` (numpy Generator) makes it reproducible; the reference uses
    the unseeded global numpy RNG."""
    num_elements = m * n
    remainder = int(num_elements * sparsity) % round_to
    num_zeros = int(num_elements * sparsity) - remainder
    num_ones = num_elements - num_zeros
    mask = np.zeros(num_elements, dtype=np.int64)
    mask[:num_ones] = 1
    (generator or np.random.default_rng()).shuffle(mask)
    return torch.from_numpy(mask).reshape(m, n).to(device)


def dense_to_sparse_3d(mask):
    """Dense [b, s, s'] mask -> (row_indices [b, s], row_offsets [b, s + 1], column_indices
    [sum nnz], nonzeros): one CSR topology per batch element in the "many mask" layout of
    tests/transformer/utils.py:17-38 (each mask's offsets start at 0, column indices
    concatenated), int32 indices, `nonzeros` a host list.  A nonzero entry is attended.
    Also [b, 1, s, s'] (the reference's module squeezes its mask; only dim 1 is dropped
    here, so b = 1 keeps its batch dimension)."""
    if mask.dim() == 4:
        mask = mask.squeeze(1)
    if mask.dim() != 3:
        raise ValueError(f"expected a [b, s, s'] or [b, 1, s, s'] mask, got {tuple(mask.shape)}")
    if mask.size(0) >= 1 and _build_served(mask, mask.size(0), mask.size(1), mask.size(2)):
        row_indices, row_offsets, column_indices, nonzeros = ops.dense_to_csr(mask.detach(), False)
        return row_indices, row_offsets, column_indices, nonzeros.tolist()
    row_indices, row_offsets, column_indices, nonzeros = [], [], [], []
    for i in range(mask.size(0)):
        csr = (mask[i] != 0).to_sparse_csr()
        offsets = csr.crow_indices().to(torch.int32)
        row_offsets.append(offsets)
        row_indices.append(diffsort(offsets))
        column_indices.append(csr.col_indices().to(torch.int32))
        nonzeros.append(int(offsets[-1]))
    return (torch.stack(row_indices), torch.stack(row_offsets), torch.cat(column_indices), nonzeros)


_PATTERN_SLAB = 2 ** 24     # elements of the largest mask image the torch path of a pattern holds
_INT64_MAX = 2 ** 63 - 1


def _pattern_keys(first_row, rows, columns, seed, offset, device):
    """int64 [rows, columns]: ``key(R, C)`` of ``ops.attention_pattern_csr`` for the block rows
    ``first_row .. first_row + rows - 1`` and the block columns ``0 .. columns - 1``"""
    seed, block = int(seed) & 0xffffffffffffffff, (int(offset) & 0xffffffffffffffff) // 4
    index = dict(dtype=torch.int64, device=device)
    quads = torch.arange((columns + 3) // 4, **index)[None, :]
    block_rows = (torch.arange(first_row, first_row + rows, **index)[:, None]) & _LO32
    words = _philox4x32_10((seed & _LO32, seed >> 32),
                           (torch.full((1, 1), block & _LO32, **index), torch.full((1, 1), block >> 32, **index),
                            quads, block_rows))
    return torch.stack(words, dim=2).reshape(rows, -1)[:, :columns] & 0x7fffffff


class AttentionPattern:
    """A structured attention pattern -- sliding and dilated windows (Longformer, Sparse
    Transformer), block-local attention, "fixed" summary columns, global tokens, BigBird's random
    blocks, and the causal form of each -- as a rule that is built straight into a CSR topology:
    ``SparseAttention(..., pattern=AttentionPattern(window=256, causal=True))``.

    The rule is ``ops.attention_pattern_csr``'s: row r sits at ``p = r + offset``, ``d = c - p``,
    and (r, c) is kept iff (not ``causal`` or d <= 0) and a component keeps it -- ``window``
    (``(left, right)`` or an int) with ``dilation``, ``block``, ``summary=(stride, width)``,
    ``global_tokens`` (a count or positions; ``global_rows``: their rows are full as well),
    ``random_blocks=(rb, probability)``.  The arguments are checked here
    (``ops.check_pattern_arguments``); positions are checked against n when a pattern is built."""

    def __init__(self, window=None, dilation=1, block=0, global_tokens=None, global_rows=True, summary=None,
                 random_blocks=None, causal=False):
        self.arguments = dict(window=window, dilation=dilation, block=block, global_tokens=global_tokens,
                              global_rows=global_rows, summary=summary, random_blocks=random_blocks, causal=causal)
        self.rule = ops.check_pattern_arguments("AttentionPattern", **self.arguments)

    def __repr__(self):
        given = ", ".join(f"{k}={v!r}" for k, v in self.arguments.items()
                          if v is not None and not (k == "dilation" and v == 1) and not (k == "block" and v == 0)
                          and not (k == "global_rows" and v is True) and not (k == "causal" and v is False))
        return f"AttentionPattern({given})"

    @property
    def random(self):
        """whether the pattern draws random blocks (and so has an ``rng_state``)"""
        return self.rule["random_blocks"] is not None

    def _state(self, op, device, rng_state):
        """(seed, offset, state tensor) of a torch-path build: the ``rng_state`` given or a fresh
        draw (``_draw_philox_state``); Nones for a pattern without random blocks"""
        if not self.random:
            return None, None, None
        if rng_state is None:
            seed, offset = _draw_philox_state(device)
            state = torch.tensor([seed, offset], dtype=torch.int64, device=device)
        else:
            state = ops.pattern_rng_state(op, rng_state)
            seed, offset = (int(v) for v in state.tolist())
        if offset % 4 != 0:
            raise ValueError(f"{op}: the offset of rng_state must be a multiple of 4, got {offset}")
        return seed, offset, state

    def _mask_rows(self, first, last, n, offset, flags, seed, rng_offset, device):
        """bool [last - first, n]: the rule at the rows ``first .. last - 1``"""
        rule = self.rule
        index = dict(dtype=torch.int64, device=device)
        rows = torch.arange(first, last, **index)[:, None]
        p = rows + offset
        c = torch.arange(n, **index)[None, :]
        d = c - p
        keep = torch.zeros(last - first, n, dtype=torch.bool, device=device)
        if rule["window"] is not None:
            dilation = min(rule["dilation"], _INT64_MAX)
            left, right = (min(w * rule["dilation"], _INT64_MAX) for w in rule["window"])
            keep |= (d >= -left) & (d <= right) & (d % dilation == 0)
        if rule["block"] > 0:
            b = min(rule["block"], _INT64_MAX)
            keep |= torch.div(c, b, rounding_mode="floor") == torch.div(p, b, rounding_mode="floor")
        if rule["summary"] is not None:
            stride, width = rule["summary"]
            # (a stride beyond int64 is beyond every column: c mod stride is c)
            keep |= (c % min(stride, _INT64_MAX)) >= min(stride - width, _INT64_MAX)
        if flags is not None:
            keep |= flags[None, :]
            if rule["global_rows"] and n > 0:
                keep |= (p >= 0) & (p < n) & flags[p.clamp(0, n - 1)]
        if rule["random_blocks"] is not None:
            rb, threshold = rule["random_blocks"]
            rb = min(rb, _INT64_MAX)
            first_block, last_block = first // rb, (last - 1) // rb
            keys = _pattern_keys(first_block, last_block - first_block + 1, (n - 1) // rb + 1 if n > 0 else 0,
                                 seed, rng_offset, device)
            block_rows = torch.div(rows[:, 0], rb, rounding_mode="floor") - first_block
            block_columns = torch.div(c[0], rb, rounding_mode="floor")
            keep |= (keys < threshold)[block_rows][:, block_columns]
        if rule["causal"]:
            keep &= d <= 0
        return keep

    def dense_mask(self, m, n=None, offset=0, device="cpu", rng_state=None):
        """bool [m, n]: the rule itself, in torch -- for tests and for looking at a pattern.  A
        pattern with random blocks needs the ``rng_state`` (int64 [2]) of the build it shows."""
        op = "AttentionPattern.dense_mask"
        m, n, offset = ops.check_pattern_sizes(op, m, m if n is None else n, offset)
        device = torch.device(device)
        if self.random and rng_state is None:
            raise ValueError(f"{op}: a pattern with random_blocks needs the rng_state of the build it shows "
                             f"(build(..., return_rng_state=True))")
        seed, rng_offset, _ = self._state(op, device, rng_state)
        flags = ops.pattern_global_flags(op, self.rule["global_tokens"], n, device)
        return self._mask_rows(0, m, n, offset, flags, seed, rng_offset, device)

    def build(self, m, n=None, offset=0, device=None, rng_state=None, return_rng_state=False):
        """-> (row_indices, row_offsets, column_indices), int32, of the pattern over ``m`` query
        rows and ``n`` key columns (default m) at that ``offset`` (``n - m`` aligns the last query
        with the last key: decoding against a cache).

        A GPU ``device`` takes the device kernels (``ops.attention_pattern_csr``: four launches,
        one synchronisation, no ``[m, n]`` array) where ``capi.attention_pattern_launch_shape``
        serves the sizes; the CPU, ``enable_device_build(False)`` and the sizes beyond (more than
        16384 rows, ``m * n`` above INT_MAX, ``|offset| >= 2**30``) take the same rule in torch,
        in row slabs of at most 2**24 mask elements -- the same integers.  ``rng_state`` (int64
        [2] {seed, offset}) reproduces a pattern with random blocks on any path; without one a GPU
        call draws 4 from the device's default generator (``torch.manual_seed`` makes runs
        repeat), a CPU call a seed from torch's CPU generator.  ``return_rng_state``: the state
        used (None without random blocks) is appended."""
        op = "AttentionPattern.build"
        m, n, offset = ops.check_pattern_sizes(op, m, m if n is None else n, offset)
        device = torch.device("cpu" if device is None else device)
        if _served(device, "attention_pattern_launch_shape", m, n, offset):
            row_indices, row_offsets, column_indices, state = ops.attention_pattern_csr(
                m, n, offset, device=device, rng_state=rng_state, **self.arguments)
        else:
            seed, rng_offset, state = self._state(op, device, rng_state)
            flags = ops.pattern_global_flags(op, self.rule["global_tokens"], n, device)
            slab = max(1, _PATTERN_SLAB // max(n, 1))
            counts, columns = [torch.zeros(1, dtype=torch.int64, device=device)], []
            for first in range(0, m, slab):
                mask = self._mask_rows(first, min(m, first + slab), n, offset, flags, seed, rng_offset, device)
                counts.append(mask.sum(dim=1))
                columns.append(mask.nonzero()[:, 1].to(torch.int32))
            row_offsets = torch.cumsum(torch.cat(counts), 0).to(torch.int32)
            column_indices = torch.cat(columns) if columns else torch.zeros(0, dtype=torch.int32, device=device)
            row_indices = diffsort(row_offsets)
        result = (row_indices, row_offsets, column_indices)
        return result + (state,) if return_rng_state else result
