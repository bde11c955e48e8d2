"""nn.Modules mirroring the reference's ``SparseLinear``
(modules/sparse_linear.py:69-89) and ``SparseAttention``
(modules/sparse_attention.py:38-128): same constructor arguments, attributes,
forward signatures and output layouts, so user code can switch imports.

Kept quirks (drop-in): ``SparseLinear.weight`` / ``bias`` are uninitialised
``torch.empty`` parameters, ``bias`` is never applied, the user must call
``setup_sparse_tensors()``; the topology tensors are plain attributes (not
buffers); ``SparseAttention.forward`` ignores its ``mask`` argument and uses
the fixed random mask drawn at construction.
Differences: the attention mask is created on the device given (default: the
current GPU) instead of a hard ``.cuda()``; ``differentiable_softmax=True``
opts in to a softmax with a gradient.
Additions: ``SparseLinear.from_dense`` builds a ready layer from a dense weight by
magnitude, ``SparseLinear.update_topology`` is one drop-and-grow step (SET, RigL),
``SparseLinear.collect_dense_grad`` / ``rigl_update`` gather RigL's grow scores in the backward,
``SparseLinear.prune_to`` is one step of gradual magnitude pruning (the layer becomes sparser),
``SparseLinear.random`` builds a ready layer with a uniformly random topology and a sparse-aware
initialisation, drawn on the device (with ``topology.erk_densities`` for the layers' densities:
the start of SET and RigL).
"""
import copy
import math

import torch
import torch.nn as nn

from . import functional, ops, topology
from .functional import (GroupProjectionFunction, HalfSparseLinearFunction, SparseAttentionFunction,
                         Sddmm, SparseLinearFunction, SparseSoftmax, Spmm)
from .topology import dense_to_sparse, dense_to_sparse_3d, generate_mask


class SparseLinear(nn.Module):
    """y[B, out, seq] = W_csr[out, in] @ x[B, seq, in]^T  (note the layout)."""

    def __init__(self, input_features, output_features):
        super().__init__()
        self.input_features = input_features
        self.output_features = output_features
        self.weight = nn.Parameter(torch.empty(output_features, input_features))
        self.bias = nn.Parameter(torch.empty(output_features))
        # RigL's grow scores (collect_dense_grad): None, or the [out, in] float32 dense weight
        # gradient summed over the backwards since it was cleared.  A plain attribute --
        # neither a Parameter nor a buffer: not in state_dict, not moved by .to().
        self.dense_grad = None
        self._collects_dense_grad = False

    def collect_dense_grad(self, enabled=True):
        """Arms (or disarms) the collection of the DENSE weight gradient: while armed, every
        backward through ``forward`` / ``project`` adds ``sum_b dy_b x_b`` -- ``[out, in]``
        float32, at the masked-out positions too -- into ``self.dense_grad``, as autograd
        adds into ``.grad``: the first backward keeps the kernel's tensor, later ones
        ``add_`` into it, so micro-batches and a layer used twice in one graph sum up.
        With half activations on the tile route the weight gradient's own launch stores it
        (its float32 tiles, whole: ``ops.half_linear_weight_gradient_dense``); otherwise one
        more tile launch (``ops.dense_weight_grad``).  The flag is looked at when the backward
        runs, so arming between forward and backward counts.  A disarmed layer launches what
        it always did.  Returns ``self``.

        Not collected: layers reached through ``SparseAttention``'s grouped self-attention
        projection (``GroupProjectionFunction``) or its ``half_storage`` projections
        (``functional.half_linear_rows``) -- their ``dense_grad`` stays None -- and armed
        layers inside ``graphs.capture_training_step`` (the attribute is rebound by Python
        code that a replay does not run)."""
        self._collects_dense_grad = bool(enabled)
        return self

    def zero_dense_grad(self):
        """Drops what ``collect_dense_grad`` gathered (``dense_grad = None``); stays armed."""
        self.dense_grad = None

    @torch.no_grad()
    def rigl_update(self, drop_fraction, per_row=False):
        """One RigL step from the collected gradient: ``update_topology(drop_fraction,
        grow_scores=self.dense_grad, per_row=per_row)`` -- drop by ``|values|``, grow where
        ``|dense_grad|`` is largest -- then ``dense_grad`` is cleared; the layer stays armed.
        Returns ``source`` as ``update_topology`` does.  RuntimeError if nothing was collected
        (not armed, no backward since the last clear, or a route that does not collect)."""
        if self.dense_grad is None:
            raise RuntimeError("rigl_update: no dense gradient collected -- call collect_dense_grad() "
                               "before the backward pass")
        source = self.update_topology(drop_fraction, grow_scores=self.dense_grad, per_row=per_row)
        self.dense_grad = None
        return source

    def setup_sparse_tensors(self):
        values, row_indices, row_offsets, column_indices = dense_to_sparse(self.weight)
        self.values = nn.Parameter(values)
        self.row_indices = row_indices
        self.row_offsets = row_offsets
        self.column_indices = column_indices
        # The module owns this pattern and never writes to it: transposed topology
        # and kernel plans are cached for as long as these tensors live.  (Replace
        # the pattern by calling setup_sparse_tensors() again -- do not write into
        # the index tensors through .data or a raw pointer: functional.py.)
        functional.register_static_topology(row_indices, row_offsets, column_indices)

    @classmethod
    def from_dense(cls, weight, density=None, nonzeros=None, per_row=False):
        """A sparse layer from a trained dense ``[out, in]`` weight (a ``nn.Linear.weight``) by
        magnitude: the ``round(density * out * in)`` (or ``nonzeros``) entries of largest
        ``|weight|`` are kept, ``per_row`` that share of every row
        (``topology.magnitude_prune``; on a GPU weight the selection and the CSR build run on
        the device without a host synchronisation).  The module lives on the weight's device,
        ``values`` is a Parameter in the weight's dtype, the topology is registered as static:
        ready to call.  As everywhere in this module ``weight`` and ``bias`` are uninitialised
        parameters and the bias is never applied -- a ``nn.Linear``'s bias is NOT carried over;
        add it behind the layer."""
        if weight.dim() != 2:
            raise ValueError(f"from_dense: expected an [out, in] weight, got {tuple(weight.shape)}")
        module = cls(weight.size(1), weight.size(0)).to(device=weight.device, dtype=weight.dtype)
        values, row_indices, row_offsets, column_indices = topology.magnitude_prune(
            weight.detach(), density=density, nonzeros=nonzeros, per_row=per_row)
        module._set_topology(nn.Parameter(values), row_indices, row_offsets, column_indices)
        return module

    @classmethod
    def random(cls, input_features, output_features, density=None, nonzeros=None, per_row=False,
               dtype=torch.float32, bound=None, device=None, rng_state=None):
        """A sparse layer with a uniformly random topology, for training sparse from scratch
        (SET, RigL): ``round(density * out * in)`` (or ``nonzeros``) positions of the matrix,
        ``per_row`` that share of every row -- exactly that many, every position equally likely
        -- and values uniform on ``[-bound, bound)``, by default ``bound = 1 / sqrt(entries per
        row)``: kaiming-uniform on the effective fan-in (``topology.random_csr`` states the
        rule).  On a GPU ``device`` pattern and values are drawn by the device kernels from the
        device's default generator (``torch.manual_seed``) without an ``[out, in]`` array and
        without a host synchronisation; ``rng_state`` (int64 [2]) reproduces a draw, on any
        device.  ``topology.erk_densities`` gives the layers of a model their densities.
        ``values`` is a Parameter of ``dtype``, the topology is registered as static: ready to
        call, and ``update_topology``, ``rigl_update`` and ``prune_to`` work on it.  As
        everywhere in this module ``weight`` and ``bias`` are uninitialised and unused."""
        device = torch.device("cpu" if device is None else device)
        module = cls(input_features, output_features).to(device=device, dtype=dtype)
        values, row_indices, row_offsets, column_indices = topology.random_csr(
            output_features, input_features, density=density, nonzeros=nonzeros, per_row=per_row, dtype=dtype,
            bound=bound, device=device, rng_state=rng_state)
        module._set_topology(nn.Parameter(values), row_indices, row_offsets, column_indices)
        return module

    def _set_topology(self, values, row_indices, row_offsets, column_indices):
        if values is not None:
            self.values = values
        self.row_indices = row_indices
        self.row_offsets = row_offsets
        self.column_indices = column_indices
        functional.register_static_topology(row_indices, row_offsets, column_indices)

    def _install_topology(self, values, row_indices, row_offsets, column_indices, into_parameter):
        """The end of a topology step: the new values are written INTO the ``values`` Parameter
        (``into_parameter``; same nnz) or replace it by a new one of its ``requires_grad``; the
        old index tensors are unregistered -- never written to -- and the new ones registered."""
        if into_parameter:
            self.values.copy_(values)
            values = None
        else:
            values = nn.Parameter(values, requires_grad=self.values.requires_grad)
        functional.unregister_static_topology(self.row_indices, self.row_offsets, self.column_indices)
        self._set_topology(values, row_indices, row_offsets, column_indices)

    def _grow_scores(self, grow_scores, generator):
        """``grow_scores`` ([out, in], checked) on the layer's device, or SET's uniform random
        scores drawn with ``generator`` on its own device"""
        shape, device = (self.output_features, self.input_features), self.values.device
        if grow_scores is None:
            where = generator.device if generator is not None else device
            return torch.rand(*shape, generator=generator, device=where).to(device)
        if tuple(grow_scores.shape) != shape:
            raise ValueError(f"update_topology: grow_scores should be [{shape[0]}, {shape[1]}], got "
                             f"{tuple(grow_scores.shape)}")
        return grow_scores.detach().to(device)

    @torch.no_grad()
    def update_topology(self, drop_fraction, grow_scores=None, generator=None, per_row=False):
        """One drop-and-grow step of dynamic sparse training (SET, RigL) with an unchanged
        number of entries ``nnz``, ranked over the whole matrix or, ``per_row=True``, inside
        every row (below).  Matrix-wide:

        1. ``d = int(drop_fraction * nnz)`` entries are dropped: the ``nnz - d`` of largest
           ``|values|`` are kept, ties to the lower entry index.
        2. ``d`` entries are grown where ``|grow_scores|`` (``[out, in]``, e.g. the magnitude of
           the dense weight gradient, RigL) is largest outside the kept positions, ties to the
           lower flat index; non-finite scores count as the largest finite value;
           ``grow_scores=None`` draws uniform random scores with ``generator`` (SET) into an
           ``[out, in]`` float32 array -- ``set_update`` is SET's step without that array.
           Positions dropped in step 1 are eligible.
        3. The new values are written INTO the existing ``values`` Parameter -- an optimizer
           keeps its handle -- kept ones bit for bit, grown ones exactly 0.  The index tensors
           are replaced by new ones (the old ones are unregistered, never written to), so no
           cached plan, transposed topology or half image of the old pattern serves the new.

        Returns ``source``, int64 ``[nnz]``: for every new entry the index of that entry in the
        old ``values``, or -1 where it was grown -- to permute or reset optimizer state.
        ``d == 0`` changes nothing (``source = arange(nnz)``).

        The step is one ``topology.regrow_total`` call.  On a GPU module it runs on the layer's
        own arrays on the device: a fixed number of kernel launches, no ``[out, in]`` temporary
        (the only dense tensor is ``grow_scores``, or the random scores of SET) and no host
        synchronisation.

        ``per_row=True`` (SET per neuron, RigL with a fixed fan-in): every row keeps its
        length.  Row r of ``len_r`` entries drops ``d_r = floor(float64(len_r) *
        drop_fraction)`` of them -- its entries of smallest ``|values|``, ties dropping the
        higher column -- and grows ``d_r`` where ``|grow_scores[r]|`` is largest outside the
        kept columns, ties to the lowest column; a layer from ``from_dense(per_row=True)``
        stays row balanced.  ``grow_scores`` is passed as it is: the sign is ignored and NaN and
        inf count as the dtype's largest finite value inside the rule
        (``topology.regrow_per_row``, which is one kernel launch without a host
        synchronisation for a GPU module).  Values, ``source`` and the replaced index tensors
        are as in 3; ``row_indices`` and ``row_offsets`` are replaced by clones.  Where not
        even a full row could drop an entry (``floor(in_features * drop_fraction) == 0``)
        nothing changes.

        The dense weight gradient for RigL's ``grow_scores`` comes from the layer itself:
        ``collect_dense_grad()`` before the backward pass leaves it in ``dense_grad``, and
        ``rigl_update`` is this call on it; ``ops.dense_weight_grad(dy, x)`` computes it from
        operands of your own."""
        if per_row:
            return self._update_topology_per_row(drop_fraction, grow_scores, generator)
        values = self.values.detach()
        nnz = values.numel()
        device = values.device
        d = int(drop_fraction * nnz)
        if not 0 <= d <= nnz:
            raise ValueError(f"update_topology: drop_fraction {drop_fraction} is outside 0 .. 1")
        if d == 0:
            return torch.arange(nnz, dtype=torch.int64, device=device)
        row_indices, row_offsets, column_indices, new_values, source = topology.regrow_total(
            values, self.row_offsets, self.column_indices, d, self._grow_scores(grow_scores, generator))
        self._install_topology(new_values, row_indices, row_offsets, column_indices, into_parameter=True)
        return source

    def _update_topology_per_row(self, drop_fraction, grow_scores, generator):
        values = self.values.detach()
        if not 0.0 <= drop_fraction <= 1.0:
            raise ValueError(f"update_topology: drop_fraction {drop_fraction} is outside 0 .. 1")
        # (given scores are checked before anything returns; random ones are drawn only for a step)
        scores = None if grow_scores is None else self._grow_scores(grow_scores, generator)
        # len_r <= in_features is known on the host; the lengths themselves are not read back
        if math.floor(float(self.input_features) * drop_fraction) == 0:
            return torch.arange(values.numel(), dtype=torch.int64, device=values.device)
        if scores is None:
            scores = self._grow_scores(None, generator)
        lengths = self.row_offsets[1:] - self.row_offsets[:-1]
        drop_counts = torch.floor(lengths.to(torch.float64) * drop_fraction).to(torch.int32)
        column_indices, new_values, source = topology.regrow_per_row(
            values, self.row_offsets, self.column_indices, drop_counts, scores)
        self._install_topology(new_values, self.row_indices.clone(), self.row_offsets.clone(), column_indices,
                               into_parameter=True)
        return source

    @torch.no_grad()
    def set_update(self, drop_fraction, per_row=False, grow_bound=None, rng_state=None, return_rng_state=False):
        """One SET step (Mocanu et al. 2018) without a dense tensor: ``update_topology(drop_fraction,
        grow_scores=None, per_row=per_row)`` with the random grow scores computed where they are
        compared instead of drawn into an ``[out, in]`` array.  The drop counts, the shortcuts
        (``d == 0``, ``floor(in_features * drop_fraction) == 0``: nothing changes, ``source =
        arange(nnz)``, no state is drawn), the error messages, the kept entries, the ties and
        the installation -- the new values INTO the ``values`` Parameter, new index tensors --
        are those of ``update_topology``.

        The scores are Philox keys of 30 bits, ``topology.regrow_total_random`` /
        ``regrow_per_row_random`` state the rule: the step is exactly ``update_topology`` under
        float32 ``grow_scores`` whose bits are those keys.  ``grow_bound=None`` grows entries of
        exactly 0 as ``update_topology`` does; a finite ``grow_bound >= 0`` re-initialises them
        uniformly on ``[-grow_bound, grow_bound)`` as ``SparseLinear.random(bound=)`` would have
        drawn those positions (SET as published).  On a GPU module the step runs on the layer's
        own arrays: a fixed number of launches, no host synchronisation, and the state comes
        from the device's default generator (``torch.manual_seed``); ``rng_state`` (int64 [2])
        reproduces a step, on any device.

        Returns ``source`` as ``update_topology`` does, and ``(source, rng_state)`` with
        ``return_rng_state`` (``rng_state`` is None where a shortcut drew nothing)."""
        values = self.values.detach()
        nnz, n = values.numel(), self.input_features
        unchanged = None
        if per_row:
            if not 0.0 <= drop_fraction <= 1.0:
                raise ValueError(f"update_topology: drop_fraction {drop_fraction} is outside 0 .. 1")
            # len_r <= in_features is known on the host; the lengths themselves are not read back
            if math.floor(float(n) * drop_fraction) == 0:
                unchanged = torch.arange(nnz, dtype=torch.int64, device=values.device)
        else:
            d = int(drop_fraction * nnz)
            if not 0 <= d <= nnz:
                raise ValueError(f"update_topology: drop_fraction {drop_fraction} is outside 0 .. 1")
            if d == 0:
                unchanged = torch.arange(nnz, dtype=torch.int64, device=values.device)
        if unchanged is not None:
            return (unchanged, None) if return_rng_state else unchanged
        if per_row:
            lengths = self.row_offsets[1:] - self.row_offsets[:-1]
            drop_counts = torch.floor(lengths.to(torch.float64) * drop_fraction).to(torch.int32)
            column_indices, new_values, source, state = topology.regrow_per_row_random(
                values, self.row_offsets, self.column_indices, drop_counts, n, grow_bound=grow_bound,
                rng_state=rng_state, return_rng_state=True)
            row_indices, row_offsets = self.row_indices.clone(), self.row_offsets.clone()
        else:
            row_indices, row_offsets, column_indices, new_values, source, state = topology.regrow_total_random(
                values, self.row_offsets, self.column_indices, d, n, grow_bound=grow_bound, rng_state=rng_state,
                return_rng_state=True)
        self._install_topology(new_values, row_indices, row_offsets, column_indices, into_parameter=True)
        return (source, state) if return_rng_state else source

    @torch.no_grad()
    def prune_to(self, density=None, nonzeros=None, per_row=False):
        """One step of gradual magnitude pruning: the layer keeps its entries of largest
        ``|values|`` and becomes sparser.  ``density``: ``round(density * out * in)`` entries of
        the matrix stay, or ``per_row`` ``round(density * in)`` of every row (a shorter row
        keeps what it has); ``nonzeros``: that number itself (of every row, ``per_row``).  Give
        exactly one of the two.  Among equal magnitudes the lower entry index stays
        (``topology.prune_csr``: on a GPU module the selection runs over the layer's own values
        on the device, no dense image is built).

        A matrix-wide target at or above the current ``nnz`` changes nothing: the same
        Parameter, ``source = arange(nnz)``.  Otherwise ``values`` is REPLACED by a new, shorter
        ``nn.Parameter`` (the old one's ``requires_grad``, no ``.grad``), kept entries bit for
        bit; the index tensors are replaced by new ones (the old ones are unregistered, never
        written to), so no cached plan, transposed topology or half image of the old pattern
        serves the new one.  ``dense_grad`` is left alone.

        Returns ``source``, int64 ``[new nnz]``, ascending: for every new entry its index in the
        old ``values``.  An optimizer holds the old Parameter; hand its state over::

            old = layer.values
            source = layer.prune_to(density=topology.gradual_density(step, t0, t1, d_i, d_f))
            topology.remap_optimizer_state(optimizer, old, layer.values, source)
        """
        out_f, in_f = self.output_features, self.input_features
        count = topology._count_of("prune_to", density, nonzeros, in_f if per_row else out_f * in_f)
        old = self.values
        nnz = old.numel()
        if not per_row and count >= nnz:
            return torch.arange(nnz, dtype=torch.int64, device=old.device)
        row_indices, row_offsets, column_indices, values, source = topology.prune_csr(
            old.detach(), self.row_offsets, self.column_indices, in_f,
            per_row=count if per_row else None, total=None if per_row else count)
        self._install_topology(values, row_indices, row_offsets, column_indices, into_parameter=False)
        return source

    def forward(self, x):
        # [B, S, in] -> the k-major operand [B, in, S] of left_spmm: the reference's
        # `x.transpose(1, 2).contiguous()` (modules/sparse_linear.py:89) as one tiled
        # kernel (same values, same layout)
        if x.dtype in (torch.float16, torch.bfloat16) and x.dim() == 3:
            # half-precision activations stay in half: the k-major operand is one tiled
            # pass without widening, the product reads it as it is (at layer densities on
            # the matrix cores, csrc/spmm_mfma.hip), and under autograd it is what the
            # backward pass keeps
            if torch.is_grad_enabled() and (x.requires_grad or self.values.requires_grad):
                return HalfSparseLinearFunction.apply(
                    self.output_features, self.input_features, self.values, self.row_indices,
                    self.row_offsets, self.column_indices, x, self)
            values = self.values.detach()
            if x.is_cuda and ops.half_linear_supported(self.output_features, self.input_features, x.size(1),
                                                       x.size(0), self.column_indices.numel(), values.dtype,
                                                       x.dtype):
                image = ops.half_linear_image(self.output_features, self.input_features, values,
                                              self.row_offsets, self.column_indices, x.dtype)
                return ops.half_linear_forward(self.output_features, image, values.dtype, x)
            return functional._linear(self.output_features, self.input_features, values,
                                      self.row_indices, self.row_offsets, self.column_indices,
                                      ops.transpose_last2(x))
        return self.project(functional._to_operand(x))

    def project(self, dense, split_rows=0, dense_blocks=0):
        """``W @ dense`` for an operand that is already k-major: [B, in, S] ->
        [B, out, S].  (SparseAttention chains its layout passes and calls this.)
        ``split_rows = d``: the product comes back head split, [B * out/d, S, d],
        written in that order by the kernel (no layout pass of its own).
        ``dense_blocks = d``: `dense` is given as [B * in/d, d, S] (merged heads, the
        same memory); see functional.SparseLinearFunction."""
        needs_grad = torch.is_grad_enabled() and (dense.requires_grad or self.values.requires_grad)
        if not needs_grad:
            # forward only: no autograd node.  (The weight's pattern is static: its
            # topology pre-pass comes from the plan cache, functional.PlanCache,
            # which is keyed on the identity and version of the index tensors.)
            if dense_blocks:
                dense = dense.reshape(-1, self.input_features, dense.size(-1))
            return functional._linear(self.output_features, self.input_features,
                                      self.values.detach(), self.row_indices, self.row_offsets,
                                      self.column_indices, dense, split_rows)
        return SparseLinearFunction.apply(
            self.output_features, self.input_features, self.values, self.row_indices,
            self.row_offsets, self.column_indices, dense, split_rows, dense_blocks,
            self)


def get_clones(module, num_of_deep_copies):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(num_of_deep_copies)])


class SparseAttention(nn.Module):
    """Multi-head attention whose score matrix only exists at the nonzeros of a
    fixed random mask: SDDMM -> sparse softmax -> SpMM, with four SparseLinear
    projections.  ``attention_dropout`` = p: dropout on the attention probabilities (between
    the softmax and the product with V) while the module is in training mode, on every path:
    inside the fused kernels' online softmax, or sparse_dropout between the softmax and the
    SpMM of the separate-operator path (the masks are the same: functional.sparse_dropout).
    ``fused_backward=True``: training runs the fused forward and the fused backward
    (functional.FusedBackwardAttentionFunction), float32 only, head dimension 64 or 128.
    ``pattern`` (a topology.AttentionPattern: windows, blocks, summary columns, global tokens,
    random blocks, causal) replaces the random mask by a structured one, built straight to CSR
    on the module's device with no dense mask (``pattern_rng_state`` reproduces its random
    blocks); ``set_pattern`` swaps it later."""

    def __init__(self, num_heads, embedding_size, max_sequence_length=512, device=None,
                 sparsity=0.9, mask_generator=None, differentiable_softmax=False,
                 fused_inference=True, low_memory_training=False, fused_training=None,
                 half_storage=False, attention_dropout=0.0, fused_backward=False,
                 pattern=None, pattern_rng_state=None):
        super().__init__()
        self.attention_dropout = ops.check_dropout_p(attention_dropout)
        if half_storage and fused_backward:
            raise ValueError("fused_backward serves float32 attention only; it cannot be "
                             "combined with half_storage=True")
        assert embedding_size % num_heads == 0, \
            "Model dimension must be divisible by the number of heads."
        self.head_dim = embedding_size // num_heads
        self.num_heads = num_heads
        self.linears = get_clones(SparseLinear(embedding_size, embedding_size), 4)

        self.m = max_sequence_length
        self.n = max_sequence_length
        device = torch.device("cuda") if device is None else device
        self.pattern = self.pattern_rng_state = None
        if pattern is not None:
            # a structured pattern (topology.AttentionPattern) is built straight to CSR: no
            # dense mask exists, `sparsity` and `mask_generator` are unused
            self.mask2d = None
            self._pattern_device = device
            self.set_pattern(pattern, pattern_rng_state)
        else:
            self.mask2d = generate_mask(self.m, self.n, device, sparsity=sparsity,
                                        generator=mask_generator)
            _, self.row_indices, self.row_offsets, self.column_indices = dense_to_sparse(self.mask2d)
            functional.register_static_topology(self.row_indices, self.row_offsets, self.column_indices)

        self.sddmm = Sddmm.apply
        self.spmm = Spmm.apply
        self.differentiable_softmax = differentiable_softmax
        # forward-only calls (no gradient wanted) take the one-kernel attention
        self.fused_inference = fused_inference
        # Training that keeps NOTHING of size [B*H, nnz] between forward and backward: the
        # one-kernel forward, and a backward that recomputes scores and weights before it
        # runs the separate operators (and, unlike the reference's raw softmax call, the
        # gradient reaches Q and K).  A MEMORY option, not a speed one: measured at config 3
        # it is slower than the separate operators that keep their weights (0.75 against
        # 0.66 ms, round 4) -- hence the name; `fused_training` (rounds 1-3) is kept as an
        # alias of the same flag.
        self.low_memory_training = bool(low_memory_training if fused_training is None
                                        else fused_training)
        # The three input projections on side streams (their grids are small).  Off:
        # measured at config 3, the event traffic costs more than the overlap gives
        # (forward 0.253 ms on one stream, 0.28-0.30 ms on three; fwd+bwd 1.04 / 1.11).
        self.parallel_projections = False
        # float16 / bfloat16 inputs (all three of one type) stay in that type through the
        # forward pass: see _forward_half_storage.  Off: today's widening path.
        self.half_storage = bool(half_storage)
        # Training on the fused forward and the fused backward: nothing of
        # size [B*H, nnz] exists at any time, the backward included.  Takes precedence over
        # low_memory_training; shapes the fused backward does not serve (head dimension other
        # than 64 or 128) train as low_memory_training does.
        self.fused_backward = bool(fused_backward)

    def set_pattern(self, pattern, rng_state=None):
        """Swaps the module's topology for that of ``pattern`` (topology.AttentionPattern) over
        its ``max_sequence_length`` rows and columns, on the device of the topology in use.
        The new index tensors are registered as static and the old ones unregistered, which
        sends the plans and transposes cached for them out of use.  ``rng_state`` reproduces a
        pattern with random blocks; the state used is kept in ``pattern_rng_state`` (None
        without random blocks)."""
        if not isinstance(pattern, topology.AttentionPattern):
            raise TypeError(f"set_pattern: expected a topology.AttentionPattern, got {type(pattern).__name__}")
        old = [getattr(self, name, None) for name in ("row_indices", "row_offsets", "column_indices")]
        device = old[1].device if old[1] is not None else self._pattern_device
        row_indices, row_offsets, column_indices, state = pattern.build(
            self.m, self.n, device=device, rng_state=rng_state, return_rng_state=True)
        if old[1] is not None:
            functional.unregister_static_topology(*old)
        self.row_indices, self.row_offsets, self.column_indices = row_indices, row_offsets, column_indices
        functional.register_static_topology(self.row_indices, self.row_offsets, self.column_indices)
        self.pattern, self.pattern_rng_state, self.mask2d = pattern, state, None
        return self

    @property
    def fused_training(self):   # the flag's name in rounds 1-3
        return self.low_memory_training

    @fused_training.setter
    def fused_training(self, value):
        self.low_memory_training = bool(value)

    def attention(self, query, key, value, mask):
        """[B, H, S, D] operands, as modules/sparse_attention.py:66-82."""
        return self._attention3d(self.four_d_to_three_d(query), self.four_d_to_three_d(key),
                                 self.four_d_to_three_d(value))

    def _dropout_p(self):
        """The attention dropout in force: p in training mode, 0 in eval()."""
        return self.attention_dropout if self.training else 0.0

    def _attention3d(self, q3d, k3d, v3d, merged=False):
        """-> [B*H, S, D]; ``merged``: transposed, [B*H, D, S] (= [B, E, S], the k-major
        operand of the output projection), written that way by the last kernel where
        it can (the SpMM of the separate-operator path), else by a layout pass."""
        scale = 1.0 / math.sqrt(self.head_dim)
        p = self._dropout_p()
        needs_grad = torch.is_grad_enabled() and (
            q3d.requires_grad or k3d.requires_grad or v3d.requires_grad)
        if self.fused_inference and not needs_grad:
            out = functional._attention_forward(q3d, k3d, v3d, self.row_indices, self.row_offsets,
                                                self.column_indices, scale, p)[0]
            return functional.transpose_last2(out) if merged else out
        if self.fused_backward and needs_grad:
            out = functional.sparse_attention(q3d, k3d, v3d, self.row_indices, self.row_offsets,
                                              self.column_indices, scale, dropout_p=p,
                                              fused_backward=True)
            return functional.transpose_last2(out) if merged else out
        if self.low_memory_training:
            out = SparseAttentionFunction.apply(q3d, k3d, v3d, self.row_indices, self.row_offsets,
                                                self.column_indices, scale, p)
            return functional.transpose_last2(out) if merged else out

        # [B*H, nnz]: scores only at the mask's nonzeros
        ours = getattr(self.sddmm, "__self__", None) is Sddmm and \
            getattr(self.spmm, "__self__", None) is Spmm
        if ours:   # gradients of q, k, v leave the kernels in the projections' layout
            scores = Sddmm.apply(self.m, self.n, self.row_indices, self.row_offsets,
                                 self.column_indices, q3d, k3d, merged)
        else:
            scores = self.sddmm(self.m, self.n, self.row_indices, self.row_offsets,
                                self.column_indices, q3d, k3d)
        # the reference divides the scores in a pass of its own
        # (modules/sparse_attention.py:72); here the softmax kernel applies it
        softmax = (SparseSoftmax.apply if self.differentiable_softmax
                   else ops.sparse_softmax_scaled)
        attention_weights = softmax(scores, self.row_indices, self.row_offsets,
                                    self.column_indices, scale)
        if p > 0.0:   # (between the softmax and the product with V, as Megatron's attention_dropout)
            attention_weights = functional.sparse_dropout(attention_weights, p)
        # [B*H, S, D] ([B*H, D, S] when merged)
        if merged and ours:
            return Spmm.apply(self.m, self.n, attention_weights, self.row_indices,
                              self.row_offsets, self.column_indices, v3d, True, True)
        out = self.spmm(self.m, self.n, attention_weights, self.row_indices, self.row_offsets,
                        self.column_indices, v3d)
        return functional.transpose_last2(out) if merged else out

    @staticmethod
    def four_d_to_three_d(tensor):
        n, c, h, w = tensor.size()
        return tensor.reshape(n * c, h, w)

    def forward(self, query, key, value, mask=None):
        """Same values and layouts as modules/sparse_attention.py:105-128 ([B, S, E] in,
        [B, S, E] out as a transposed view of [B, E, S]); the layout passes are chained:

          reference, per projection      here
          x^T copy (SparseLinear)        transpose_last2(x)            [B, E, S]
          y^T copy                       (none)
          head-split copy                transpose_last2(y as [B*H, D, S])  -> [B*H, S, D]
          context: head-merge copy       transpose_last2(ctx)          -> [B*H, D, S] = [B, E, S],
          + x^T copy of the last layer   which IS the last layer's k-major operand

        i.e. 7 passes (5 when query, key and value are one tensor) instead of 11, each
        one tiled kernel.  (`parallel_projections` runs the three input projections on
        side streams; measured slower at config 3, off by default.)"""
        if self.half_storage and query.dtype in (torch.float16, torch.bfloat16) and \
                key.dtype == query.dtype and value.dtype == query.dtype and query.dim() == 3:
            return self._forward_half_storage(query, key, value)
        batch_size, seq = query.size(0), query.size(1)
        heads, dim = self.num_heads, self.head_dim
        inputs = (query, key, value)
        if query is key and key is value:
            shared = functional._to_operand(query)
            operands = (shared, shared, shared)
        else:
            operands = tuple(functional._to_operand(x) for x in inputs)

        def head_split(projected):   # [B, H*D, S] -> [B*H, S, D]
            return functional.transpose_last2(projected.reshape(batch_size * heads, dim, seq))

        if query is key and key is value and not self.parallel_projections:
            # self-attention: the three projections of the one input in ONE launch
            # (one copy of the input's panel per workgroup), each stored head split
            q3d, k3d, v3d = self._project_group(self.linears[:3], operands[0], dim)
        elif not (query.is_cuda and self.parallel_projections):
            # (the projection kernel stores its product head split: [B*H, S, D])
            q3d, k3d, v3d = (net.project(d, split_rows=dim)
                             for net, d in zip(self.linears, operands))
        else:
            # (under autograd the backward of each projection runs on the stream its
            # forward ran on, so the three weight / input gradients overlap as well)
            main = torch.cuda.current_stream(query.device)
            results = [None, None, None]
            results[0] = head_split(self.linears[0].project(operands[0]))
            for i in (1, 2):
                side = self._side_stream(i, query.device)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    results[i] = head_split(self.linears[i].project(operands[i]))
                    results[i].record_stream(main)
            for i in (1, 2):
                main.wait_stream(self._side_stream(i, query.device))
            q3d, k3d, v3d = results

        context = self._attention3d(q3d, k3d, v3d, merged=True)         # [B*H, D, S]
        # = [B, E, S], the k-major operand of the output projection (handed over in the
        # per-head shape so that its gradient can come back in the layout the
        # attention's backward wants, without a pass of its own)
        return self.linears[-1].project(context, dense_blocks=dim).transpose(1, 2)

    def _forward_half_storage(self, query, key, value):
        """``half_storage=True`` with float16 / bfloat16 inputs of one type: [B, S, E] in,
        [B, S, E] out in that type, and every tensor the pass writes -- q, k, v, the context,
        the output -- stored in it.  No head split or merge and no widening pass: the
        projections are row-orientation tile products (functional.half_linear_rows), the
        attention one fused launch on the heads' strided views
        (functional.sparse_attention_heads).  Values are rounded to the storage type at the
        projection outputs, the context and the output; scores, weights and every sum are
        float32.  Under autograd the attention's backward recomputes the weights (as with
        ``low_memory_training``), so the gradient goes through the softmax to q and k;
        gradients come back in the type of what they differentiate (float32 `values` get
        float32 gradients, half inputs half ones).  ``fused_inference``,
        ``low_memory_training``, ``differentiable_softmax`` and ``parallel_projections`` do
        not apply in this mode.  Shapes the kernels do not serve (head dimension other than
        64, sizes off the tiles) are composed from the typed operators."""
        def project(net, x):
            return functional.half_linear_rows(net.output_features, net.input_features, net.values,
                                               net.row_indices, net.row_offsets, net.column_indices, x)

        q, k, v = (project(net, x) for net, x in zip(self.linears, (query, key, value)))
        context = functional.sparse_attention_heads(q, k, v, self.num_heads, self.row_indices,
                                                    self.row_offsets, self.column_indices,
                                                    1.0 / math.sqrt(self.head_dim), self._dropout_p())
        return project(self.linears[-1], context)

    @staticmethod
    def _project_group(nets, dense, split_rows):
        first = nets[0]
        m, k = first.output_features, first.input_features
        needs_grad = torch.is_grad_enabled() and (
            dense.requires_grad or any(net.values.requires_grad for net in nets))
        if not needs_grad:
            return ops.left_spmm_group(m, k, [net.values.detach() for net in nets],
                                       [net.row_indices for net in nets],
                                       [net.row_offsets for net in nets],
                                       [net.column_indices for net in nets], dense, split_rows)
        flat = []
        for net in nets:
            flat += [net.values, net.row_indices, net.row_offsets, net.column_indices]
        return GroupProjectionFunction.apply(m, k, split_rows, dense, *flat)

    def _side_stream(self, index, device):
        streams = self.__dict__.setdefault("_streams", {})
        key = (index, str(device))
        if key not in streams:
            streams[key] = torch.cuda.Stream(device=device)
        return streams[key]


class SparseCoreAttention(nn.Module):
    """The attention core of the reference's transformer (tests/transformer/modules.py:9-81):
    ``forward(query, key, value, mask)`` with query, key, value [b, s, n, hn] and `mask`
    [b, 1, s, s] (a nonzero entry is attended; one mask per batch element, shared by its
    heads) -> the context [s, b, n * hn].  The reference runs sddmm_many_mask,
    sparse_softmax_many_mask and spmm_many_mask on [b*n, s, hn] copies; here the forward is
    ONE fused kernel (functional.sparse_attention_heads_many_mask): float16 / bfloat16
    inputs are read in place as head views, float32 inputs are copied once to [b*n, s, hn]
    as the reference does.  ``topology=`` (the tuple topology.dense_to_sparse_3d returns)
    lets a caller with a static mask skip the per-call conversion; `mask` is then unused.
    A dynamic GPU mask costs one device build per forward (topology.dense_to_sparse_3d ->
    ops.dense_to_csr): five small launches and ONE host synchronisation for any b, where the
    torch loop took a dozen launches and a synchronisation per batch element
    (tools/topology_build_bench.py measures both; topology.enable_device_build(False) brings
    the loop back).
    ``attention_dropout`` = p: Megatron's dropout on the attention probabilities, applied in
    training mode inside the fused kernel (functional.sparse_attention_heads_many_mask)."""

    def __init__(self, seq_length, hidden_size, num_attention_heads, attention_dropout=0.0):
        super().__init__()
        if hidden_size % num_attention_heads != 0:
            raise ValueError(f"{hidden_size} is not divisible by {num_attention_heads}")
        self.attention_dropout = ops.check_dropout_p(attention_dropout)
        self.seq_length = seq_length
        self.hidden_size_per_attention_head = hidden_size // num_attention_heads

    def forward(self, query, key, value, mask=None, topology=None):
        if topology is None:
            topology = dense_to_sparse_3d(mask)
        row_indices, row_offsets, column_indices, nonzeros = topology
        b, s = query.size(0), query.size(1)
        scale = 1.0 / math.sqrt(self.hidden_size_per_attention_head)
        p = self.attention_dropout if self.training else 0.0
        out = functional.sparse_attention_heads_many_mask(query, key, value, nonzeros, row_indices,
                                                          row_offsets, column_indices, scale, p)
        # [b, s, n, hn] -> [s, b, n * hn]
        return out.permute(1, 0, 2, 3).reshape(s, b, -1)
