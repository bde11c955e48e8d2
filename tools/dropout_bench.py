#!/usr/bin/env python3
"""Attention dropout: what it costs at config 3's geometry (S = 1024, 8 heads x batch 8,
head_dim 64, mask density 0.1) and at the bench's many-mask workload (b = 8 masks of
densities 0.1 / 0.2 / 0.05 / 0.5, 8 heads each).  One JSON line per measurement (event
timing, median of --reps); run under `rocprofv3 --kernel-trace --stats -- python ...` for
the device-side kernel times.

  fused forward with / without dropout (float32 [R, S, D]; float16 head views)
  the composed chain with dropout (SDDMM + softmax + sparse_dropout + SpMM)
  sparse_dropout alone at [64, nnz] and its bytes against 8 TB/s
  the SparseAttention training step (forward + backward) with / without dropout
  many-mask: fused float32 and float16 heads forms with / without dropout

--compare-lib PATH: also the A/B of the fused forward kernels against the library at PATH (a
build of the parent commit), through the C ABI of both in this process, alternating
--alternations times: float32 and float16 heads forms x one mask or many x with and without
dropout, both libraries from one fixed Philox state.  --check-equal: first assert that out and
lse of the two libraries are equal bit for bit at config 3's shape and at small shapes that
reach every kernel path (m = 136 x n = 200: a partial row block and a partial last stage, a
row of 40 entries in one chunk, a reversed row, a row and a mask without entries), for
float32, float16 and bfloat16 storage and both output types.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def emit(name, ms, **extra):
    print(json.dumps({"name": name, "ms": round(ms, 5), **extra}), flush=True)


def bind(path):
    from torch_sputnik_amd import capi
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        if name.startswith("sputnik_hip_sparse_attention_"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


class FusedProblem:
    """One fused-forward problem on the device, callable through any build's C ABI: `batch`
    x `heads` replicas of m x n attention at d = 64 under one mask (csr = (ri, ro, ci),
    counts = its entry count) or one mask per batch element (concatenated csr, counts = a
    list).  Operands are drawn once: float32 [R, rows, 64] and, for the heads forms, their
    [B, rows, H * 64] images in float16 and bfloat16."""
    CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    RNG = dict(seed=0x5EED0123456789, offset=40)   # sputnik_hip_philox_state by value

    def __init__(self, dev, m, n, batch, heads, csr, counts, seed=0):
        self.m, self.n, self.d, self.batch, self.heads = m, n, 64, batch, heads
        self.many = not isinstance(counts, int)
        self.csr, self.counts = csr, counts
        g = torch.Generator(device=dev).manual_seed(seed)
        self.f32 = [torch.randn(batch * heads, rows, 64, device=dev, generator=g) for rows in (m, n, n)]
        self.half = {t: [x.view(batch, heads, -1, 64).transpose(1, 2).reshape(batch, -1, heads * 64).to(t)
                         for x in self.f32] for t in (torch.float16, torch.bfloat16)}
        self.plans = {}

    def plan(self, lib):
        if lib not in self.plans:
            stream = torch.cuda.current_stream().cuda_stream
            ptrs = [t.data_ptr() for t in self.csr]
            if self.many:
                counts = (ctypes.c_int * len(self.counts))(*self.counts)
                size = lib.sputnik_hip_sparse_attention_many_mask_workspace_bytes(
                    len(self.counts), self.m, self.n, self.d, max(self.counts))
                ws = torch.empty(size, dtype=torch.uint8, device=self.csr[0].device)
                st = lib.sputnik_hip_sparse_attention_many_mask_plan(
                    len(self.counts), self.m, self.n, self.d, counts, *ptrs, ws.data_ptr(), size, stream)
            else:
                size = lib.sputnik_hip_sparse_attention_workspace_bytes(self.m, self.n, self.d, self.counts)
                ws = torch.empty(size, dtype=torch.uint8, device=self.csr[0].device)
                st = lib.sputnik_hip_sparse_attention_plan(self.m, self.n, self.d, self.counts, *ptrs,
                                                           ws.data_ptr(), size, stream)
            assert st == 0 and size > 0
            self.plans[lib] = ws
        return self.plans[lib]

    def outputs(self, dtype, out_dtype):
        """(out, lse) buffers of a form: dtype float32 = the [R, rows, 64] form."""
        dev = self.csr[0].device
        shape = (self.batch * self.heads, self.m, 64) if dtype == torch.float32 else \
            (self.batch, self.m, self.heads * 64)
        return (torch.full(shape, float("nan"), dtype=out_dtype, device=dev),
                torch.full((self.batch * self.heads, self.m), float("nan"), device=dev))

    def forward(self, lib, dtype, p, out, lse):
        """The planned fused forward of `lib` for operands of `dtype`, with dropout p > 0."""
        from torch_sputnik_amd import capi
        ws, half = self.plan(lib), dtype != torch.float32
        name = "sputnik_hip_sparse_attention_" + ("heads_" if half else "") + \
            ("many_mask_" if self.many else "") + "forward_planned" + ("_dropout" if p > 0 else "")
        args = [self.m, self.n, self.d]
        if self.many:
            args = [len(self.counts)] + args + [(ctypes.c_int * len(self.counts))(*self.counts)]
        else:
            args += [self.counts]
        topo = [t.data_ptr() for t in self.csr]
        if half:
            E = self.heads * 64
            q, k, v = self.half[dtype]
            args += [self.batch, self.heads, *topo, self.CODES[dtype]]
            for t in (q, k, v):
                args += [t.data_ptr(), t.size(1) * E, 64, E]
            args += [1 / math.sqrt(64), out.data_ptr(), self.CODES[out.dtype], self.m * E, 64, E]
        else:
            args += [self.batch * self.heads, *topo]
            for t in self.f32:
                args += [t.data_ptr(), t.size(1) * 64]
            args += [1 / math.sqrt(64), out.data_ptr(), self.m * 64]
        args += [lse.data_ptr(), self.m]
        if p > 0:
            args += [p, capi.PhiloxState(self.RNG["seed"], self.RNG["offset"], None, None, 0), None]
        args += [ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream]
        st = getattr(lib, name)(*args)
        assert st == 0, (name, st)


def edge_csr(dev, masks, m, n, seed, empty_mask=None):
    """CSR of `masks` random m x n masks (density 0.15) that reach every kernel path: mask 0 has
    a row with 40 entries inside the first 128-key chunk (the on-demand loop), a row without
    entries and a reversed row, whose row block takes the order-independent path.  The kernel
    deals entry p of row_indices to row block p % blocks (dealt_index), so the reversed row is
    taken from another block than the 40-entry row's, which then has ascending rows only."""
    rng = np.random.default_rng(seed)
    dense = rng.random((masks, m, n)) < 0.15
    long_row, blocks = 3, -(-m // 128)
    dense[0, long_row, :] = False
    dense[0, long_row, :40] = True
    dense[0, 5, :] = False
    if empty_mask is not None:
        dense[empty_mask] = False
    ri, ro, ci, counts = [], [], [], []
    for i in range(masks):
        rows, cols = np.nonzero(dense[i])
        offsets = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
        order = np.argsort(-np.diff(offsets), kind="stable")
        if i == 0:
            block_of = {int(row): at % blocks for at, row in enumerate(order)}
            reversed_row = next(int(row) for row in order if block_of[int(row)] != block_of[long_row])
            a, b = offsets[reversed_row], offsets[reversed_row + 1]
            assert blocks > 1 and b - a > 1
            cols[a:b] = cols[a:b][::-1].copy()
            ascending = [bool(np.all(np.diff(cols[offsets[r]:offsets[r + 1]]) > 0)) for r in range(m)]
            assert not ascending[reversed_row]
            assert all(ascending[r] for r in range(m) if block_of[r] == block_of[long_row])
            in_chunk = np.bincount(rows[cols < 128], minlength=m)
            assert in_chunk[long_row] == 40 > 32
        ri.append(order)
        ro.append(offsets)
        ci.append(cols)
        counts.append(len(cols))
    csr = tuple(torch.from_numpy(np.concatenate(x).astype(np.int32)).to(dev) for x in (ri, ro, ci))
    return csr, counts


def compare_libs(other, problems, p, reps, alternations, check_equal):
    """The planned fused forwards (float32 and float16 heads x one mask or many x with and
    without dropout) through this build and the library at `other`, both from one fixed
    Philox state.  Timing: the two libraries alternate `alternations` times in this process;
    per form and library the median of `reps` events per alternation, the median of those,
    and their spread (max - min).  check_equal: out and lse of both libraries must be equal
    bit for bit, for every problem, storage type and output type."""
    from torch_sputnik_amd import _native
    libs = (("this_build", bind(_native.KERNEL_LIB)), ("compare_lib", bind(other)))
    if check_equal:
        checked = 0
        for name, prob in problems.items():
            for dtype in (torch.float32, torch.float16, torch.bfloat16):
                for out_dtype in {dtype, torch.float32}:
                    for drop in (0.0, p):
                        got = []
                        for _, lib in libs:
                            out, lse = prob.outputs(dtype, out_dtype)
                            prob.forward(lib, dtype, drop, out, lse)
                            got.append((out, lse))
                        torch.cuda.synchronize()
                        assert not torch.isnan(got[0][0]).any(), (name, dtype, out_dtype, drop)
                        assert torch.equal(got[0][0], got[1][0]), ("out", name, dtype, out_dtype, drop)
                        assert torch.equal(got[0][1], got[1][1]), ("lse", name, dtype, out_dtype, drop)
                        checked += 1
        print(json.dumps({"name": "compare_libs_bit_identical", "cases": checked}), flush=True)
    forms = [(f"{'many_mask_' if key == 'c3_many' else ''}fused_{'f32' if dtype == torch.float32 else 'heads_f16'}"
              f"{'_dropout' if drop else ''}", problems[key], dtype, drop)
             for key in ("c3", "c3_many") for dtype in (torch.float32, torch.float16) for drop in (0.0, p)]
    medians = {(form[0], label): [] for form in forms for label, _ in libs}
    for _ in range(alternations):
        for label, lib in libs:
            for name, prob, dtype, drop in forms:
                out, lse = prob.outputs(dtype, dtype)
                medians[name, label].append(event_ms(lambda: prob.forward(lib, dtype, drop, out, lse), reps))
    for (name, label), ms in medians.items():
        emit(f"{name}[{label}]", statistics.median(ms), per_alternation=[round(t, 5) for t in ms],
             spread=round(max(ms) - min(ms), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--check-equal", action="store_true")
    args = ap.parse_args()
    from torch_sputnik_amd import SparseAttention, functional, ops
    from torch_sputnik_amd.topology import dense_to_sparse, dense_to_sparse_3d, generate_mask

    dev = torch.device("cuda:0")
    p, reps = args.p, args.reps
    s, d, heads, batch = 1024, 64, 8, 8
    R = heads * batch
    torch.manual_seed(0)
    mask = generate_mask(s, s, dev, sparsity=0.9, generator=np.random.default_rng(0))
    _, ri, ro, ci = dense_to_sparse(mask)
    nnz = ci.numel()
    topo = (ri, ro, ci)
    scale = 1 / math.sqrt(d)
    q, k, v = (torch.randn(R, s, d, device=dev) for _ in range(3))
    qh, kh, vh = (torch.randn(batch, s, heads * d, device=dev).half() for _ in range(3))
    hv = [t.unflatten(-1, (heads, d)).transpose(1, 2) for t in (qh, kh, vh)]
    plan = ops.sparse_attention_plan(s, s, d, *topo)
    common = dict(R=R, S=s, d=d, nnz=nnz, p=p)

    emit("fused_f32", event_ms(lambda: ops.sparse_attention_planned(q, k, v, *topo, scale, plan), reps), **common)
    emit("fused_f32_dropout", event_ms(lambda: ops.sparse_attention_dropout(q, k, v, *topo, scale, p, plan),
                                       reps), **common)
    emit("fused_heads_f16", event_ms(lambda: ops.sparse_attention_heads(*hv, *topo, scale, plan=plan), reps),
         **common)
    emit("fused_heads_f16_dropout",
         event_ms(lambda: ops.sparse_attention_heads_dropout(*hv, *topo, scale, p, plan=plan), reps), **common)

    def composed():
        w = ops.sparse_softmax_scaled(ops.sddmm(s, s, *topo, q, k), *topo, scale)
        return ops.spmm(s, s, ops.sparse_dropout(w, p)[0], *topo, v)
    emit("composed_f32_dropout", event_ms(composed, reps), **common)
    w = torch.rand(R, nnz, device=dev)
    t = event_ms(lambda: ops.sparse_dropout(w, p), reps)
    gbytes = 2 * 4 * R * nnz / 1e9
    emit("sparse_dropout_64xnnz_f32", t, bytes=2 * 4 * R * nnz, tbs=round(gbytes / t, 3),
         fraction_of_8tbs=round(gbytes / t / 8.0, 3))
    wh = w.half()
    t = event_ms(lambda: ops.sparse_dropout(wh, p), reps)
    emit("sparse_dropout_64xnnz_f16", t, tbs=round(gbytes / 2 / t, 3), fraction_of_8tbs=round(gbytes / 2 / t / 8.0, 3))

    # the module's training step (the bench's config 3 layer, low_memory_training as well)
    x = torch.randn(batch, s, heads * d, device=dev)
    go = torch.randn_like(x)
    for low_memory in (False, True):
        for drop in (0.0, p):
            attn = SparseAttention(heads, heads * d, max_sequence_length=s, device=dev, sparsity=0.9,
                                   mask_generator=np.random.default_rng(0), low_memory_training=low_memory,
                                   attention_dropout=drop).to(dev).train()
            for lin in attn.linears:
                with torch.no_grad():
                    lin.weight.copy_((torch.rand(heads * d, heads * d, device=dev) < 0.1) *
                                     torch.randn(heads * d, heads * d, device=dev) / 8)
                lin.setup_sparse_tensors()
            xg = x.clone().requires_grad_()

            def step():
                attn(xg, xg, xg).backward(go)
            emit(f"module_step{'_low_memory' if low_memory else ''}{'_dropout' if drop else ''}",
                 event_ms(step, max(reps // 5, 5)))

    # many masks: b = 8, densities 0.1 / 0.2 / 0.05 / 0.5, 8 heads each
    dens = (0.1, 0.2, 0.05, 0.5)
    rng = np.random.default_rng(1)
    m3 = torch.from_numpy(np.stack([rng.random((s, s)) < dens[i % 4] for i in range(batch)])[:, None]).to(dev)
    mri, mro, mci, mnnz = dense_to_sparse_3d(m3)
    mt = (mri, mro, mci)
    qm, km, vm = (torch.randn(batch, s, heads, d, device=dev) for _ in range(3))
    qmh, kmh, vmh = (t.half() for t in (qm, km, vm))
    for name, args3 in (("many_mask_f32", (qm, km, vm)), ("many_mask_heads_f16", (qmh, kmh, vmh))):
        with torch.no_grad():
            emit(name, event_ms(lambda: functional.sparse_attention_heads_many_mask(*args3, mnnz, *mt, scale),
                                reps))
            emit(name + "_dropout", event_ms(
                lambda: functional.sparse_attention_heads_many_mask(*args3, mnnz, *mt, scale, p), reps))
    if args.compare_lib:
        small, small_counts = edge_csr(dev, 1, 136, 200, 3)
        small_many, small_many_counts = edge_csr(dev, 3, 136, 200, 4, empty_mask=1)
        problems = {"c3": FusedProblem(dev, s, s, batch, heads, topo, nnz),
                    "c3_many": FusedProblem(dev, s, s, batch, heads, mt, [int(c) for c in mnnz]),
                    "small": FusedProblem(dev, 136, 200, 1, 3, small, small_counts[0]),
                    "small_many": FusedProblem(dev, 136, 200, 3, 2, small_many, small_many_counts)}
        compare_libs(args.compare_lib, problems, p, reps, args.alternations, args.check_equal)


if __name__ == "__main__":
    main()
