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

--compare-lib PATH: also time the fused forwards WITHOUT dropout through the C ABI of this
build and of the library at PATH (a build of the parent commit): the A/B of the no-dropout
kernels.
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
    for name in ("sputnik_hip_sparse_attention_workspace_bytes", "sputnik_hip_sparse_attention_plan",
                 "sputnik_hip_sparse_attention_forward_planned",
                 "sputnik_hip_sparse_attention_heads_forward_planned"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.SIGNATURES[name]
    return lib


def compare_libs(other, q, k, v, qh, kh, vh, topo, nnz, s, d, reps):
    """The no-dropout fused forwards through two builds of the library."""
    from torch_sputnik_amd import _native
    ri, ro, ci = topo
    R = q.size(0)
    stream = torch.cuda.current_stream().cuda_stream
    for label, path in (("this_build", _native.KERNEL_LIB), ("compare_lib", other)):
        lib = bind(path)
        ws_bytes = lib.sputnik_hip_sparse_attention_workspace_bytes(s, s, d, nnz)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        assert lib.sputnik_hip_sparse_attention_plan(s, s, d, nnz, ri.data_ptr(), ro.data_ptr(), ci.data_ptr(),
                                                     ws.data_ptr(), ws_bytes, stream) == 0
        out = torch.empty_like(q)
        lse = torch.empty(R, s, device=q.device)

        def f32():
            st = lib.sputnik_hip_sparse_attention_forward_planned(
                s, s, d, nnz, R, ri.data_ptr(), ro.data_ptr(), ci.data_ptr(), q.data_ptr(), s * d,
                k.data_ptr(), s * d, v.data_ptr(), s * d, 1 / math.sqrt(d), out.data_ptr(), s * d,
                lse.data_ptr(), s, ws.data_ptr(), ws_bytes, stream)
            assert st == 0
        emit(f"nodrop_fused_f32[{label}]", event_ms(f32, reps))
        B, S, E = qh.shape
        H = E // d
        outh = torch.empty(B, S, E, dtype=torch.float16, device=q.device)

        def f16():
            st = lib.sputnik_hip_sparse_attention_heads_forward_planned(
                s, s, d, nnz, B, H, ri.data_ptr(), ro.data_ptr(), ci.data_ptr(), 1,
                qh.data_ptr(), S * E, d, E, kh.data_ptr(), S * E, d, E, vh.data_ptr(), S * E, d, E,
                1 / math.sqrt(d), outh.data_ptr(), 1, S * E, d, E, lse.data_ptr(), s, ws.data_ptr(),
                ws_bytes, stream)
            assert st == 0
        emit(f"nodrop_fused_heads_f16[{label}]", event_ms(f16, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--compare-lib", default=None)
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
        compare_libs(args.compare_lib, q, k, v, qh, kh, vh, topo, nnz, s, d, reps)


if __name__ == "__main__":
    main()
