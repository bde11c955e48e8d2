#!/usr/bin/env python3
"""The fused sparse attention backward (SparseAttention(fused_backward=True),
functional.FusedBackwardAttentionFunction) against the composed one (low_memory_training,
functional.SparseAttentionFunction): the forward ALONE and the backward ALONE, each timed with
device events (median of --reps windows of --steps calls after --warmup), and the peak memory
one forward and one backward allocate on top of what was live before them.  --head-dim 64
(the LDS-staged forward) or 128 (the row-group forward, ops.sparse_attention_rows); at any
other width both routes are the composed one.  The mask is registered as static, so both backwards take
the transposed topology and the kernel plans from the caches, as a module's do.

  c3:   config 3's attention, B = 8 x H = 8 replicas, S = 1024, d = 64, density 0.1
  long: S = 8192, R = 16, density 0.05

One JSON line per shape, route and dropout p.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/attention_backward_bench.py --shapes c3`
for the kernel times.

    python tools/attention_backward_bench.py [--shapes c3,long] [--p 0,0.1] [--head-dim 64]
                                             [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from torch_sputnik_amd import functional  # noqa: E402
from torch_sputnik_amd.synthetic import random_csr  # noqa: E402

SHAPES = {
    "c3": dict(R=64, S=1024, density=0.1),
    "long": dict(R=16, S=8192, density=0.05),
}


def time_call(call, steps, warmup, reps):
    """Median and minimum over `reps` windows of the per-call time (ms) of `call`."""
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(steps):
            call()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / steps)
    return statistics.median(times), min(times)


def peak_bytes(call):
    """Peak of what `call` allocates on top of what was live before it (its result included)."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    result = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del result
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,long")
    ap.add_argument("--p", default="0,0.1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_backward_bench: no GPU")
    dev = torch.device("cuda:0")
    out = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        R, S, d = shape["R"], shape["S"], args.head_dim
        scale = d ** -0.5
        topo = random_csr(S, S, shape["density"], dev, seed=3)[:3]
        nnz = topo[2].numel()
        functional.register_static_topology(*topo)
        g = torch.Generator(device=dev).manual_seed(7)
        q, k, v = (torch.randn(R, S, d, device=dev, generator=g).requires_grad_() for _ in range(3))
        go = torch.randn(R, S, d, device=dev, generator=g)
        for p in (float(x) for x in args.p.split(",")):
            results = {}
            # alternate the two routes, so that drift on the host touches both alike
            for rep in range(2):
                for fused in (True, False):
                    def forward():
                        return functional.sparse_attention(q, k, v, *topo, scale, dropout_p=p,
                                                           fused_backward=fused)

                    y = forward()

                    def backward():
                        return torch.autograd.grad(y, (q, k, v), go, retain_graph=True)

                    med, best = time_call(backward, args.steps, args.warmup, args.reps)
                    fwd, _ = time_call(forward, args.steps, args.warmup, args.reps)
                    results.setdefault(fused, []).append(
                        (med, best, peak_bytes(backward), fwd, peak_bytes(forward)))
                    del y
            for fused in (True, False):
                med = min(r[0] for r in results[fused])
                line = dict(shape=name, R=R, S=S, d=d, density=shape["density"], nnz=nnz, p=p,
                            route="fused_backward" if fused else "composed",
                            backward_ms=round(med, 4),
                            backward_min_ms=round(min(r[1] for r in results[fused]), 4),
                            peak_backward_mb=round(max(r[2] for r in results[fused]) / 1e6, 2),
                            forward_ms=round(min(r[3] for r in results[fused]), 4),
                            peak_forward_mb=round(max(r[4] for r in results[fused]) / 1e6, 2),
                            r_nnz_f32_mb=round(R * nnz * 4 / 1e6, 2),
                            grads_mb=round(3 * R * S * d * 4 / 1e6, 2),
                            device=torch.cuda.get_device_name(dev))
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
        functional.unregister_static_topology(*topo)
        del q, k, v, go
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
