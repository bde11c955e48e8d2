#!/usr/bin/env python3
"""The bench line's many-mask workload (8 masks of density 0.1 / 0.2 / 0.05 / 0.5, 8 heads
each, S = 1024, d = 64) through the fused many-mask attention and through the three-op chain
(sddmm_many_mask, scaled sparse_softmax_many_mask, spmm_many_mask), in float32, float16 and
bfloat16, forward and forward + backward.  One process; after warm-up the variants are
alternated round by round and the median per variant is reported (CUDA events).  Prints one
JSON object; ``--out FILE`` also writes it."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    from torch_sputnik_amd import dense_to_sparse_3d, functional as F, ops

    dev = torch.device("cuda:0")
    b, heads, s, d = 8, 8, 1024, 64
    dens = (0.1, 0.2, 0.05, 0.5)
    g = torch.Generator(device="cpu").manual_seed(70)
    mask = torch.stack([torch.rand(s, s, generator=g) < dens[i % 4] for i in range(b)]).to(dev)
    ri, ro, ci, nnz = dense_to_sparse_3d(mask)
    scale = 1.0 / math.sqrt(d)
    R = b * heads
    base = [torch.empty(R, s, d).uniform_(-2, 2, generator=g).to(dev) for _ in range(3)]
    grad = torch.randn(R, s, d, device=dev)

    def chain(q, k, v):
        qf, kf, vf = (x.float() for x in (q, k, v))
        sc = F.SddmmManyMask.apply(b, s, s, nnz, ri, ro, ci, qf, kf)
        w = F.CsrSoftmaxManyMask.apply(b, s, nnz, sc, ri, ro, ci, scale)
        return F.SpmmManyMask.apply(b, s, s, nnz, w, ri, ro, ci, vf)

    def fused(q, k, v):
        return F.sparse_attention_many_mask(b, s, s, nnz, ri, ro, ci, q, k, v, scale)

    variants = {}
    for dt_name, dt in (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16)):
        qkv = [x.to(dt) for x in base]
        qkv_g = [x.detach().clone().requires_grad_(True) for x in qkv]
        for kind, fn in (("fused", fused), ("chain", chain)):
            def fwd(fn=fn, qkv=qkv):
                with torch.no_grad():
                    fn(*qkv)

            def fwd_bwd(fn=fn, qkv=qkv_g):
                out = fn(*qkv)
                out.float().backward(grad)
            variants[f"{kind}_{dt_name}_fwd"] = fwd
            variants[f"{kind}_{dt_name}_fwd_bwd"] = fwd_bwd

    # same numbers from both paths (float32)
    with torch.no_grad():
        err = float((fused(*base) - chain(*base)).abs().max())

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) * 1000.0)
    result = {
        "workload": {"masks": b, "heads": heads, "S": s, "d": d, "densities": list(dens),
                     "nonzeros": nnz, "replica_entries": heads * sum(nnz)},
        "rounds": args.rounds, "warmup": args.warmup,
        "median_us": {name: round(statistics.median(t), 1) for name, t in times.items()},
        "fused_vs_chain_fp32_max_abs_diff": err,
        "chain_intermediates_bytes": 2 * R * max(nnz) * 4,
        "device": torch.cuda.get_device_name(0),
    }
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
