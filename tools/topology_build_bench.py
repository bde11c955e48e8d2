#!/usr/bin/env python3
"""What the CSR topology of a dynamic mask costs: the device build (csrc/topology.hip) against
the torch path it replaces, in ONE process, the two alternated round by round
(``topology.enable_device_build``).

Workloads: the bench line's many-mask workload (8 masks of density 0.1 / 0.2 / 0.05 / 0.5,
S = 1024, 8 heads, d = 64, float32) with bool and int64 masks, and S = 4096 with b = 8.
Timed: ``dense_to_sparse_3d`` alone, ``SparseCoreAttention.forward(q, k, v, mask)``, and one
forward + backward of ``functional.sparse_attention_many_mask`` on a built topology (its
backward runs ``diffsort_many_mask`` on the transposed offsets; S = 1024 only -- the composed
backward's [R, nnz] intermediates at S = 4096 are out of this tool's scope).

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of both paths.  Per case one JSON line: median, min, 10th and 90th percentile per
path, and ``device_not_slower``: the device median is at most the torch median plus the
torch path's own spread (p90 - p10).  ``--out FILE`` appends the lines there."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def percentile(sorted_values, q):
    return sorted_values[min(len(sorted_values) - 1, int(q * len(sorted_values)))]


def measure(fn, set_path, rounds, warmup, inner):
    samples = {"device": [], "torch": []}
    for enabled in (True, False):
        set_path(enabled)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, enabled in (("device", True), ("torch", False)):
            set_path(enabled)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) / inner * 1e6)
    set_path(True)
    out = {}
    for name, values in samples.items():
        values.sort()
        out[name] = {"median_us": round(statistics.median(values), 1), "min_us": round(values[0], 1),
                     "p10_us": round(percentile(values, 0.1), 1), "p90_us": round(percentile(values, 0.9), 1)}
    spread = out["torch"]["p90_us"] - out["torch"]["p10_us"]
    out["torch_spread_us"] = round(spread, 1)
    out["device_not_slower"] = out["device"]["median_us"] <= out["torch"]["median_us"] + spread
    out["speedup"] = round(out["torch"]["median_us"] / out["device"]["median_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topology_build_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseCoreAttention, functional as F, topology

    dev = torch.device("cuda:0")
    heads, d = 8, 64
    dens = (0.1, 0.2, 0.05, 0.5)
    lines = []

    def report(case, **fields):
        line = dict(case=case, **fields)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for s, b in ((1024, 8), (4096, 8)):
        g = torch.Generator(device="cpu").manual_seed(70 + s)
        mask_bool = torch.stack([torch.rand(s, s, generator=g) < dens[i % 4] for i in range(b)])
        q, k, v = (torch.empty(b, s, heads, d).uniform_(-2, 2, generator=g).to(dev) for _ in range(3))
        module = SparseCoreAttention(s, heads * d, heads).to(dev).eval()
        for mask_name, mask in (("bool", mask_bool), ("int64", mask_bool.to(torch.int64))):
            mask = mask[:, None].to(dev)                      # [b, 1, s, s], as the transformer passes it
            # the same integers from both paths before anything is timed
            topology.enable_device_build(True)
            built = topology.dense_to_sparse_3d(mask)
            topology.enable_device_build(False)
            loop = topology.dense_to_sparse_3d(mask)
            topology.enable_device_build(True)
            same = all(torch.equal(x, y) for x, y in zip(built[:3], loop[:3])) and built[3] == loop[3]
            shape = dict(b=b, s=s, heads=heads, mask=mask_name, nonzeros=sum(built[3]), same_result=same)

            report("dense_to_sparse_3d", **shape,
                   **measure(lambda: topology.dense_to_sparse_3d(mask), topology.enable_device_build,
                             args.rounds, args.warmup, args.inner))

            def forward():
                with torch.no_grad():
                    module(q, k, v, mask)
            report("SparseCoreAttention.forward(q, k, v, mask)", **shape, dtype="float32",
                   **measure(forward, topology.enable_device_build, args.rounds, args.warmup, args.inner))

        if s == 1024:
            ri, ro, ci, nnz = built
            scale = 1.0 / math.sqrt(d)
            qkv = [x.permute(0, 2, 1, 3).reshape(b * heads, s, d).contiguous().requires_grad_(True)
                   for x in (q, k, v)]
            grad = torch.randn(b * heads, s, d, device=dev)

            def forward_backward():
                out = F.sparse_attention_many_mask(b, s, s, nnz, ri, ro, ci, *qkv, scale)
                out.backward(grad)
            report("sparse_attention_many_mask forward + backward", b=b, s=s, heads=heads, dtype="float32",
                   nonzeros=sum(nnz),
                   **measure(forward_backward, topology.enable_device_build, args.rounds, args.warmup,
                             max(1, args.inner // 2)))

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
