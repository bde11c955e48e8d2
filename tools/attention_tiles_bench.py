#!/usr/bin/env python3
"""The fused attention forward on half storage: the matrix-core tile kernel
(``ops.sparse_attention_tiles``) against the vector kernel (``ops.sparse_attention_heads``) on
the same operands and topology, both through their plans, in ONE process, the two alternated
round by round.

Shapes (B = 8 batch elements of H = 8 heads of 64, float16 and bfloat16):
  * config 3: S = 1024, random mask of density 0.1;
  * S = 4096 with the README's Longformer pattern (window 256 + 16 global tokens);
  * S = 4096 with the README's BigBird pattern (block 64, window 64, 128 global tokens, random
    blocks (64, 0.05)).

Every sample is device-event time around ``inner`` calls, after warm-up of both routes.  Per
shape one JSON line: median, 10th and 90th percentile per route in microseconds, the tile
plan's time alone, the share of 128 x 64 tiles the kernel walks, and ``tiles_faster``: true /
false only where the medians differ by more than the vector route's own p10 - p90 spread in
that run, else "within spread".  The results of the two routes are compared (largest
difference relative to the largest value) before anything is timed.  ``--out FILE`` appends
the lines.

``--head-dim 128``: H = 8 heads of 128 on the D = 128 instances of the tile kernel.  No fused
vector kernel serves half storage there: the other route is what the same call cost before
those instances existed, ``ops.sparse_attention_heads`` COMPOSED from the typed SDDMM, softmax
and SpMM on per-head copies, and the keys read ``composed`` / ``composed_over_tiles`` (plus
``head_dim``).  Kernel times alone: run with ``--rounds 2 --inner 1`` under
``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, HEADS = 8, 8
SHAPES = (
    ("config3_random_0.1", 1024, None),
    ("longformer_window_256_global_16", 4096, dict(window=256, global_tokens=16)),
    ("bigbird_block_64", 4096, dict(block=64, window=64, global_tokens=128, random_blocks=(64, 0.05))),
)


def percentile(sorted_values, q):
    return sorted_values[min(len(sorted_values) - 1, int(q * len(sorted_values)))]


def event_time_us(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / inner


def measure(fns, rounds, warmup, inner):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            samples[name].append(event_time_us(fn, inner))
    out = {}
    for name, values in samples.items():
        values.sort()
        out[name] = {"median_us": round(statistics.median(values), 1),
                     "p10_us": round(percentile(values, 0.1), 1), "p90_us": round(percentile(values, 0.9), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--head-dim", type=int, choices=(64, 128), default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_tiles_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import functional, ops, topology

    dev = torch.device("cuda:0")
    D = args.head_dim
    other = "vector" if D == 64 else "composed"
    lines = []
    for name, size, pattern in SHAPES:
        if pattern is None:
            g = torch.Generator(device="cpu").manual_seed(size)
            mask = (torch.rand(size, size, generator=g) < 0.1).to(dev)
            topo = topology.dense_to_sparse(mask)[1:]
        else:
            state = torch.tensor([size, 0], dtype=torch.int64, device=dev)
            built = topology.AttentionPattern(**pattern)
            topo = built.build(size, device=dev, rng_state=state if built.random else None)
        nonzeros = topo[2].numel()
        tile_plan = ops.sparse_attention_tiles_plan(size, size, topo[1], topo[2])
        vector_plan = ops.sparse_attention_plan(size, size, D, *topo) if D == 64 else None
        blocks, tiles = (size + 127) // 128, (size + 63) // 64
        lists = tile_plan[:blocks * (1 + tiles) * 4].view(torch.int32).view(blocks, 1 + tiles)
        walked = int(lists[:, 0].sum())
        for dtype in (torch.float16, torch.bfloat16):
            g = torch.Generator(device="cpu").manual_seed(size + 1)
            q, k, v = (functional._heads(torch.empty(BATCH, size, HEADS * D).uniform_(-1, 1, generator=g)
                                         .to(dtype).to(dev), HEADS) for _ in range(3))
            scale = 1.0 / D ** 0.5
            fns = {
                "tiles": lambda: ops.sparse_attention_tiles(q, k, v, *topo, scale, plan=tile_plan),
                other: lambda: ops.sparse_attention_heads(q, k, v, *topo, scale, plan=vector_plan),
                "tiles_plan": lambda: ops.sparse_attention_tiles_plan(size, size, topo[1], topo[2]),
            }
            a, b = fns["tiles"]().float(), fns[other]().float()
            difference = float((a - b).abs().max() / b.abs().max())
            timed = measure(fns, args.rounds, args.warmup, args.inner)
            spread = timed[other]["p90_us"] - timed[other]["p10_us"]
            gap = timed[other]["median_us"] - timed["tiles"]["median_us"]
            extra = {} if D == 64 else {"head_dim": D}
            line = dict(case="sparse_attention_tiles vs sparse_attention_heads", shape=name, rows=size, **extra,
                        batch=BATCH, heads=HEADS, dtype=str(dtype).replace("torch.", ""), nonzeros=nonzeros,
                        tiles_walked=walked, tiles_total=blocks * tiles,
                        largest_difference_over_largest_value=difference, **timed,
                        **{other + "_over_tiles": round(timed[other]["median_us"] / timed["tiles"]["median_us"], 2)},
                        tiles_faster=(gap > 0) if abs(gap) > spread else "within spread")
            lines.append(line)
            print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
