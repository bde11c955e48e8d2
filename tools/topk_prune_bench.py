#!/usr/bin/env python3
"""What magnitude pruning and one drop-and-grow step cost: the device top-k-to-CSR build
(csrc/topology.hip, ``ops.topk_to_csr``) against the torch path it replaces (a stable sort of
the keys), in ONE process, the two alternated round by round (``topology.enable_device_build``).

Cases: ``topology.magnitude_prune`` (matrix-wide and per row) and
``SparseLinear.update_topology(0.3, grow_scores)`` at 2048 x 2048, density 0.2 (the layer of
BASELINE.json's config 5), float32 and float16, and at 4096 x 4096, density 0.1, float32.

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of both paths.  Per case one JSON line: median, min, 10th and 90th percentile per
path, ``speedup`` (torch median over device median) and ``device_not_slower``: the device
median is at most the torch median plus the torch path's own spread (p90 - p10).
``--out FILE`` appends the lines there."""
import argparse
import json
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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_prune_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, topology

    dev = torch.device("cuda:0")
    lines = []

    def report(case, **fields):
        line = dict(case=case, **fields)
        lines.append(line)
        print(json.dumps(line), flush=True)

    def both_paths(fn):
        topology.enable_device_build(True)
        built = fn()
        topology.enable_device_build(False)
        sorted_ = fn()
        topology.enable_device_build(True)
        return all(torch.equal(a, b) for a, b in zip(built, sorted_))

    for size, density, dtype in ((2048, 0.2, torch.float32), (2048, 0.2, torch.float16), (4096, 0.1, torch.float32)):
        g = torch.Generator(device="cpu").manual_seed(size)
        weight = torch.randn(size, size, generator=g).to(dtype).to(dev)
        scores = torch.randn(size, size, generator=g).to(dtype).to(dev)
        shape = dict(out_features=size, in_features=size, density=density, dtype=str(dtype).split(".")[-1])

        for per_row in (False, True):
            def prune():
                return topology.magnitude_prune(weight, density=density, per_row=per_row)
            same = both_paths(prune)      # the same integers and value bits before anything is timed
            report("magnitude_prune", **shape, per_row=per_row, nonzeros=prune()[0].numel(), same_result=same,
                   **measure(prune, topology.enable_device_build, args.rounds, args.warmup, args.inner))

        module = SparseLinear.from_dense(weight, density=density)
        reference = [t.clone() for t in (module.values.detach(), module.row_indices, module.row_offsets,
                                         module.column_indices)]

        def restore():
            # the step is timed from the same pattern every time: put the first one back
            from torch_sputnik_amd import functional
            with torch.no_grad():
                module.values.copy_(reference[0])
            functional.unregister_static_topology(module.row_indices, module.row_offsets, module.column_indices)
            module._set_topology(None, *(t.clone() for t in reference[1:]))

        def update():
            restore()
            source = module.update_topology(0.3, scores)
            return source, module.values.detach().clone(), module.row_offsets, module.column_indices

        same = both_paths(update)
        restore_only = measure(restore, topology.enable_device_build, 5, 1, args.inner)
        report("SparseLinear.update_topology(0.3, grow_scores)", **shape, nonzeros=reference[0].numel(),
               same_result=same, restore_us=restore_only["device"]["median_us"],
               **measure(update, topology.enable_device_build, args.rounds, args.warmup, args.inner))

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
