#!/usr/bin/env python3
"""What one per-row drop-and-grow step costs: ``SparseLinear.update_topology(0.3, scores,
per_row=True)`` on the device kernel (csrc/topology.hip, ``ops.csr_regrow``), the same call on
the torch path (``topology.enable_device_build(False)``), and the matrix-wide
``update_topology(0.3, scores)`` as it is, in ONE process, the three alternated round by round.

Cases: layers from ``SparseLinear.from_dense(per_row=True)`` at 2048 x 2048, density 0.2
(float32 and float16) and at 4096 x 4096, density 0.1 (float32).  Every step starts from the
same pattern: the first one is put back before each call (``restore_us``, measured alone).

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all paths.  The two per-row paths must give equal tensors before anything is timed.
Per case one JSON line: median, min, 10th and 90th percentile per path, ``speedup_over_torch``
and ``speedup_over_matrix_wide`` (their medians over the device median) and
``device_not_slower``: the device median is at most the torch median plus the torch path's own
spread (p90 - p10).  ``--out FILE`` appends the lines there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PATHS = ("per_row_device", "per_row_torch", "matrix_wide")


def percentile(sorted_values, q):
    return sorted_values[min(len(sorted_values) - 1, int(q * len(sorted_values)))]


def measure(fns, rounds, warmup, inner):
    samples = {name: [] for name in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) / inner * 1e6)
    out = {}
    for name, values in samples.items():
        values.sort()
        out[name] = {"median_us": round(statistics.median(values), 1), "min_us": round(values[0], 1),
                     "p10_us": round(percentile(values, 0.1), 1), "p90_us": round(percentile(values, 0.9), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regrow_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, functional, topology

    dev = torch.device("cuda:0")
    lines = []
    for size, density, dtype in ((2048, 0.2, torch.float32), (2048, 0.2, torch.float16), (4096, 0.1, torch.float32)):
        g = torch.Generator(device="cpu").manual_seed(size)
        weight = torch.randn(size, size, generator=g).to(dtype).to(dev)
        scores = torch.randn(size, size, generator=g).to(dtype).to(dev)
        module = SparseLinear.from_dense(weight, density=density, per_row=True)
        reference = [t.clone() for t in (module.values.detach(), module.row_indices, module.row_offsets,
                                         module.column_indices)]

        def restore():
            # the step is timed from the same pattern every time: put the first one back
            with torch.no_grad():
                module.values.copy_(reference[0])
            functional.unregister_static_topology(module.row_indices, module.row_offsets, module.column_indices)
            module._set_topology(None, *(t.clone() for t in reference[1:]))

        def update(device_build, per_row):
            topology.enable_device_build(device_build)
            try:
                restore()
                source = module.update_topology(0.3, scores, per_row=per_row)
            finally:
                topology.enable_device_build(True)
            return source, module.values.detach().clone(), module.row_offsets, module.column_indices

        fns = {"per_row_device": lambda: update(True, True), "per_row_torch": lambda: update(False, True),
               "matrix_wide": lambda: update(True, False)}
        built, sorted_ = fns["per_row_device"](), fns["per_row_torch"]()
        same = all(torch.equal(a, b) for a, b in zip(built, sorted_))
        assert same, "regrow_bench: the device path and the torch path differ"
        lengths = built[2][1:] - built[2][:-1]
        assert int(lengths.min()) == int(lengths.max()) and int((built[0] == -1).sum()) > 0
        restore_only = measure({"restore": restore}, 5, 1, args.inner)["restore"]["median_us"]
        timed = measure(fns, args.rounds, args.warmup, args.inner)
        spread = timed["per_row_torch"]["p90_us"] - timed["per_row_torch"]["p10_us"]
        device = timed["per_row_device"]["median_us"]
        line = dict(case="SparseLinear.update_topology(0.3, grow_scores)", out_features=size, in_features=size,
                    density=density, dtype=str(dtype).split(".")[-1], nonzeros=reference[0].numel(),
                    row_length=int(lengths[0]), same_result=same, restore_us=restore_only, **timed,
                    torch_spread_us=round(spread, 1),
                    device_not_slower=device <= timed["per_row_torch"]["median_us"] + spread,
                    speedup_over_torch=round(timed["per_row_torch"]["median_us"] / device, 2),
                    speedup_over_matrix_wide=round(timed["matrix_wide"]["median_us"] / device, 2))
        lines.append(line)
        print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
