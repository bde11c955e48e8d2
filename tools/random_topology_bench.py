#!/usr/bin/env python3
"""What drawing a random topology with its initial values costs (``topology.random_csr``):

* ``device``: ``ops.random_csr`` -- the keys are computed inside the selection kernels
  (csrc/topology.hip), one launch per row or nine matrix-wide, no ``[m, n]`` array;
* ``composed``: ``torch.rand(m, n, device)`` followed by ``topology.topk_to_csr(scores, ...)`` on
  the device build, the values being the scores -- what a user does today;
* ``torch_path``: the same rule as ``device`` in torch (``topology.enable_device_build(False)``);

in ONE process, the three alternated round by round.

Cases, matrix-wide and per row: 2048 x 2048 at density 0.2 with float32 and float16 values and
4096 x 4096 at density 0.1 with float32 values.

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all paths.  ``device`` and ``torch_path`` must give equal tensors for one rng_state
before anything is timed.  Per case one JSON line: median, min, 10th and 90th percentile per
path, ``composed_spread_us`` (p90 - p10 of ``composed``), ``speedup_over_composed`` and
``device_faster_beyond_spread``: the device median is below the ``composed`` median by more than
that path's own spread.  ``--out FILE`` appends the lines there.

``--kernels-only`` runs the ``device`` path ``--rounds`` times per case and nothing else, for
the kernel time alone: ``rocprofv3 --kernel-trace --stats -- python tools/random_topology_bench.py
--kernels-only``."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PATHS = ("device", "composed", "torch_path")
CASES = ((2048, 0.2, torch.float32), (2048, 0.2, torch.float16), (4096, 0.1, torch.float32))


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
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("random_topology_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import capi, topology

    dev = torch.device("cuda:0")
    lines = []
    for size, density, dtype in CASES:
        for per_row in (False, True):
            count = round(density * size) if per_row else round(density * size * size)
            nnz = count * size if per_row else count

            def device(rng_state=None):
                return topology.random_csr(size, size, nonzeros=count, per_row=per_row, dtype=dtype, device=dev,
                                           rng_state=rng_state)

            def composed():
                scores = torch.rand(size, size, device=dev, dtype=dtype)
                return topology.topk_to_csr(scores, per_row=count if per_row else None,
                                            total=None if per_row else count)

            def torch_path(rng_state=None):
                topology.enable_device_build(False)
                try:
                    return device(rng_state)
                finally:
                    topology.enable_device_build(True)

            if args.kernels_only:
                for _ in range(args.rounds):
                    device()
                torch.cuda.synchronize()
                continue
            state = torch.tensor([size, 4 * 10 ** 9], dtype=torch.int64, device=dev)
            got, want = device(state), torch_path(state)
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))
            assert same, "random_topology_bench: the device draw and the torch path differ"
            assert got[0].numel() == nnz and int(got[2][-1]) == nnz
            shape = capi.random_csr_launch_shape(size, size, not per_row)
            assert shape["served"]
            timed = measure({"device": device, "composed": composed, "torch_path": torch_path}, args.rounds,
                            args.warmup, args.inner)
            yardstick = timed["composed"]
            spread = yardstick["p90_us"] - yardstick["p10_us"]
            median = timed["device"]["median_us"]
            line = dict(case="topology.random_csr", rows=size, columns=size, density=density, per_row=per_row,
                        dtype=str(dtype).split(".")[-1], nonzeros=nnz, launches=shape["launches"],
                        workspace_bytes=capi.random_csr_workspace_bytes(size, size, not per_row), same_result=same,
                        **timed, composed_spread_us=round(spread, 1),
                        device_faster_beyond_spread=median < yardstick["median_us"] - spread,
                        speedup_over_composed=round(yardstick["median_us"] / median, 2),
                        speedup_over_torch_path=round(timed["torch_path"]["median_us"] / median, 2))
            lines.append(line)
            print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
