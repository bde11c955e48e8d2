#!/usr/bin/env python3
"""What building the CSR topology of a structured attention pattern costs
(``topology.AttentionPattern.build``):

* ``device``: ``ops.attention_pattern_csr`` -- the rule is evaluated inside the count and fill
  kernels (csrc/topology.hip), four launches and one synchronisation, no ``[S, S]`` array;
* ``dense_route``: the former route -- ``pattern.dense_mask(S, device=gpu)``, an ``[S, S]`` bool
  image made by torch on the GPU, then ``topology.dense_to_sparse`` on the device build;
* ``torch_path``: the same rule in torch in row slabs (``topology.enable_device_build(False)``);

in ONE process, the three alternated round by round.

Cases: S = 1024, 4096, 16384 with causal window 256; window 256 + 16 global tokens; BigBird-like
(block 64, window 64, 128 global tokens, random blocks (64, 0.05)).

Every sample is a host clock around ``inner`` builds that end in a device synchronise, after
warm-up of all routes.  The three routes must give equal tensors (for one rng_state) before
anything is timed.  Per case one JSON line: median, min, 10th and 90th percentile per route in
microseconds, the peak rise of allocated device memory over one build per route, the bytes of
the outputs and of one bool image, and the speedups of ``device`` (medians; below 1 where it
loses).  Kernel times alone are not taken here.  ``--out FILE`` appends the lines there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = (1024, 4096, 16384)
PATTERNS = (
    ("causal_window_256", dict(window=(256, 0), causal=True)),
    ("window_256_global_16", dict(window=256, global_tokens=16)),
    ("bigbird_like", dict(block=64, window=64, global_tokens=128, random_blocks=(64, 0.05))),
)


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


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    kept = fn()
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - before
    del kept
    return raised


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_pattern_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import capi, topology

    dev = torch.device("cuda:0")
    lines = []
    for size in SIZES:
        for name, arguments in PATTERNS:
            pattern = topology.AttentionPattern(**arguments)
            state = torch.tensor([size, 4 * 10 ** 9], dtype=torch.int64, device=dev) if pattern.random else None

            def device():
                return pattern.build(size, device=dev, rng_state=state)

            def dense_route():
                mask = pattern.dense_mask(size, device=dev, rng_state=state)
                return topology.dense_to_sparse(mask)[1:]

            def torch_path():
                topology.enable_device_build(False)
                try:
                    return device()
                finally:
                    topology.enable_device_build(True)

            shape = capi.attention_pattern_launch_shape(size, size, 0)
            assert shape["served"]
            got = device()
            for other in (dense_route(), torch_path()):
                assert all(torch.equal(a, b) for a, b in zip(got, other)), \
                    "attention_pattern_bench: the routes give different topologies"
            fns = {"device": device, "dense_route": dense_route, "torch_path": torch_path}
            timed = measure(fns, args.rounds, args.warmup, args.inner)
            peaks = {f"{route}_peak_bytes": peak_rise(fn) for route, fn in fns.items()}
            median = timed["device"]["median_us"]
            line = dict(case="topology.AttentionPattern.build", pattern=name, rows=size, columns=size,
                        nonzeros=got[2].numel(), launches=shape["launches"], rows_per_wave=shape["rows_per_wave"],
                        output_bytes=sum(t.numel() * t.element_size() for t in got), bool_image_bytes=size * size,
                        same_result=True, **timed, **peaks, kernel_time_us="not measured",
                        speedup_over_dense_route=round(timed["dense_route"]["median_us"] / median, 2),
                        speedup_over_torch_path=round(timed["torch_path"]["median_us"] / median, 2))
            lines.append(line)
            print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
