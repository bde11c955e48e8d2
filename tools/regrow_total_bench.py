#!/usr/bin/env python3
"""What one matrix-wide drop-and-grow step costs: ``SparseLinear.update_topology(0.3, scores)``

* ``device``: as it is, ``topology.regrow_total`` on the device step (csrc/topology.hip,
  ``ops.csr_regrow_total``);
* ``composed_device_build``: the same call with ``topology.regrow_total_composed`` in its place
  and the device build on -- torch indexing around the device top-k, the step before the device
  step existed;
* ``composed_torch``: that with ``topology.enable_device_build(False)``;
* ``per_row_device``: ``update_topology(0.3, scores, per_row=True)``, another rule, for orientation;

in ONE process, the four alternated round by round.

Cases: layers from ``SparseLinear.from_dense(per_row=True)`` at 2048 x 2048, density 0.2
(float32 and float16) and at 4096 x 4096, density 0.1 (float32), those of tools/regrow_bench.py.
Every step starts from the same pattern: the first one is put back before each call
(``restore_us``, measured alone).

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all paths.  The three matrix-wide paths must give equal tensors before anything is
timed.  Per case one JSON line: median, min, 10th and 90th percentile per path,
``composed_spread_us`` (p90 - p10 of ``composed_device_build``), ``speedup_over_composed`` and
``device_faster_beyond_spread``: the device median is below the ``composed_device_build`` median
by more than that path's own spread.  ``--out FILE`` appends the lines there."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PATHS = ("device", "composed_device_build", "composed_torch", "per_row_device")


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
        raise SystemExit("regrow_total_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, capi, functional, topology

    @contextlib.contextmanager
    def composed(device_build):
        """update_topology on the composed path, the device build on or off"""
        served = topology.regrow_total
        topology.regrow_total = topology.regrow_total_composed
        topology.enable_device_build(device_build)
        try:
            yield
        finally:
            topology.regrow_total = served
            topology.enable_device_build(True)

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

        def update(per_row=False):
            restore()
            source = module.update_topology(0.3, scores, per_row=per_row)
            return source, module.values.detach().clone(), module.row_indices, module.row_offsets, module.column_indices

        def update_composed(device_build):
            with composed(device_build):
                return update()

        fns = {"device": update, "composed_device_build": lambda: update_composed(True),
               "composed_torch": lambda: update_composed(False), "per_row_device": lambda: update(True)}
        results = [fns[name]() for name in PATHS[:3]]
        same = all(torch.equal(a, b) for other in results[1:] for a, b in zip(results[0], other))
        assert same, "regrow_total_bench: the device step and the composed paths differ"
        nnz = reference[0].numel()
        assert int((results[0][0] == -1).sum()) == int(0.3 * nnz) and int(results[0][3][-1]) == nnz
        shape = capi.csr_regrow_total_launch_shape(size, size, nnz, scores.element_size(), weight.element_size())
        assert shape["served"]
        restore_only = measure({"restore": restore}, 5, 1, args.inner)["restore"]["median_us"]
        timed = measure(fns, args.rounds, args.warmup, args.inner)
        yardstick = timed["composed_device_build"]
        spread = yardstick["p90_us"] - yardstick["p10_us"]
        device = timed["device"]["median_us"]
        line = dict(case="SparseLinear.update_topology(0.3, grow_scores)", out_features=size, in_features=size,
                    density=density, dtype=str(dtype).split(".")[-1], nonzeros=nnz, launches=shape["launches"],
                    workspace_bytes=capi.csr_regrow_total_workspace_bytes(size, size, nnz), same_result=same,
                    restore_us=restore_only, **timed, composed_spread_us=round(spread, 1),
                    device_faster_beyond_spread=device < yardstick["median_us"] - spread,
                    speedup_over_composed=round(yardstick["median_us"] / device, 2),
                    speedup_over_composed_torch=round(timed["composed_torch"]["median_us"] / device, 2),
                    ratio_to_per_row=round(device / timed["per_row_device"]["median_us"], 2))
        lines.append(line)
        print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
