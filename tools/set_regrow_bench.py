#!/usr/bin/env python3
"""What one SET step costs, with and without a dense score array:

* ``set_update``: ``SparseLinear.set_update(0.3)`` -- random grow scores computed where they are
  compared (csrc/topology.hip, ``ops.csr_regrow_total_random`` / ``ops.csr_regrow_random``);
* ``update_topology``: ``SparseLinear.update_topology(0.3, grow_scores=None)`` -- the route before
  ``set_update`` existed and the yardstick: ``torch.rand`` fills an ``[out, in]`` float32 array and
  the stored-score step walks it;
* ``set_update_reinit``: ``set_update(0.3, grow_bound=bound)``, grown entries re-initialised, for
  orientation;

matrix-wide and ``per_row``, in ONE process, the routes alternated round by round.

Cases: layers from ``SparseLinear.random`` at 2048 x 2048, density 0.2 (float32 and float16) and at
4096 x 4096, density 0.1 (float32), the shapes of tools/regrow_total_bench.py.  Every step starts
from the same pattern: the first one is put back before each call (``restore_us``, measured
alone, is part of every sample).

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all routes.  Before anything is timed ``set_update`` at a given rng_state must equal
``update_topology`` under float32 scores whose bits are the keys of that state.  Per case and
mode one JSON line: median, min, 10th and 90th percentile per route, ``yardstick_spread_us``
(p90 - p10 of ``update_topology``), ``speedup`` and ``faster_beyond_spread`` /
``slower_beyond_spread``: the ``set_update`` median is below / above the ``update_topology`` median
by more than that route's own spread.  ``--out FILE`` appends the lines there."""
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
        raise SystemExit("set_regrow_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

    dev = torch.device("cuda:0")
    lines = []
    for size, density, dtype in ((2048, 0.2, torch.float32), (2048, 0.2, torch.float16), (4096, 0.1, torch.float32)):
        for per_row in (False, True):
            torch.manual_seed(size)
            module = SparseLinear.random(size, size, density=density, per_row=per_row, dtype=dtype, device=dev)
            reference = [t.clone() for t in (module.values.detach(), module.row_indices, module.row_offsets,
                                             module.column_indices)]
            nnz = reference[0].numel()
            bound = 1.0 / (nnz / size) ** 0.5

            def restore():
                # the step is timed from the same pattern every time: put the first one back
                with torch.no_grad():
                    module.values.copy_(reference[0])
                functional.unregister_static_topology(module.row_indices, module.row_offsets, module.column_indices)
                module._set_topology(None, *(t.clone() for t in reference[1:]))

            def result(source):
                return source, module.values.detach().clone(), module.row_indices, module.row_offsets, module.column_indices

            def set_update(**more):
                restore()
                return result(module.set_update(0.3, per_row=per_row, **more))

            def update_topology(scores=None):
                restore()
                return result(module.update_topology(0.3, grow_scores=scores, per_row=per_row))

            # the same step: set_update at a state, update_topology under the keys of that state
            state = torch.tensor([size, 8], dtype=torch.int64, device=dev)
            keys = topology._random_words(size, size, size, 8, dev, False) & ops.REGROW_KEY_MASK
            stored = update_topology(keys.to(torch.int32).view(torch.float32))
            same = all(torch.equal(a, b) for a, b in zip(set_update(rng_state=state), stored))
            assert same, "set_regrow_bench: set_update and update_topology under the same keys differ"
            del keys, stored
            shape = capi.csr_regrow_random_launch_shape(size, size, nnz, reference[0].element_size(), not per_row)
            assert shape["served"]

            fns = {"set_update": set_update, "update_topology": update_topology,
                   "set_update_reinit": lambda: set_update(grow_bound=bound)}
            restore_only = measure({"restore": restore}, 5, 1, args.inner)["restore"]["median_us"]
            timed = measure(fns, args.rounds, args.warmup, args.inner)
            yardstick = timed["update_topology"]
            spread = yardstick["p90_us"] - yardstick["p10_us"]
            device = timed["set_update"]["median_us"]
            line = dict(case="SparseLinear.set_update(0.3) against update_topology(0.3, grow_scores=None)",
                        per_row=per_row, out_features=size, in_features=size, density=density,
                        dtype=str(dtype).split(".")[-1], nonzeros=nnz, launches=shape["launches"],
                        workspace_bytes=capi.csr_regrow_random_workspace_bytes(size, size, nnz, not per_row),
                        score_array_bytes=size * size * 4, same_result=same, restore_us=restore_only, **timed,
                        yardstick_spread_us=round(spread, 1),
                        faster_beyond_spread=device < yardstick["median_us"] - spread,
                        slower_beyond_spread=device > yardstick["median_us"] + spread,
                        speedup=round(yardstick["median_us"] / device, 2))
            lines.append(line)
            print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
