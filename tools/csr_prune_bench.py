#!/usr/bin/env python3
"""What one step of gradual magnitude pruning costs: ``SparseLinear.prune_to(density)`` on the
device kernels (csrc/topology.hip, ``ops.csr_topk``), the same call on the torch path
(``topology.enable_device_build(False)``), and the dense detour a user had to take before --
scatter the values into a dense ``[out, in]`` image and ``topology.magnitude_prune`` it (on the
device top-k-to-CSR build) -- in ONE process, the three alternated round by round.

Cases: layers from ``SparseLinear.from_dense`` at 2048 x 2048 pruned from density 0.5 to 0.4 and
from 0.2 to 0.15 (float32 and float16) and at 4096 x 4096 from 0.2 to 0.1 (float32), each
matrix-wide and ``per_row``.  Every step starts from the same layer: the first Parameter and
pattern are put back before each call (``restore_us``, measured alone).

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all paths.  The two ``prune_to`` paths must give equal tensors before anything is
timed, and the detour the same pattern.  Per case one JSON line: median, min, 10th and 90th
percentile per path, ``speedup_over_torch`` and ``speedup_over_dense_detour`` (their medians
over the device median) and ``device_not_slower``: the device median is at most the torch median
plus the torch path's own spread (p90 - p10).  ``--out FILE`` appends the lines there."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.regrow_bench import measure  # noqa: E402

CASES = ((2048, 0.5, 0.4, torch.float32), (2048, 0.5, 0.4, torch.float16),
         (2048, 0.2, 0.15, torch.float32), (2048, 0.2, 0.15, torch.float16),
         (4096, 0.2, 0.1, torch.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("csr_prune_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, functional, topology

    dev = torch.device("cuda:0")
    lines = []
    for size, start, target, dtype in CASES:
        for per_row in (False, True):
            g = torch.Generator(device="cpu").manual_seed(size)
            weight = torch.randn(size, size, generator=g).to(dtype).to(dev)
            module = SparseLinear.from_dense(weight, density=start, per_row=per_row)
            first = module.values
            reference = [t.clone() for t in (module.row_indices, module.row_offsets, module.column_indices)]

            def restore():
                # the step is timed from the same layer every time: put the first one back
                functional.unregister_static_topology(module.row_indices, module.row_offsets, module.column_indices)
                module._set_topology(first, *(t.clone() for t in reference))

            def prune(device_build):
                topology.enable_device_build(device_build)
                try:
                    restore()
                    source = module.prune_to(density=target, per_row=per_row)
                finally:
                    topology.enable_device_build(True)
                return source, module.values.detach(), module.row_indices, module.row_offsets, module.column_indices

            def detour():
                restore()
                values = module.values.detach()
                lengths = (module.row_offsets[1:] - module.row_offsets[:-1]).to(torch.int64)
                rows = torch.repeat_interleave(torch.arange(size, device=dev), lengths, output_size=values.numel())
                image = torch.zeros(size, size, dtype=dtype, device=dev)
                image[rows, module.column_indices.to(torch.int64)] = values
                return topology.magnitude_prune(image, density=target, per_row=per_row)

            fns = {"prune_device": lambda: prune(True), "prune_torch": lambda: prune(False), "dense_detour": detour}
            built, sorted_, dense = fns["prune_device"](), fns["prune_torch"](), fns["dense_detour"]()
            same = all(torch.equal(a, b) for a, b in zip(built, sorted_))
            assert same, "csr_prune_bench: the device path and the torch path differ"
            assert all(torch.equal(a, b) for a, b in zip((built[1],) + built[2:], dense)), \
                "csr_prune_bench: the dense detour gives another pattern"
            restore_only = measure({"restore": restore}, 5, 1, args.inner)["restore"]["median_us"]
            timed = measure(fns, args.rounds, args.warmup, args.inner)
            spread = timed["prune_torch"]["p90_us"] - timed["prune_torch"]["p10_us"]
            device = timed["prune_device"]["median_us"]
            line = dict(case=f"SparseLinear.prune_to(density={target}, per_row={per_row})", out_features=size,
                        in_features=size, density_from=start, density_to=target, per_row=per_row,
                        dtype=str(dtype).split(".")[-1], nonzeros_from=first.numel(), nonzeros_to=built[1].numel(),
                        same_result=same, restore_us=restore_only, **timed, torch_spread_us=round(spread, 1),
                        device_not_slower=device <= timed["prune_torch"]["median_us"] + spread,
                        speedup_over_torch=round(timed["prune_torch"]["median_us"] / device, 2),
                        speedup_over_dense_detour=round(timed["dense_detour"]["median_us"] / device, 2))
            lines.append(line)
            print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
