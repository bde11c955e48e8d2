#!/usr/bin/env python3
"""What one step of GLOBAL magnitude pruning costs: ``topology.prune_layers_to(modules, density)``
on the device kernels (csrc/topology.hip, ``ops.csr_topk_global``), the same call on the torch
path (``topology.enable_device_build(False)``), and what a user pays today -- a loop of
``SparseLinear.prune_to`` per layer at the same density, which ranks inside each layer and so
keeps ANOTHER set; it is shown as a cost only -- in ONE process, the three alternated round by
round.

Models: four 2048 x 2048 float32 layers from overall density 0.5 to 0.4, and twelve float16
layers alternating 1024 x 4096 and 4096 x 1024 from 0.2 to 0.1, each layer from
``SparseLinear.from_dense`` of a weight whose scale differs per layer (a global threshold cuts
the layers unequally).  Every step starts from the same layers: the first Parameters and
patterns are put back before each call (``restore_us``, measured alone, and its share of the
device median, ``restore_share``).

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all paths.  The device path and the torch path must give equal tensors before
anything is timed.  Per model one JSON line: median, min, 10th and 90th percentile per path,
``speedup_over_torch`` and ``speedup_over_per_layer`` (their medians over the device median)
and ``device_not_slower``: the device median is at most the torch median plus the torch path's
own spread (p90 - p10).  Kernel times alone are not measured.  ``--out FILE`` appends the
lines there."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.regrow_bench import measure  # noqa: E402

MODELS = (("4 x 2048^2", [(2048, 2048)] * 4, 0.5, 0.4, torch.float32),
          ("12 x (1024x4096, 4096x1024)", [(1024, 4096), (4096, 1024)] * 6, 0.2, 0.1, torch.float16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("global_prune_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, functional, topology

    dev = torch.device("cuda:0")
    lines = []
    for name, shapes, start, target, dtype in MODELS:
        g = torch.Generator(device="cpu").manual_seed(len(shapes))
        modules = []
        for l, (out_f, in_f) in enumerate(shapes):
            weight = (torch.randn(out_f, in_f, generator=g) * (1.0 + 0.25 * (l % 4))).to(dtype).to(dev)
            modules.append(SparseLinear.from_dense(weight, density=start))
        firsts = [m.values for m in modules]
        references = [[t.clone() for t in (m.row_indices, m.row_offsets, m.column_indices)] for m in modules]

        def restore():
            # the step is timed from the same layers every time: put the first ones back
            for module, first, reference in zip(modules, firsts, references):
                functional.unregister_static_topology(module.row_indices, module.row_offsets, module.column_indices)
                module._set_topology(first, *(t.clone() for t in reference))

        def snapshot(sources):
            return [(s, m.values.detach(), m.row_indices, m.row_offsets, m.column_indices)
                    for s, m in zip(sources, modules)]

        def prune(device_build):
            topology.enable_device_build(device_build)
            try:
                restore()
                sources = topology.prune_layers_to(modules, density=target)
            finally:
                topology.enable_device_build(True)
            return snapshot(sources)

        def per_layer():
            restore()
            return snapshot([module.prune_to(density=target) for module in modules])

        fns = {"global_device": lambda: prune(True), "global_torch": lambda: prune(False), "per_layer_prune_to": per_layer}
        built, sorted_, looped = fns["global_device"](), fns["global_torch"](), fns["per_layer_prune_to"]()
        same = all(torch.equal(a, b) for x, y in zip(built, sorted_) for a, b in zip(x, y))
        assert same, "global_prune_bench: the device path and the torch path differ"
        restore_only = measure({"restore": restore}, 5, 1, args.inner)["restore"]["median_us"]
        timed = measure(fns, args.rounds, args.warmup, args.inner)
        spread = timed["global_torch"]["p90_us"] - timed["global_torch"]["p10_us"]
        device = timed["global_device"]["median_us"]
        line = dict(case=f"topology.prune_layers_to(density={target})", model=name, layers=len(shapes),
                    positions=sum(o * i for o, i in shapes), density_from=start, density_to=target,
                    dtype=str(dtype).split(".")[-1], nonzeros_from=sum(f.numel() for f in firsts),
                    nonzeros_to=sum(b[1].numel() for b in built),
                    nonzeros_to_per_layer=[b[1].numel() for b in built],
                    per_layer_prune_to_keeps=[b[1].numel() for b in looped], same_result=same,
                    restore_us=restore_only, restore_share=round(restore_only / device, 3), **timed,
                    torch_spread_us=round(spread, 1), kernel_times="not measured",
                    device_not_slower=device <= timed["global_torch"]["median_us"] + spread,
                    speedup_over_torch=round(timed["global_torch"]["median_us"] / device, 2),
                    speedup_over_per_layer=round(timed["per_layer_prune_to"]["median_us"] / device, 2))
        lines.append(line)
        print(json.dumps(line), flush=True)

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
