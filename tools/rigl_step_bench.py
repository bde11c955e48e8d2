#!/usr/bin/env python3
"""What RigL's grow scores cost on ``SparseLinear``: the dense weight gradient collected in
the backward pass (``collect_dense_grad``), the standalone ``ops.dense_weight_grad`` against
torch's einsum, and one ``rigl_update`` -- in ONE process, the paths of a group alternated
round by round.

Shape: a 2048 x 2048 layer at density 0.2, batch 8 x seq 512.  Operand pairs (dy x x):
half x half (the op only: autograd hands a layer the float32 dy of its float32 output),
float32 dy x half x (float16 activations) and float32 x float32 (a float32 layer).

  (a) backward   float16 activations: the layer's backward (weight and input gradient, on a
                 retained graph) ``disarmed``, ``armed`` (the weight gradient's launch stores
                 its tiles whole) and ``disarmed_plus_op`` (disarmed, then
                 ``ops.dense_weight_grad`` on its own); a float32 layer: ``disarmed`` and
                 ``armed`` (one more tile launch)
  (b) op         ``ops.dense_weight_grad(dy, x)`` and ``torch.einsum("bos,bsi->oi", dy, x)`` on
                 the same tensors (torch in the operands' type; its result is in that type too)
  (c) rigl       ``rigl_update(0.3, per_row=True)`` from the same pattern and scores every time
                 (the pattern is put back before each call; ``restore_us`` alone)

Every sample is a host clock around ``inner`` calls that end in a device synchronise, after
warm-up of all paths.  Per group one JSON line with median, min, 10th and 90th percentile per
path.  ``--out FILE`` appends the lines there (profiles/rigl_step.jsonl)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.regrow_bench import measure  # noqa: E402

PAIRS = (("half_x_half", torch.float16, torch.float16), ("float32_x_half", torch.float32, torch.float16),
         ("float32_x_float32", torch.float32, torch.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rigl_step_bench: needs a GPU (no CPU timing stands in for it)")

    from torch_sputnik_amd import SparseLinear, functional, ops

    dev = torch.device("cuda:0")
    size, batch, seq = args.size, args.batch, args.seq
    shape = dict(out_features=size, in_features=size, density=args.density, batch=batch, seq=seq)
    gen = torch.Generator(device="cpu").manual_seed(size)
    weight = torch.randn(size, size, generator=gen).to(dev)
    x32 = torch.randn(batch, seq, size, generator=gen).to(dev)
    dy32 = torch.randn(batch, size, seq, generator=gen).to(dev)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for name, dy_dtype, x_dtype in PAIRS:
        layer = SparseLinear.from_dense(weight, density=args.density, per_row=True)
        x = x32.to(x_dtype).requires_grad_(True)
        dy = dy32.to(dy_dtype)
        # (autograd hands the layer a float32 dy -- its output is float32 -- so the backward is
        # timed for the float32 dy only; the half x half pair is the op's, (b))
        upstream = dy.float()

        # ---- (a) the layer's backward ----
        y = layer(x)

        def backward(armed, extra_op=False):
            layer.collect_dense_grad(armed)   # (looked at when the backward runs)
            layer.zero_dense_grad()
            layer.values.grad = None
            x.grad = None
            y.backward(upstream, retain_graph=True)
            if extra_op:
                return ops.dense_weight_grad(upstream, x.detach(), "bsi")
            return layer.dense_grad

        fns = {"disarmed": lambda: backward(False), "armed": lambda: backward(True)}
        if x_dtype != torch.float32:
            fns["disarmed_plus_op"] = lambda: backward(False, True)
        if dy_dtype == torch.float32:   # (the backward sees a float32 dy either way)
            assert backward(False) is None and backward(True) is not None
            timed = measure(fns, args.rounds, args.warmup, args.inner)
            emit(dict(case="backward", operands=name, **shape, **timed,
                      armed_over_disarmed=round(timed["armed"]["median_us"] / timed["disarmed"]["median_us"], 3)))
        layer.collect_dense_grad(False)
        layer.zero_dense_grad()

        # ---- (b) the op against torch ----
        xd = x.detach()
        wide = dy_dtype if dy_dtype == x_dtype else torch.float32
        dy_t, x_t = dy.to(wide), xd.to(wide)      # (torch.einsum wants one type: widened once, untimed)
        got = ops.dense_weight_grad(dy, xd, "bsi")
        want = torch.einsum("bos,bsi->oi", dy.double(), xd.double())
        worst = float(((got.double() - want).abs() / (want.abs() + want.abs().mean())).max())
        assert worst < 1e-4, f"rigl_step_bench: dense_weight_grad is off by {worst}"
        timed = measure({"dense_weight_grad": lambda: ops.dense_weight_grad(dy, xd, "bsi"),
                         "torch_einsum": lambda: torch.einsum("bos,bsi->oi", dy_t, x_t)},
                        args.rounds, args.warmup, args.inner)
        emit(dict(case="op", operands=name, **shape, torch_operand_dtype=str(wide).split(".")[-1],
                  max_rel_err=worst, **timed,
                  speedup_over_torch=round(timed["torch_einsum"]["median_us"] /
                                           timed["dense_weight_grad"]["median_us"], 2)))

        # ---- (c) one RigL step ----
        if dy_dtype == torch.float32:
            scores = got
            reference = [t.clone() for t in (layer.values.detach(), layer.row_indices, layer.row_offsets,
                                             layer.column_indices)]

            def restore():
                with torch.no_grad():
                    layer.values.copy_(reference[0])
                functional.unregister_static_topology(layer.row_indices, layer.row_offsets, layer.column_indices)
                layer._set_topology(None, *(t.clone() for t in reference[1:]))

            def rigl():
                restore()
                layer.dense_grad = scores
                return layer.rigl_update(0.3, per_row=True)

            assert int((rigl() < 0).sum()) > 0
            restore_only = measure({"restore": restore}, 5, 1, args.inner)["restore"]["median_us"]
            timed = measure({"rigl_update": rigl}, args.rounds, args.warmup, args.inner)
            emit(dict(case="rigl_update(0.3, per_row=True)", operands=name, **shape, restore_us=restore_only,
                      **timed))

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
