#!/usr/bin/env python3
"""SparseAttention on half storage against today's paths, config 3 (seq 1024, 8 heads of
64, batch 8, projection density 0.1, mask density 0.1; the module as bench.py builds it),
in ONE process: device events per call, the variants alternated round by round after a
warm-up, the median per variant.

  fp32            float32 inputs (the flagship forward)
  widen_<t>       <t> inputs, default flag: widened to float32 in the first layout pass
  half_<t>_w<v>   half_storage=True, <t> inputs, <v> (float32 | half) projection values
  fwdbwd_*        forward + backward of fp32 and of half_<t>_w<v>

    python tools/half_attention_bench.py [--rounds 20] [--out profiles/half_attention_c3.json]

The per-kernel table comes from a separate run under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torch_sputnik_amd import SparseAttention, capi  # noqa: E402


def build(dev, seq, emb, heads, half_storage, values_dtype=None):
    torch.manual_seed(0)
    attn = SparseAttention(heads, emb, max_sequence_length=seq, device=dev, sparsity=0.9,
                           mask_generator=np.random.default_rng(0), half_storage=half_storage)
    for lin in attn.linears:
        w = torch.randn(emb, emb, device=dev) * (torch.rand(emb, emb, device=dev) < 0.1)
        lin.weight = torch.nn.Parameter(w)
        lin.setup_sparse_tensors()
        if values_dtype is not None:
            lin.values = torch.nn.Parameter(lin.values.detach().to(values_dtype))
    return attn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="profiles/half_attention_c3.json")
    ap.add_argument("--only", default="", help="comma-separated variant names (profiling runs)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    seq, emb, heads, batch = 1024, 512, 8, 8
    g = torch.Generator(device="cpu").manual_seed(1)
    x32 = torch.randn(batch, seq, emb, generator=g).to(dev)
    go32 = torch.randn(batch, seq, emb, generator=g).to(dev)

    variants = {}
    base = build(dev, seq, emb, heads, False)

    def forward(module, x):
        def run():
            with torch.no_grad():
                module(x, x, x)
        return run

    def train(module, x, go):
        def run():
            xg = x.detach().requires_grad_(True)
            module(xg, xg, xg).backward(go)
            module.zero_grad(set_to_none=True)
        return run

    variants["fp32"] = forward(base, x32)
    variants["fwdbwd_fp32"] = train(base, x32, go32)
    for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        variants[f"widen_{name}"] = forward(base, x32.to(dt))
        for vname, vdt in (("f32", None), ("half", dt)):
            module = build(dev, seq, emb, heads, True, vdt)
            variants[f"half_{name}_w{vname}"] = forward(module, x32.to(dt))
            variants[f"fwdbwd_half_{name}_w{vname}"] = train(module, x32.to(dt), go32.to(dt))
    if args.only:
        keep = set(args.only.split(","))
        variants = {k: v for k, v in variants.items() if k in keep}

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(args.per_round)]
            for s, e in events:
                s.record()
                fn()
                e.record()
            torch.cuda.synchronize()
            times[name] += [s.elapsed_time(e) for s, e in events]
    result = {"build_id": capi.build_id(), "config": "c3 seq 1024 emb 512 heads 8 batch 8",
              "rounds": args.rounds, "per_round": args.per_round,
              "ms_median": {k: float(np.median(v)) for k, v in times.items()},
              "ms_min": {k: float(np.min(v)) for k, v in times.items()}}
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
