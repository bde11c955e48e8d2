#!/usr/bin/env python3
"""Prints the case table of tests/test_gpu_structured_masks.py (profiles/structured_mask_routes.txt):
the masks by distinct shape (nnz and nnz / m per kind), then per route its shape, replica counts
and what the library's host-only queries report -- one line where every kind reports the same,
one line per differing kind otherwise.  Host only; the panel SpMM kernel is reported where a
device offers its LDS, so the committed table was printed on the MI355X."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import test_gpu_structured_masks as S   # noqa: E402
from helpers import STRUCTURED_KINDS   # noqa: E402
from torch_sputnik_amd import capi   # noqa: E402


def main():
    routes = {r.id: r for r in S.ALL_ROUTES}
    shapes, reports = {}, {}
    with pytest.MonkeyPatch.context() as patch:
        for rid, kind, nnz, mean, replicas, reported in S.walk_routes(capi, patch):
            route = routes[rid.split("-loop")[0]]
            shapes.setdefault(route.mask_shape + (route.min_mean_row, route.chunk), {})[kind] = (nnz, mean)
            reports.setdefault(rid, {}).setdefault((replicas, reported), []).append(kind)
    print("masks: rows x columns, asked mean row, chunk -> nnz (nnz / m) per kind")
    for (rows, cols, mean, chunk), kinds in shapes.items():
        print(f"\n{rows} x {cols}, nnz >= {mean} m, chunk {chunk}")
        for kind in STRUCTURED_KINDS:
            print(f"  {kind:<26} {kinds[kind][0]:>6} ({kinds[kind][1]:.1f})")
    print("\nroutes: m x k x n, mask, knobs -> replicas: reported (kinds, where they differ)")
    for rid, by in reports.items():
        route = routes[rid.split("-loop")[0]]
        rows, cols = route.mask_shape
        print(f"\n{rid}: {route.m} x {route.k} x {route.n}, mask {rows} x {cols} at >= {route.min_mean_row} m, "
              f"{route.knobs}")
        for (replicas, reported), kinds in by.items():
            which = "every kind" if len(kinds) == len(STRUCTURED_KINDS) else ", ".join(kinds)
            print(f"  {replicas} replica(s): {reported}  ({which})")


if __name__ == "__main__":
    main()
