"""The SDDMM host decisions over a grid of shapes, storage types and knobs, against a recorded
table (tests/golden/sddmm_route_table.json): which kernel a plain call takes, the route of a
summed call, and what the workspace / scratch queries answer.  Host only.

The launch paths and these queries share one route function per form (csrc/sddmm.hip:
plain_route, sum_route), so a change of this table is a change of what the calls launch.

Run as a script, the module records the table from the library as built:
    python tests/test_sddmm_route_table_cpu.py
"""
import ctypes
import itertools
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sddmm_route_table.json")

M = (16, 203, 267, 1024, 4096)
N = (16, 300, 2048)
K = (64, 100, 128, 256, 320, 384, 512, 1024, 4096)
REPLICAS = (1, 3, 8, 64, 70000)
KNOBS = (
    {},
    {"SPUTNIK_HIP_SDDMM_KERNEL": "tiled"},
    {"SPUTNIK_HIP_SDDMM_KERNEL": "wave"},
    {"SPUTNIK_HIP_SDDMM_KERNEL": "mfma"},
    {"SPUTNIK_HIP_SDDMM_PANEL": "128"},
    {"SPUTNIK_HIP_SDDMM_SLAB": "80"},
    {"SPUTNIK_HIP_SDDMM_SLAB": "128"},
    {"SPUTNIK_HIP_SDDMM_FLAT": "0"},
)
KNOB_NAMES = ("SPUTNIK_HIP_SDDMM_KERNEL", "SPUTNIK_HIP_SDDMM_PANEL", "SPUTNIK_HIP_SDDMM_SLAB",
              "SPUTNIK_HIP_SDDMM_FLAT", "SPUTNIK_HIP_SDDMM_DEBUG", "SPUTNIK_HIP_MFMA_TILE")
F32, F16, BF16 = 0, 1, 2   # SPUTNIK_HIP_F32 / _F16 / _BF16
TYPES = (("f32", F32, 4), ("f16", F16, 2), ("bf16", BF16, 2))


def nonzero_counts(m, n):
    return (3 * m, 4 * m, 32 * m, min(m * n // 2, 1 << 20))


def shapes():
    """(m, k, n, nnz); every one is asked at each of REPLICAS."""
    for m, n, k in itertools.product(M, N, K):
        for nnz in nonzero_counts(m, n):
            yield m, k, n, nnz


def answers_of(capi, shape):
    """Every answer of the queries for one shape under the current knobs: {column: value}."""
    m, k, n, nnz, replicas = shape
    L = capi.lib()
    out = {
        "workspace_bytes": L.sputnik_hip_sddmm_workspace_bytes(m, k, n, nnz),
        "sum_workspace_bytes": L.sputnik_hip_sddmm_sum_workspace_bytes(m, k, n, nnz),
    }
    # (whole partial vectors of nnz floats: stored as their number, which repeats across shapes)
    scratch = L.sputnik_hip_sddmm_sum_scratch_bytes(m, k, n, nnz, replicas)
    assert scratch % (4 * nnz) == 0
    out["sum_scratch_bytes / (4 nnz)"] = scratch // (4 * nnz)
    for name, code, elem_bytes in TYPES:
        for planned in (0, 1):
            out[f"kernel_name/{name}/planned={planned}"] = \
                L.sputnik_hip_sddmm_kernel_name(m, k, n, nnz, replicas, elem_bytes, planned).decode()
            for mixed in ((0,) if code == F32 else (0, 1)):
                outs = [ctypes.c_int(-1) for _ in range(5)]
                status = L.sputnik_hip_sddmm_sum_route(
                    m, k, n, nnz, replicas, code, planned, mixed,
                    *[ctypes.cast(ctypes.pointer(o), ctypes.c_void_p) for o in outs])
                route = f"status {status}" if status != 0 else \
                    "%s %d %d %d %d" % ((capi.SUM_KERNELS[outs[0].value],) + tuple(o.value for o in outs[1:]))
                out[f"sum_route/{name}/planned={planned}/mixed={mixed}"] = route
                if mixed and not planned:
                    # the (float32, half) pairs, either way round: the float32 operand's half planes,
                    # then `splits` partial vectors -- stored without the vectors, whose bytes
                    # differ with every nnz
                    vectors = 4 * nnz * outs[4].value if status == 0 else 0
                    for pair, lhs, rhs in ((f"f32,{name}", F32, code), (f"{name},f32", code, F32)):
                        out[f"mixed_scratch_bytes/{pair} - 4 nnz splits"] = \
                            L.sputnik_hip_sddmm_sum_mixed_scratch_bytes(m, k, n, nnz, replicas, lhs, rhs) - vectors
    return out


def walk(capi):
    """{column: [for every knob set: [for every shape: the answers at each of REPLICAS]]}"""
    saved = {name: os.environ.pop(name, None) for name in KNOB_NAMES}
    columns = {}
    try:
        for knobs in KNOBS:
            os.environ.update(knobs)
            capi.reload_options()
            for column in columns.values():
                column.append([])
            for shape in shapes():
                at_replicas = [answers_of(capi, shape + (replicas,)) for replicas in REPLICAS]
                for column in at_replicas[0]:
                    columns.setdefault(column, [[]])[-1].append(tuple(a[column] for a in at_replicas))
            for name in knobs:
                del os.environ[name]
    finally:
        for name, value in saved.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value
        capi.reload_options()
    return columns


def pack(by_knobs):
    """One row per distinct answer ("values"), one per distinct run of them over REPLICAS
    ("tuples", of rows of values), and per knob set the shapes' tuples as runs
    [tuple, length, tuple, length, ...] -- or the number of an earlier knob set that answers alike."""
    values, tuples, sequences = {}, {}, []
    for sequence in by_knobs:
        runs = []
        for answers in sequence:
            t = tuples.setdefault(tuple(values.setdefault(v, len(values)) for v in answers), len(tuples))
            if runs and runs[-2] == t:
                runs[-1] += 1
            else:
                runs += [t, 1]
        sequences.append(sequences.index(runs) if runs in sequences else runs)
    return {"values": list(values), "tuples": [list(t) for t in tuples], "knobs": sequences}


def pack_columns(columns):
    """Columns that answer alike (float16 and bfloat16, mostly) are stored once."""
    packed, first = {}, {}
    for name, by_knobs in sorted(columns.items()):
        same = first.setdefault(json.dumps(by_knobs), name)
        packed[name] = pack(by_knobs) if same == name else {"same_as": same}
    return packed


def unpack(packed, name):
    column = packed[name]
    if "same_as" in column:
        return unpack(packed, column["same_as"])
    tuples = [tuple(column["values"][row] for row in t) for t in column["tuples"]]
    by_knobs = []
    for runs in column["knobs"]:
        if isinstance(runs, int):
            runs = column["knobs"][runs]
        by_knobs.append([tuples[t] for t, length in zip(runs[::2], runs[1::2]) for _ in range(length)])
    return by_knobs


def test_sddmm_decisions_match_the_recorded_table():
    from torch_sputnik_amd import capi
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["knobs"] == [[list(i) for i in sorted(k.items())] for k in KNOBS]
    assert golden["replicas"] == list(REPLICAS)
    columns = walk(capi)
    assert sorted(columns) == sorted(golden["columns"])
    for column, got in columns.items():
        want = unpack(golden["columns"], column)
        assert [len(g) for g in got] == [len(w) for w in want] == [len(list(shapes()))] * len(KNOBS)
        differ = [(sorted(knobs.items()), shape, g, w) for knobs, gs, ws in zip(KNOBS, got, want)
                  for shape, g, w in zip(shapes(), gs, ws) if g != w]
        assert not differ, f"{column}: {len(differ)} answers differ, first under knobs {differ[0][0]} at " \
                           f"(m, k, n, nnz) = {differ[0][1]} for replicas {REPLICAS}: got {differ[0][2]!r}, " \
                           f"recorded {differ[0][3]!r}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from torch_sputnik_amd import capi
    table = {"knobs": [[list(i) for i in sorted(k.items())] for k in KNOBS], "replicas": list(REPLICAS),
             "columns": pack_columns(walk(capi))}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print("recorded", GOLDEN, os.path.getsize(GOLDEN), "bytes")
