"""CPU: the case list of tests/spmm_flat_cases.py reaches what it claims.  Every edge is recounted
from the plan model by the walk models of the three loops (spmm_flat_cases.edges): each case is
held to the edges it is in the list for, the whole list to every boundary slot, drain path, vmcnt
counter class and all 64 + 64 group-loop labels; the plan model is checked against an independent
per-entry recount; the run list is asked of the host-only launch query under knob
SPUTNIK_HIP_SPMM_KERNEL=flat, and stays inside the budget written in spmm_flat_cases.  No GPU."""
import numpy as np
import pytest
import torch

import spmm_flat_cases as F
from torch_sputnik_amd import capi

KNOB_NAMES = ("SPUTNIK_HIP_SPMM_KERNEL", "SPUTNIK_HIP_SPMM_SPARSE", "SPUTNIK_HIP_SPMM_MEDIUM",
              "SPUTNIK_HIP_SPMM_DEBUG")
RUNS = F.runs()
EXTENDED = f"extended_64x{F.EXTENDED_K}"


@pytest.fixture
def knobs(monkeypatch):
    """Sets SPUTNIK_HIP_SPMM_* for one query; the library looks again, and once more afterwards."""
    def set_knobs(env):
        for name in KNOB_NAMES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        capi.reload_options()
    yield set_knobs
    monkeypatch.undo()
    capi.reload_options()


# ---------------------------------------------------------------------------
# the matrices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_case_is_a_valid_served_matrix(name):
    c = F.case(name)
    ri, ro, ci = c.csr
    assert np.array_equal(np.sort(ri), np.arange(c.m))
    assert np.array_equal(np.sort(c.other_order()), np.arange(c.m)) and not np.array_equal(c.other_order(), ri)
    assert ro[0] == 0 and ro[-1] == c.nnz and (np.diff(ro) >= 0).all()
    assert c.m >= 64 and c.k >= 32 and c.nnz >= 16 * c.m, (name, c.m, c.k, c.nnz)
    column_k = [row for row, kind in c.faults.items() if kind == "column_k"]
    for row in range(c.m):
        cols = ci[ro[row]:ro[row + 1]]
        if row in c.faults:
            assert not (np.diff(cols) > 0).all() or cols[-1] >= c.k, (name, row)
            assert row in column_k or (cols.min() >= 0 and cols.max() < c.k), (name, row)
        else:
            assert (np.diff(cols) > 0).all() and (len(cols) == 0 or (cols[0] >= 0 and cols[-1] < c.k)), (name, row)
    assert set(c.unsorted_rows) == set(c.faults)
    # an out-of-range column only in a case whose runs launch no product
    if column_k:
        assert all(run.plan_only for run in RUNS if run.case_name == name)


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_case_shows_the_edges_it_is_named_for(name):
    missing = F.CLAIMS[name] - F.case_edges(name)
    assert not missing, (name, sorted(missing, key=str))


def test_the_list_reaches_every_label_of_every_loop():
    """Over the whole list, each required edge through the case that claims it: a case taken out
    of CASE_NAMES makes this test name the labels that are no longer reached."""
    assert set(F.CLAIMS) >= set(F.CASE_NAMES)
    reached = set()
    for name in F.CASE_NAMES:
        reached |= F.CLAIMS[name] & F.case_edges(name)
    required = set().union(*F.CLAIMS.values())
    for loop in ("entry", "group"):
        required |= {("boundary", loop, slot) for slot in range(16)}
        required |= {("nsw", loop, v) for v in range(4)} | {("sb", loop, v) for v in range(3)}
    required |= {("drain", path) for path in range(4)} | F.ALL_LABELS
    assert len(F.ALL_LABELS) == 2 * 128      # 64 + 64 in each group layout
    missing = required - reached
    assert not missing, ("no longer reached", sorted(missing, key=str))
    run_cases = {run.case_name for run in RUNS}
    assert run_cases == set(F.CASE_NAMES), set(F.CASE_NAMES) ^ run_cases


def test_every_case_claims_an_edge_of_its_own():
    """Every case claims at least one edge that no other case claims, so that no case can leave
    the list unnoticed."""
    for name in F.CASE_NAMES:
        others = set().union(*(v for k, v in F.CLAIMS.items() if k != name))
        assert F.CLAIMS[name] - others, name


# ---------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------
def recount_group(c, ri, g, k):
    """(ok, [(column, wave-row, position)] sorted) of group g, entry by entry."""
    slots = F.ceil_div(c.m, F.PER) * F.PER
    entries, ok = [], True
    for r in range(F.RPW):
        e = F.dealt_index(g * F.RPW + r, slots, F.PER)
        if e >= c.m:
            continue
        row = int(ri[e])
        prev = -1
        for p in range(int(c.row_offsets[row]), int(c.row_offsets[row + 1])):
            col = int(c.column_indices[p])
            ok &= prev < col < k
            prev = col
            entries.append((col, r, p))
    return ok, sorted(entries)


@pytest.mark.parametrize("name,other", [(n, o) for n in F.CASE_NAMES for o in (False, True)
                                        if not n.startswith(("extended", "groups544")) or not o])
def test_plan_model_against_a_recount(name, other):
    """The vectorised model against a walk over single entries: layout, row_ok, ChunkInfo, gwin,
    every window entry's three fields, the padding entries, the tail windows, and which bytes
    are defined."""
    c = F.case(name)
    p = F.plan(name, 384, other)
    ri = c.other_order() if other else c.row_indices
    lay = p.layout
    assert lay.cinfo_off % 256 == 0 and lay.gwin_off % 256 == 0 and lay.stream_off % 256 == 0 and lay.bytes % 256 == 0
    assert lay.cinfo_off >= 4 * lay.slots and lay.gwin_off >= lay.cinfo_off + 16 * (lay.nchunks + 1) * lay.groups
    words = p.bytes.view(np.uint32)
    defined = p.defined.reshape(-1, 4)
    assert (defined.all(axis=1) | ~defined.any(axis=1)).all()
    window = 0
    groups = range(lay.groups) if lay.groups <= 64 else list(range(0, lay.groups, 37)) + [lay.groups - 1]
    for g in range(lay.groups):
        ok, entries = recount_group(c, ri, g, c.k) if g in groups else (None, None)
        assert words[lay.gwin_off // 4 + g] == window, (name, g)
        if g not in groups:
            window += int(p.windows[g])
            continue
        assert ok == p.ok[g] and len(entries) == p.total[g]
        nwin = F.ceil_div(len(entries), 16)
        info = words[lay.cinfo_off // 4 + 4 * g * (lay.nchunks + 1):][:4 * (lay.nchunks + 1)].reshape(-1, 4)
        stream = p.bytes[lay.stream_off + window * 144:][:nwin * 144].reshape(nwin, 144)
        assert not info[lay.nchunks].any()
        if not ok:
            assert not info.any() and not stream[:, :128].any() and (stream[:, 128:] == 0x80).all()
            window += nwin
            continue
        columns = sorted({col for col, _, _ in entries})
        for ch in range(lay.nchunks) if lay.nchunks <= 70 else (0, 1, 700, lay.nchunks - 1):
            mine = [col for col in columns if col // 32 == ch]
            first = sum(((ch & 1) * 32 + col % 32) << (8 * q) for q, col in enumerate(mine[:3]))
            assert info[ch].tolist() == [len(mine), first, 0, sum(1 for e in entries if e[0] // 32 == ch)], (name, g, ch)
        for at, (col, r, pos) in enumerate(entries):
            ch, j = divmod(col, 32)
            starts = at == 0 or entries[at - 1][0] != col
            want = (ch & 1) * 32 + j
            if starts:
                i = columns.index(col)
                if i + 3 < len(columns) and columns[i + 3] // 32 == ch:
                    want |= ((ch & 1) * 32 + columns[i + 3] % 32) << 8
            record = stream[at // 16]
            got = record[8 * (at % 16):8 * (at % 16) + 8].view(np.uint32)
            assert (int(got[0]), int(got[1]), int(record[128 + at % 16])) == (want, 4 * pos, 8 * r | (0x80 if starts else 0)), \
                (name, g, at)
        for at in range(len(entries), 16 * nwin):
            record = stream[at // 16]
            assert not record[8 * (at % 16):8 * (at % 16) + 8].any() and record[128 + at % 16] == 0x80
        window += nwin
    tail = p.bytes[lay.stream_off + window * 144:][:4 * 144].reshape(4, 144)
    assert not tail[:, :128].any() and (tail[:, 128:] == 0x80).all()
    end = lay.stream_off + (window + 4) * 144
    assert p.defined[lay.stream_off:end].all() and not p.defined[end:].any() and end <= lay.bytes
    assert p.defined[:4 * lay.slots].all() and not p.defined[4 * lay.slots:lay.cinfo_off].any()
    assert not p.defined[lay.cinfo_off + 16 * (lay.nchunks + 1) * lay.groups:lay.gwin_off].any()
    assert not p.defined[lay.gwin_off + 4 * lay.groups:lay.stream_off].any()
    for slot in range(lay.slots):
        e = F.dealt_index(slot, lay.slots, F.PER)
        assert words[slot] == (0 if e < c.m and int(ri[e]) in c.faults else 1), (name, slot)


def test_walk_models_on_hand_made_streams():
    """The walks on streams small enough to follow by hand."""
    # two chunks of 16 and 1 entries: the switch behind slot 15 comes before the boundary at slot 0
    w = F.walk_entry([16, 1])
    assert [b[0] for b in w.boundaries] == [0, 1] and w.drain == 1 and w.consumed == 17
    assert w.switches == [1, 0] and [b[1:] for b in w.boundaries] == [(2, True), (0, False)]
    # three chunks, the middle one empty: two boundaries at slot 3 with no switch in between
    w = F.walk_entry([3, 0, 2])
    assert [b[0] for b in w.boundaries] == [3, 3, 5] and w.drain == 1
    assert [b[1:] for b in w.boundaries] == [(1, True), (0, True), (0, False)]
    # one chunk: nothing is staged behind the prologue
    w = F.walk_entry([0])
    assert w.boundaries == [(0, 1, False)] and w.switches == [0] and w.drain == 0
    # the group loop: groups of 2, 1 | 3 entries, then padding
    flag = 0x80
    rows = [flag, 8, flag | 16, flag, 8, 16] + [flag] * 10
    for layout in F.LAYOUTS:
        w = F.walk_group([2, 1], rows, layout)
        assert w.starts == [(3, 0), (0, 2), (3, 3)] and w.continued == [(0, 1), (0, 4), (0, 5)], layout
        assert [b[0] for b in w.boundaries] == [3, 6] and w.consumed == 6
        # twenty single-entry groups in one chunk: the strip goes round, the switch falls between
        w = F.walk_group([20], [flag] * 32, layout)
        assert w.starts == [((3 + i) % 4, i % 16) for i in range(20)] and w.switches == [0, 0], layout
        assert w.boundaries == [(4, 2, False)]


def test_entry_and_group_walks_agree_on_every_wave():
    """Both loops take their boundaries at the same slots with the same counters (asserted inside
    edges() for every wave of every case); here: the counters of one designed wave by hand."""
    p = F.plan("counts_248x352", 384)
    g = [g for g, name in F.case("counts_248x352").waves.items() if name == "short_chunks"][0]
    assert p.centries[g].tolist() == [3, 4, 2, 5, 1, 3, 2, 6, 4, 1, 2]
    w = F.walk_entry(p.centries[g])
    assert [b[0] for b in w.boundaries] == [3, 7, 9, 14, 15, 2, 4, 10, 14, 15, 1]
    assert max(w.switches) >= 2 and [b[1] for b in w.boundaries][:5] == [1, 0, 0, 0, 0]


# ---------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------
def has_device():
    return torch.cuda.is_available()


@pytest.mark.parametrize("run", RUNS, ids=lambda run: run.id)
def test_launch_query_answers_the_run(run, knobs):
    c = run.case
    assert F.applicable(c.m, c.k, run.n, c.nnz), run.id
    knobs(run.knobs())
    got = capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 4)
    if run.case_name == EXTENDED and not has_device():
        pytest.skip("the fill kernel's tables of this k need the extended LDS, which the library asks the device "
                    "for: without a device it answers for the default 64 KiB; asserted where there is one")
    assert (got["family"], got["table_offset"]) == ("flat", 0), (run.id, got)
    assert F.plan(run.case_name, run.n).layout.bytes == capi.spmm_workspace_bytes(c.m, c.k, run.n, c.nnz), run.id
    for loop in range(3):
        knobs(run.knobs(loop))
        assert capi.spmm_kernel_name(c.m, c.k, run.n, c.nnz, run.replicas) == f"spmm_flat_kernel<{loop}>"
    if run.wide512:
        knobs({"SPUTNIK_HIP_SPMM_KERNEL": "wide512"})
        assert capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 16)["family"] == "wide512", run.id


def test_extended_case_is_the_smallest_k_past_the_default_lds():
    c = F.case(EXTENDED)
    assert F.fill_tables_bytes(F.ceil_div(c.k, 32)) > 64 * 1024 >= F.fill_tables_bytes(F.ceil_div(c.k - 1, 32))
    assert F.fill_stage_windows(F.ceil_div(c.k, 32), c.nnz, 32) == 0
    assert 64 <= c.m <= 256 and all(run.n == 384 for run in RUNS if run.case_name == EXTENDED)


@pytest.mark.parametrize("name", sorted(F.OFF_ROUTE))
def test_shapes_meant_to_fall_off_the_flat_route_do(name, knobs):
    shape = F.OFF_ROUTE[name]
    assert not F.applicable(*shape)
    knobs({"SPUTNIK_HIP_SPMM_KERNEL": "flat"})
    assert capi.spmm_launch_shape(*shape, 1, 4)["family"] != "flat", name


def test_runs_cover_the_mappings_and_the_operand_forms():
    by_mapping = {}
    for run in RUNS:
        if not run.plan_only:
            by_mapping.setdefault(run.mapping(), []).append(run)
    assert set(by_mapping) == {"xcd1", "xcd2", "xcd3", "eighths", "linear"}, set(by_mapping)
    eighths = {(run.n_tiles, run.debug) for run in by_mapping["eighths"]}
    # code 0 at eight tiles, code 2 where the row blocks do not divide, sixteen tiles
    assert eighths == {(8, F.xcd(0)), (8, F.xcd(2)), (16, 0)}, eighths
    linear = {(run.n_tiles, run.replicas) for run in by_mapping["linear"]}
    assert linear >= {(t, r) for t in (1, 3) for r in (1, 3, 4)}, linear
    totals = {run.grid_total() % 8 == 0 for run in by_mapping["linear"]}
    assert totals == {True, False}
    assert {run.n for run in RUNS} >= {384, 510, 512, 768, 771, 3588, 7684}
    three = {run.n % 4 for run in RUNS if run.n_tiles == 3}
    assert three >= {1, 3}, three
    assert {run.shared for run in RUNS if run.replicas > 1} == {True, False}
    assert {F.case(run.case_name).k for run in RUNS} >= {32, 33, 63, 64, 65, 352, 2080, F.EXTENDED_K}
    stage = [run for run in RUNS if run.debug & F.STAGE_ALL_OFF]
    assert len(stage) == 1 and not F.plan(stage[0].case_name, stage[0].n).staged(stage[0].debug).any()
    assert all(run.debug & ~0xf000 == 0 for run in RUNS), "bits 0-5 and 8-10 are timing experiments"
    fallback = [run for run in RUNS if F.case(run.case_name).faults and not run.plan_only]
    assert {run.n % 4 == 0 for run in fallback} == {True, False} and len(fallback) == 2


def test_the_list_stays_inside_its_budget():
    assert len(RUNS) <= F.MAX_RUNS
    largest = max(4 * max(run.replicas * (run.case.k * run.n + F.STRIDE_PAD), run.replicas * (run.case.m * run.n + F.STRIDE_PAD))
                  for run in RUNS)
    assert largest <= F.MAX_OPERAND_BYTES, largest
    flops = sum(F.reference_flops(run) for run in RUNS if not run.plan_only)
    assert flops <= F.MAX_REFERENCE_FLOPS, flops
    for run in RUNS:
        c = run.case
        assert c.m <= 256 or run.case_name.startswith(("unsorted", "groups544", "map_1024")), run.id
        assert F.plan(run.case_name, run.n).layout.bytes <= 1 << 20, run.id
