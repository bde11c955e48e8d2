"""CPU: the matrices of tests/spmm_panel_cases.py reach the edges they are named for -- every edge
is RECOUNTED here from the CSR arrays and the placement alone, through the models of
stream_pairs, search_cuts, stream_masked and the fallback vote -- the search model equals the true
cut exhaustively, and the run list of tests/test_gpu_spmm_panel_instances.py reaches all 24
kernel instances of csrc/spmm_panel.hip with the replica counts, strides and knobs it means to.
Deleting a case or a run fails the test that names the lost edge or label.  No GPU, no library."""
import itertools

import numpy as np
import pytest

import spmm_panel_cases as P

RUNS = P.runs()
MATRICES = {}
for _run in RUNS:
    for _mat in _run.matrices():
        MATRICES.setdefault(_mat.name, _mat)
UNSORTED_BY_DESIGN = ("partitioned_unsorted", "fallback_", "walk_", "mask_cuts_reversed")


def waves(mat, identity=None, row_indices=None):
    for s0 in range(0, P.slots_of(mat.m), P.WAVE_ROWS):
        yield s0, P.wave_bounds(mat, s0, identity, row_indices)


def pairs(mat, identity=None):
    """(slot of the pair, cnt_a [4], cnt_b [4]) of every quad pair."""
    for s0, (_, _, cnt) in waves(mat, identity):
        for t in (0, 2):
            yield s0 + 4 * t, cnt[t], cnt[t + 1]


# ---------------------------------------------------------------------------
# the matrices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_matrix_is_valid_and_small(name):
    mat = MATRICES[name]
    ro, ci = mat.row_offsets, mat.column_indices
    assert ro[0] == 0 and ro[-1] == mat.nnz == len(ci) and (np.diff(ro) >= 0).all()
    assert mat.nnz == 0 or (ci.min() >= 0 and ci.max() < mat.k)
    assert 16 <= mat.m <= 528 and (mat.k <= 1537 or mat.k == 4096)
    for row, cols in enumerate(mat.rows):
        assert len(set(cols.tolist())) == len(cols), (name, row, "a column twice")
    if not name.startswith(UNSORTED_BY_DESIGN):
        assert mat.sorted_rows().all(), name
    assert np.array_equal(np.sort(mat.other_order()), np.arange(mat.m))


def test_shapes_stay_within_the_limits():
    for run in RUNS:
        assert run.n <= 132 and (run.case.k != 4096 or run.n == 64), run.id
        assert all(mat.nnz > 0 for mat in run.matrices()) or run.masks == "three", run.id


WINDOWS = [("windows:16,dealt", 16), ("windows:272,dealt", 272), ("windows:512,dealt", 512),
           ("windows:272,identity", 272), ("windows:320,identity", 320), ("windows:512,identity", 512)]


@pytest.mark.parametrize("name,m", WINDOWS)
def test_windows_case_reaches_every_step_and_request(name, m):
    mat = P.case(name)
    assert mat.m == m and mat.k == 509 and any(run.case_name == name for run in RUNS), name
    longest, lefts, sources, shapes, long_group = set(), set(), set(), set(), set()
    for _, a, b in pairs(mat):
        top = int(max(a.max(), b.max()))
        longest.add(top)
        schedule = P.window_schedule(a, b)
        assert [w[0] for w in schedule] == list(range(0, top, 16))       # every window visited was requested
        for w0, source, steps, left in schedule:
            sources.add((source, top))
            lefts.update(v for v in left if v > 0)
            assert all(s == min(4, max(0, (v + 3) // 4)) for s, v in zip(steps, left))
        if top >= 17:
            if a.max() == 0 or b.max() == 0:
                shapes.add("empty_long" if a.max() == 0 else "long_empty")
            for g in range(4):
                if max(a[g], b[g]) == top and sorted(np.concatenate((a, b)))[-2] < top:
                    long_group.add(g)
    # the pair whose longest row is L, for every designed L: the request rules see exactly L
    assert longest >= set(mat.claims["lengths"]) - {0}, (name, sorted(longest))
    assert mat.lengths[m - 1] == P.LAST_ROW == mat.lengths.max() and mat.row_offsets[m] == mat.nnz
    assert mat.lengths[0] > 0 and mat.row_offsets[0] == 0       # the first row at p0 = 0
    assert mat.column_indices[-1] == 508 and 0 in mat.rows[m - 1]
    if m == 16:
        assert 13 in lefts and ("loop", 65) in sources
        return
    # `left > 4 / 8 / 12`: both sides of every step, in some window of some lane group
    assert lefts >= {1, 4, 5, 8, 9, 12, 13, 15, 16}, sorted(lefts)
    # set-up request `16 < longest`: 16 no, 17 yes; the loop's `w0 + 32 < longest`: 32 / 33, 48 / 49, 64 / 65
    for no, yes, source in ((16, 17, "setup"), (32, 33, "loop"), (48, 49, "loop"), (64, 65, "loop")):
        assert no in longest and yes in longest
        count = lambda top: sum(1 for w in P.window_schedule([top, 0, 0, 0], [0] * 4) if w[1] == source)   # noqa: E731
        assert count(yes) == count(no) + 1, (no, yes)
    assert shapes == {"empty_long", "long_empty"}, shapes
    assert long_group >= {0, 3}, long_group        # `longest` is read from lanes 0 / 16 / 32 / 48
    live = (P.matrix_slot_rows(mat) >= 0).reshape(-1, P.WAVE_ROWS).all(axis=1)
    if name == "windows:272,identity":
        assert live.reshape(2, 16)[1].tolist() == [True] + [False] * 15     # one live wave, fifteen of padding
    if name == "windows:272,dealt":
        assert live.reshape(2, 16).sum(axis=1).tolist() == [8, 8]           # and a half-live ninth wave each
        assert (P.matrix_slot_rows(mat) >= 0).reshape(2, 256).sum(axis=1).tolist() == [136, 136]


def test_every_windows_case_is_run_on_both_placements():
    used = {run.case_name for run in RUNS}
    assert used >= {name for name, _ in WINDOWS}
    assert {P.case(name).m for name, _ in WINDOWS} >= {16, 272, 512}


ALL_K = P.K_ONE + P.K_TWO + P.K_MANY


@pytest.mark.parametrize("k", ALL_K)
def test_k_case_holds_both_sides_of_every_boundary(k):
    assert ALL_K == (1, 3, 4, 511, 512, 513, 516, 1023, 1024, 1025, 1537, 4096)
    mat = P.case(f"k:{k}")
    runs = [run for run in RUNS if run.case_name == f"k:{k}" and run.entry == "batched"]
    assert runs and mat.k == k and P.panels_of(k) == (k + 511) // 512
    assert {run.path() for run in runs} == {"one" if k <= 512 else "cut" if k <= 1024 else "walk"}
    want = P.boundary_columns(k)
    assert set(want) >= {0, k - 1} | {c for b in range(512, k, 512) for c in (b - 1, b)}
    assert set(want) <= set(mat.column_indices.tolist())
    for b in range(512, k, 512):        # side by side in one row
        assert any(((r[:-1] == b - 1) & (r[1:] == b)).any() for r in mat.rows if len(r) > 1), (k, b)
    assert k % 4 == 0 or k in (1, 3, 511, 513, 1023, 1025, 1537)       # k off a multiple of 4, and k = 1
    if 512 < k <= 1024:     # sorted rows on the cut path: the wave-level search finds every cut, nobody falls back
        cuts, rounds = P.model_cuts(mat)
        at = P.matrix_slot_rows(mat)
        assert all(cuts[s] == P.true_cut(mat.rows[r]) for s, r in enumerate(at) if r >= 0) and rounds <= 2
        assert not P.fallback_blocks(mat).any()


def test_every_path_meets_every_column_tile_edge():
    """n = 64 (one full tile), 68 (a last tile with one live lane group), 128, 132."""
    assert P.N_EDGES == (64, 68, 128, 132)
    reached = {(run.path(), run.n) for run in RUNS if run.entry in ("batched", "permuted")}
    assert reached >= set(itertools.product(("one", "cut", "walk"), P.N_EDGES)), sorted(reached)
    assert {run.case.m for run in RUNS if run.identity} >= {272, 320}       # a workgroup with 1 / 4 live waves


# ---------------------------------------------------------------------------
# the cut search
# ---------------------------------------------------------------------------
def fast_cut(length, cut):
    """search_cuts on one row of `length` entries whose first `cut` lie below the boundary."""
    lo, hi, rounds = 0, length, 0
    while hi - lo > 0:
        rounds += 1
        span = hi - lo
        if span <= 16:
            lo = hi = lo + sum(1 for i in range(16) if i < span and lo + i < cut)
        else:
            f = sum(1 for i in range(16) if lo + ((i * span) >> 4) < cut)
            new_lo = lo + (((f - 1) * span) >> 4) + 1 if f > 0 else lo
            new_hi = lo + ((f * span) >> 4) if f < 16 else hi
            lo, hi = new_lo, max(new_hi, new_lo)
    return min(max(lo, 0), length), rounds


SEARCH_LENGTHS = tuple(range(300)) + (511, 512, 513, 1000, 1023, 1024)


def test_search_model_equals_the_true_cut_exhaustively():
    """Every length 0 .. 299, 511 .. 513, 1000, 1023, 1024 and every cut position: the 16-ary
    search ends on the true cut, in at most 3 rounds (2 up to 256 entries)."""
    most = 0
    for length in SEARCH_LENGTHS:
        for cut in range(length + 1):
            got, rounds = fast_cut(length, cut)
            assert got == cut, (length, cut, got)
            assert rounds <= (1 if length <= 16 else 2 if length <= 256 else 3), (length, cut, rounds)
            most = max(most, rounds)
    assert most == 3


def test_fast_search_is_the_wave_model_on_single_rows():
    rng = np.random.default_rng(5)
    for length in (0, 1, 16, 17, 255, 256, 257, 600, 1024):
        for cut in {0, length, int(rng.integers(0, length + 1)), length // 2}:
            cols = np.where(np.arange(length) < cut, 0, 512)
            assert P.search_cut_row(cols) == fast_cut(length, cut) == (P.true_cut(cols), fast_cut(length, cut)[1])


CUT_NAMES = ("cuts:dealt", "cuts:identity", "partitioned:dealt")


@pytest.mark.parametrize("name", CUT_NAMES)
def test_cut_case_holds_its_pairs_and_the_search_finds_them(name):
    mat = P.case(name)
    assert mat.k == 1024 and any(run.case_name == name and run.path() == "cut" for run in RUNS)
    at = P.matrix_slot_rows(mat)
    cuts, most = P.model_cuts(mat)
    assert most == 3        # a third round: rows of 257 and more
    got = []
    for slot, row in enumerate(at):
        if row >= 0:
            cols = mat.rows[row]
            cut = int((cols < 512).sum())
            assert (cols[:cut] < 512).all() and (cols[cut:] >= 512).all(), (name, row, "not partitioned")
            assert cuts[slot] == cut == P.true_cut(cols), (name, slot, cuts[slot], cut)
            got.append((len(cols), cut))
    pairs_ = mat.claims["pairs"]
    assert got[:len(pairs_)] == pairs_
    have = set(pairs_)
    lengths = {length for length, _ in have}
    assert lengths >= {0, 1, 5, 16, 17, 255, 256, 257, 1024} and (1024, 512) in have
    for length in (5, 16, 17, 255, 256, 257):
        assert have >= {(length, 0), (length, 1), (length, length - 1), (length, length)}, length
    for length in (17, 255, 256, 257, 600, 1000):       # a cut on a probe position and one to either side
        on = [c for _, c in have if _ == length and c in P.probes(length)[1:]]
        assert any((length, c - 1) in have and (length, c + 1) in have for c in on), length
    adjacent = sum(1 for r in mat.rows if len(r) > 1 and ((r[:-1] == 511) & (r[1:] == 512)).any())
    assert adjacent >= 10 or name.startswith("partitioned")
    assert not P.fallback_blocks(mat).any()      # the cut holds: no fallback
    # rows of very different lengths in one wave: a bracket resolved in round 1 idles through round 3
    idle = False
    for s0, (_, p0, cnt) in waves(mat):
        _, rounds, history = P.search_cuts_wave(p0, cnt, mat.column_indices, mat.nnz - 1)
        if rounds == 3:
            lo, hi = history[0]
            idle = idle or bool(((hi - lo == 0) & (cnt > 0)).any())
    assert idle
    if name.startswith("partitioned"):
        assert (~mat.sorted_rows()).sum() >= 30      # unsorted, yet partitioned
    else:
        assert mat.sorted_rows().all()


def test_second_mask_of_the_cut_design_has_other_cuts():
    a, b = P.many_mask_cases("cuts")
    cut = lambda mat: [int((r < 512).sum()) for r in mat.rows]     # noqa: E731
    assert cut(a) != cut(b) and a.nnz == b.nnz and not P.fallback_blocks(b).any()


FALLBACKS = (("fallback:one", None, [True, False]), ("fallback:one,identity", None, [True, False]),
             ("fallback:descending", None, [True, True]))


@pytest.mark.parametrize("name,_,blocks", FALLBACKS)
def test_fallback_case_sends_the_named_workgroups_back(name, _, blocks):
    mat = P.case(name)
    assert any(run.case_name == name and run.path() == "cut" for run in RUNS), name
    assert P.fallback_blocks(mat).tolist() == blocks == list(mat.claims["blocks"])
    unsorted_rows = np.nonzero(~mat.sorted_rows())[0]
    if "one" in name:
        row = int(P.matrix_slot_rows(mat)[P.FALLBACK_SLOT])
        assert unsorted_rows.tolist() == [row] and mat.rows[row][:4].tolist() == [600, 3, 700, 5]
        assert mat.m == 512 and (mat.lengths > 0).all()      # sorted rows beside it, in its workgroup and the next
        if mat.placement == "dealt":    # under the second row order the row still sends one workgroup back
            assert P.fallback_blocks(mat, row_indices=mat.other_order()).sum() == 1
    else:
        assert len(unsorted_rows) >= 250 and all((np.diff(r) < 0).all() for r in mat.rows)


def test_the_never_cut_form_is_run_on_sorted_and_on_unsorted_rows():
    never = {run.case_name for run in RUNS if run.debug & P.DEBUG_NEVER_CUT}
    assert never >= {"cuts:dealt", "fallback:one"}
    for name in never:      # ... beside the same call on the cut path
        twin = [r for r in RUNS if r.case_name == name and r.entry == "batched"]
        assert len({(r.n, r.replicas, r.shared) for r in twin if r.case_name == "fallback:one"}) <= 1
        assert {r.path() for r in twin} == {"cut", "walk"}


# ---------------------------------------------------------------------------
# the masked walk
# ---------------------------------------------------------------------------
WALKS = ("walk:1537", "walk:4096", "k:1025", "k:1537", "k:4096", "fallback:one", "fallback:descending", "store:320,1025")


@pytest.mark.parametrize("name", WALKS)
def test_masked_walk_takes_every_entry_exactly_once(name):
    mat = P.case(name)
    for s0, (rows, p0, cnt) in waves(mat):
        log, taken = P.masked_walk_wave(p0, cnt, mat.column_indices, mat.k)
        for (t, g), entries in taken.items():
            assert sorted(entries) == list(range(int(cnt[t][g]))), (name, s0, t, g)
        for (p, t), (visited, start) in log.items():
            assert start % 16 == 0 and (p == 0 or not visited or visited[0] == log[(p - 1, t)][1])


@pytest.mark.parametrize("k", (1537, 4096))
def test_walk_case_reaches_the_start_skip_edges(k):
    mat = P.case(f"walk:{k}")
    passes = P.panels_of(k)
    assert passes == {1537: 4, 4096: 8}[k] and any(r.case_name == f"walk:{k}" for r in RUNS)
    rows, p0, cnt = P.wave_bounds(mat, 0)
    log, _ = P.masked_walk_wave(p0, cnt, mat.column_indices, k)
    panel = lambda cols: np.asarray(cols) // 512      # noqa: E731
    # quad 0: three ascending rows and one descending: the vote holds the quad's start at window 0
    quad = [mat.rows[r] for r in rows[0]]
    assert sum(bool((np.diff(r) > 0).all()) for r in quad) == 3 and sum(bool((np.diff(r) < 0).all()) for r in quad) == 1
    assert all(log[(p, 0)][1] == 0 for p in range(passes - 1))
    assert all(log[(p, 0)][0] == [0, 16, 32] for p in range(passes))
    # quad 1: ascending rows; the skip moves on, and a window straddles a boundary
    starts = [log[(p, 1)][1] for p in range(passes)]
    assert starts == sorted(starts) and starts[0] < starts[-2] < starts[-1] == 128 and len(set(starts)) >= 3
    straddle = [r for r in (mat.rows[x] for x in rows[1]) for w in range(0, len(r), 16)
                if len(set(panel(r[w:w + 16]).tolist())) > 1]
    assert straddle
    # quad 2: first window with an entry of the last panel, later windows panel 0 alone; a row
    # wholly in the last panel; an empty row; one entry at column k - 1
    mixed, last_panel, empty, single = (mat.rows[r] for r in rows[2])
    assert (panel(mixed[:16]) == passes - 1).any() and len(mixed) > 32 and (panel(mixed[16:]) == 0).all()
    assert len(last_panel) > 0 and (panel(last_panel) == passes - 1).all()
    assert len(empty) == 0 and single.tolist() == [k - 1]
    assert all(log[(p, 2)][1] == 0 for p in range(passes - 1))
    # quad 3: descending rows
    assert all((np.diff(mat.rows[r]) < 0).all() for r in rows[3])
    assert set(P.boundary_columns(k)) <= set(mat.column_indices.tolist())


# ---------------------------------------------------------------------------
# the transposing store, groups, many masks
# ---------------------------------------------------------------------------
def test_transposed_runs_reach_every_row_block():
    assert P.TRANSPOSED_SHAPES == ((256, 64), (320, 64), (384, 128), (256, 256), (512, 512), (512, 256), (320, 320))
    runs = [run for run in RUNS if run.entry == "transposed"]
    reached = {(run.case.m, run.block_rows) for run in runs}
    for shape in P.TRANSPOSED_SHAPES:
        assert (shape in reached) == P.block_rows_ok(*shape) == (shape not in P.TRANSPOSED_DECLINED), shape
    assert all(P.block_rows_ok(run.case.m, run.block_rows) for run in runs)
    assert {run.block_rows for run in runs} >= {64, 128, 256, 512}
    assert any(run.block_rows == run.case.m and run.case.m % 256 for run in runs)      # the whole C^T, a partial workgroup
    assert any(run.case.m % 256 and run.block_rows == 64 for run in runs)
    assert sum(run.n == 68 for run in runs) >= 3 and any(run.n % 64 == 0 for run in runs)
    assert any(run.bias and run.relu for run in runs) and any(run.bias and not run.relu for run in runs)
    assert {run.path() for run in runs} == {"one", "cut", "walk"}


def test_group_runs_reach_the_resident_panel_and_the_tile_behind_it():
    runs = [run for run in RUNS if run.entry == "group"]
    assert {run.label for run in runs} == set(P.GROUP_LABELS)
    for label in P.GROUP_LABELS:
        mine = [run for run in runs if run.label == label]
        assert {run.group["count"] for run in mine} >= ({1, 2, 4} if label != "group<1,0,1>" else {2, 4}), label
        assert {run.case.k for run in mine} >= ({512, 5} if label != "group<1,0,1>" else {512}), label
    # the same dense operand (the panel stays) and one per problem (copied again), on every store
    for accumulate, tout in ((False, True), (True, False), (False, False)):
        mine = [r for r in runs if r.group["accumulate"] == accumulate and bool(r.block_rows) == tout and r.group["count"] > 1]
        assert {r.group["same_dense"] for r in mine} == {True, False}, (accumulate, tout)
    # the full 128 KiB panel with the 64-row tile behind it
    assert any(run.case.k == 512 and run.block_rows and run.group["count"] == 4 for run in runs)
    for run in runs:
        counts = [mat.nnz for mat in run.matrices()]
        assert len(counts) == run.group["count"] and len(set(counts)) == len(counts) and min(counts) > 0, run.id
        assert all(mat.m == run.case.m and mat.k == run.case.k <= 512 for mat in run.matrices())
        assert not run.block_rows or P.block_rows_ok(run.case.m, run.block_rows)
        assert run.identity == (run.label != "group<0,0,0>")
    assert any(run.case_name == "windows:272,identity" and run.group["accumulate"] for run in runs)


def test_many_mask_runs():
    runs = {run.masks: run for run in RUNS if run.entry == "many"}
    three, cuts = runs["three"], runs["cuts"]
    assert (len(three.matrices()), three.heads, three.replicas) == (3, 2, 6)
    assert (len(cuts.matrices()), cuts.heads, cuts.replicas) == (2, 4, 8)       # 8 replicas: dealt over the XCDs
    assert three.matrices()[-1].nnz == 0 and three.matrices()[0].nnz != three.matrices()[1].nnz
    assert cuts.case.k == 1024 and three.case.k <= 512
    assert three.label == "panel<0,0,0>" and cuts.label == "panel<1,0,0>"


# ---------------------------------------------------------------------------
# the run list
# ---------------------------------------------------------------------------
def test_runs_reach_all_24_instances():
    assert len(P.LABELS) == len(set(P.LABELS)) == 24
    by_label = {}
    for run in RUNS:
        by_label.setdefault(run.label, []).append(run)
    assert set(by_label) == set(P.LABELS), set(P.LABELS) ^ set(by_label)
    assert len({run.id for run in RUNS}) == len(RUNS)


@pytest.mark.parametrize("label", P.PANEL_LABELS)
def test_panel_instance_runs(label):
    mine = [run for run in RUNS if run.label == label]
    multi, perm, tout = (c == "1" for c in label[6:11:2])
    entries = {run.entry for run in mine}
    assert entries >= {(False, False): {"batched"}, (True, False): {"permuted"}}.get((perm, tout), {"transposed"})
    if label in ("panel<0,0,0>", "panel<1,0,0>"):
        assert "many" in entries
    assert {run.replicas for run in mine if run.entry != "many"} >= ({1, 3} if tout or perm else {1, 3, 8})
    if multi:       # the cut path and the masked walk; three panels through the C entries at k = 1025
        assert {run.path() for run in mine} == {"cut", "walk"}, label
        if perm or tout:
            assert any(run.case.k == 1025 for run in mine), label
    assert all(run.knobs()["SPUTNIK_HIP_SPMM_KERNEL"] == "panel" for run in mine)


def test_replicas_and_strides():
    plain = [run for run in RUNS if run.entry not in ("typed", "many")]
    assert {run.replicas for run in plain} == {1, 3, 8}
    assert {run.shared for run in plain if run.entry != "group"} == {True, False}      # values stride 0 and nnz
    for entry in ("batched", "permuted", "transposed", "group"):
        assert 8 in {run.replicas for run in plain if run.entry == entry}, entry     # a launch total divisible by 8


@pytest.mark.parametrize("label", P.TYPED_LABELS)
def test_typed_instance_runs_stay_on_the_panel_route(label):
    mine = [run for run in RUNS if run.label == label]
    assert mine, label
    for run in mine:
        mat = run.case
        assert mat.nnz * run.n * run.replicas >= P.TYPED_MIN_WORK, (run.id, mat.nnz * run.n * run.replicas)
        assert run.types in P.TYPE_PAIRS and not (run.shared and run.types[1] != P.F32)
        assert run.path() == ("walk" if run.multi else "one")
    if label.startswith("typed<1"):
        assert any(not P.case(run.case_name).sorted_rows().all() for run in mine)


def test_off_route_shapes():
    assert set(P.OFF_ROUTE) == {"m12", "n60", "n66", "k4097", "dense_unaligned"}
    assert P.OFF_ROUTE["m12"][0] == 12 and P.OFF_ROUTE["n60"][2] == 60 and P.OFF_ROUTE["n66"][2] == 66
    assert P.OFF_ROUTE["k4097"][1] == 4097 and P.OFF_ROUTE["dense_unaligned"][3] % 4 != 0
    for name in P.OFF_ROUTE:
        assert P.off_route_case(name).nnz > 0


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def test_reference_and_layouts_against_plain_loops():
    mat = P.case("fallback:descending")
    values, dense, _ = P.operands(mat, 8, 2, shared=False, integers=True)
    want = np.zeros((2, mat.m, 8))
    for r in range(2):
        for row in range(mat.m):
            for p in range(mat.row_offsets[row], mat.row_offsets[row + 1]):
                want[r, row] += float(values[r, p]) * dense[r, mat.column_indices[p]].astype(np.float64)
    got = P.reference(mat, values, dense)
    assert np.array_equal(got, want) and np.abs(values).min() >= 1 and np.abs(values).max() <= 2 and np.abs(dense).max() <= 3
    hd = 16
    flat = P.transposed_layout(got, hd).reshape(2, -1)
    for row, col in ((0, 0), (17, 3), (271, 7), (100, 5)):
        assert flat[1, (row // hd) * 8 * hd + col * hd + row % hd] == got[1, row, col]
    shared = P.operands(mat, 8, 3, shared=True)[0]
    assert shared.shape == (1, mat.nnz) and np.array_equal(np.sort(P.permutation(mat)), np.arange(mat.nnz))
