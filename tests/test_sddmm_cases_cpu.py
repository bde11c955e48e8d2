"""CPU: the cases of tests/sddmm_cases.py reach the edges they are named for (recounted from the
CSR arrays), the plan model agrees with an independent recount, the reference with the oracle,
and the run list of tests/test_gpu_sddmm_instances.py reaches what it means to reach: every run
is asked of the host-only launch query (capi.sddmm_launch_shape) under its knobs, and together
the runs reach all 35 instances of launch_typed, each with a walked grid, a count above 32, an
unsorted row and a partial last slab.  No GPU."""
import collections

import numpy as np
import pytest
import torch

import sddmm_cases as S
from oracle import sputnik_oracle as O
from torch_sputnik_amd import capi

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EDGE_CASES = tuple(S.EDGE_SHAPES)
ALL = [(name, rows) for name in S.CASE_NAMES for rows in S.SLAB_HEIGHTS]


@pytest.fixture
def knobs(monkeypatch):
    """Sets SPUTNIK_HIP_* for one query; the library looks again, and once more afterwards."""
    def set_knobs(env):
        for name in ("SPUTNIK_HIP_SDDMM_KERNEL", "SPUTNIK_HIP_SDDMM_FLAT", "SPUTNIK_HIP_SDDMM_DEBUG",
                     "SPUTNIK_HIP_SDDMM_SLAB", "SPUTNIK_HIP_SDDMM_PANEL"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        capi.reload_options()
    yield set_knobs
    monkeypatch.undo()
    capi.reload_options()


def row_share(case, row, rows):
    """[slabs] lists of the positions of `row`'s entries per slab, in storage order."""
    a, b = int(case.row_offsets[row]), int(case.row_offsets[row + 1])
    shares = [[] for _ in range(S.ceil_div(case.n, rows))]
    for p in range(a, b):
        shares[int(case.column_indices[p]) // rows].append(p)
    return shares


@pytest.mark.parametrize("name,rows", ALL)
def test_case_is_a_valid_served_mask(name, rows):
    c = S.case(name, rows)
    ri, ro, ci = c.csr
    assert np.array_equal(np.sort(ri), np.arange(c.m)), name
    assert ro[0] == 0 and ro[-1] == c.nnz and (np.diff(ro) >= 0).all(), name
    assert ci.min() >= 0 and ci.max() < c.n, name
    # what the tiled route asks of a shape (sddmm_tiled_applicable)
    assert c.m >= 16 and c.n >= 16 and c.nnz >= 4 * c.m, (name, c.m, c.n, c.nnz)
    assert c.m <= 1283 and c.n <= 600
    for row in range(c.m):      # columns distinct inside a row; ascending unless named unsorted
        cols = ci[ro[row]:ro[row + 1]]
        assert len(set(cols.tolist())) == len(cols), (name, row)
        if row not in c.unsorted_rows:
            assert (np.diff(cols) > 0).all(), (name, row)


@pytest.mark.parametrize("rows", S.SLAB_HEIGHTS)
@pytest.mark.parametrize("name", EDGE_CASES)
def test_counts_per_row_and_slab(name, rows):
    """Every count of COUNTS in slab 0 and in the last slab (clipped to its width, which at
    n = 313 holds 49), in block 0 and in the last block, as the specification says."""
    c = S.case(name, rows)
    counts, slabs = c.counts(rows), S.ceil_div(c.n, rows)
    width = [min(rows, c.n - s * rows) for s in range(slabs)]
    want = lambda v, s: width[s] if v == S.SLAB else min(v, width[s])   # noqa: E731
    block = c.block_of_row()
    seen = collections.defaultdict(set)     # (block, slab) -> counts there
    for row, (first, last) in c.spec.items():
        assert counts[row, 0] == want(first, 0), (name, rows, row, first)
        if slabs > 1:
            assert counts[row, slabs - 1] == want(last, slabs - 1), (name, rows, row, last)
            assert counts[row, 1:slabs - 1].sum() == 0, (name, rows, row)   # (empty slabs between)
        seen[int(block[row]), 0].add(first)
        seen[int(block[row]), slabs - 1].add(last)
    if c.order != "by_length":      # (by_length re-deals the rows: the counts stay, the blocks do not)
        for b in {0, c.row_blocks - 1}:
            assert set(S.COUNTS) <= seen[b, 0], (name, rows, b)
            assert set(S.COUNTS) <= seen[b, slabs - 1], (name, rows, b)
    if c.n == S.N_EDGES:            # a partial last slab that holds 49 entries of one row
        assert 49 <= width[-1] < rows and (counts[:, -1] == 49).any() and (counts[:, -1] == width[-1]).any()
        assert (counts[:, 0] == rows).any()
    # a row whose entries lie only in the last slab, with empty slabs before it
    if slabs > 1:
        some = min(width[-1], 33)   # (n = slab height + 1: the last slab is one column)
        assert ((counts[:, :-1].sum(axis=1) == 0) & (counts[:, -1] >= some)).any(), (name, rows)
    assert ci_has_last_column(c), (name, rows)


def ci_has_last_column(c):
    return bool((c.column_indices == c.n - 1).any())


@pytest.mark.parametrize("rows", S.SLAB_HEIGHTS)
@pytest.mark.parametrize("name", [n for n in EDGE_CASES if "by_length" not in n])
def test_longest_sets(name, rows):
    """Four rows behind one `longest` (the maximum over lanes 0, 16, 32, 48): a count above 32
    beside a short one, beside a row with entries in another slab only and beside one with none;
    around the last slab too; the long row as the fourth of its set; in block 0 and in the last."""
    c = S.case(name, rows)
    counts, slabs = c.counts(rows), S.ceil_div(c.n, rows)
    sets = S.wave_sets(c.row_indices, c.m)
    blocks_of_sets = np.arange(len(sets)) * 4 // S.PER
    found = collections.defaultdict(set)
    for four, b in zip(sets, blocks_of_sets):
        if (four < 0).any():
            continue
        for slab in {0, slabs - 1}:
            here = counts[four, slab]
            total = counts[four].sum(axis=1)
            elsewhere = ((here == 0) & (total > 0)).any() or slabs == 1    # (one slab: no elsewhere)
            if here.max() > 32 and ((here >= 1) & (here <= 4)).any() and elsewhere and (total == 0).any():
                found[int(b)].add(("mixed", slab))
            if here[3] > 32 and here[:3].max() <= 2:
                found[int(b)].add(("fourth", slab))
    for b in {0, c.row_blocks - 1}:
        assert ("mixed", 0) in found[b] and ("fourth", 0) in found[b], (name, rows, b, found[b])
        if slabs > 1 and min(rows, c.n - (slabs - 1) * rows) > 32:
            assert ("mixed", slabs - 1) in found[b], (name, rows, b, found[b])


@pytest.mark.parametrize("rows", S.SLAB_HEIGHTS)
def test_last_entry_of_column_indices(rows):
    """The global last entry belongs to a row of 1, of 2 and of 33 entries; its position inside
    the row's share of its slab is even (1, 33) and odd (2); and a last row without entries."""
    seen = {}
    for name in EDGE_CASES:
        c = S.case(name, rows)
        last_row = int(np.nonzero(np.diff(c.row_offsets) > 0)[0][-1])
        length = int(c.row_offsets[last_row + 1] - c.row_offsets[last_row])
        share = [s for s in row_share(c, last_row, rows) if s][-1]
        assert share[-1] == c.nnz - 1
        seen[name] = (length, (len(share) - 1) % 2)
        if c.last == "last_empty":
            assert last_row < c.m - 1 and c.row_offsets[c.m - 1] == c.nnz, name
        elif c.n - (S.ceil_div(c.n, rows) - 1) * rows >= S.LAST_ROWS[c.last]:
            assert last_row == c.m - 1 and length == S.LAST_ROWS[c.last], (name, length)
    assert {(1, 0), (2, 1), (33, 0)} <= set(seen.values()), seen


@pytest.mark.parametrize("rows", S.SLAB_HEIGHTS)
def test_shape_edges(rows):
    """n = slab height, one less, one more; one, three, four and six row blocks with padding
    slots in every block; the three row orders; m = n = 16 dense."""
    shapes = {name: (S.case(name, rows).m, S.case(name, rows).n) for name in S.CASE_NAMES}
    assert {n for _, n in shapes.values()} >= {rows - 1, rows, rows + 1, S.N_EDGES, 16}
    assert {S.ceil_div(m, S.PER) for m, _ in shapes.values()} >= {1, 3, 4, 6}
    assert {S.case(name, rows).order for name in EDGE_CASES} == {"identity", "by_length", "permuted"}
    for name in S.WALKED_EDGE_CASES + S.STRUCTURED_CASES:
        c = S.case(name, rows)
        padding = (S.slot_rows(c.row_indices, c.m).reshape(-1, S.PER) < 0).sum(axis=1)
        assert c.row_blocks >= 3 and (padding > 0).all(), (name, padding)   # dealt over all blocks
    d = S.case("dense_16x16", rows)
    assert d.nnz == 256 and (d.counts(rows)[:, 0] == 16).all()


@pytest.mark.parametrize("rows", S.SLAB_HEIGHTS)
@pytest.mark.parametrize("name", EDGE_CASES)
def test_unsorted_rows_sit_where_a_walk_reaches_them_second(name, rows):
    """Rows that are not ok (reversed, or one pair swapped) in block 0 and -- three of them -- in
    the LAST block, which a workgroup of every walked grid (grid y < blocks) takes after another."""
    c = S.case(name, rows)
    row_ok, _, _ = S.plan_model(*c.csr, c.m, c.n, rows)
    srows = S.slot_rows(c.row_indices, c.m)
    bad = sorted(int(r) for r in srows[row_ok == 0])
    assert bad == sorted(c.unsorted_rows) and len(bad) == 4, (name, bad, c.unsorted_rows)
    blocks = np.nonzero(row_ok == 0)[0] // S.PER
    if c.order != "by_length":
        assert sorted(blocks.tolist()) == sorted([0] + [c.row_blocks - 1] * 3), (name, blocks)
    if name in S.WALKED_Y:
        y = S.WALKED_Y[name]
        assert y < c.row_blocks and c.row_blocks % y != 0
        later = [b for b in blocks if b >= y]      # blocks some workgroup walks after its first
        assert later, (name, blocks, y)


@pytest.mark.parametrize("name,rows", ALL)
def test_plan_model_against_a_recount(name, rows):
    """Independent of plan_model's walk: for an ok row, word c is the row's start plus the number
    of its columns below c * rows (searchsorted); padding slots hold zeros."""
    c = S.case(name, rows)
    row_ok, table, defined = S.plan_model(*c.csr, c.m, c.n, rows)
    slots, slabs = S.slots_of(c.m), S.ceil_div(c.n, rows)
    table, defined = table.reshape(slabs + 1, slots), defined.reshape(slabs + 1, slots)
    entry = S.dealt_index(np.arange(slots), slots)
    assert sorted(entry.tolist()) == list(range(slots))
    for slot in range(slots):
        if entry[slot] >= c.m:
            assert row_ok[slot] == 1 and not table[:, slot].any() and defined[:, slot].all()
            continue
        row = int(c.row_indices[entry[slot]])
        a, b = int(c.row_offsets[row]), int(c.row_offsets[row + 1])
        cols = c.column_indices[a:b]
        assert bool(row_ok[slot]) == bool((np.diff(cols) > 0).all()) == (row not in c.unsorted_rows)
        if row_ok[slot]:
            want = a + np.searchsorted(cols, np.arange(slabs + 1) * rows)
            assert np.array_equal(table[:, slot], want) and defined[:, slot].all(), (name, slot)
            assert np.array_equal(np.diff(want), c.counts(rows)[row])
        else:
            assert not defined[:, slot].any()
    words, wdefined = S.workspace_model(*c.csr, c.m, c.n, rows)
    assert len(words) == slots + (slabs + 1) * slots and wdefined[:slots].all()   # (slots % 64 == 0)


@pytest.mark.parametrize("name,rows", [(name, rows) for name, rows in ALL if rows in (256, 80)])
def test_reference_against_the_oracle(name, rows):
    c = S.case(name, rows)
    rng = np.random.default_rng(5)
    lhs = rng.uniform(-1, 1, (2, c.m, 8)).astype(np.float32)
    rhs = rng.uniform(-1, 1, (2, c.n, 8)).astype(np.float32)
    got = S.reference(c.row_offsets, c.column_indices, lhs, rhs)
    want = np.asarray(O.sddmm(c.m, c.n, *c.csr, lhs, rhs), np.float64)
    assert got.shape == want.shape == (2, c.nnz)
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(S.reference(c.row_offsets, c.column_indices, lhs, rhs, summed=True) - want.sum(axis=0)).max() < 1e-12


# ---------------------------------------------------------------------------
# the run list
# ---------------------------------------------------------------------------
def query(run, walked, planned=False):
    c, config = run.case, run.config
    return capi.sddmm_launch_shape(c.m, config.k, c.n, c.nnz, run.replicas, DTYPES[config.in_type],
                                   DTYPES[config.out_type], planned=planned, summed=config.summed)


def expected_shape(run, walked):
    return run.launch_shape(walked)


@pytest.mark.parametrize("run", S.runs(), ids=lambda run: run.id)
def test_run_reaches_its_instance_and_grid(run, knobs):
    """Family, panel width, slab rows, passes and grid of every run, under the run's knobs, with
    and without the walk knob, planned and not; a walked run spreads fewer workgroups over y than
    there are row blocks, on the grid y the list states."""
    c = run.case
    for walked in (False, True) if run.walked_y else (False,):
        knobs(run.config.knobs(walked))
        for planned in (False, True):
            assert query(run, walked, planned) == expected_shape(run, walked), (run.id, walked, planned)
    if run.walked_y:
        assert expected_shape(run, True)["grid_y"] == run.walked_y < c.row_blocks
        assert expected_shape(run, False)["grid_y"] == c.row_blocks
    assert S.largest_operand_bytes(run) <= 64 << 20, run.id


def test_run_list_reaches_all_35_instances_at_their_edges():
    instances = S.instances()
    assert len(instances) == len(set(instances)) == 35
    reached = collections.defaultdict(set)
    bodies = collections.defaultdict(set)
    for run in S.runs():
        c, config = run.case, run.config
        counts = c.counts(config.rows)
        slabs = config.slabs(c.n)
        facts = set()
        if run.walked_y and c.row_blocks % run.walked_y != 0 and c.row_blocks >= run.walked_y + 1:
            facts.add("walked")     # (grid y no divisor of the blocks: workgroup 0 walks two or more)
        if (counts > S.PREFETCHED).any():
            facts.add("above_32")
        if c.unsorted_rows:
            facts.add("unsorted")
        if c.n % config.rows != 0 and slabs > 1:
            facts.add("partial_last_slab")
        if run.walked_y and c.unsorted_rows:
            row_ok, _, _ = S.plan_model(*c.csr, c.m, c.n, config.rows)
            if (np.nonzero(row_ok == 0)[0] // S.PER >= run.walked_y).any():
                facts.add("unsorted_in_a_later_block")
        for inst in config.instances:
            assert inst in instances, inst
            reached[inst] |= facts
        body = (config.family, "float32" if config.in_type == "float32" else "half")
        if run.walked_y:
            bodies[body].add(run.walked_y)
    for inst in instances:
        assert reached[inst] >= {"walked", "above_32", "unsorted", "partial_last_slab",
                                 "unsorted_in_a_later_block"}, (inst, reached[inst])
    for body in (("stationary", "float32"), ("quad", "float32"), ("quad", "half")):
        assert {1, 2} <= bodies[body], (body, bodies[body])


def test_walk_knob_leaves_a_many_mask_launch_on_all_row_blocks(knobs):
    """kMasksLargestFirst: a launch that holds ALL replicas of several masks keeps grid y at the
    number of row blocks whatever the knob says (its order is that of the grid); the same shape
    as ONE mask of as many heads walks."""
    m, k, n, nnz = 523, 64, 300, 523 * 20
    knobs(dict(S.BASE_KNOBS, SPUTNIK_HIP_SDDMM_DEBUG=str(S.WALK)))
    one = capi.sddmm_launch_shape(m, k, n, nnz, 60, mask_heads=60)
    many = capi.sddmm_launch_shape(m, k, n, nnz, 60, mask_heads=2)
    plain = capi.sddmm_launch_shape(m, k, n, nnz, 60)
    assert one["row_blocks"] == many["row_blocks"] == 3 and one["grid_z"] == many["grid_z"] == 60
    assert one["grid_y"] == plain["grid_y"] == 1        # 2 slabs x 60 replicas >= 100 workgroups
    assert many["grid_y"] == 3
    # the GPU file's batch: heads = 2, replicas = 6
    assert capi.sddmm_launch_shape(m, k, n, nnz, 6, mask_heads=2)["grid_y"] == 3


def test_query_refuses_what_no_entry_point_accepts():
    with pytest.raises(RuntimeError):
        capi.sddmm_launch_shape(0, 64, 64, 10, 1)
    with pytest.raises(RuntimeError):   # float32 operands, half output
        capi.sddmm_launch_shape(64, 64, 64, 1024, 1, torch.float32, torch.float16)
    with pytest.raises(RuntimeError):   # the summed form's output is float32
        capi.sddmm_launch_shape(64, 64, 64, 1024, 1, torch.float16, torch.float16, summed=True)
    with pytest.raises(RuntimeError):   # replicas no multiple of the heads
        capi.sddmm_launch_shape(64, 64, 64, 1024, 3, mask_heads=2)
    assert capi.sddmm_launch_shape(72, 72, 72, 500, 1)["family"] == "rowwave"


# ---------------------------------------------------------------------------
# the pair-flat kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", (1, 2))
def test_flat_case_fills_every_tile_to_its_step_count(geometry):
    """Steps of every (row block, slab) tile, counted from the CSR arrays as the plan's count
    kernel pairs the entries (CSR neighbours inside one slab, the rest alone): 0, 1, fewer than
    the compute waves, kCap - 1, kCap, kCap + 1, 2 kCap + 1; odd runs give singles; one tile
    holds column n - 1 and nothing else."""
    g = S.FLAT_GEOMETRIES[geometry]
    c = S.flat_case(geometry)
    assert (c.m, c.n) == S.FLAT_SHAPE and c.nnz >= 4 * c.m and c.m >= 128 and c.n >= 128
    steps = S.flat_steps(c, geometry)
    descriptors, singles = S.flat_descriptors(c, geometry)
    targets = S.flat_tile_targets(geometry)
    cap, waves = g["cap"], g["compute_waves"]
    assert (cap, waves) == ((112, 15) if geometry == 1 else (56, 7))
    for b, row in enumerate(targets):
        for s, target in enumerate(row):
            if target == S.FLAT_CORNER:
                assert descriptors[b, s] == singles[b, s] == 1 and steps[b, s] == 1
                lo = s * g["slab"]
                rows = np.repeat(np.arange(c.m), np.diff(c.row_offsets))
                here = (c.column_indices >= lo) & (c.block_of_row_for(g["block"])[rows] == b)
                assert c.column_indices[here].tolist() == [c.n - 1]
            else:
                assert steps[b, s] == target, (geometry, b, s, steps[b, s], target)
                assert target == 0 or singles[b, s] > 0     # rows with an odd number of entries there
    reached = set(steps.reshape(-1).tolist())
    assert {0, 1, waves - 1, cap - 1, cap, cap + 1, 2 * cap + 1} <= reached
    assert 1 < waves - 1 < waves
    assert sorted(c.unsorted_rows) == [5, 6]


@pytest.mark.parametrize("run", S.flat_runs(), ids=lambda run: run.id)
def test_flat_run_reaches_the_pair_flat_kernel(run, knobs):
    """Planned: the pair-flat kernel; the same call unplanned plans the tables alone and takes
    the quad kernel; with the knob at 0 the planned call takes the quad kernel too."""
    c, config = run.case, run.config
    knobs(config.knobs(False))
    assert query(run, False, planned=True) == run.launch_shape(False)
    assert query(run, False, planned=False)["family"] == "quad"
    knobs(dict(config.knobs(False), SPUTNIK_HIP_SDDMM_FLAT="0"))
    assert query(run, False, planned=True)["family"] == "quad"
    assert len(S.flat_runs()) == 10
    assert {(r.config.flat, r.config.in_type, r.config.k) for r in S.flat_runs()} == {
        (f, t, k) for f in (1, 2) for t, k in (("float32", 64), ("float16", 64), ("float16", 128),
                                               ("bfloat16", 64), ("bfloat16", 128))}
