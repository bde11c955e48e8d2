"""CPU: the matrices of tests/spmm_cases.py reach the edges they are named for -- every edge is
RECOUNTED here from the CSR arrays and the row order alone, through the dealt_index model, for the
tile of the run that claims it -- the plan model agrees with an independent recount, the
reference with the oracle, and the run list of tests/test_gpu_spmm_instances.py reaches what it
means to reach: every run is asked of the host-only launch query (capi.spmm_launch_shape) under
its knobs, and together the runs reach all eight instances of spmm_tiled_kernel, the 64-column
kernel unsplit and split, and each (instance, applicable edge) pair.  No GPU."""
import collections
import functools

import numpy as np
import pytest

import sddmm_cases as S
import spmm_cases as C
from oracle import sputnik_oracle as O
from torch_sputnik_amd import capi

KNOB_NAMES = ("SPUTNIK_HIP_SPMM_KERNEL", "SPUTNIK_HIP_SPMM_SPARSE", "SPUTNIK_HIP_SPMM_MEDIUM",
              "SPUTNIK_HIP_SPMM_DEBUG")
RUNS = C.runs()
CASES = sorted({(run.case_name, run.bk) for run in RUNS})


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
@pytest.mark.parametrize("name,bk", CASES)
def test_case_is_a_valid_served_matrix(name, bk):
    c = C.case(name, bk)
    ri, ro, ci = c.csr
    assert np.array_equal(np.sort(ri), np.arange(c.m)), name
    assert np.array_equal(np.sort(c.other_order()), np.arange(c.m)) and not np.array_equal(c.other_order(), ri)
    assert ro[0] == 0 and ro[-1] == c.nnz and (np.diff(ro) >= 0).all(), name
    assert ci.min() >= 0 and ci.max() < c.k, name
    # what the routes ask of a shape whatever the knob (tiled_applicable, tiled512_applicable,
    # spmm_tiled64_applicable)
    assert c.nnz >= C.MIN_MEAN[bk] * c.m and c.m >= 64 and c.k >= bk, (name, c.m, c.k, c.nnz)
    assert c.m <= 1300 and c.k <= 600
    for row in range(c.m):      # columns distinct inside a row; ascending unless named unsorted
        cols = ci[ro[row]:ro[row + 1]]
        assert len(set(cols.tolist())) == len(cols), (name, row)
        if row not in c.unsorted_rows:
            assert (np.diff(cols) > 0).all(), (name, row)
    assert name.startswith("structured_") or (ci == c.k - 1).any(), (name, "column k - 1")


@pytest.mark.parametrize("name,bk", [cb for cb in CASES if not cb[0].startswith("structured_")])
def test_designed_rows_hold_their_counts(name, bk):
    """Every designed row holds, chunk by chunk, the count it was specified with (clipped to the
    chunk's width); rows of the last chunk alone hold column k - 1."""
    c = C.case(name, bk)
    counts = C.chunk_counts(c.row_offsets, c.column_indices, c.k, bk)
    nchunks = counts.shape[1]
    width = [min(bk, c.k - ch * bk) for ch in range(nchunks)]
    assert len(c.spec) >= len(C.COUNTS[bk])
    for row, spec in c.spec.items():
        if spec[0] == C.ONLY_LAST:
            assert counts[row, :-1].sum() == 0 and counts[row, -1] == min(spec[1], width[-1]), (name, row)
            assert c.column_indices[c.row_offsets[row + 1] - 1] == c.k - 1, (name, row)
        else:
            assert counts[row].tolist() == [min(v, w) for v, w in zip(spec, width)], (name, row, spec)
    if c.last is not None:
        assert counts[c.m - 1].tolist() == [0] * (nchunks - 1) + [min(c.last, width[-1])], name


@pytest.mark.parametrize("name,bk", CASES)
@pytest.mark.parametrize("other", (False, True))
def test_plan_model_against_a_recount(name, bk, other):
    """row_ok and the chunk table of the model against searchsorted on every ok row; the words
    of rows that are not ok are undefined; padding slots are ok and hold zeros."""
    c = C.case(name, bk)
    per = 128 if bk == 128 else 256
    ri = c.other_order() if other else c.row_indices
    words, defined = C.plan_words(name, bk, other)
    rows = S.slot_rows(ri, c.m, per)
    slots, nchunks = len(rows), C.ceil_div(c.k, bk)
    first = S.row_ok_ints(slots)
    assert first * 4 % 256 == 0 and len(words) == first + (nchunks + 1) * slots
    table = words[first:].reshape(nchunks + 1, slots)
    table_defined = defined[first:].reshape(nchunks + 1, slots)
    assert defined[:slots].all() and not defined[slots:first].any()
    for slot, row in enumerate(rows):
        if row < 0:
            assert words[slot] == 1 and not table[:, slot].any() and table_defined[:, slot].all()
            continue
        p0, p1 = int(c.row_offsets[row]), int(c.row_offsets[row + 1])
        cols = c.column_indices[p0:p1]
        ok = bool((np.diff(cols) > 0).all())
        assert words[slot] == int(ok) and ok == (row not in c.unsorted_rows), (name, slot, row)
        if ok:
            want = p0 + np.searchsorted(cols, np.arange(nchunks + 1) * bk, side="left")
            assert np.array_equal(table[:, slot], want) and table_defined[:, slot].all(), (name, slot)
            assert table[0, slot] == p0 and table[nchunks, slot] == p1
        else:
            assert not table_defined[:, slot].any()


def test_reference_against_the_oracle():
    for name, bk, n, shared in (("pad_203_identity", 64, 196, True), ("edges_523_permuted_last2", 128, 72, False),
                                ("structured_band", 32, 388, False)):
        c = C.case(name, bk)
        rng = np.random.default_rng(5)
        values = rng.uniform(-1, 1, (1 if shared else 2, c.nnz)).astype(np.float32)
        dense = rng.uniform(-1, 1, (2, c.k, n)).astype(np.float32)
        got = C.reference(c.row_offsets, c.column_indices, values, dense)
        for r in range(2):
            want = O.spmm(c.m, c.k, values[0 if shared else r], c.row_indices, c.row_offsets, c.column_indices, dense[r])
            assert np.abs(got[r] - want).max() < 1e-4, (name, r)


# ---------------------------------------------------------------------------
# the edges a run reaches, recounted
# ---------------------------------------------------------------------------
def chunk_place(ch, nchunks):
    return {"first"} if ch == 0 and nchunks > 1 else {"first", "last"} if nchunks == 1 else \
        {"last"} if ch == nchunks - 1 else {"middle"}


@functools.lru_cache(maxsize=None)
def edges_of(run_index):
    """The set of edge labels that run RUNS[run_index] puts in front of its kernel instance."""
    run = RUNS[run_index]
    c, t = run.case, run.tile
    counts = C.slot_counts(c, t.chunk, t.per)           # [slots, nchunks]; -1: padding
    slots, nchunks = counts.shape
    ok = run.blocks_ok()                                # per row block of the tile
    staged = np.repeat(ok, t.rows)
    real = counts[:, 0] >= 0
    n_tiles = C.ceil_div(run.n, t.cols)
    out = set()
    # entries of a row in one chunk, on the staged path
    for ch in range(nchunks):
        for v in np.unique(counts[staged & real, ch]):
            out |= {("count", int(v), place) for place in chunk_place(ch, nchunks)}
    out.add(("last_chunk_width", c.k - (nchunks - 1) * t.chunk))
    out.add(("chunks", nchunks))
    # a row of the last chunk alone, behind empty chunks, holding column k - 1
    if nchunks > 1:
        for slot in np.nonzero(staged & real & (counts[:, :-1].sum(axis=1) == 0) & (counts[:, -1] > 0))[0]:
            row = S.slot_rows(c.row_indices, c.m, t.per)[slot]
            if c.column_indices[c.row_offsets[row + 1] - 1] == c.k - 1:
                out.add(("only_last_chunk",))
    # the end of the arrays
    lengths = np.diff(c.row_offsets.astype(np.int64))
    holder = int(np.nonzero(lengths)[0][-1])             # the row of the last entry of column_indices
    holder_slot = int(np.nonzero(S.slot_rows(c.row_indices, c.m, t.per) == holder)[0][0])
    if staged[holder_slot]:
        out.add(("last_entry_in_a_row_of", int(lengths[holder])))
    if lengths[c.m - 1] == 0:
        out.add(("empty_last_row",))
    # rows, slots, blocks
    per_block = real.reshape(-1, t.rows).sum(axis=1)
    if (~real).any():
        out.add(("padding_slots",))
    if (per_block == 1).any():
        out.add(("block_with_one_real_row",))
    if (per_block == 0).any():
        out.add(("block_of_padding",))
    out.add(("runs_of_slots", min(slots // t.per, 3)))
    if not ok.all():
        if ok.any():        # (rows by length deal the unsorted rows anywhere: the largest tile may gather it all)
            out.add(("gather_block_beside_staged",))
        if not ok[np.nonzero(per_block)[0][-1]]:
            out.add(("last_block_gathered",))
        if run.n % t.cols:
            out.add(("gather_block_partial_tile",))
        reversed_or_swapped = len(c.unsorted_rows)
        assert reversed_or_swapped >= 2
    # columns
    if t.name == "narrow":
        out.add(("n", run.n))
    else:
        last_width = run.n - (n_tiles - 1) * t.cols
        out.add(("n_tiles", "eight" if n_tiles % 8 == 0 else n_tiles))
        out.add(("last_tile", "full" if last_width == t.cols else "piece1_partial" if last_width > 256 else "partial"))
        if n_tiles % 8:
            out.add(("grid_divides_by_8", (slots // t.rows * n_tiles * run.replicas) % 8 == 0))
    out.add(("replicas", min(run.replicas, 4)))
    out.add(("values", "shared" if run.shared else "per_replica"))
    if run.case_name.startswith("structured_"):
        out.add(("structured", run.case_name))
    if t.name == "narrow":
        # the four rows of a quad share one `longest`
        quads = counts.reshape(-1, 4, nchunks)
        quad_staged = staged.reshape(-1, 4).all(axis=1)
        for quad in quads[quad_staged]:
            for ch in range(nchunks):
                here = quad[:, ch]
                for g in np.nonzero(here > 2 * C.WINDOW)[0]:
                    others = np.delete(here, g)
                    kind = ("padding" if (others < 0).any() else "short" if ((others >= 1) & (others <= 3)).all()
                            else "empty" if (others == 0).all() else None)
                    if kind:
                        out.add(("longest", int(g), kind))
        shares = C.share_chunks(nchunks, run.ksplits())
        if run.ksplits() > 1:
            out |= {("share", end - begin) for begin, end in shares}
            if any(begin % 2 == 1 and end > begin for begin, end in shares):
                out.add(("share_starts_on_an_odd_chunk",))
            out.add(("split_epilogue", "relu" if run.relu else "bias" if run.bias else "none"))
            if not ok.all():
                out.add(("split_gather_block",))
        elif run.splits > 1:
            out.add(("no_split", "unaligned_out" if run.out_offset else "n_not_a_multiple_of_4"))
    elif run.sparse:
        # a segment longer than the window (the on-demand drain) at wave-row r, and the D - 1
        # visits of the wave's walk behind it
        waves = counts.reshape(-1, t.rows_per_wave, nchunks)
        wave_staged = staged.reshape(-1, t.rows_per_wave).all(axis=1)
        rpw, depth = t.rows_per_wave, t.depth
        for wave in waves[wave_staged]:
            walk = wave.T.reshape(-1)                   # visit ch * RPW + r
            for at in np.nonzero(walk > C.WINDOW)[0]:
                ch, r = divmod(int(at), rpw)
                place = "last" if ch == nchunks - 1 else "not_last"
                behind = walk[at + 1:at + depth]
                in_wave = wave[r + 1:, ch]
                if len(in_wave) and (in_wave < 0).all():
                    out.add(("drain", r, "padding", place))
                elif len(behind) == 0:
                    out.add(("drain", r, "end", place))
                elif ((behind >= 1) & (behind <= 3)).all():
                    out.add(("drain", r, "short", place))
                elif (behind == 0).all():
                    out.add(("drain", r, "empty", place))
    return frozenset(out)


def required(form):
    """The edges of the issue's table that apply to one of the ten forms."""
    tile_name, _, variant = form.partition("_")
    t = C.TILES[tile_name]
    counts = C.COUNTS[t.chunk]
    need = {("count", v, place) for v in counts for place in ("first", "middle")}
    need |= {("count", v, "last") for v in counts if v <= C.TAIL}
    need |= {("only_last_chunk",), ("empty_last_row",), ("padding_slots",), ("block_of_padding",),
             ("gather_block_beside_staged",), ("last_block_gathered",), ("gather_block_partial_tile",),
             ("runs_of_slots", 1), ("runs_of_slots", 3), ("chunks", 1),
             ("last_chunk_width", 1), ("last_chunk_width", t.chunk - 1), ("last_chunk_width", t.chunk),
             ("last_chunk_width", C.TAIL)}
    need |= {("last_entry_in_a_row_of", v) for v in (1, 2, 17)}
    if tile_name == "narrow":
        need |= {("n", n) for n in (64, 68, 72, 132, 66, 67, 71)}
        need |= {("longest", g, kind) for g in range(4) for kind in C.QUAD_FOLLOWERS}
        need |= {("longest", g, "padding") for g in range(3)}
        need |= {("chunks", 3), ("chunks", 5)}
        need -= {("block_of_padding",), ("runs_of_slots", 1)}   # (a block is a whole run of 128 slots here)
        need.add(("runs_of_slots", 2))
        if variant == "split":
            need = {("share", v) for v in (0, 1, 2, 3)} | {("share_starts_on_an_odd_chunk",), ("split_gather_block",)}
            need |= {("split_epilogue", e) for e in ("none", "bias", "relu")} | {("chunks", 3), ("chunks", 5)}
        else:
            need |= {("no_split", "unaligned_out"), ("no_split", "n_not_a_multiple_of_4"), ("replicas", 1), ("replicas", 3)}
            need |= {("structured", name) for name in C.STRUCTURED_CASES}
        return need
    need |= {("n_tiles", 1), ("n_tiles", 2), ("n_tiles", "eight"), ("last_tile", "full"), ("last_tile", "partial"),
             ("grid_divides_by_8", True), ("grid_divides_by_8", False), ("block_with_one_real_row",)}
    if t.cols == 512:
        need.add(("last_tile", "piece1_partial"))
    if tile_name == "large":                    # (a block is a whole run of 256 dealt slots)
        need -= {("block_of_padding",), ("block_with_one_real_row",)}
    if tile_name in ("large", "wide512"):       # (the replica count selects these tiles)
        need |= {("values", "shared"), ("replicas", 4)}
    else:
        need |= {("values", "shared"), ("values", "per_replica"), ("replicas", 1), ("replicas", 3)}
    if variant == "short":
        rpw, depth = t.rows_per_wave, t.depth
        for r in sorted({0, depth - 1, depth % rpw, rpw - 1}):
            need |= {("drain", r, kind, "not_last") for kind in ("short", "empty")}
            if r < rpw - 1:
                need |= {("drain", r, kind, "last") for kind in ("short", "empty")}
                need |= {("drain", r, "padding", place) for place in ("not_last", "last")}
            else:
                need.add(("drain", r, "end", "last"))
    return need


@pytest.mark.parametrize("form", C.FORMS)
def test_runs_reach_every_edge_of_the_form(form):
    """Each (instance, applicable edge) pair: the edges recounted over the form's runs."""
    mine = [i for i, run in enumerate(RUNS) if run.form == form]
    assert mine, form
    reached = set().union(*(edges_of(i) for i in mine))
    missing = required(form) - reached
    assert not missing, (form, sorted(missing, key=str))
    if form.split("_")[0] != "narrow":      # one structured kind per instance, every kind in turn
        assert any(label[0] == "structured" for label in reached), form


def test_every_structured_kind_runs_on_the_tiled_kernels():
    kinds = {run.case_name for run in RUNS if run.case_name.startswith("structured_") and run.tile.name != "narrow"}
    assert kinds == set(C.STRUCTURED_CASES)


def test_shapes_stay_small():
    for run in RUNS:
        c = run.case
        assert c.m <= 1300 and c.k <= 600, run.id
        assert run.n <= 512 or run.case_name == "pad_257_identity" or run.tile.cols == 512, run.id
        # (the replica-count runs: the output of a call stays under 48 MB)
        assert 4 * run.replicas * c.m * run.n <= 48e6, run.id


# ---------------------------------------------------------------------------
# the launch query
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=lambda run: run.id)
def test_launch_query_answers_the_run(run, knobs):
    """The query under the run's knobs: the instance, the grid and the offsets of its tables;
    the same for a call whose workspace sputnik_hip_spmm_plan filled (one layout for both)."""
    c = run.case
    knobs(run.knobs())
    got = capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 4 if run.out_offset % 4 else 16)
    assert got == run.launch_shape(), (run.id, got)
    assert got["workspace_bytes"] == capi.spmm_workspace_bytes(c.m, c.k, run.n, c.nnz)
    words, _ = C.plan_words(run.case_name, run.bk)
    assert got["table_offset"] - got["row_ok_offset"] == 4 * S.row_ok_ints(got["slots"])
    assert got["row_ok_offset"] + 4 * len(words) <= got["workspace_bytes"]
    if got["ksplits"] > 1:
        assert got["partials_offset"] >= got["row_ok_offset"] + 4 * len(words)
        assert got["partials_offset"] + 4 * got["ksplits"] * c.m * run.n <= got["workspace_bytes"]


def test_query_reaches_all_ten_forms(knobs):
    seen = collections.Counter()
    for run in RUNS:
        c = run.case
        knobs(run.knobs())
        got = capi.spmm_launch_shape(c.m, c.k, run.n, c.nnz, run.replicas, 4 if run.out_offset % 4 else 16)
        if got["family"] == "narrow64":
            seen["narrow_split" if got["ksplits"] > 1 else "narrow_unsplit"] += 1
        else:
            tile = [t for t in C.TILES.values() if (t.cols, t.rows, t.rows_per_wave) ==
                    (got["tile_cols"], got["tile_rows"], got["rows_per_wave"])]
            assert len(tile) == 1, got
            seen[f"{tile[0].name}_{'short' if got['sparse'] else 'long'}"] += 1
    assert set(seen) == set(C.FORMS) and len(C.FORMS) == 10, seen
    assert min(seen.values()) >= 12, seen


def test_query_without_knobs_reports_the_side_by_side_layouts(knobs):
    """Automatic dispatch, where a plan made without the replica count carries the tables of
    every kernel a later call may take: the 64-column kernel's behind the 256-column kernel's
    (2048 x 2048 x 256: 4 replicas take the one, 16 the other), the 512-column kernel's behind
    both (n = 512), the flat-stream plan behind everything."""
    knobs({})
    m = k = 2048
    nnz = m * k // 5
    narrow, wide = (capi.spmm_launch_shape(m, k, 256, nnz, r) for r in (4, 16))
    assert (narrow["family"], wide["family"], wide["tile_rows"]) == ("narrow64", "wide256", 128)
    wide_bytes = 4 * (S.row_ok_ints(2048) + 33 * 2048)
    assert (wide["row_ok_offset"], wide["table_offset"]) == (0, 4 * S.row_ok_ints(2048))
    assert narrow["row_ok_offset"] == wide_bytes and narrow["table_offset"] == wide_bytes + 4 * S.row_ok_ints(2048)
    assert narrow["workspace_bytes"] == wide["workspace_bytes"] >= narrow["table_offset"] + 4 * 17 * 2048
    nnz = m * k * 3 // 10
    narrow, wide512, flat = (capi.spmm_launch_shape(m, k, 512, nnz, r) for r in (2, 8, 64))
    assert (narrow["family"], wide512["family"], wide512["tile_rows"], flat["family"]) == \
        ("narrow64", "wide512", 64, "flat")
    assert narrow["row_ok_offset"] == wide_bytes
    behind = narrow["workspace_bytes"] - flat["table_offset"]
    assert wide512["row_ok_offset"] % 256 == 0 and wide512["row_ok_offset"] >= narrow["table_offset"] + 4 * 17 * 2048
    assert wide512["table_offset"] == wide512["row_ok_offset"] + 4 * S.row_ok_ints(2048)
    assert flat["table_offset"] % 256 == 0 and flat["table_offset"] >= wide512["table_offset"] + 4 * 65 * 2048
    assert behind > 0 and flat["row_ok_offset"] == -1


def test_query_names_the_other_families(knobs):
    knobs({})
    assert capi.spmm_launch_shape(72, 64, 7, 464, 1)["family"] == "rowgather"
    assert capi.spmm_launch_shape(4096, 4096, 4096, 1677721, 1)["family"] == "flat"
    # (the panel kernel asks the device for its LDS: a machine without one never reports it; the
    # query and the name query must agree either way)
    names = {"spmm_rowgather_kernel": "rowgather", "spmm_panel64_kernel": "panel", "spmm_tiled64_kernel": "narrow64",
             "spmm_tiled_kernel<TileConfig<256": "wide256", "spmm_tiled_kernel<TileConfig<512": "wide512"}
    for shape in ((1024, 1024, 64, 104857, 64), (512, 512, 256, 78643, 64), (2048, 512, 64, 209715, 8),
                  (2048, 2048, 512, 1258291, 8), (1024, 512, 128, 104857, 64)):
        assert names[capi.spmm_kernel_name(*shape)] == capi.spmm_launch_shape(*shape)["family"], shape
    knobs({"SPUTNIK_HIP_SPMM_KERNEL": "gather"})
    gather = capi.spmm_launch_shape(2048, 2048, 256, 838860, 16)
    assert gather["family"] == "rowgather" and gather["tile_cols"] == 0 and gather["table_offset"] == -1
    with pytest.raises(RuntimeError):
        capi.spmm_launch_shape(0, 64, 64, 0, 1)
    with pytest.raises(RuntimeError):
        capi.spmm_launch_shape(64, 64, 64, 1024, 1, out_alignment=6)


def test_what_reaches_the_large_tile_without_a_knob(knobs):
    """spmm_tiled_kernel<CfgLarge, *> needs >= 192 tiles of 256 x 256 in one launch, its long form
    nonzeros >= 15 m nchunks on top, and neither the flat-stream kernel (from 192 of ITS tiles,
    n a multiple of 512) nor the panel kernel (k <= 512 at n <= 256) may take the call: the
    full-size 4096^3 products go to the flat kernel, a batch of 64 products of 1024 x 640 x 256
    reaches the large tile in either form."""
    knobs({})
    assert capi.spmm_launch_shape(4096, 4096, 4096, 1677721, 1)["family"] == "flat"
    for density, sparse in ((0.1, True), (0.25, False), (0.9, False)):
        got = capi.spmm_launch_shape(1024, 640, 256, int(1024 * 640 * density), 64)
        assert (got["family"], got["tile_rows"], got["sparse"], got["grid_x"], got["grid_y"]) == \
            ("wide256", 256, sparse, 4, 64), (density, got)
