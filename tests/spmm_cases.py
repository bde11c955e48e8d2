"""Named matrices and runs for the LDS-tiled SpMM kernels that share chunk_table_body: the eight
instances of spmm_tiled_kernel<Cfg, SPARSE> (csrc/spmm_tiled.hip) and spmm_tiled64_kernel with its
K split (csrc/spmm_tiled64.hip).  Each matrix is built to put a stated edge of the kernels'
hand-made logic in front of them: how many entries a row holds in one K chunk, where in a wave's
window ring a long segment sits and what follows it, padding slots, rows that are not ok, the
clamps at the end of the arrays.  Rows are placed by POSITION -- row slot = (workgroup, wave,
wave-row) -- through the dealt_index model; the plan model (row_ok and the chunk table as
chunk_table_body<BK> writes them) is the one of tests/sddmm_cases.py, which the SDDMM kernels
share.  A float64 reference, the operands, and the (instance x case) run list with the knobs, the
replica count and the launch each run means to reach.  numpy only, explicit seeds; no kernel, no
oracle.

tests/test_spmm_cases_cpu.py proves that the matrices reach the edges they are named for and that
the run list reaches every instance; tests/test_gpu_spmm_instances.py runs the list.
"""
import functools

import numpy as np

import sddmm_cases as S

ceil_div = S.ceil_div
dealt_index = S.dealt_index
CANARY_INT, GUARD = S.CANARY_INT, S.GUARD
WINDOW = 16         # entries of a segment that arrive with the row (short form); 2 * 16 in the 64-column kernel


# ---------------------------------------------------------------------------
# the kernels' geometry
# ---------------------------------------------------------------------------
class Tile:
    """One kernel body's tile: `per` = run of slots the rows are dealt in, `depth` = windows in
    flight (D), `batch` = kBatch of the short form."""

    def __init__(self, name, family, cols, waves, rows_per_wave, chunk, per, depth, batch):
        self.name, self.family, self.cols, self.waves = name, family, cols, waves
        self.rows_per_wave, self.chunk, self.per, self.depth, self.batch = rows_per_wave, chunk, per, depth, batch
        self.rows = waves * rows_per_wave

    def slots(self, m):
        return ceil_div(m, self.per) * self.per


TILES = {t.name: t for t in (
    Tile("large", "wide256", 256, 16, 16, 64, 256, 8, 4),
    Tile("medium", "wide256", 256, 16, 8, 64, 256, 8, 8),
    Tile("small", "wide256", 256, 8, 8, 64, 256, 8, 8),
    Tile("wide512", "wide512", 512, 16, 8, 32, 256, 4, 4),
    Tile("wide512half", "wide512", 512, 16, 4, 32, 256, 4, 4),
    Tile("narrow", "narrow64", 64, 8, 16, 128, 128, 0, 0))}

# the ten forms: (tile, SPARSE) of spmm_tiled_kernel, the 64-column kernel unsplit and split
TILED_INSTANCES = (("large", False), ("large", True), ("medium", False), ("medium", True),
                   ("small", False), ("small", True), ("wide512", True), ("wide512half", True))
FORMS = tuple(f"{t}_{'short' if s else 'long'}" for t, s in TILED_INSTANCES) + ("narrow_unsplit", "narrow_split")

# entries of a row in one K chunk.  Short form: both sides of a batch (4 / 8), `tail & 4 / 2 / 1`,
# the full window and the on-demand loop past it (16 at a time: 17, 32, 33, 48, 49, 64); long
# form: groups of 16 with a padded last group of four.  64-column kernel: `left > 4 / 8 / 12`,
# the two prefetched windows, the first and second on-demand window, the whole chunk.
COUNTS = {64: (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64),
          32: (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 23, 24, 25, 31, 32),
          128: (0, 1, 4, 5, 8, 9, 12, 13, 16, 17, 31, 32, 33, 48, 49, 128)}
# the long segments of a window-ring design, in (chunk 0, a middle chunk, the last chunk)
LONG = {64: (17, 33, 18, 49), 32: (17, 29, 18, 32), 128: (40, 33, 49, 128)}
# wave-row of the long segment (slot % run): 0, D - 1, D, RPW - 1 of every tile that shares the table
RING_RUN = {64: 16, 32: 8}
RING_AT = {64: (0, 7, 8, 15), 32: (0, 3, 4, 7)}
TAIL = 20           # rows of B in the partial last chunk of the main shapes
K_MAIN = {64: 3 * 64 + TAIL, 32: 3 * 32 + TAIL, 128: 4 * 128 + TAIL}       # 212, 116, 532
K_THREE = 2 * 128 + TAIL                                                    # 276: three chunks of 128
# k = BK (one chunk), c * BK + 1 (every staged row but one clamps to k - 1), c * BK - 1
K_EDGES = {bk: (bk, 2 * bk + 1, 3 * bk - 1) for bk in (64, 32, 128)}
MIN_MEAN = {64: 16, 32: 16, 128: 4}       # what the routes ask for: nonzeros >= MIN_MEAN * m


# ---------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------
def chunk_counts(row_offsets, column_indices, k, bk):
    """[m, ceil(k / bk)] entries of each row per K chunk."""
    return S.slab_counts(row_offsets, column_indices, k, bk)


def slot_counts(case, bk, per, row_indices=None):
    """[slots, nchunks] entries per (row slot, chunk); -1 in every chunk of a padding slot."""
    rows = S.slot_rows(case.row_indices if row_indices is None else row_indices, case.m, per)
    counts = chunk_counts(case.row_offsets, case.column_indices, case.k, bk)
    out = np.full((len(rows), counts.shape[1]), -1, dtype=np.int64)
    out[rows >= 0] = counts[rows[rows >= 0]]
    return out


def reference(row_offsets, column_indices, values, dense):
    """float64 [R, m, n]: the dense image of the CSR matrix of every replica (values [R, nnz], or
    [1, nnz] shared) times dense [R, k, n]."""
    ro = np.asarray(row_offsets, np.int64)
    rows = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    a = np.zeros((values.shape[0], len(ro) - 1, dense.shape[1]), dtype=np.float64)
    a[:, rows, np.asarray(column_indices, np.int64)] = values
    return a @ np.asarray(dense, np.float64)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class Case(S.Case):
    """CSR of a dense [m, k] bool pattern (S.Case: `n` there is k here), `row_indices` in the
    order that places the designed rows; `spec`: row -> entries per chunk it was built with."""

    @property
    def k(self):
        return self.n

    def other_order(self):
        """A second row order of the same matrix: rows by length, longest first (what callers
        pass); a random permutation where that is the case's own."""
        if self.order == "by_length":
            return np.random.default_rng(self.m).permutation(self.m).astype(np.int32)
        lengths = np.diff(self.row_offsets.astype(np.int64))
        return np.argsort(-lengths, kind="stable").astype(np.int32)


def _fill(dense, row, chunk, count, rng, k, bk, must=None):
    """`count` entries of `row` inside K chunk `chunk` (clipped to its width): a random subset
    that holds the chunk's last column for even rows, its first for rows 0, 3, ..; `must`: a
    column it holds in any case."""
    lo, hi = chunk * bk, min((chunk + 1) * bk, k)
    count = min(count, hi - lo)
    if count <= 0:
        return
    cols = np.sort(rng.choice(np.arange(lo, hi), size=count, replace=False))
    if row % 2 == 0:
        cols[-1] = hi - 1
    if row % 3 == 0 and count > 1:
        cols[0] = lo
    if must is not None and must not in cols:
        cols[-1] = must
    dense[row, cols] = True


def _three(first, middle, last, nchunks):
    """Counts per chunk: `first` in chunk 0, `middle` in chunk nchunks // 2, `last` in the last."""
    out = [0] * nchunks
    out[nchunks - 1] = last
    if nchunks > 2:
        out[nchunks // 2] = middle
    out[0] = first
    return out


def table_design(bk, nchunks, at):
    """slot -> counts: COUNTS[bk][j] in chunk 0, shifted copies in a middle and the last chunk."""
    c = COUNTS[bk]
    n = len(c)
    return {at + j: _three(c[j], c[(j + n // 3) % n], c[(j + 2 * n // 3) % n], nchunks) for j in range(n)}


def ring_design(bk, nchunks, at, index, long_at, run, followers):
    """One run of `run` slots starting at `at`: the row at `long_at` holds a segment longer than
    the window in chunk 0, a middle chunk and the last chunk; every other row of the run holds 1,
    2 or 3 entries in every chunk (`followers` = "short") or none at all ("empty")."""
    longs = LONG[bk]
    out = {}
    for j in range(run):
        if j == long_at:
            out[at + j] = _three(longs[index % 4], longs[(index + 1) % 4], longs[(index + 2) % 4], nchunks)
        else:
            out[at + j] = [1 + (j + c) % 3 if followers == "short" else 0 for c in range(nchunks)]
    return out


ONLY_LAST = "only_last"     # a spec value: entries in the last chunk alone, column k - 1 among them


def tiled_layout(bk, nchunks, base, rings=True):
    """The designed slots of one run of 256 starting at `base` (tables of 64- and 32-row chunks):
    positions 0.. the counts table and, with `rings`, the window-ring designs (long segment at
    wave-row 0, D - 1, D, RPW - 1; followers short, then empty), then two rows with entries in
    the last chunk only: 162 positions at the most."""
    run, spec = RING_RUN[bk], {}
    spec.update(table_design(bk, nchunks, base))
    if not rings:
        return spec
    at = base + ceil_div(len(COUNTS[bk]), run) * run
    for index, (followers, long_at) in enumerate((f, r) for f in ("short", "empty") for r in RING_AT[bk]):
        spec.update(ring_design(bk, nchunks, at, index, long_at, run, followers))
        at += run
    spec[at], spec[at + 1] = (ONLY_LAST, 3), (ONLY_LAST, bk)
    return spec


# the 64-column kernel: the four rows of a quad share one `longest`
QUAD_FOLLOWERS = ("short", "empty")


def narrow_layout(nchunks, base, rings=True):
    """The designed slots of one run of 128 (the 64-column kernel): positions 0..15 the counts
    table (wave 0) and, with `rings`, 16..47 eight quads whose row `g` holds more than 32 entries
    in chunk 0, a middle and the last chunk beside three rows of 1..3 entries (g = 0..3), then
    beside three empty rows; 48, 49 rows with entries in the last chunk only."""
    spec = dict(table_design(128, nchunks, base))
    if not rings:
        return spec
    at = base + 16
    for index, (followers, g) in enumerate((f, g) for f in QUAD_FOLLOWERS for g in range(4)):
        spec.update(ring_design(128, nchunks, at, index, g, 4, followers))
        at += 4
    spec[at], spec[at + 1] = (ONLY_LAST, 3), (ONLY_LAST, 128)
    return spec


def build_case(name, m, k, bk, per, order, last, seed, rings=True, unsorted=True):
    """Rows by specification in the first and the last run of `per` slots (tiled_layout /
    narrow_layout; `rings` False: the counts table alone), and:
      * the LAST REAL SLOT of run 0 holds a segment longer than the window in every chunk, the
        real slots before it in its wave 1..3 entries: with m off a multiple of the wave's rows
        the slots behind it are padding (`pad_*` shapes pick m for the wave-row they want);
      * `last` = 1, 2, 17: the last row of the matrix holds that many entries in the last chunk
        -- the global last entry of column_indices -- 0: it is empty (skipped where the last row
        is a designed one);
      * unsorted rows: with three runs or more one reversed row and one with a swapped pair in
        run 1 and two more near the end of the last run, so that run 0 stays staged for every
        tile; with fewer runs the two highest free slots of run 0 below the wave of its last
        real slot (the 64-row tile keeps staged blocks on both sides of them);
      * every other row: 0..20 entries in a chunk with probability 0.7, then whole rows filled
        from the highest free slot down until nonzeros >= MIN_MEAN * m + 8."""
    rng = np.random.default_rng(seed)
    nchunks, runs = ceil_div(k, bk), ceil_div(m, per)
    slots = runs * per
    if order == "permuted":
        ri = np.random.default_rng(900 + seed).permutation(m)
    else:
        ri = np.arange(m)
    layout = narrow_layout if per == 128 else functools.partial(tiled_layout, bk)
    spec = dict(layout(nchunks, 0, rings))
    if runs > 1:
        spec.update(layout(nchunks, (runs - 1) * per, rings))
    real = lambda slot: dealt_index(slot, slots, per) < m     # noqa: E731
    assert all(real(s) for s in spec), (name, "a designed slot is padding")
    # the last real slot of run 0 and its wave (aligned run of 16 slots: one wave of the largest tile)
    tail = max(s for s in range(per) if real(s))
    if tail not in spec:
        for s in range(tail // 16 * 16, tail):
            if s not in spec:
                spec[s] = [1 + (s + c) % 3 for c in range(nchunks)]
        longs = LONG[bk]
        spec[tail] = [longs[(tail + c) % 4] for c in range(nchunks)]
    row_of = lambda slot: int(ri[dealt_index(slot, slots, per)])      # noqa: E731
    by_row = {row_of(s): counts for s, counts in spec.items()}
    assert len(by_row) == len(spec)
    if order == "permuted" and (m - 1) in by_row and last is not None:      # keep the last row free
        free = next(r for r in range(m - 2, 0, -1) if r not in by_row)
        a, b = int(np.nonzero(ri == m - 1)[0][0]), int(np.nonzero(ri == free)[0][0])
        ri[[a, b]] = ri[[b, a]]
        by_row = {row_of(s): counts for s, counts in spec.items()}
    dense = np.zeros((m, k), dtype=bool)
    free_rows = []
    for slot in range(slots):
        if not real(slot):
            continue
        row = row_of(slot)
        counts = spec.get(slot)
        if counts is None:
            free_rows.append(row)
            for c in range(nchunks):
                if rng.random() < 0.7:
                    _fill(dense, row, c, int(rng.integers(0, 21)), rng, k, bk)
        elif counts[0] == ONLY_LAST:
            _fill(dense, row, nchunks - 1, counts[1], rng, k, bk, must=k - 1)
        else:
            for c, count in enumerate(counts):
                _fill(dense, row, c, count, rng, k, bk)
    if (m - 1) not in by_row and last is not None:
        dense[m - 1] = False
        _fill(dense, m - 1, nchunks - 1, last, rng, k, bk)
        free_rows = [r for r in free_rows if r != m - 1]
    unsorted_rows = []
    if unsorted:
        if runs >= 3:
            at = [per + 33, per + 34] + [max(s for s in range((runs - 1) * per, slots) if real(s)) - d for d in (2, 3)]
        else:
            at = [s for s in range(tail // 16 * 16 - 1, 0, -1) if s not in spec][:2]
        for s in at:
            assert real(s) and s not in spec, (name, s)
            row = row_of(s)
            if row == m - 1:
                continue
            dense[row] = False
            dense[row, rng.choice(k, size=int(rng.integers(12, min(41, k))), replace=False)] = True
            unsorted_rows.append(row)
            free_rows = [r for r in free_rows if r != row]
    need = MIN_MEAN[bk] * m + 8
    for row in reversed(free_rows):
        if np.count_nonzero(dense) >= need:
            break
        dense[row] = True
    assert np.count_nonzero(dense) >= need, (name, np.count_nonzero(dense), need)
    case = Case(name, dense, None if order == "by_length" else ri, order,
                reversed_rows=unsorted_rows[0::2], swapped_rows=unsorted_rows[1::2])
    case.spec = by_row
    case.last = last if (m - 1) not in by_row else None
    case.bk = bk
    return case


STRUCTURED_KINDS = ("causal", "band", "last_chunk", "heavy_rows_block", "corner")
STRUCTURED_M = 523


def structured_case(kind, bk):
    """helpers.structured_mask at three runs of 256 rows (five of 128) and the main k of the
    chunk height (212, 116, 532); `last_chunk` fills exactly the partial last chunk."""
    from helpers import structured_mask   # (imports the oracle package: layout code only)
    m, k = STRUCTURED_M, K_MAIN[bk]
    dense = structured_mask(kind, m, k, MIN_MEAN[bk], np.random.default_rng(77), chunk=bk)
    case = Case(f"structured_{kind}_{m}x{k}", dense, None, "by_length")
    case.spec, case.last, case.bk = {}, None, bk
    return case


# name -> (m, k as a function of the chunk height, order, last row, seed).  edges_*: several runs
# of slots at the main k (a partial last chunk of 20 rows).  pad_*: one run (257: two) whose last
# real slot is followed by padding, m chosen for the wave-row of that slot: (m - 1) % 16 = 0, 7, 8
# (wave-row 0, D - 1, D of the 16-row wave; 0, 7, 0 of the 8-row waves), (m - 1) % 8 = 3, 4
# (D - 1, D of the 512-column tile), 203 and 256 / 257 as everywhere in this suite; k = BK (193),
# 2 BK + 1 (256, 257), 3 BK - 1 (196, 201) or the main k.
EDGE_SHAPES = {
    "edges_1283_identity_last1": (1283, lambda bk: K_MAIN[bk], "identity", 1, 1),
    "edges_523_permuted_last2": (523, lambda bk: K_MAIN[bk], "permuted", 2, 2),
    "edges_779_identity_last17": (779, lambda bk: K_MAIN[bk], "identity", 17, 3),
    "edges_524_by_length_last0": (524, lambda bk: K_MAIN[bk], "by_length", 0, 4),
    "pad_193_identity": (193, lambda bk: K_EDGES[bk][0], "identity", 1, 5),
    "pad_200_permuted": (200, lambda bk: K_MAIN[bk], "permuted", 2, 6),
    "pad_201_identity": (201, lambda bk: K_EDGES[bk][2], "identity", 1, 7),
    "pad_196_identity": (196, lambda bk: K_EDGES[bk][2], "identity", 1, 8),
    "pad_197_permuted": (197, lambda bk: K_MAIN[bk], "permuted", 17, 9),
    "pad_203_identity": (203, lambda bk: K_MAIN[bk], "identity", 1, 10),
    "pad_256_permuted": (256, lambda bk: K_EDGES[bk][1], "permuted", 17, 11),
    "pad_257_identity": (257, lambda bk: K_EDGES[bk][1], "identity", 1, 12),
    # the 64-column kernel: three chunks of 128, and the long row as group 1 / 3 of the last quad
    "edges_779_identity_k276": (779, lambda bk: K_THREE, "identity", 2, 13),
    "pad_202_identity_k276": (202, lambda bk: K_THREE, "identity", 1, 14),
    "pad_200_identity_k532": (200, lambda bk: K_MAIN[128], "identity", 1, 15),
}
STRUCTURED_CASES = tuple(f"structured_{kind}" for kind in STRUCTURED_KINDS)


@functools.lru_cache(maxsize=None)
def case(name, bk):
    """The case `name` laid out for K chunks of `bk` rows of B."""
    assert bk in COUNTS, bk
    if name.startswith("structured_"):
        return structured_case(name[len("structured_"):], bk)
    m, k_of, order, last, seed = EDGE_SHAPES[name]
    per = 128 if bk == 128 else 256
    edges = name.startswith("edges_")
    return build_case(f"{name}_bk{bk}", m, k_of(bk), bk, per, order, last, seed, rings=edges,
                      unsorted=edges or name.startswith("pad_203"))


@functools.lru_cache(maxsize=None)
def plan_words(name, bk, other_order=False):
    """(words, defined) of the case's tables as the pre-pass writes them: row_ok, then the chunk
    table 256-byte aligned behind it (S.workspace_model)."""
    c = case(name, bk)
    ri = c.other_order() if other_order else c.row_indices
    return S.workspace_model(ri, c.row_offsets, c.column_indices, c.m, c.k, bk, per=128 if bk == 128 else 256)


# ---------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------
LARGE_FROM = 192        # tiles of a launch from which the 256-row / the 128 x 512 tile is taken


def narrow_ksplits(m, k, n, forced):
    """ksplits_of (spmm_tiled64.hip) under SPUTNIK_HIP_SPMM_MEDIUM = `forced` (0: automatic)."""
    if n % 4:
        return 1
    chunks, groups = ceil_div(k, 128), ceil_div(m, 128) * ceil_div(n, 64)
    if forced >= 16:
        return max(1, min(forced - 16, chunks))
    splits = 1
    while splits < 8 and groups * splits * 2 <= 512 and chunks >= 4 * splits:
        splits *= 2
    return splits


class Run:
    """One call: the form it means to reach, the case, n, the replica count, shared or per-replica
    values, the epilogue, the knobs -- and the launch the query must report for it."""

    def __init__(self, form, case_name, n, replicas, shared, splits=0, bias=False, relu=False, out_offset=0):
        self.form, self.case_name, self.n, self.replicas, self.shared = form, case_name, n, replicas, shared
        self.splits, self.bias, self.relu, self.out_offset = splits, bias, relu, out_offset
        tile_name, _, variant = form.partition("_")
        self.tile = TILES[tile_name]
        self.sparse = variant == "short"
        self.id = (f"{form}-{case_name}-n{n}-r{replicas}{'s' if shared else ''}" + (f"-split{splits}" if splits else "") +
                   ("-bias" if bias else "") + ("-relu" if relu else "") + ("-unaligned" if out_offset else ""))

    @property
    def case(self):
        return case(self.case_name, self.tile.chunk)

    @property
    def bk(self):
        return self.tile.chunk

    def knobs(self):
        t = self.tile
        if t.name == "narrow":
            return {"SPUTNIK_HIP_SPMM_KERNEL": "narrow", "SPUTNIK_HIP_SPMM_MEDIUM": str(16 + max(self.splits, 1))}
        env = {"SPUTNIK_HIP_SPMM_KERNEL": "wide512" if t.cols == 512 else "wide"}
        if t.cols == 256:
            env["SPUTNIK_HIP_SPMM_SPARSE"] = "1" if self.sparse else "0"
        if t.name == "medium":
            env["SPUTNIK_HIP_SPMM_MEDIUM"] = "1"
        return env

    def ksplits(self):
        """Splits the launch runs: one replica, a 16-byte aligned `out`, n a multiple of 4."""
        c = self.case
        if self.tile.name != "narrow" or self.replicas != 1 or self.out_offset % 4:
            return 1
        return narrow_ksplits(c.m, c.k, self.n, 16 + max(self.splits, 1))

    def launch_shape(self):
        """What capi.spmm_launch_shape must answer under knobs()."""
        c, t = self.case, self.tile
        slots, nchunks, n_tiles = t.slots(c.m), ceil_div(c.k, t.chunk), ceil_div(self.n, t.cols)
        ksplits = self.ksplits()
        row_ok = S.row_ok_ints(slots) * 4
        tables = row_ok + 4 * (nchunks + 1) * slots
        if t.name == "narrow":
            tables = ceil_div(tables, 256) * 256
            planned_splits = narrow_ksplits(c.m, c.k, self.n, 16 + max(self.splits, 1))
            bytes_ = tables + (4 * planned_splits * c.m * self.n if planned_splits > 1 else 0)
        else:
            bytes_ = ceil_div(tables, 16) * 16
        return dict(family=t.family, tile_cols=t.cols, tile_rows=t.rows, waves=t.waves,
                    rows_per_wave=t.rows_per_wave, chunk=t.chunk, sparse=self.sparse,
                    batch=t.batch if self.sparse else 0, grid_x=slots // t.rows * n_tiles * ksplits,
                    grid_y=self.replicas, slots=slots, nchunks=nchunks, n_tiles=n_tiles, ksplits=ksplits,
                    workspace_bytes=bytes_, row_ok_offset=0, table_offset=row_ok,
                    partials_offset=tables if ksplits > 1 else -1)

    def blocks_ok(self, row_indices=None):
        """[row blocks of the tile] bool: every row slot of the block is ok (the staged path)."""
        c, t = self.case, self.tile
        rows = S.slot_rows(c.row_indices if row_indices is None else row_indices, c.m, t.per)
        bad = np.isin(rows, c.unsorted_rows)
        return ~bad.reshape(-1, t.rows).any(axis=1)


def large_replicas(tile, m, n):
    """Fewest replicas that give the launch LARGE_FROM tiles of the large kind."""
    rows = 256 if tile.cols == 256 else 128
    per_replica = (ceil_div(m, 256) * 256 // rows if tile.cols == 256 else ceil_div(m, 128)) * ceil_div(n, tile.cols)
    return ceil_div(LARGE_FROM, per_replica)


# n per case for the 256- / 512-column tiles: one full tile, a partial one (196), two with the
# second partial (388: piece h = 1 of the 512-column tile partial), eight with the last four
# columns wide (1796 / 3588: the `n_tiles % 8 == 0` decode, two runs of row slots)
TILED_N = {"edges_1283_identity_last1": 388, "edges_523_permuted_last2": 196,
           "edges_779_identity_last17": "full", "edges_524_by_length_last0": 388,
           "pad_193_identity": 196, "pad_200_permuted": "full", "pad_201_identity": 388,
           "pad_196_identity": 388, "pad_197_permuted": 196, "pad_203_identity": 388,
           "pad_256_permuted": 196, "pad_257_identity": "eight"}
NARROW_N = {"edges_1283_identity_last1": 72, "edges_523_permuted_last2": 132, "edges_779_identity_k276": 68,
            "edges_524_by_length_last0": 67, "pad_193_identity": 64, "pad_200_permuted": 66,
            "pad_201_identity": 71, "pad_196_identity": 68, "pad_197_permuted": 72, "pad_202_identity_k276": 72, "pad_203_identity": 132,
            "pad_256_permuted": 68, "pad_257_identity": 64, "pad_200_identity_k532": 72}


def runs():
    out = []
    for j, (tile_name, sparse) in enumerate(TILED_INSTANCES):
        t = TILES[tile_name]
        form = f"{tile_name}_{'short' if sparse else 'long'}"
        names = list(TILED_N) + [STRUCTURED_CASES[j % len(STRUCTURED_CASES)]]
        for i, name in enumerate(names):
            m = case(name, t.chunk).m
            n = TILED_N.get(name, 388)
            # (196 columns do not fill a 512-column tile to three quarters: two tiles there, the
            # second with four columns in its piece h = 1)
            n = {"full": t.cols, "eight": 7 * t.cols + 4, 196: 196 if t.cols == 256 else 772}.get(n, n)
            if tile_name in ("large", "wide512"):       # the replica count selects these tiles
                # (one more on the first case: a grid whose total does not divide by 8)
                out.append(Run(form, name, n, large_replicas(t, m, n) + (i == 0), shared=True))
            else:
                out.append(Run(form, name, n, 1 if (i + j) % 2 else 3, shared=i % 3 == 0))
    for i, name in enumerate(list(NARROW_N) + list(STRUCTURED_CASES)):
        n = NARROW_N.get(name, (64, 72, 132, 68, 71)[i % 5])
        out.append(Run("narrow_unsplit", name, n, 1 if i % 2 else 3, shared=i % 3 == 0))
    # the K split: s = 2, 3, 4, 8 over five chunks (shares of 3 + 2; 2 + 2 + 1; 2 + 2 + 1 + 0; five of
    # one chunk, every second starting on an odd chunk) and over three (2 + 1; then one each); bias
    # and bias + ReLU behind the sum; `out` off 16-byte alignment: no split
    five = ("edges_523_permuted_last2", "pad_203_identity", "pad_200_identity_k532")
    three = ("edges_779_identity_k276", "pad_202_identity_k276")
    for s in (2, 3, 4, 8):
        for i, name in enumerate(five + three):
            n = (72, 132, 64, 68, 72)[(i + s) % 5]
            out.append(Run("narrow_split", name, n, 1, shared=False, splits=s, bias=(i + s) % 3 >= 1,
                           relu=(i + s) % 3 == 2))
    out.append(Run("narrow_unsplit", five[0], 72, 1, shared=False, splits=4, out_offset=1))
    out.append(Run("narrow_unsplit", three[0], 66, 1, shared=False, splits=3))     # any n: no split
    return out


def share_chunks(nchunks, ksplits):
    """[(c_begin, c_end)] of every split, as spmm_tiled64_kernel cuts the K walk."""
    per_split = ceil_div(nchunks, ksplits)
    out = []
    for s in range(ksplits):
        begin = min(s * per_split, nchunks)
        out.append((begin, min(begin + per_split, nchunks)))
    return out


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def operands(run, seed=0, integers=False):
    """(values [R or 1, nnz], dense [R, k, n], bias [m]) float32: magnitudes in [0.1, 1) with
    random signs, or small integers (values 1..3 with signs, dense -4..4: every partial sum is an
    integer below 2^24)."""
    c = run.case
    rng = np.random.default_rng(2000 + seed)
    vr = 1 if run.shared else run.replicas
    if integers:
        values = rng.integers(1, 4, size=(vr, c.nnz)) * rng.choice((-1, 1), size=(vr, c.nnz))
        dense = rng.integers(-4, 5, size=(run.replicas, c.k, run.n))
        bias = rng.integers(-8, 9, size=c.m)
    else:
        values = rng.uniform(0.1, 1.0, size=(vr, c.nnz)) * rng.choice((-1, 1), size=(vr, c.nnz))
        dense = rng.uniform(-1, 1, size=(run.replicas, c.k, run.n))
        bias = rng.uniform(-1, 1, size=c.m)
    return values.astype(np.float32), dense.astype(np.float32), bias.astype(np.float32)


def expected(run, values, dense, bias):
    """float64 [R, m, n] of the call: the product, plus bias[row] and ReLU where the run asks."""
    c = run.case
    want = reference(c.row_offsets, c.column_indices, values, dense)
    if run.bias:
        want = want + np.asarray(bias, np.float64)[None, :, None]
    if run.relu:
        want = np.maximum(want, 0.0)
    return want
