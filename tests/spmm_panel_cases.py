"""Named matrices, models and runs for the panel-resident SpMM kernels (csrc/spmm_panel.hip): the
eight instances of spmm_panel64_kernel<MULTI, PERM, TOUT>, the twelve of
spmm_panel64_typed_kernel<MULTI, TV, TB> and the four of spmm_panel64_group_kernel<PERM, TOUT,
ACCUM>.  Each matrix is built to put a stated edge of the kernels' hand-made logic in front of
them: how many entries the rows of a quad pair hold (the `left > 4 / 8 / 12` steps, the window
requested at set-up and the one requested in the loop), where a sorted row is cut at the panel
boundary, a row whose order the cut cannot trust beside rows it can, the `start[t]` skip of the
masked walk, padding slots, the clamps at the ends of the arrays, partial column tiles, the
transposing store's row blocks, the group kernel's resident panel.

Rows are placed by POSITION: slot = mblock * 256 + wave * 16 + 4 t + g (quad t, lane group g),
and the row at a slot is row_indices[dealt_index(slot, slots, 256)], or the slot itself for the
instances that take contiguous rows (TOUT, the accumulating group kernel).  The models below are
written from the source text of spmm_panel.hip:
  (a) window_schedule   stream_pairs: which windows of a quad pair arrive with the row, at
                        set-up, in the loop, and the groups of four entries each one works on;
  (b) search_cuts_wave  search_cuts for the sixteen rows of a wave, round by round;
  (c) masked_walk_wave  stream_masked: windows visited per quad and pass, start[t] after it;
  (d) fallback_blocks   the workgroups whose cut passes meet an entry outside their panel;
  (e) reference / transposed_layout   float64 product and the stored layouts.
numpy only, explicit seeds; no kernel, no oracle.

tests/test_spmm_panel_cases_cpu.py proves that the matrices reach the edges they are named for
and that the run list reaches all 24 instances; tests/test_gpu_spmm_panel_instances.py runs it.
"""
import functools

import numpy as np

from sddmm_cases import GUARD, ceil_div, dealt_index    # noqa: F401  (GUARD: re-exported)

PER = 256           # kPBM: rows (slots) of a workgroup
TILE = 64           # kPBN: columns of C per workgroup
PANEL = 512         # kPMaxK: rows of B per panel
WAVE_ROWS = 16      # 4 quads x 4 lane groups
MAX_PASSES = 8      # kPMaxPasses
# row lengths of the one-panel design: both sides of `left > 4 / 8 / 12`, of the window that
# arrives with the row (16), of the set-up request (`16 < longest`: 17 .. 32) and of the loop's
# requests (`w0 + 32 < longest`: 33, 49, 65)
LENGTHS = (49, 13, 17, 33, 0, 1, 3, 4, 5, 8, 9, 12, 15, 16, 31, 32, 47, 48, 64, 65)
LAST_ROW = 65       # the last row of the one-panel matrices: the longest, ends at entry nnz - 1


def slots_of(m):
    return ceil_div(m, PER) * PER


def panels_of(k):
    return ceil_div(k, PANEL)


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
class Matrix:
    """A CSR matrix [m, k] whose rows keep the STORAGE order of their columns (a row need not
    ascend), `row_indices` the order the dealt instances are called with, `placement` the one
    its designed positions were laid out for ("dealt": row_indices = 0 .. m - 1 through
    dealt_index; "identity": slot = row), `claims`: what the builder means it to reach, by name
    (recounted from the arrays by the CPU tests)."""

    def __init__(self, name, m, k, rows, placement, **claims):
        assert len(rows) == m
        self.name, self.m, self.k, self.placement, self.claims = name, m, k, placement, claims
        self.rows = [np.asarray(r, dtype=np.int32) for r in rows]
        self.row_offsets = np.concatenate(([0], np.cumsum([len(r) for r in self.rows]))).astype(np.int32)
        self.column_indices = (np.concatenate(self.rows) if self.nnz else np.zeros(0)).astype(np.int32)
        self.row_indices = np.arange(m, dtype=np.int32)

    @property
    def nnz(self):
        return int(self.row_offsets[-1])

    @property
    def lengths(self):
        return np.diff(self.row_offsets.astype(np.int64))

    def other_order(self):
        """Rows by length, longest first (what callers pass), ties by row number."""
        return np.argsort(-self.lengths, kind="stable").astype(np.int32)

    def sorted_rows(self):
        return np.array([bool((np.diff(r) > 0).all()) for r in self.rows])


def slot_rows(m, identity, row_indices=None):
    """[slots] row at every slot as load_rows<IDENTITY> finds it, -1 for padding."""
    slots = slots_of(m)
    out = np.full(slots, -1, dtype=np.int64)
    for slot in range(slots):
        entry = slot if identity else dealt_index(slot, slots, PER)
        if entry < m:
            out[slot] = entry if identity else (entry if row_indices is None else row_indices[entry])
    return out


def matrix_slot_rows(mat, identity=None, row_indices=None):
    identity = (mat.placement == "identity") if identity is None else identity
    return slot_rows(mat.m, identity, mat.row_indices if row_indices is None else row_indices)


def _row(rng, k, length, lo=0, hi=None, must=()):
    """`length` distinct ascending columns of [lo, hi) that hold the columns of `must`."""
    hi = k if hi is None else hi
    length = min(length, hi - lo)
    must = [c for c in must if lo <= c < hi][:length]
    free = np.setdiff1d(np.arange(lo, hi), must)
    cols = np.concatenate((must, rng.choice(free, size=length - len(must), replace=False))).astype(np.int64)
    return np.sort(cols)


def boundary_columns(k):
    """0, k - 1 and both sides of every panel boundary inside [0, k)."""
    cols = {0, k - 1}
    for b in range(PANEL, k, PANEL):
        cols.update((b - 1, b))
    return sorted(c for c in cols if 0 <= c < k)


def from_slots(name, m, k, placement, spec, seed, fill=(1, 9), last_row=None, **claims):
    """Rows by slot: `spec` slot -> columns in storage order (or a length: that many ascending
    random columns); every other live slot a sorted row of fill[0] .. fill[1] - 1 entries, each
    holding one of boundary_columns(k) in turn.  `last_row`: length of row m - 1."""
    rng = np.random.default_rng(seed)
    at = slot_rows(m, placement == "identity")
    bcols = boundary_columns(k)
    rows = [None] * m
    for slot, row in enumerate(at):
        if row < 0:
            assert slot not in spec, (name, slot, "a designed slot is padding")
            continue
        want = spec.get(slot)
        if want is None:
            want = int(rng.integers(fill[0], fill[1]))
            rows[row] = _row(rng, k, want, must=(bcols[row % len(bcols)],) if want else ())
        elif np.isscalar(want):
            rows[row] = _row(rng, k, int(want), must=(bcols[row % len(bcols)],) if want else ())
        else:
            rows[row] = np.asarray(want)
    if last_row is not None:
        rows[m - 1] = _row(rng, k, last_row, must=(0, k - 1))
    return Matrix(name, m, k, rows, placement, **claims)


# -- one panel: the windows of stream_pairs -----------------------------------------------------
def windows_spec(first_slot, lengths):
    """One quad pair per length, from `first_slot` on (two pairs per wave): the long row in quad
    j % 2 of its pair, lane group (j // 2) % 4; the other seven rows empty (j % 3 == 0: the whole
    other quad is empty), of 1 .. 3 entries, or as long as the long row."""
    spec = {}
    for j, length in enumerate(lengths):
        base = first_slot + 8 * j
        side, g = j % 2, (j // 2) % 4
        for q in range(2):
            for gg in range(4):
                other = (0, min(length, 1 + (gg + q) % 3), length)[j % 3]
                spec[base + 4 * q + gg] = length if (q, gg) == (side, g) else other
    return spec


def windows_case(m, placement):
    """k = 509, one panel.  m = 16: two pairs (13, and the last row); 272, 320 and 512: all of
    LENGTHS, one quad pair each; with contiguous rows and m = 272 the second workgroup is one
    live wave and fifteen of padding.  The last row is the longest and ends at entry nnz - 1."""
    if m == 16:         # the pair of 13, and the last row (65, lane group 3 of the second quad) beside short rows
        spec = windows_spec(0, (13,))
        spec.update({slot: 1 + slot % 3 for slot in range(8, 15)})
    elif placement == "identity":
        spec = windows_spec(0, LENGTHS)
        spec.update(windows_spec(PER, LENGTHS[2:4]))
    else:               # (dealt rows, m = 272: a workgroup has 136 live slots)
        spec = windows_spec(0, LENGTHS[:16])
        spec.update(windows_spec(PER, LENGTHS[16:]))
    return from_slots(f"windows_{m}_{placement}", m, 509, placement, spec, seed=10 + m, fill=(4, 28),
                      last_row=LAST_ROW, lengths=(13, LAST_ROW) if m == 16 else LENGTHS)


# -- k edges ------------------------------------------------------------------------------------
K_ONE = (1, 3, 4, 511, 512)
K_TWO = (513, 516, 1023, 1024)
K_MANY = (1025, 1537, 4096)
N_EDGES = (64, 68, 128, 132)


def k_case(k, placement="dealt"):
    """48 sorted rows (three waves) of 0 .. 70 entries (at most k); rows 0 .. 7 hold every column
    of boundary_columns(k) that fits, so that both sides of every panel boundary sit in one
    window of one row."""
    rng = np.random.default_rng(100 + k)
    m, bcols = 48, boundary_columns(k)
    lengths = [min(k, length) for length in (70, 33, 17, 16, 13, 49, 5, 64) + tuple(rng.integers(0, 40, size=m - 8))]
    rows = []
    for r, length in enumerate(lengths):
        rows.append(_row(rng, k, max(length, min(k, len(bcols))) if r < 8 else length, must=bcols if r < 8 else ()))
    return Matrix(f"k{k}_{placement}", m, k, rows, placement)


# -- two panels: where a sorted row is cut ---------------------------------------------------------
def probes(length):
    return [(i * length) >> 4 for i in range(16)]


def cut_pairs():
    """(length, cut) of the designed rows, in slot order; every wave mixes long and short rows
    (a resolved bracket idles through the rounds of the widest one)."""
    pairs = [(1024, 512), (0, 0), (1, 0), (1, 1)]
    for length, inner in ((5, (4,)), (16, (8, 15)), (17, (7, 8, 9, 16)), (255, (126, 127, 128, 254)),
                          (256, (127, 128, 129, 255)), (257, (127, 128, 129, 256)), (600, (299, 300, 301)),
                          (1000, (488, 499, 500, 501, 512))):
        pairs += [(length, c) for c in (0, 1) + inner + (length,)
                  if c <= PANEL and length - c <= PANEL]
    # long rows dealt over the waves: sort so that every run of 16 slots holds both kinds
    long_ = [p for p in pairs if p[0] > 17]
    short = [p for p in pairs if p[0] <= 17]
    out = []
    while long_ or short:
        out += long_[:5] + short[:11]
        long_, short = long_[5:], short[11:]
    return out


def cut_row(rng, length, cut, k=2 * PANEL, adjacent=True):
    """`cut` ascending columns below the boundary, length - cut at or above it; `adjacent`: 511
    and 512 side by side where the row has both parts."""
    both = adjacent and 0 < cut < length
    return np.concatenate((_row(rng, k, cut, 0, PANEL, must=(PANEL - 1,) if both else ()),
                           _row(rng, k, length - cut, PANEL, k, must=(PANEL,) if both else ())))


CUTS_M = 128        # (a row block the transposing store takes: block_rows = m, a partial workgroup)


def cuts_case(placement="dealt", shuffled=False):
    """k = 1024, m = 128:the rows of cut_pairs() in slots 0 .., the rest short sorted rows.
    `shuffled`: each part of every row in random order -- unsorted, yet partitioned at the
    boundary, so the cut holds."""
    rng = np.random.default_rng(31)
    pairs, spec = cut_pairs(), {}
    for slot, (length, cut) in enumerate(pairs):
        cols = cut_row(rng, length, cut, adjacent=slot % 2 == 0)
        if shuffled:
            cols = np.concatenate((rng.permutation(cols[:cut]), rng.permutation(cols[cut:])))
        spec[slot] = cols
    name = ("partitioned_unsorted_" if shuffled else "cuts_") + placement
    return from_slots(name, CUTS_M, 2 * PANEL, placement, spec, seed=32, pairs=pairs)


# -- two panels: rows the cut cannot trust ----------------------------------------------------------
FALLBACK_SLOT = 37


def fallback_case(kind, placement="dealt"):
    """k = 1024.  "one": m = 512, two workgroups of sorted rows of 8 .. 39 entries but for the row
    at slot 37 of workgroup 0, whose storage order starts 600, 3, 700, 5 (unsorted ACROSS the
    boundary); "descending": m = 272, every row in descending order."""
    k = 2 * PANEL
    if kind == "one":
        rng = np.random.default_rng(41)
        tail = rng.permutation(np.setdiff1d(_row(rng, k, 30), (600, 3, 700, 5)))
        spec = {FALLBACK_SLOT: np.concatenate(((600, 3, 700, 5), tail))}
        return from_slots(f"fallback_one_{placement}", 512, k, placement, spec, seed=42, fill=(8, 40), blocks=(True, False))
    mat = from_slots(f"fallback_descending_{placement}", 272, k, placement, {}, seed=43, fill=(2, 40))
    return Matrix(mat.name, mat.m, k, [r[::-1] for r in mat.rows], placement, blocks=(True, True))


# -- three panels and more: the masked walk --------------------------------------------------------
def walk_case(k, placement="dealt"):
    """m = 64 at k = 1537 / 4096 (4 / 8 panels).  Wave 0, quad 0: three ascending rows of 40
    entries over all panels and one descending row; quad 1: ascending rows of 70 .. 120 entries
    whose windows straddle every boundary (the start skip moves on from pass to pass); quad 2: a row whose first window holds an entry of the last panel and whose
    later windows hold panel 0 alone, a row wholly in the last panel, an empty row, a row of one
    entry (column k - 1); quad 3: descending rows.  Waves 1 .. 3: sorted rows of 0 .. 47 entries."""
    rng = np.random.default_rng(50 + k)
    last0 = (panels_of(k) - 1) * PANEL
    asc = lambda n: _row(rng, k, n, must=boundary_columns(k))      # noqa: E731
    mixed = np.concatenate(((k - 1,), _row(rng, k, 15, 0, PANEL), _row(rng, k, 20, 0, PANEL)[::-1]))
    spec = {0: asc(40), 1: asc(40), 2: asc(40)[::-1], 3: asc(40),
            4: asc(100), 5: asc(70), 6: asc(120), 7: asc(90),
            8: _dedupe(mixed), 9: _row(rng, k, min(24, k - last0), last0, k, must=(k - 1,)), 10: 0, 11: np.array([k - 1]),
            12: asc(20)[::-1], 13: asc(35)[::-1], 14: asc(5)[::-1], 15: asc(48)[::-1]}
    return from_slots(f"walk_k{k}_{placement}", 64, k, placement, spec, seed=51, fill=(0, 48),
                      mixed_slot=8, last_panel_slot=9, held_quad=0)


def _dedupe(cols):
    """First occurrence of every column, order kept."""
    _, first = np.unique(cols, return_index=True)
    return cols[np.sort(first)]


# -- the transposing store ------------------------------------------------------------------------
TRANSPOSED_SHAPES = ((256, 64), (320, 64), (384, 128), (256, 256), (512, 512), (512, 256), (320, 320))
# block_rows_ok (csrc/spmm.hip) takes a multiple of 64 that divides m and either divides 256 or is
# a multiple of it: 320-row blocks are neither, the entry answers UNSUPPORTED and writes nothing.
# (The whole C^T of a matrix with a partial last workgroup is reached at m = block_rows = 128.)
TRANSPOSED_DECLINED = ((320, 320),)


def block_rows_ok(m, block_rows):
    return block_rows >= 64 and block_rows % 64 == 0 and m % block_rows == 0 and \
        (PER % block_rows == 0 or block_rows % PER == 0)


def store_case(m, k=200):
    """Contiguous rows of 0 .. 39 sorted entries; every 7th row empty."""
    spec = {slot: 0 for slot in range(0, m, 7)}
    return from_slots(f"store_{m}_k{k}", m, k, "identity", spec, seed=60 + m + k, fill=(1, 40))


# -- groups ---------------------------------------------------------------------------------------
def group_case(m, k, index, placement):
    """Problem `index` of a group: sorted rows whose lengths differ from problem to problem (0 ..
    8 + 12 * index entries, at most k), so the problems' nonzero counts differ."""
    spec = {0: min(k, 33), 5: 0, 17: min(k, 17 + index)}
    return from_slots(f"group_{m}_k{k}_{index}_{placement}", m, k, placement, spec, seed=70 + index + k,
                      fill=(0, min(k, 8 + 12 * index) + 1))


# -- many masks -----------------------------------------------------------------------------------
def many_mask_cases(name):
    """The masks of one many-mask call: "three": k = 509, m = 272, the last mask EMPTY;
    "cuts": k = 1024, m = 80, the cut design and a second mask with other cuts (its rows
    reversed in slot order)."""
    if name == "three":
        a, b = windows_case(272, "dealt"), from_slots("mask_b", 272, 509, "dealt", {}, seed=81, fill=(0, 30))
        return [a, b, Matrix("mask_empty", 272, 509, [[]] * 272, "dealt")]
    a = cuts_case()
    return [a, Matrix("mask_cuts_reversed", a.m, a.k, a.rows[::-1], "dealt")]


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, rest = name.partition(":")
    args = rest.split(",") if rest else []
    if kind == "windows":
        return windows_case(int(args[0]), args[1])
    if kind == "k":
        return k_case(int(args[0]), *args[1:])
    if kind == "cuts":
        return cuts_case(*args)
    if kind == "partitioned":
        return cuts_case(*args, shuffled=True)
    if kind == "fallback":
        return fallback_case(*args)
    if kind == "walk":
        return walk_case(int(args[0]), *args[1:])
    if kind == "store":
        return store_case(*(int(a) for a in args))
    if kind == "group":
        return group_case(int(args[0]), int(args[1]), int(args[2]), args[3])
    raise KeyError(name)


# ---------------------------------------------------------------------------
# models, from the source text
# ---------------------------------------------------------------------------
def wave_bounds(mat, wave_slot0, identity=None, row_indices=None):
    """(rows, p0, cnt) [4 quads][4 groups] of the wave whose first slot is `wave_slot0`, as
    load_rows leaves them: a padding slot has row -1, p0 = row_offsets[0], cnt = 0."""
    at = matrix_slot_rows(mat, identity, row_indices)
    rows = at[wave_slot0:wave_slot0 + WAVE_ROWS].reshape(4, 4)
    ro = mat.row_offsets.astype(np.int64)
    p0 = ro[np.maximum(rows, 0)]
    cnt = np.where(rows >= 0, ro[np.maximum(rows, 0) + 1] - p0, 0)
    return rows, p0, cnt


def window_schedule(cnt_a, cnt_b):
    """(a) stream_pairs on one quad pair: cnt_a / cnt_b [4] the lengths of the two quads' rows
    by lane group.  -> [(w0, source, steps)]: `source` how window w0 came ("row": with the row,
    fetch_first_windows; "setup": `16 * d < longest`; "loop": `w0' + 32 < longest` at w0' =
    w0 - 32), steps[g] = how many of the four `left > 0 / 4 / 8 / 12` groups lane group g works."""
    longest = int(max(max(cnt_a), max(cnt_b)))
    requested = {0: "row"}
    if 16 < longest:
        requested[16] = "setup"
    out = []
    for w0 in range(0, longest, 16):
        if w0 + 32 < longest:
            requested[w0 + 32] = "loop"
        left = [max(int(a) - w0, int(b) - w0) for a, b in zip(cnt_a, cnt_b)]
        out.append((w0, requested[w0], [sum(v > c for c in (0, 4, 8, 12)) for v in left], left))
    return out


def search_cuts_wave(p0, cnt, column_indices, last, boundary=PANEL):
    """(b) search_cuts for one wave: p0, cnt [4][4] (quad, lane group).  -> (cut [4][4], rounds,
    history) with history[r] = (lo, hi) [4][4] after round r."""
    ci = column_indices
    lo = np.zeros((4, 4), dtype=np.int64)
    hi = np.array(cnt, dtype=np.int64)
    history = []
    while True:
        if int((hi - lo).max()) <= 0:       # `widest`: over the quads, then lanes 0 / 16 / 32 / 48
            break
        new_lo, new_hi = lo.copy(), hi.copy()
        for t in range(4):
            for g in range(4):
                length = int(hi[t, g] - lo[t, g])
                small = length <= 16
                f = 0
                for i in range(16):
                    probe = lo[t, g] + i if small else lo[t, g] + ((i * length) >> 4)
                    col = ci[max(min(int(p0[t][g]) + int(probe), last), 0)] if len(ci) else 0
                    f += int(col < boundary and (not small or i < length))
                if small:
                    new_lo[t, g] = lo[t, g] + f
                    new_hi[t, g] = new_lo[t, g]
                else:
                    new_lo[t, g] = lo[t, g] + (((f - 1) * length) >> 4) + 1 if f > 0 else lo[t, g]
                    new_hi[t, g] = lo[t, g] + ((f * length) >> 4) if f < 16 else hi[t, g]
        lo, hi = new_lo, np.maximum(new_hi, new_lo)
        history.append((lo.copy(), hi.copy()))
        assert len(history) <= 64, "the search does not end"
    return np.minimum(np.maximum(lo, 0), np.array(cnt)), len(history), history


def search_cut_row(cols, boundary=PANEL):
    """The search on a single row (the other fifteen of its wave empty): (cut, rounds)."""
    p0 = np.zeros((4, 4), dtype=np.int64)
    cnt = np.zeros((4, 4), dtype=np.int64)
    cnt[0, 0] = len(cols)
    cut, rounds, _ = search_cuts_wave(p0, cnt, np.asarray(cols), max(len(cols) - 1, 0), boundary)
    return int(cut[0, 0]), rounds


def true_cut(cols, boundary=PANEL):
    """Entries in front of the first one at or above the boundary."""
    at = np.nonzero(np.asarray(cols) >= boundary)[0]
    return int(at[0]) if len(at) else len(cols)


def masked_walk_wave(p0, cnt, column_indices, k):
    """(c) stream_masked over all passes of one wave.  -> (log, taken): log[(pass, t)] =
    (windows visited, start[t] after the pass), taken[(t, g)] = the row's entry numbers in the
    order they were worked on (each must appear exactly once)."""
    start = [0] * 4
    log, taken = {}, {(t, g): [] for t in range(4) for g in range(4)}
    last = max(len(column_indices) - 1, 0)
    for p, kbase in enumerate(range(0, k, PANEL)):
        for t in range(4):
            longest = int(max(cnt[t]))
            begin, first_later, visited = start[t], None, []
            for w0 in range(begin, longest, 16):
                visited.append(w0)
                later = False
                for g in range(4):
                    for i in range(16):
                        if i < int(cnt[t][g]) - w0:
                            col = int(column_indices[min(int(p0[t][g]) + w0 + i, last)]) - kbase
                            if 0 <= col < PANEL:
                                taken[(t, g)].append(w0 + i)
                            later = later or col >= PANEL
                if later and first_later is None:
                    first_later = w0
            start[t] = first_later if first_later is not None else (longest + 15) & ~15
            log[(p, t)] = (visited, start[t])
    return log, taken


def model_cuts(mat, identity=None, row_indices=None):
    """[slots] the cut search_cuts gives every slot (0 for padding), and the most rounds of a wave."""
    slots = slots_of(mat.m)
    cuts, most = np.zeros(slots, dtype=np.int64), 0
    for s0 in range(0, slots, WAVE_ROWS):
        _, p0, cnt = wave_bounds(mat, s0, identity, row_indices)
        cut, rounds, _ = search_cuts_wave(p0, cnt, mat.column_indices, max(mat.nnz - 1, 0))
        cuts[s0:s0 + WAVE_ROWS] = cut.reshape(-1)
        most = max(most, rounds)
    return cuts, most


def fallback_blocks(mat, identity=None, row_indices=None):
    """(d) [workgroups] bool: the two-panel cut passes (stream_pairs<CHECK>) of the workgroup meet
    an entry outside its panel -- in front of the model's cut at or above 512, or behind it
    below 512 -- and the workgroup re-runs the masked walk."""
    assert PANEL < mat.k <= 2 * PANEL
    at = matrix_slot_rows(mat, identity, row_indices)
    cuts, _ = model_cuts(mat, identity, row_indices)
    out = np.zeros(len(at) // PER, dtype=bool)
    for slot, row in enumerate(at):
        if row >= 0:
            cols, cut = mat.rows[row], int(cuts[slot])
            if (cols[:cut] >= PANEL).any() or (cols[cut:] < PANEL).any():
                out[slot // PER] = True
    return out


def reference(mat, values, dense):
    """(e) float64 [R, m, n]: values [R or 1, nnz] in storage order, dense [R, k, n]."""
    rows = np.repeat(np.arange(mat.m), mat.lengths)
    a = np.zeros((values.shape[0], mat.m, mat.k), dtype=np.float64)
    a[:, rows, mat.column_indices.astype(np.int64)] = values
    return a @ np.asarray(dense, np.float64)


def transposed_layout(product, block_rows):
    """[R, m, n] -> [R, m / hd, n, hd]: out[(row / hd) * n * hd + col * hd + row % hd]."""
    r, m, n = product.shape
    return product.reshape(r, m // block_rows, block_rows, n).transpose(0, 1, 3, 2)


# ---------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------
F32, F16, BF16 = "float32", "float16", "bfloat16"
TYPE_PAIRS = ((F16, F16), (BF16, BF16), (F16, F32), (BF16, F32), (F32, F16), (F32, BF16))
SHORT = {F32: "f", F16: "h", BF16: "b"}
PANEL_LABELS = tuple(f"panel<{int(mu)},{int(pe)},{int(to)}>" for mu in (0, 1) for pe in (0, 1) for to in (0, 1))
TYPED_LABELS = tuple(f"typed<{mu},{SHORT[tv]},{SHORT[tb]}>" for mu in (0, 1) for tv, tb in TYPE_PAIRS)
GROUP_LABELS = ("group<0,1,0>", "group<1,0,1>", "group<0,0,1>", "group<0,0,0>")
LABELS = PANEL_LABELS + TYPED_LABELS + GROUP_LABELS
TYPED_MIN_WORK = 1 << 22        # typed_takes_panel: nonzeros * n * replicas, forced or not
DEBUG_NEVER_CUT = 16            # SPUTNIK_HIP_SPMM_DEBUG bit 4


class Run:
    """One call.  entry: "batched" (sputnik_hip_spmm_batched and _bias_batched under the panel
    knob), "permuted", "transposed", "typed", "many" or "group"."""

    def __init__(self, entry, case_name, n, replicas=1, shared=False, perm=False, block_rows=0, bias=False,
                 relu=False, debug=0, types=(F32, F32), group=None, masks=None, heads=0):
        self.entry, self.case_name, self.n, self.replicas, self.shared = entry, case_name, n, replicas, shared
        self.perm, self.block_rows, self.bias, self.relu, self.debug = perm, block_rows, bias, relu, debug
        self.types, self.group, self.masks, self.heads = types, group, masks, heads
        tags = [entry, masks or case_name, f"n{n}", f"r{replicas}{'s' if shared else ''}"]
        tags += ["perm"] if perm else []
        tags += [f"hd{block_rows}"] if block_rows else []
        tags += ["bias"] if bias else []
        tags += ["relu"] if relu else []
        tags += [f"debug{debug}"] if debug else []
        tags += ["".join(SHORT[t] for t in types)] if types != (F32, F32) else []
        if group:
            tags.append(f"g{group['count']}{'same' if group['same_dense'] else 'own'}{'acc' if group['accumulate'] else ''}")
        self.id = "-".join(tags)

    @property
    def case(self):
        """The matrix (group runs: problem 0; many-mask runs: mask 0)."""
        if self.masks:
            return many_mask_cases(self.masks)[0]
        return case(self.case_name)

    def matrices(self):
        if self.masks:
            return many_mask_cases(self.masks)
        if self.group:       # problem 0 is the named matrix, the others group_case 1 ..
            first = self.case
            return [first] + [group_case(first.m, first.k, j, first.placement) for j in range(1, self.group["count"])]
        return [self.case]

    @property
    def identity(self):
        """Rows are the slots: the transposing store and the accumulating group kernel."""
        return bool(self.block_rows) or bool(self.group and self.group["accumulate"])

    @property
    def multi(self):
        return self.case.k > PANEL

    @property
    def label(self):
        if self.entry == "typed":
            return f"typed<{int(self.multi)},{SHORT[self.types[0]]},{SHORT[self.types[1]]}>"
        if self.entry == "group":
            return f"group<{int(self.perm)},{int(bool(self.block_rows))},{int(self.group['accumulate'])}>"
        return f"panel<{int(self.multi)},{int(self.perm)},{int(bool(self.block_rows))}>"

    def knobs(self):
        env = {"SPUTNIK_HIP_SPMM_KERNEL": "panel"}
        if self.debug:
            env["SPUTNIK_HIP_SPMM_DEBUG"] = str(self.debug)
        return env

    def path(self):
        """What the kernel does with the rows: "one" panel, "cut" (two panels, search + check),
        "walk" (the masked walk: three panels and more, DEBUG = 16, every typed MULTI)."""
        if not self.multi:
            return "one"
        if self.entry == "typed" or self.debug & DEBUG_NEVER_CUT or self.case.k > 2 * PANEL:
            return "walk"
        return "cut"


def runs():
    out = []
    add = lambda *a, **kw: out.append(Run(*a, **kw))     # noqa: E731
    # <0,0,0> / <1,0,0> through _batched / _bias_batched under the knob
    for i, m in enumerate((16, 272, 512)):
        add("batched", f"windows:{m},dealt", N_EDGES[i], replicas=(1, 3, 8)[i], shared=i == 1)
    for i, k in enumerate(K_ONE + K_TWO + K_MANY):
        add("batched", f"k:{k}", 64 if k == 4096 else N_EDGES[i % 4], replicas=(3, 1, 8)[i % 3], shared=i % 2 == 0)
    add("batched", "cuts:dealt", 68, replicas=3)
    add("batched", "cuts:dealt", 64, replicas=1, debug=DEBUG_NEVER_CUT)
    add("batched", "partitioned:dealt", 132, replicas=1)
    add("batched", "fallback:one", 64, replicas=3, shared=True)
    add("batched", "fallback:one", 64, replicas=3, shared=True, debug=DEBUG_NEVER_CUT)
    add("batched", "fallback:descending", 68, replicas=8)
    add("batched", "walk:1537", 68, replicas=3)
    add("batched", "walk:4096", 64, replicas=1)
    # <*,1,0>: the permuted entry; three panels at k = 1025 (the _supported query declines them)
    add("permuted", "windows:272,dealt", 68, replicas=3, perm=True)
    add("permuted", "k:4", 64, replicas=1, perm=True)
    add("permuted", "k:512", 132, replicas=8, shared=True, perm=True)
    add("permuted", "cuts:dealt", 64, replicas=1, perm=True)
    add("permuted", "fallback:one", 68, replicas=3, perm=True)
    add("permuted", "k:1025", 64, replicas=3, perm=True)
    add("permuted", "walk:1537", 132, replicas=1, shared=True, perm=True)
    # <*,*,1>: the transposing store
    for i, (m, hd) in enumerate(TRANSPOSED_SHAPES):
        if (m, hd) not in TRANSPOSED_DECLINED:
            add("transposed", f"store:{m},200", 68 if i % 2 else (64, 128, 132)[i % 3], replicas=(1, 3, 8)[i % 3],
                shared=i % 2 == 0, perm=i % 3 == 1, block_rows=hd, bias=i % 2 == 1, relu=i % 4 == 1)
    add("transposed", "windows:320,identity", 68, replicas=3, block_rows=64)
    add("transposed", "windows:512,identity", 64, replicas=1, block_rows=128, perm=True, bias=True, relu=True)
    add("transposed", "cuts:identity", 68, replicas=3, block_rows=CUTS_M)
    add("transposed", "fallback:one,identity", 64, replicas=1, block_rows=64, perm=True)
    add("transposed", "fallback:one,identity", 68, replicas=3, shared=True, block_rows=256, bias=True)
    add("transposed", "store:320,1025", 64, replicas=1, block_rows=64)
    add("transposed", "store:384,1025", 68, replicas=3, block_rows=128, perm=True, bias=True, relu=True)
    # typed: replicas for nonzeros * n * replicas >= 2^22
    for i, (tv, tb) in enumerate(TYPE_PAIRS):
        add("typed", "windows:512,dealt", 132, replicas=8, shared=tb == F32 and i % 2 == 0, types=(tv, tb), bias=i % 2 == 1,
            relu=i % 3 == 0)
        add("typed", "fallback:one", N_EDGES[i % 4] if i % 4 else 128, replicas=8, shared=False, types=(tv, tb))
    add("typed", "walk:1537", 132, replicas=24, types=(F16, F16))
    # groups
    g = lambda count, same, accum: dict(count=count, same_dense=same, accumulate=accum)     # noqa: E731
    add("group", "windows:320,identity", 68, replicas=3, block_rows=64, group=g(2, True, False))
    add("group", "group:512,512,0,identity", 64, replicas=1, block_rows=64, group=g(4, True, False))
    add("group", "group:512,512,0,identity", 132, replicas=8, block_rows=256, group=g(1, True, False))
    add("group", "group:320,5,0,identity", 64, replicas=3, block_rows=64, group=g(2, False, False))
    add("group", "windows:272,identity", 68, replicas=3, perm=True, group=g(4, False, True))
    add("group", "group:512,512,0,identity", 64, replicas=1, perm=True, group=g(2, False, True))
    add("group", "group:272,200,0,identity", 132, replicas=8, group=g(4, False, True))
    add("group", "group:320,5,0,identity", 64, replicas=1, group=g(2, True, True))
    add("group", "group:512,512,0,identity", 68, replicas=3, group=g(1, False, True))
    add("group", "group:272,200,0,dealt", 68, replicas=3, group=g(4, True, False))
    add("group", "group:512,512,0,dealt", 64, replicas=8, group=g(2, False, False))
    add("group", "group:320,5,0,dealt", 132, replicas=1, group=g(1, True, False))
    # many masks: 3 x 2 and 2 x 4 replicas (8: the replicas dealt over the XCDs)
    add("many", None, 64, replicas=6, masks="three", heads=2)
    add("many", None, 68, replicas=8, masks="cuts", heads=4)
    return out


# shapes that must fall OFF the panel route under the knob and still give the product:
# (m, k, n, dense element offset)
OFF_ROUTE = {"m12": (12, 100, 64, 0), "n60": (64, 100, 60, 0), "n66": (64, 100, 66, 0),
             "k4097": (64, MAX_PASSES * PANEL + 1, 64, 0), "dense_unaligned": (64, 100, 64, 1)}


def off_route_case(name):
    m, k, _, _ = OFF_ROUTE[name]
    return from_slots(f"off_{name}", m, k, "dealt", {}, seed=90, fill=(1, 30))


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def operands(mat, n, replicas, shared, seed=0, integers=False):
    """(values [R or 1, nnz], dense [R, k, n], bias [m]) float32.  integers: values of +-1, +-2 and
    dense in -3 .. 3 (exact in float16 and bfloat16; |sum| <= 6 * nnz of a row < 2^24)."""
    rng = np.random.default_rng(3000 + seed)
    vr = 1 if shared else replicas
    if integers:
        values = rng.choice((-2, -1, 1, 2), size=(vr, mat.nnz))
        dense = rng.integers(-3, 4, size=(replicas, mat.k, n))
        bias = rng.integers(-8, 9, size=mat.m)
    else:
        values = rng.uniform(0.1, 1.0, size=(vr, mat.nnz)) * rng.choice((-1, 1), size=(vr, mat.nnz))
        dense = rng.uniform(-1, 1, size=(replicas, mat.k, n))
        bias = rng.uniform(-1, 1, size=mat.m)
    return values.astype(np.float32), dense.astype(np.float32), bias.astype(np.float32)


def permutation(mat, seed=0):
    """A value permutation: entry p takes values[perm[p]]."""
    return np.random.default_rng(4000 + seed + mat.nnz).permutation(mat.nnz).astype(np.int32)
