"""Models and named matrices for the flat-stream SpMM (csrc/spmm_flat.hip and the three loops that
csrc/gen_spmm_flat.py generates).  Three parts, numpy only, explicit seeds, no kernel, no oracle:

  (a) the PLAN model, written from the text of spmm_flat.hip: the workspace layout of
      make_flat_plan and every byte that spmm_flat_fill_kernel writes there, as (bytes, defined)
      -- a byte the kernel does not write (rounding gaps, the stream area behind the tail
      windows) is not defined and must stay a canary;
  (b) the WALK model of the loops, from the structure of gen_spmm_flat.py: for one wave's stream
      the slot of every boundary, the two counters the vmcnt immediates are picked from, the
      drain path of the entry loop and the (strip, slot) label of every group start and every
      continued entry of the group loops.  The two layouts hold the same N_ and B_ labels and
      differ in where they lie and which path falls through: walk_group follows each layout's
      own placement (the copy of the slot code the program counter is in), the labels are
      counted per layout, and the two walks must pass the same labels in the same order;
  (c) the CASE list: matrices whose rows are placed by POSITION -- row slot = (workgroup, wave,
      wave-row) through dealt_index with runs of 256 -- one design per wave, and the run list.

tests/test_spmm_flat_cases_cpu.py proves that the list reaches what it claims;
tests/test_gpu_spmm_flat_instances.py runs it.
"""
import functools

import numpy as np

import sddmm_cases as S
import spmm_cases as C

ceil_div, dealt_index, slot_rows = S.ceil_div, S.dealt_index, S.slot_rows
CANARY_INT, GUARD = S.CANARY_INT, S.GUARD
reference, row_ok_ints = C.reference, S.row_ok_ints

BN, BK, WAVES, RPW = 512, 32, 16, 8
BM = WAVES * RPW            # 128 row slots per workgroup
AHEAD = 3                   # column groups read ahead
PER = 256                   # run of slots the rows are dealt in
WINDOW, WINDOW_BYTES, TAIL_WINDOWS = 16, 144, 4
NEW_GROUP = 0x80
NSTRIP = 4
MAX_COLUMNS = 65536
STAGE_ALL_OFF = 0x1000      # SPUTNIK_HIP_SPMM_DEBUG: the fill kernel stages nothing in LDS
XCD_FORCED = 0x8000         # SPUTNIK_HIP_SPMM_DEBUG: take the XCD column code from bits 13-14


def up256(v):
    return (v + 255) // 256 * 256


# ---------------------------------------------------------------------------
# (a) the plan
# ---------------------------------------------------------------------------
class Layout:
    """make_flat_plan: row_ok | cinfo[groups][nchunks + 1] | gwin[groups] | stream."""

    def __init__(self, m, k, n, nnz):
        self.slots = ceil_div(m, PER) * PER
        self.nchunks, self.n_tiles, self.groups = ceil_div(k, BK), ceil_div(n, BN), self.slots // RPW
        self.row_ok_off = 0
        self.cinfo_off = 4 * row_ok_ints(self.slots)
        self.gwin_off = up256(self.cinfo_off + 16 * (self.nchunks + 1) * self.groups)
        self.stream_off = up256(self.gwin_off + 4 * self.groups)
        self.windows = nnz // WINDOW + self.groups + TAIL_WINDOWS
        self.bytes = up256(self.stream_off + self.windows * WINDOW_BYTES)


def fill_tables_bytes(nchunks):
    return (4 * (nchunks * (BK // 4 + 4) + 2 * RPW + 2) + 15) // 16 * 16


def fill_stage_windows(nchunks, nnz, groups):
    """Windows of a group's stream that the fill kernel assembles in LDS (0: none)."""
    tables = fill_tables_bytes(nchunks)
    if tables + WINDOW_BYTES > 64 * 1024:
        return 0
    room = (64 * 1024 - tables) // WINDOW_BYTES
    return min(room, nnz // WINDOW // groups * 5 // 4 + TAIL_WINDOWS + 2)


def applicable(m, k, n, nnz):
    """spmm_flat_applicable, on a device that grants the fill kernel its extended LDS."""
    if n < 4 or k < BK or m < 64 or nnz < 16 * m or nnz >= 1 << 29:
        return False
    return ceil_div(n, BN) * BN * 3 <= n * 4 and k <= MAX_COLUMNS and m <= 16384


class Plan:
    """What spmm_flat_fill_kernel leaves in the workspace for (row_indices, row_offsets,
    column_indices): `bytes` uint8 [layout.bytes] and `defined` (False: never written).  Per group
    of eight row slots (one wave's): `ok`, `total` entries, `windows`, `gwin`; per (group, chunk)
    `cgroups` and `centries` as ChunkInfo holds them (zero in a group with a row that is not ok)."""

    def __init__(self, row_indices, row_offsets, column_indices, m, k, n):
        ro, ci = np.asarray(row_offsets, np.int64), np.asarray(column_indices, np.int64)
        self.layout = lay = Layout(m, k, n, len(ci))
        self.m, self.k = m, k
        srows = slot_rows(row_indices, m, PER)
        groups, nchunks = lay.groups, lay.nchunks
        out = np.zeros(lay.bytes, dtype=np.uint8)
        defined = np.zeros(lay.bytes, dtype=bool)
        row_ok = np.ones(lay.slots, dtype=np.int32)
        cinfo = np.zeros((groups, nchunks + 1, 4), dtype=np.uint32)
        self.total = np.zeros(groups, dtype=np.int64)
        self.ok = np.ones(groups, dtype=bool)
        streams = []
        for g in range(groups):
            cols, rows, pos = [], [], []
            for r in range(RPW):
                row = srows[g * RPW + r]
                if row < 0:
                    continue
                p0, p1 = int(ro[row]), int(ro[row + 1])
                c = ci[p0:p1]
                # the order check: every entry against the one before it (-1 in front of the row)
                if p1 > p0 and not ((np.diff(np.concatenate(([-1], c))) > 0).all() and c.max() < k):
                    row_ok[g * RPW + r] = 0
                    self.ok[g] = False
                cols.append(c)
                rows.append(np.full(p1 - p0, r))
                pos.append(np.arange(p0, p1))
            cols, rows, pos = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (cols, rows, pos))
            self.total[g] = len(cols)
            windows = ceil_div(len(cols), WINDOW)
            words = np.zeros((windows, WINDOW_BYTES // 4), dtype=np.uint32)
            if not self.ok[g]:
                words[:, 32:] = 0x80808080      # zero value offsets, every entry a group start
                streams.append(words)
                continue
            order = np.lexsort((rows, cols))
            cols, rows, pos = cols[order], rows[order], pos[order]
            chunk, j = cols // BK, cols % BK
            start = np.concatenate(([True], cols[1:] != cols[:-1])) if len(cols) else np.zeros(0, bool)
            held = cols[start]                                  # the column groups, ascending
            index = np.cumsum(start) - 1                        # column group of every entry
            tile_rows = ((chunk & 1) * BK + j).astype(np.uint32)
            ahead = index + AHEAD
            has = start & (ahead < len(held))
            has[has] &= held[ahead[has]] // BK == chunk[has]     # ... of the same chunk only
            ahead_col = held[np.minimum(ahead, max(len(held) - 1, 0))] if len(held) else ahead
            tile_rows[has] |= (((chunk[has] & 1) * BK + ahead_col[has] % BK) << 8).astype(np.uint32)
            rowbyte = (rows * 8 | np.where(start, NEW_GROUP, 0)).astype(np.uint8)
            as_bytes = words.view(np.uint8).reshape(windows, WINDOW_BYTES)
            as_bytes[:, 128:] = NEW_GROUP                       # unused entries: (0, 0, 0x80)
            at = np.arange(len(cols))
            words[at // WINDOW, 2 * (at % WINDOW)] = tile_rows
            words[at // WINDOW, 2 * (at % WINDOW) + 1] = (4 * pos).astype(np.uint32)
            as_bytes[at // WINDOW, 128 + at % WINDOW] = rowbyte
            streams.append(words)
            for c in range(nchunks):
                mine = held[held // BK == c] % BK
                first = 0
                for q, jj in enumerate(mine[:AHEAD]):
                    first |= ((c & 1) * BK + int(jj)) << (8 * q)
                cinfo[g, c] = (len(mine), first, 0, int(np.count_nonzero(chunk == c)))
        self.windows = np.array([len(w) for w in streams], dtype=np.int64)
        self.gwin = np.concatenate(([0], np.cumsum(self.windows)[:-1])).astype(np.int32)
        tail = np.zeros((TAIL_WINDOWS, WINDOW_BYTES // 4), dtype=np.uint32)
        tail[:, 32:] = 0x80808080
        stream = np.concatenate(streams + [tail]).view(np.uint8).reshape(-1)
        assert len(stream) // WINDOW_BYTES <= lay.windows
        self.cgroups, self.centries = cinfo[:, :nchunks, 0].astype(np.int64), cinfo[:, :nchunks, 3].astype(np.int64)
        self.row_ok, self.cinfo = row_ok, cinfo
        self.stream_windows = len(stream) // WINDOW_BYTES
        for off, part in ((lay.row_ok_off, row_ok.view(np.uint8)), (lay.cinfo_off, cinfo.view(np.uint8).reshape(-1)),
                          (lay.gwin_off, self.gwin.view(np.uint8)), (lay.stream_off, stream)):
            out[off:off + len(part)] = part
            defined[off:off + len(part)] = True
        self.bytes, self.defined = out, defined

    def row_bytes(self, g):
        """The row bytes a wave of group `g` meets from the start of its stream to the end of the
        written stream (what follows its own entries included)."""
        lay = self.layout
        s = self.bytes[lay.stream_off + int(self.gwin[g]) * WINDOW_BYTES:lay.stream_off + self.stream_windows * WINDOW_BYTES]
        return s.reshape(-1, WINDOW_BYTES)[:, 128:].reshape(-1)

    def staged(self, debug=0):
        """[groups] bool: the group's stream is assembled in LDS."""
        lay = self.layout
        stage = fill_stage_windows(lay.nchunks, int(self.total.sum()), lay.groups)
        out_windows = self.windows.copy()
        out_windows[-1] += TAIL_WINDOWS
        return (out_windows <= stage) & (not debug & STAGE_ALL_OFF) & self.ok

    def describe(self, offset):
        """Where a byte offset of the workspace lies, for a failure message."""
        lay = self.layout
        if offset >= lay.stream_off:
            window, rest = divmod(offset - lay.stream_off, WINDOW_BYTES)
            if window >= self.stream_windows:
                return f"stream window {window}: behind the tail windows"
            g = int(np.searchsorted(self.gwin, window, side="right")) - 1
            while g + 1 < lay.groups and self.gwin[g + 1] == window and self.windows[g] == 0:
                g += 1
            where = f"(group {g}, window {window - int(self.gwin[g])}" if window < self.gwin[-1] + self.windows[-1] \
                else f"(tail window {window - int(self.gwin[-1] + self.windows[-1])}"
            if rest >= 128:
                return f"{where}, entry {rest - 128}, row byte)"
            return f"{where}, entry {rest // 8}, {('tile rows', 'value offset')[rest % 8 // 4]} byte {rest % 4})"
        if offset >= lay.gwin_off:
            return f"gwin[{(offset - lay.gwin_off) // 4}]" if offset < lay.gwin_off + 4 * lay.groups else "gap behind gwin"
        if offset >= lay.cinfo_off:
            record, rest = divmod(offset - lay.cinfo_off, 16)
            if record >= lay.groups * (lay.nchunks + 1):
                return "gap behind cinfo"
            return (f"cinfo (group {record // (lay.nchunks + 1)}, chunk {record % (lay.nchunks + 1)}, "
                    f"{('groups', 'first_rows', 'unused', 'entries')[rest // 4]})")
        return f"row_ok[{offset // 4}]" if offset < 4 * lay.slots else "gap behind row_ok"


# ---------------------------------------------------------------------------
# (b) the walks
# ---------------------------------------------------------------------------
class Walk:
    """What one wave passes: `boundaries` [(slot, nsw, copies_pending)] -- nsw = window switches
    since the last boundary, which picks the vmcnt immediate where copies are pending --
    `switches` [sb] (copy batches since the last window switch; the first is the prologue's),
    `drain` (entry loop), `starts` / `continued` [(strip, slot)] (group loops: the N_ and B_
    labels), `consumed` entries."""

    def __init__(self, nchunks):
        self.nchunks, self.c = nchunks, 0
        self.boundaries, self.switches, self.starts, self.continued = [], [], [], []
        self.drain, self.consumed = None, 0
        self.nsw = self.sb = self.mine = 0
        if nchunks >= 2:        # the prologue stages chunk 1
            self.sb = self.mine = 1
        self.switch()

    def switch(self):
        self.switches.append(self.sb)
        self.sb = 0
        self.nsw += 1

    def boundary(self, slot):
        """-> True when the last chunk is done."""
        self.boundaries.append((slot, self.nsw, bool(self.mine)))
        self.c += 1
        if self.c == self.nchunks:
            return True
        self.nsw = self.mine = 0
        if self.c + 1 < self.nchunks:
            self.sb += 1
            self.mine = 1
        return False

    def advance(self):
        self.consumed += 1
        if self.consumed % WINDOW == 0:
            self.switch()

    @property
    def slot(self):
        return self.consumed % WINDOW


def walk_entry(centries):
    """The entry loop over chunks of `centries` entries: E_slot counts the chunk's entries down
    and takes bnd_slot on a borrow; the stub comes back to E_slot, or leaves by drain_(slot % 4)."""
    w = Walk(len(centries))
    rem = int(centries[0])
    while True:
        rem -= 1
        if rem < 0:
            if w.boundary(w.slot):
                w.drain = w.slot % NSTRIP
                return w
            rem = int(centries[w.c])
            continue
        w.advance()


LAYOUTS = ("straight", "diagonal")


def walk_group(cgroups, row_bytes, layout="straight"):
    """A group loop over chunks of `cgroups` column groups: a flagged entry at E_strip_slot goes
    to N_strip_slot, which counts the chunk's groups down and takes bnd_slot on a borrow (the stub
    comes back to N_3_slot); otherwise the reads of the group three ahead go into `strip` and
    strip + 1 becomes current.  An entry without the flag passes B_strip_slot.

    The state that is followed is the COPY of the slot code the program counter is in, as each
    layout places its labels.  "straight": copy r holds E_r_slot and B_r_slot of every slot; a
    group start leaves for N_r_slot and comes back into copy r + 1, a continued entry falls
    through.  "diagonal": copy d holds E_((d + slot) % 4)_slot, falls through N_ of that strip
    into B_((d + slot + 1) % 4)_slot, and a continued entry jumps to its B_ label, which lies in
    copy d - 1; the stub's N_3_slot lies in copy (3 - slot) % 4.  Both start at E_3_0 and come back
    to slot 0 of the same copy behind slot 15."""
    assert layout in LAYOUTS
    straight = layout == "straight"
    w = Walk(len(cgroups))
    rem, copy = int(cgroups[0]), NSTRIP - 1
    while True:
        assert w.consumed < len(row_bytes), "the walk runs off the written stream"
        slot = w.slot
        strip = copy if straight else (copy + slot) % NSTRIP
        if row_bytes[w.consumed] & NEW_GROUP:
            rem -= 1
            if rem < 0:
                if w.boundary(slot):
                    return w
                rem = int(cgroups[w.c])
                copy = NSTRIP - 1 if straight else (NSTRIP - 1 - slot) % NSTRIP
                continue
            w.starts.append((strip, slot))
            if straight:
                copy = (copy + 1) % NSTRIP
        else:
            w.continued.append((strip, slot))
            if not straight:
                copy = (copy - 1) % NSTRIP
        w.advance()


# ---------------------------------------------------------------------------
# (c) wave designs: eight sorted column lists, one per wave-row
# ---------------------------------------------------------------------------
def rows_of(size, start):
    return tuple(sorted((start + i) % RPW for i in range(size)))


def wave_of(k, chunks):
    """chunks: {chunk: [(j, wave-rows)]}: column chunk * 32 + j held by those rows of the wave."""
    cols = [[] for _ in range(RPW)]
    for c, groups in sorted(chunks.items()):
        assert len({j for j, _ in groups}) == len(groups)
        for j, rows in sorted(groups):
            assert 0 <= j < min(BK, k - c * BK), (c, j)
            for r in rows:
                cols[r].append(c * BK + j)
    return cols


SIZES = (2, 1, 3, 1, 4, 2, 8, 5, 6, 7)


def groups_for(k, c, entries, rotate=0):
    """Column groups of chunk `c` that hold `entries` entries: sizes from SIZES in turn (all 8
    where the chunk is too narrow otherwise), at the low columns of an even chunk and the high
    columns of an odd one, so that j = 0 and j = width - 1 are both held."""
    width = min(BK, k - c * BK)
    entries = min(entries, RPW * width)
    sizes, i = [], rotate
    while sum(sizes) < entries:
        sizes.append(min(SIZES[i % len(SIZES)], entries - sum(sizes)))
        i += 1
    if len(sizes) > width:
        full, rest = divmod(entries, RPW)
        sizes = [RPW] * full + ([rest] if rest else [])
    assert len(sizes) <= width, (c, entries)
    first = 0 if c % 2 == 0 else width - len(sizes)
    return [(first + i, rows_of(s, i + c + rotate)) for i, s in enumerate(sizes)]


def by_entries(k, centries, rotate=0):
    return wave_of(k, {c: groups_for(k, c, e, rotate) for c, e in enumerate(centries)})


def by_groups(k, cgroups, size=lambda c, i: 1 + (c + i) % RPW, columns=None):
    """`cgroups[c]` column groups in chunk c, group i of `size(c, i)` rows, spread over the
    chunk's width with its first and last column held (columns(c, count): another choice)."""
    chunks = {}
    for c, count in enumerate(cgroups):
        width = min(BK, k - c * BK)
        count = min(count, width)
        js = columns(c, count) if columns else \
            sorted({round(i * (width - 1) / max(count - 1, 1)) for i in range(count)}) if count > 1 else [width - 1][:count]
        assert len(js) == count, (c, count, js)
        chunks[c] = [(j, rows_of(size(c, i), c + i)) for i, j in enumerate(js)]
    return wave_of(k, chunks)


def random_wave(k, seed):
    """4..12 column groups of 1..8 rows in every chunk: label coverage."""
    rng = np.random.default_rng(seed)
    chunks = {}
    for c in range(ceil_div(k, BK)):
        width = min(BK, k - c * BK)
        js = np.sort(rng.choice(width, size=min(width, int(rng.integers(4, 13))), replace=False))
        chunks[c] = [(int(j), rows_of(int(rng.integers(1, 9)), int(rng.integers(0, 8)))) for j in js]
    return wave_of(k, chunks)


def lengths_wave(k, lengths, seed):
    """Rows of the given lengths (random columns; the first nonempty row holds column k - 1)."""
    rng = np.random.default_rng(seed)
    out, done = [], False
    for length in lengths:
        cols = np.sort(rng.choice(k, size=length, replace=False))
        if length and not done and k - 1 not in cols:
            cols[-1], done = k - 1, True
        out.append(cols.tolist())
    return out


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class Case(C.Case):
    """C.Case with the designs by group (`waves`: group -> design name) and the faults put into
    rows afterwards (`faults`: row -> kind)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.waves, self.faults = {}, {}


FAULTS = ("swap_63_64", "swap_255_256", "dup_63_64", "dup_255_256", "last_only", "column_k")


def apply_fault(case, row, kind):
    ci, p0, p1 = case.column_indices, int(case.row_offsets[row]), int(case.row_offsets[row + 1])
    assert p1 - p0 >= 258, (case.name, row, "a faulty row spans two rounds of 256 entries")
    if kind.startswith("swap"):
        a = p0 + int(kind.split("_")[1])
        ci[[a, a + 1]] = ci[[a + 1, a]]
    elif kind.startswith("dup"):
        a = p0 + int(kind.split("_")[1])
        ci[a + 1] = ci[a]
    elif kind == "last_only":
        ci[p1 - 1] = ci[p1 - 2] - 1
    elif kind == "column_k":
        ci[p1 - 1] = case.k
    else:
        raise KeyError(kind)


def build_case(name, m, k, waves, seed, order="identity", faults=None, fill=(12, 29), top_up=True):
    """`waves`: {group: (design name, eight column lists)} placed at slots 8 group .. 8 group + 7
    (a design may only give empty rows to padding slots).  Every other row: `fill` entries at
    random columns; then, `top_up`, whole rows are filled from the highest free slot down until
    nonzeros >= 16 m + 8.  `faults`: {group: kind}: wave-row 0 of that group gets 260 entries and
    the fault."""
    rng = np.random.default_rng(seed)
    slots = ceil_div(m, PER) * PER
    ri = np.arange(m) if order == "identity" else np.random.default_rng(900 + seed).permutation(m)
    dense = np.zeros((m, k), dtype=bool)
    free, fault_rows = [], {}
    for slot in range(slots):
        entry = int(dealt_index(slot, slots, PER))
        g, r = divmod(slot, RPW)
        design = waves.get(g)
        if entry >= m:
            assert design is None or not design[1][r], (name, slot, "a designed row in a padding slot")
            continue
        row = int(ri[entry])
        if faults and g in faults and r == 0:
            dense[row, rng.choice(k, size=260, replace=False)] = True
            fault_rows[row] = faults[g]
        elif design is not None:
            dense[row, design[1][r]] = True
        else:
            free.append(row)
            dense[row, rng.choice(k, size=min(k, int(rng.integers(*fill))), replace=False)] = True
    need = 16 * m + 8
    for row in reversed(free):
        if not top_up or np.count_nonzero(dense) >= need:
            break
        dense[row] = True
    assert np.count_nonzero(dense) >= need, (name, np.count_nonzero(dense), need)
    case = Case(name, dense, ri.astype(np.int32), order)
    for row, kind in fault_rows.items():
        apply_fault(case, row, kind)
    case.unsorted_rows = tuple(fault_rows)
    case.waves = {g: d[0] for g, d in waves.items()}
    case.faults = fault_rows
    return case


K_MAIN = 352        # 11 chunks, an odd count; rows of up to 352 entries
E = 8               # entries of the chunks around a run of empty ones


def counts_waves(k):
    """Designs by entries per chunk.  Uniform 16 / 17 / 28 / 29 put the 11 boundaries of a wave
    on slots {0}, 1..11, {12, 8, 4, 0}, 13, 10, 7, 4, 1, 14, ..: all 16 between them."""
    nc = ceil_div(k, BK)
    assert nc == 11
    d = {}
    for g, e in enumerate((16, 17, 28, 29)):
        d[g] = (f"uniform_{e}", by_entries(k, [e] * nc, rotate=g))
    # empty chunks: runs of 1, 2, 3 at the start, in the middle, at the end of k
    d[4] = ("empty_start_1", by_entries(k, [0] + [E] * 10))
    d[5] = ("empty_start_2", by_entries(k, [0, 0] + [E + 1] * 9))
    d[6] = ("empty_start_3", by_entries(k, [0, 0, 0] + [E + 2] * 8))
    d[7] = ("empty_middle_1_2_3", by_entries(k, [5, 0, 6, 0, 0, 7, 0, 0, 0, 4, 3]))
    d[8] = ("empty_end_1", by_entries(k, [E] * 10 + [0]))
    d[9] = ("empty_end_2", by_entries(k, [E + 3] * 9 + [0, 0]))
    d[10] = ("empty_end_3", by_entries(k, [E + 5] * 8 + [0, 0, 0]))
    d[11] = ("empty_wave", [[] for _ in range(RPW)])
    # wave totals: every drain path, and a multiple of 16
    for i, total in enumerate((64 + 1, 64 + 2, 64 + 3, 64 + 4, 96)):
        share = [total // nc + (c < total % nc) for c in range(nc)]
        d[12 + i] = (f"total_{total}", by_entries(k, share, rotate=i))
    # three or more window switches between two boundaries; two boundaries between two switches
    d[17] = ("long_chunks", by_entries(k, [49, 64, 3, 50, 0, 81, 48, 1, 65, 2, 52]))
    d[18] = ("short_chunks", by_entries(k, [3, 4, 2, 5, 1, 3, 2, 6, 4, 1, 2]))
    d[19] = ("one_entry", by_entries(k, [0] * 5 + [1] + [0] * 5))
    return d


def groups_waves(k):
    """Designs by column groups per chunk."""
    nc = ceil_div(k, BK)
    d = {}
    # 0, 1, 2, 3, 4, 5, 8, 32 groups: in turn over the chunks, shifted from wave to wave so that
    # each count meets even and odd chunks and every neighbour
    counts = (0, 1, 2, 3, 4, 5, 8, 32)
    for g in range(4):
        d[g] = (f"group_counts_{g}", by_groups(k, [counts[(c * (2 * g + 1) + g) % 8] for c in range(nc)]))
    # group sizes 1..8, one size per wave, 5 groups a chunk
    for s in range(1, 9):
        d[3 + s] = (f"group_size_{s}", by_groups(k, [5] * nc, size=lambda c, i, s=s: s))
    # j = 0 and j = 31 alone; j = 28..31: the read-ahead mask of a group start at the chunk's end
    d[12] = ("first_and_last_column", by_groups(k, [2] * nc, columns=lambda c, n: [0, BK - 1]))
    d[13] = ("last_four_columns", by_groups(k, [4] * nc, columns=lambda c, n: [28, 29, 30, 31]))
    d[14] = ("only_last_column", by_groups(k, [1] * nc, size=lambda c, i: 8, columns=lambda c, n: [BK - 1]))
    # a group whose first entry sits in slot 15: 8 + 7 entries in front of it, in chunk 0
    d[15] = ("start_in_slot_15", wave_of(k, {0: [(0, rows_of(8, 0)), (1, rows_of(7, 0)), (2, rows_of(5, 2)),
                                                 (9, rows_of(1, 3))],
                                             3: [(31, rows_of(8, 0))], 10: [(0, rows_of(3, 1))]}))
    for i in range(8):
        d[16 + i] = (f"random_{i}", random_wave(k, 70 + i))
    return d


def lengths_waves(k):
    """Row lengths for the pre-pass: the round of 256 entries, a lane's four loads (64 apart)."""
    lengths = (0, 1, 63, 64, 65, 255, 256, 257, 320, k)
    d = {}
    for g, length in enumerate(lengths):
        rows = [3, 0, 2, 5, 1, 4, 0, 2]
        rows[g % RPW] = length
        d[g] = (f"row_of_{length}", lengths_wave(k, rows, 40 + g))
    d[10] = ("all_long", lengths_wave(k, [256, 257, 255, 64, 65, 63, 320, 1], 60))
    return d


def staging_waves(k):
    """Eight full rows in one group among short ones: its stream is written straight to memory."""
    return {5: ("eight_full_rows", [list(range(k)) for _ in range(RPW)])}


def spread_waves(k, groups, seed):
    """Long k: rows whose entries span every chunk (one or two a chunk), and a row of every 7th
    column; sparse waves with empty chunks in between."""
    nc = ceil_div(k, BK)
    d = {}
    for g in groups:
        rng = np.random.default_rng(seed + g)
        chunks = {}
        for c in range(nc):
            width = min(BK, k - c * BK)
            if g % 2 and c % 3 == 1:
                continue
            js = np.sort(rng.choice(width, size=min(width, 1 + (c + g) % 3), replace=False))
            chunks[c] = [(int(j), rows_of(1 + (c + i + g) % RPW, c + i)) for i, j in enumerate(js)]
        chunks[nc - 1] = [(min(BK, k - (nc - 1) * BK) - 1, rows_of(8, 0))]      # column k - 1
        d[g] = (f"spread_{g}", wave_of(k, chunks))
    return d


def _extended_k():
    """Smallest k whose fill tables exceed 64 KiB: chunks * 48 + 72 > 65536."""
    nchunks = 1
    while fill_tables_bytes(nchunks) <= 64 * 1024:
        nchunks += 1
    return (nchunks - 1) * BK + 1


EXTENDED_K = _extended_k()      # 43617: 1364 chunks


@functools.lru_cache(maxsize=None)
def case(name):
    k = K_MAIN
    if name == "counts_248x352":            # m = 248: group 31 is eight padding slots
        return build_case(name, 248, k, counts_waves(k), 1)
    if name == "groups_256x352":
        return build_case(name, 256, k, groups_waves(k), 2, order="permuted")
    if name == "lengths_256x352":
        return build_case(name, 256, k, lengths_waves(k), 3)
    if name == "unsorted_a_512x352":        # 64 groups, four blocks of 16: faults in blocks 0, 2, 3
        return build_case(name, 512, k, {}, 4, faults={0: "swap_63_64", 37: "swap_255_256", 63: "dup_63_64"})
    if name == "unsorted_b_512x352":
        return build_case(name, 512, k, {}, 5, order="permuted",
                          faults={0: "dup_255_256", 37: "last_only", 63: "swap_63_64"})
    if name == "unsorted_column_k_256x352":     # plan only
        return build_case(name, 256, k, {}, 6, faults={31: "column_k"})
    if name == "staging_256x352":
        return build_case(name, 256, k, staging_waves(k), 7, fill=(16, 25), top_up=False)
    if name == "long_256x2080":             # 65 chunks
        return build_case(name, 256, 2080, spread_waves(2080, range(0, 32, 3), 100), 8, fill=(14, 40))
    if name == f"extended_64x{EXTENDED_K}":
        return build_case(name, 64, EXTENDED_K, spread_waves(EXTENDED_K, (0, 5), 200), 9, fill=(14, 30))
    if name == "groups544_4100x64":         # 4352 slots, 544 groups, 252 padding slots in the last run
        return build_case(name, 4100, 64, {}, 10, order="permuted", fill=(10, 30))
    if name.startswith("kedge_256x"):
        kk = int(name.split("x")[1])
        d = {0: ("group_counts", by_groups(kk, [(5, 32, 1, 3)[c % 4] for c in range(ceil_div(kk, BK))])),
             1: ("entries", by_entries(kk, [17, 29][:ceil_div(kk, BK)])),
             2: ("last_column", wave_of(kk, {ceil_div(kk, BK) - 1: [((kk - 1) % BK, rows_of(8, 0))]}))}
        return build_case(name, 256, kk, d, 11 + kk, fill=(10, min(kk, 30)))
    if name.startswith("map_"):             # map_<m>x64
        mm = int(name[4:].split("x")[0])
        return build_case(name, mm, 64, {0: ("random", random_wave(64, 5))}, 12 + mm, order="permuted", fill=(12, 30))
    raise KeyError(name)


CASE_NAMES = ("counts_248x352", "groups_256x352", "lengths_256x352", "unsorted_a_512x352", "unsorted_b_512x352",
              "unsorted_column_k_256x352", "staging_256x352", "long_256x2080", f"extended_64x{EXTENDED_K}",
              "groups544_4100x64", "kedge_256x32", "kedge_256x33", "kedge_256x63", "kedge_256x64", "kedge_256x65",
              "map_1024x64", "map_256x64")


@functools.lru_cache(maxsize=None)
def plan(name, n, other_order=False):
    c = case(name)
    ri = c.other_order() if other_order else c.row_indices
    return Plan(ri, c.row_offsets, c.column_indices, c.m, c.k, n)


# ---------------------------------------------------------------------------
# what a case puts in front of the code: edge labels, recounted from the plan model by the walks
# ---------------------------------------------------------------------------
def clamp(v, top):
    return min(int(v), top)


@functools.lru_cache(maxsize=None)
def edges(name, n=384):
    """frozenset of edge labels of case `name`, over the waves of its staged (all-ok) blocks:
      ("boundary", loop, slot) ("drain", path) ("nsw", loop, 0..3) ("sb", loop, 0..2)
      ("start", layout, strip, slot) ("continued", layout, strip, slot)
      (loop: "entry" / "group"; layout: "straight" / "diagonal")
      ("chunk_groups", count) ("group_size", rows) ("chunk_parity", 0 / 1) ("column_j", 0 / 31)
      ("empty_run", place, length) ("empty_wave", "rows" / "padding") ("ends_on_switch",)
      ("total_multiple_of_16",) ("start_in_slot_15_continues",) ("row_length", v) ("column_k_1",)
      ("fault", kind, place) ("staged", bool) ("chunks", n) ("groups_over_512",) ("padding_slots",)
      ("written_straight_beside_staged",)"""
    c, p = case(name), plan(name, n)
    lay = p.layout
    out = {("chunks", lay.nchunks)}
    block_ok = p.ok.reshape(-1, WAVES).all(axis=1)
    srows = slot_rows(c.row_indices, c.m, PER)
    lengths = np.diff(c.row_offsets.astype(np.int64))
    if lay.groups > 512:
        out.add(("groups_over_512",))
    if (srows < 0).any():
        out.add(("padding_slots",))
    for staged in np.unique(p.staged()[p.ok]):
        out.add(("staged", bool(staged)))
    if {("staged", False), ("staged", True)} <= out:
        out.add(("written_straight_beside_staged",))
    for row, kind in c.faults.items():
        g = int(np.nonzero(srows == row)[0][0]) // RPW
        out.add(("fault", kind, "first" if g == 0 else "last" if g == lay.groups - 1 else "middle"))
    for g in range(lay.groups):
        if not block_ok[g // WAVES]:
            continue
        rows = srows[g * RPW:(g + 1) * RPW]
        out |= {("row_length", int(lengths[r])) for r in rows if r >= 0}
        if any(r >= 0 and lengths[r] and c.column_indices[c.row_offsets[r + 1] - 1] == c.k - 1 for r in rows):
            out.add(("column_k_1",))
        ce, cg = p.centries[g], p.cgroups[g]
        if p.total[g] == 0:
            out.add(("empty_wave", "padding" if (rows < 0).all() else "rows"))
        elif p.total[g] % WINDOW == 0:
            out.add(("total_multiple_of_16",))
        # runs of empty chunks
        c0 = 0
        while c0 < lay.nchunks and p.total[g]:
            if ce[c0]:
                c0 += 1
                continue
            c1 = c0
            while c1 < lay.nchunks and ce[c1] == 0:
                c1 += 1
            place = "start" if c0 == 0 else "end" if c1 == lay.nchunks else "middle"
            out.add(("empty_run", place, clamp(c1 - c0, 3)))
            c0 = c1
        ends = np.cumsum(ce)
        if ((ends % WINDOW == 0) & (ce > 0)).any():
            out.add(("ends_on_switch",))
        out |= {("chunk_groups", int(v)) for v in np.unique(cg)}
        out |= {("chunk_parity", int(ch % 2)) for ch in np.nonzero(ce)[0]}
        rb = p.row_bytes(g)
        mine = rb[:int(p.total[g])]
        starts = np.nonzero(mine & NEW_GROUP)[0]
        out |= {("group_size", int(s)) for s in np.unique(np.diff(np.concatenate((starts, [len(mine)]))))} if len(mine) else set()
        sizes = np.diff(np.concatenate((starts, [len(mine)])))
        if ((starts % WINDOW == WINDOW - 1) & (sizes > 1)).any():
            out.add(("start_in_slot_15_continues",))
        at = lay.stream_off + int(p.gwin[g]) * WINDOW_BYTES
        stream = p.bytes[at:at + int(p.windows[g]) * WINDOW_BYTES].reshape(-1, WINDOW_BYTES)
        own = stream[:, 0:128:8].reshape(-1)[:len(mine)] % BK
        out |= {("column_j", int(j)) for j in (0, BK - 1) if (own == j).any()}
        we, wg, wd = walk_entry(ce), walk_group(cg, rb, "straight"), walk_group(cg, rb, "diagonal")
        assert (wg.starts, wg.continued, wg.boundaries, wg.switches) == (wd.starts, wd.continued, wd.boundaries, wd.switches), \
            (name, g, "the two layouts pass other labels")
        assert we.consumed == wg.consumed == p.total[g], (name, g, we.consumed, wg.consumed, int(p.total[g]))
        assert [b[0] for b in we.boundaries] == [b[0] for b in wg.boundaries], (name, g)
        out.add(("drain", we.drain))
        for loop, w in (("entry", we), ("group", wg)):
            out |= {("boundary", loop, slot) for slot, _, _ in w.boundaries}
            out |= {("nsw", loop, clamp(nsw, 3)) for _, nsw, pending in w.boundaries if pending}
            out |= {("sb", loop, clamp(sb, 2)) for sb in w.switches}
        for layout, w in (("straight", wg), ("diagonal", wd)):
            out |= {("start", layout) + label for label in w.starts}
            out |= {("continued", layout) + label for label in w.continued}
    return frozenset(out)


ALL_LABELS = {(kind, layout, s, e) for kind in ("start", "continued") for layout in LAYOUTS
              for s in range(NSTRIP) for e in range(WINDOW)}

# What each case is in the list for: the edges it must show by itself.  (test_spmm_flat_cases_cpu
# holds every case to its claims, and the whole list to REQUIRED.)
CLAIMS = {
    "counts_248x352":
        {("boundary", loop, s) for loop in ("entry", "group") for s in range(WINDOW)} |
        {("drain", d) for d in range(NSTRIP)} |
        {("nsw", loop, v) for loop in ("entry", "group") for v in range(4)} |
        {("sb", loop, v) for loop in ("entry", "group") for v in range(3)} |
        {("empty_run", place, v) for place in ("start", "middle", "end") for v in (1, 2, 3)} |
        {("empty_wave", "rows"), ("empty_wave", "padding"), ("ends_on_switch",), ("total_multiple_of_16",),
         ("padding_slots",), ("chunks", 11)},
    "groups_256x352":
        ALL_LABELS | {("chunk_groups", v) for v in (0, 1, 2, 3, 4, 5, 8, 32)} |
        {("group_size", v) for v in range(1, 9)} | {("column_j", 0), ("column_j", 31), ("chunk_parity", 0),
                                                     ("chunk_parity", 1), ("start_in_slot_15_continues",)},
    "lengths_256x352":
        {("row_length", v) for v in (0, 1, 63, 64, 65, 255, 256, 257, 320, 352)} | {("column_k_1",)},
    "unsorted_a_512x352": {("fault", "swap_63_64", "first"), ("fault", "swap_255_256", "middle"),
                           ("fault", "dup_63_64", "last")},
    "unsorted_b_512x352": {("fault", "dup_255_256", "first"), ("fault", "last_only", "middle"),
                           ("fault", "swap_63_64", "last")},
    "unsorted_column_k_256x352": {("fault", "column_k", "last")},
    "staging_256x352": {("staged", False), ("staged", True), ("written_straight_beside_staged",)},
    "long_256x2080": {("chunks", 65), ("staged", True)},
    f"extended_64x{EXTENDED_K}": {("chunks", ceil_div(EXTENDED_K, BK)), ("staged", False)},
    "groups544_4100x64": {("groups_over_512",), ("padding_slots",), ("chunks", 2)},
    "kedge_256x32": {("chunks", 1), ("chunk_groups", 32)},
    "kedge_256x33": {("chunks", 2), ("k", 33)},
    "kedge_256x63": {("k", 63)},
    "kedge_256x64": {("k", 64)},
    "kedge_256x65": {("chunks", 3), ("k", 65)},
    "map_1024x64": {("row_blocks", 8)},
    "map_256x64": {("row_blocks", 2)},
}


def case_edges(name):
    c = case(name)
    return edges(name) | {("k", c.k), ("row_blocks", ceil_div(c.m, PER) * PER // BM)}


# ---------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------
class Run:
    """One (case, n, replicas, values, knob) combination.  `debug`: SPUTNIK_HIP_SPMM_DEBUG (bits
    12-15 only: the low bits are timing experiments that skip copies, barriers and waits);
    `plan_only`: no product is launched; `wide512`: n is a multiple of 4, so the visit-per-row
    512-column kernel serves the same operands and must give the same bits."""

    def __init__(self, case_name, n, replicas=1, shared=True, debug=0, plan_only=False):
        assert debug & ~0xf000 == 0
        self.case_name, self.n, self.replicas, self.shared = case_name, n, replicas, shared
        self.debug, self.plan_only = debug, plan_only
        self.wide512 = n % 4 == 0 and not plan_only
        self.id = (f"{case_name}-n{n}-r{replicas}{'s' if shared else ''}" + (f"-debug{debug:#x}" if debug else "") +
                   ("-plan_only" if plan_only else ""))

    @property
    def case(self):
        return case(self.case_name)

    def knobs(self, loop=None):
        env = {"SPUTNIK_HIP_SPMM_KERNEL": "flat"}
        if self.debug:
            env["SPUTNIK_HIP_SPMM_DEBUG"] = str(self.debug)
        if loop is not None:
            env["SPUTNIK_HIP_SPMM_SPARSE"] = str(2 + loop)
        return env

    @property
    def n_tiles(self):
        return ceil_div(self.n, BN)

    def mapping(self):
        """The workgroup-to-tile mapping spmm_flat_kernel takes: "xcd<code>", "eighths", "linear"."""
        code = (self.debug >> 13) & 3 if self.debug & XCD_FORCED else 0
        grid_x = ceil_div(self.case.m, PER) * PER // BM * self.n_tiles
        if code and self.n_tiles == 8 and (grid_x // 8) % (1 << code) == 0:
            return f"xcd{code}"
        return "eighths" if self.n_tiles % 8 == 0 else "linear"

    def grid_total(self):
        return ceil_div(self.case.m, PER) * PER // BM * self.n_tiles * self.replicas


def xcd(code):
    return XCD_FORCED | code << 13


def runs():
    ext = f"extended_64x{EXTENDED_K}"
    out = [
        # the designs; n_tiles = 1 and 3 with 1, 3, 4 replicas (grid totals 2 6 8 / 6 18 24)
        Run("counts_248x352", 384, 1), Run("counts_248x352", 1153, 3, shared=False),
        Run("groups_256x352", 384, 3, shared=False), Run("groups_256x352", 1155, 4),
        Run("lengths_256x352", 384, 4, shared=False), Run("lengths_256x352", 1152, 1),
        Run("unsorted_a_512x352", 512, 1), Run("unsorted_b_512x352", 771, 3, shared=False),
        Run("unsorted_column_k_256x352", 384, plan_only=True),
        Run("staging_256x352", 512, 1), Run("staging_256x352", 512, debug=STAGE_ALL_OFF, plan_only=True),
        Run("long_256x2080", 384, 1), Run(ext, 384, 1), Run("groups544_4100x64", 384, 1),
        # k edges x n edges
        Run("kedge_256x32", 384, 1), Run("kedge_256x33", 510, 3), Run("kedge_256x63", 512, 1, shared=False),
        Run("kedge_256x64", 768, 1), Run("kedge_256x65", 771, 4, shared=False),
        # mappings: eight column tiles under the XCD codes, sixteen
        Run("map_1024x64", 3588, debug=xcd(0)), Run("map_1024x64", 3588, debug=xcd(1)),
        Run("map_1024x64", 3588, debug=xcd(2)), Run("map_1024x64", 3588, debug=xcd(3)),
        Run("map_256x64", 3588, debug=xcd(2)), Run("map_256x64", 7684, 1),
    ]
    return out


# runs that must fall OFF the flat route under the knob: (m, k, n, nonzeros)
OFF_ROUTE = {"k_below_a_chunk": (256, 31, 384, 4200), "k_above_the_column_masks": (256, MAX_COLUMNS + 1, 384, 4200),
             "n_513": (256, 352, 513, 4200)}

# the budget of tests/test_gpu_spmm_flat_instances.py (held by test_spmm_flat_cases_cpu)
MAX_RUNS = 28
MAX_OPERAND_BYTES = 72 << 20         # the dense operand of the extended-LDS case: 43617 x 384 floats
MAX_REFERENCE_FLOPS = 3e10           # float64 multiply-adds of all references together

STRIDE_PAD = 3      # elements between replicas: strides of k * n + 3 and m * n + 3
OUT_OFFSET = 1      # `out` one float past 16-byte alignment


def reference_from_entries(c, values, dense):
    """float64 [R, m, n] from the entries alone (no dense [m, k] image): a long k stays cheap."""
    ro = c.row_offsets.astype(np.int64)
    out = np.zeros((dense.shape[0], c.m, dense.shape[2]))
    for r in range(dense.shape[0]):
        v = values[0 if values.shape[0] == 1 else r].astype(np.float64)
        for row in range(c.m):
            p0, p1 = ro[row], ro[row + 1]
            out[r, row] = v[p0:p1] @ dense[r, c.column_indices[p0:p1]].astype(np.float64)
    return out


def operands(run, integers=False, seed=0):
    """(values [R or 1, nnz], dense [R, k, n], bias [m]) float32, as spmm_cases.operands."""
    c = run.case
    rng = np.random.default_rng(3000 + seed)
    vr = 1 if run.shared else run.replicas
    if integers:
        values = rng.integers(1, 4, size=(vr, c.nnz)) * rng.choice((-1, 1), size=(vr, c.nnz))
        dense = rng.integers(-4, 5, size=(run.replicas, c.k, run.n))
        bias = rng.integers(-8, 9, size=c.m)
    else:
        values = rng.uniform(0.1, 1.0, size=(vr, c.nnz)) * rng.choice((-1, 1), size=(vr, c.nnz))
        dense = rng.random(size=(run.replicas, c.k, run.n), dtype=np.float32) * 2 - 1
        bias = rng.uniform(-1, 1, size=c.m)
    return values.astype(np.float32), dense.astype(np.float32), bias.astype(np.float32)


def from_entries(c):
    """The reference walks the entries: a long k stays cheap, and a duplicate column counts as
    the two entries it is (the dense image would hold one)."""
    return c.k > 4096 or bool(c.faults)


def expected(run, values, dense):
    c = run.case
    if from_entries(c):
        return reference_from_entries(c, values, dense)
    return reference(c.row_offsets, c.column_indices, values, dense)


def reference_flops(run):
    c = run.case
    return run.replicas * run.n * (c.nnz if from_entries(c) else c.m * c.k)
