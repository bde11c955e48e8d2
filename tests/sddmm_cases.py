"""Named masks and runs for the LDS-tiled SDDMM kernels (csrc/sddmm_tiled.hip: the stationary
and the quad kernel, 35 compute instances) and the pair-flat kernel (csrc/sddmm_flat.hip), each
built to put a stated edge of the kernels' hand-made logic in front of them; a numpy model of the
plan (the row in every row slot, row_ok and the chunk table as chunk_table_body<ROWS> writes
them); the float64 reference; and the (instance x case) run list with the knobs, the replica
count and the launch each run means to reach.  numpy only, explicit seeds; no kernel, no oracle.

tests/test_sddmm_cases_cpu.py proves that the cases reach the edges they are named for and that
the run list reaches every instance; tests/test_gpu_sddmm_instances.py runs the list.
"""
import functools

import numpy as np

PER = 256           # mask rows of a row block (kSGroups * kSRows): one workgroup's share
PREFETCHED = 32     # entries of a row and slab that arrive with the row (two windows / 16 pairs)
# with_geometry: slab rows per panel width; the summed form's 256-wide panels also on 80 rows
SLAB_ROWS = {64: 256, 128: 128, 256: 128, 512: 64}
SLAB_HEIGHTS = (256, 128, 80, 64)
SLAB = "slab"       # a count: every column of the slab
# entries of a row in one slab: both sides of `left > 4 / 8 / 12`, of a full window, of the two
# prefetched windows (the quad kernel's 16 pairs), of the first and second on-demand window
COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 31, 32, 33, 47, 48, 49, SLAB)
N_EDGES = 313       # 313 = 256 + 57 = 2 * 128 + 57 = 3 * 80 + 73 = 4 * 64 + 57: 2, 3, 4, 5 slabs,
                    # the last partial and wide enough for 49 entries

CANARY_INT = -7777777
CANARY_HALF = -768.0          # exact in float16 and bfloat16
GUARD = 16                    # canary elements in front of and behind every guarded region


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def dealt_index(slot, slots, per=PER):
    """spmm_tiled_common.h: the entry of row_indices that row slot `slot` holds."""
    return (slot % per) * (slots // per) + slot // per


def slots_of(m, per=PER):
    return ceil_div(m, per) * per


def slot_rows(row_indices, m, per=PER):
    """[slots] the row in every row slot; -1: padding.  `per`: the run of slots the rows are dealt
    in (256 for the SDDMM and the 256- / 512-column SpMM kernels, 128 for the 64-column SpMM)."""
    slots = slots_of(m, per)
    entry = dealt_index(np.arange(slots), slots, per)
    rows = np.full(slots, -1, dtype=np.int64)
    rows[entry < m] = np.asarray(row_indices, np.int64)[entry[entry < m]]
    return rows


def wave_sets(row_indices, m):
    """[slots / 4, 4] the rows (or -1) of the four 16-lane groups that share a wave at one step
    (four consecutive slots of a block): one `longest` each."""
    return slot_rows(row_indices, m).reshape(-1, 4)


def slab_counts(row_offsets, column_indices, n, rows):
    """[m, ceil(n / rows)] entries of each mask row per slab of `rows` columns."""
    ro = np.asarray(row_offsets, np.int64)
    m = len(ro) - 1
    ids = np.repeat(np.arange(m), np.diff(ro))
    out = np.zeros((m, ceil_div(n, rows)), dtype=np.int64)
    np.add.at(out, (ids, np.asarray(column_indices, np.int64) // rows), 1)
    return out


def row_ok_ints(slots):
    """row_ok_bytes / 4: the chunk table starts 256-byte aligned behind the status words."""
    return ceil_div(4 * slots, 256) * 64


def plan_model(row_indices, row_offsets, column_indices, m, n, rows, per=PER):
    """(row_ok [slots], table [(slabs + 1) * slots], defined [like table]) as
    chunk_table_body<rows> writes them: table[c * slots + slot] = position of the first entry of
    the slot's row in a slab >= c (the row's end if none).  A row is ok iff its columns ascend
    strictly and lie in [0, n); padding slots: ok, zeros.  The pre-pass writes every word of an
    ok row once; in a row that is not ok an entry that breaks the order writes nothing and the
    others may write a word twice or never -- `defined` is False there (slab 0 computes such a
    row whole, from global memory, and no slab reads its table words)."""
    ro = np.asarray(row_offsets, np.int64)
    ci = np.asarray(column_indices, np.int64)
    srows = slot_rows(row_indices, m, per)
    slots, slabs = len(srows), ceil_div(n, rows)
    row_ok = np.ones(slots, dtype=np.int32)
    table = np.zeros((slabs + 1, slots), dtype=np.int32)
    writes = np.ones((slabs + 1, slots), dtype=np.int64)
    for slot, row in enumerate(srows):
        if row < 0:
            continue
        writes[:, slot] = 0
        p0, p1 = int(ro[row]), int(ro[row + 1])
        for p in range(p0, p1):
            cur, prev = int(ci[p]), (int(ci[p - 1]) if p > p0 else -1)
            if cur <= prev or cur >= n:
                row_ok[slot] = 0
                continue
            for c in range((prev // rows if prev >= 0 else -1) + 1, cur // rows + 1):
                table[c, slot] = p
                writes[c, slot] += 1
        last = -1
        if p1 > p0:
            lc = int(ci[p1 - 1])
            last = lc // rows if 0 <= lc < n else slabs
        for c in range(last + 1, slabs + 1):
            table[c, slot] = p1
            writes[c, slot] += 1
    defined = (writes == 1) & (row_ok == 1)[None, :]
    return row_ok, table.reshape(-1), defined.reshape(-1)


def workspace_model(row_indices, row_offsets, column_indices, m, n, rows, per=PER):
    """(words, defined) of the front of a plan's workspace: row_ok, then the table."""
    row_ok, table, table_defined = plan_model(row_indices, row_offsets, column_indices, m, n, rows, per)
    first = row_ok_ints(len(row_ok))
    words = np.zeros(first + len(table), dtype=np.int32)
    defined = np.zeros(len(words), dtype=bool)
    words[:len(row_ok)] = row_ok
    defined[:len(row_ok)] = True
    words[first:] = table
    defined[first:] = table_defined
    return words, defined


def reference(row_offsets, column_indices, lhs, rhs, summed=False):
    """float64 [R, nnz] (summed: [nnz]): out[r, p] = lhs[r, row_of(p), :] . rhs[r, col(p), :] on
    the operands as they are stored (half operands: pass the rounded values)."""
    rows = np.repeat(np.arange(len(row_offsets) - 1), np.diff(np.asarray(row_offsets, np.int64)))
    full = np.asarray(lhs, np.float64) @ np.asarray(rhs, np.float64).transpose(0, 2, 1)
    out = full[:, rows, np.asarray(column_indices, np.int64)]
    return out.sum(axis=0) if summed else out


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class Case:
    """CSR (int32) of a dense [m, n] bool mask; row_indices in the named order.  The columns of
    the rows in `reversed_rows` descend, those of `swapped_rows` have one pair exchanged."""

    def __init__(self, name, dense, row_indices, order, reversed_rows=(), swapped_rows=()):
        self.name, self.order = name, order
        dense = np.ascontiguousarray(dense, dtype=bool)
        self.m, self.n = dense.shape
        lengths = dense.sum(axis=1)
        self.row_offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
        ci = np.nonzero(dense)[1].astype(np.int32)
        for r in reversed_rows:
            a, b = self.row_offsets[r], self.row_offsets[r + 1]
            assert b - a >= 2, (name, r)
            ci[a:b] = ci[a:b][::-1].copy()
        for r in swapped_rows:
            a, b = self.row_offsets[r], self.row_offsets[r + 1]
            assert b - a >= 3, (name, r)
            mid = a + (b - a) // 2
            ci[[mid - 1, mid]] = ci[[mid, mid - 1]]
        self.column_indices = ci
        self.unsorted_rows = tuple(int(r) for r in reversed_rows) + tuple(int(r) for r in swapped_rows)
        if row_indices is None:         # what callers pass: longest first, ties by row number
            assert order == "by_length", order
            row_indices = np.argsort(-lengths, kind="stable")
        self.row_indices = np.asarray(row_indices).astype(np.int32)

    @property
    def nnz(self):
        return len(self.column_indices)

    @property
    def csr(self):
        return self.row_indices, self.row_offsets, self.column_indices

    @property
    def row_blocks(self):
        return ceil_div(self.m, PER)

    def counts(self, rows):
        return slab_counts(self.row_offsets, self.column_indices, self.n, rows)

    def block_of_row(self):
        """[m] the row block that holds each row."""
        srows = slot_rows(self.row_indices, self.m)
        block = np.full(self.m, -1, dtype=np.int64)
        block[srows[srows >= 0]] = np.nonzero(srows >= 0)[0] // PER
        return block

    def block_of_row_for(self, per):
        """The same for row blocks of `per` rows (the pair-flat kernel's)."""
        slots = ceil_div(self.m, per) * per
        entry = dealt_index(np.arange(slots), slots, per)
        block = np.full(self.m, -1, dtype=np.int64)
        block[self.row_indices[entry[entry < self.m]]] = np.nonzero(entry < self.m)[0] // per
        return block


def _fill(dense, row, slab, count, rng, n, rows):
    """`count` entries of `row` inside slab `slab` (SLAB: all of it; clipped to its width): a
    random subset that holds the slab's last column for even rows and its first for rows 0, 3, .."""
    lo, hi = slab * rows, min((slab + 1) * rows, n)
    if lo >= n:
        return
    count = hi - lo if count == SLAB else min(count, hi - lo)
    if count == 0:
        return
    cols = np.sort(rng.choice(np.arange(lo, hi), size=count, replace=False))
    if row % 2 == 0:
        cols[-1] = hi - 1
    if row % 3 == 0 and count > 1:
        cols[0] = lo
    dense[row, cols] = True


# positions inside a row block (block 0 and the LAST block, which every walking workgroup
# reaches as a later block): the counts table, the `longest` sets, the unsorted rows
TABLE_AT = {"first": 0, "last": 40}
SETS_AT = {"first": 20, "last": 60}
UNSORTED_AT = {"first": (33,), "last": (80, 81, 82)}
# (slab 0, last slab) of the four rows behind one `longest`: a long row beside a short one, one
# that has entries elsewhere only and one without any; the same around the last slab (rows whose
# entries lie only there); the long row as the fourth of its set (lane 48)
LONGEST_SETS = (((40, 0), (2, 0), (0, 3), (0, 0)),
                ((0, 37), (0, 1), (5, 0), (0, 0)),
                ((0, 0), (1, 0), (0, 2), (45, 0)))
LAST_ROWS = {"last1": 1, "last2": 2, "last33": 33, "last_empty": 0}


def designed_case(name, m, n, rows, order, last, seed):
    """Rows by specification, placed by POSITION in a row block (so that the identity and the
    permuted order put them where the edge needs them; by_length re-sorts and keeps the counts):
      positions 0..18 of block 0     COUNTS[j] entries in slab 0, COUNTS[(j + 7) % 19] in the last
      positions 40..58 of the last   COUNTS[(j + 3) % 19] in slab 0, COUNTS[(j + 11) % 19] in the last
      positions 20.. / 60..          LONGEST_SETS, four consecutive slots each
      position 33 / 80, 81, 82       unsorted rows (12 .. 40 entries over all slabs)
    every other row: random, 0 .. 20 entries in a slab with probability 0.6.  The last row holds
    `last` entries in its last slab (the global last entry of column_indices) or none."""
    rng = np.random.default_rng(seed)
    slabs = ceil_div(n, rows)
    blocks = ceil_div(m, PER)
    if order == "permuted":
        ri = np.random.default_rng(900 + seed).permutation(m)
        while ri[0] == m - 1 or np.nonzero(ri == m - 1)[0][0] // blocks < 90:
            ri = np.roll(ri, 97)        # (the last row is no designed position)
    else:
        ri = np.arange(m)
    entry = lambda block, position: position * blocks + block   # noqa: E731 (dealt_index backwards)
    spec = {}       # entry of row_indices -> (count in slab 0, count in the last slab)
    for which, block in (("first", 0), ("last", blocks - 1)):
        shift = (0, 7) if which == "first" else (3, 11)
        for j in range(len(COUNTS)):
            spec[entry(block, TABLE_AT[which] + j)] = (COUNTS[(j + shift[0]) % 19], COUNTS[(j + shift[1]) % 19])
        for s, four in enumerate(LONGEST_SETS):
            for i, counts in enumerate(four):
                spec[entry(block, SETS_AT[which] + 4 * s + i)] = counts
    unsorted = sorted({entry(0, p) for p in UNSORTED_AT["first"]} |
                      {entry(blocks - 1, p) for p in UNSORTED_AT["last"]})
    assert max(max(spec), max(unsorted)) < m - 1, (name, m)
    dense = np.zeros((m, n), dtype=bool)
    for e in range(m):
        row = int(ri[e])
        if e in spec:
            _fill(dense, row, 0, spec[e][0], rng, n, rows)
            if slabs > 1:
                _fill(dense, row, slabs - 1, spec[e][1], rng, n, rows)
        elif e in unsorted:
            cols = rng.choice(n, size=int(rng.integers(12, min(41, n))), replace=False)
            dense[row, cols] = True
        else:
            for slab in range(slabs):
                if rng.random() < 0.6:
                    _fill(dense, row, slab, int(rng.integers(0, 21)), rng, n, rows)
    dense[m - 1] = False
    if LAST_ROWS[last]:
        _fill(dense, m - 1, slabs - 1, LAST_ROWS[last], rng, n, rows)
        if not dense[m - 1].any():      # (_fill clips to the slab: a last slab of one column)
            dense[m - 1, n - 1] = True
    unsorted_rows = [int(ri[e]) for e in unsorted]
    if order == "by_length":
        # the order follows the lengths: take rows of 12 and more entries that are no designed
        # ones from where the sorted order deals them, one to block 0 and three to the last block
        lengths = dense.sum(axis=1)
        by_length = np.argsort(-lengths, kind="stable")
        free = [(int(e) % blocks, int(r)) for e, r in enumerate(by_length)
                if lengths[r] >= 12 and int(r) not in spec and r != m - 1]
        unsorted_rows = ([r for b, r in free if b == 0][:1] + [r for b, r in free if b == blocks - 1][-3:])
        unsorted_rows = [unsorted_rows[i] for i in (1, 0, 2, 3)]    # (block 0's row among the swapped)
    case = Case(name, dense, None if order == "by_length" else ri, order,
                reversed_rows=unsorted_rows[0::2], swapped_rows=unsorted_rows[1::2])
    case.spec = {int(ri[e]): counts for e, counts in spec.items()}
    case.last = last
    return case


STRUCTURED_KINDS = ("causal", "band", "last_chunk", "heavy_rows_block", "corner")
STRUCTURED_SHAPE = (523, 300)


def structured_case(kind, rows):
    """helpers.structured_csr at three row blocks (tests/test_gpu_structured_masks.py runs the
    kinds at 203 rows); `last_chunk` fills the partial last slab of `rows`."""
    from helpers import structured_mask   # (imports the oracle package: layout code only)
    m, n = STRUCTURED_SHAPE
    dense = structured_mask(kind, m, n, 4, np.random.default_rng(77), chunk=rows)
    return Case(f"{kind}_{m}x{n}", dense, None, "by_length")


# name -> (m, n as a function of the slab height, order, last row, seed); n = rows, rows - 1 and
# rows + 1 at one row block, 313 columns at three, four and six
EDGE_SHAPES = {
    "edges_1283x313_identity_last1": (1283, lambda rows: N_EDGES, "identity", "last1", 1),
    "edges_523x313_by_length_last2": (523, lambda rows: N_EDGES, "by_length", "last2", 2),
    "edges_779x313_permuted_last33": (779, lambda rows: N_EDGES, "permuted", "last33", 3),
    "edges_203xslab+1_identity_last_empty": (203, lambda rows: rows + 1, "identity", "last_empty", 4),
    "edges_203xslab_by_length_last1": (203, lambda rows: rows, "by_length", "last1", 5),
    "edges_203xslab-1_permuted_last2": (203, lambda rows: rows - 1, "permuted", "last2", 6),
}
WALKED_EDGE_CASES = tuple(name for name in EDGE_SHAPES if not name.startswith("edges_203"))
SMALL_CASES = tuple(name for name in EDGE_SHAPES if name.startswith("edges_203")) + ("dense_16x16",)
STRUCTURED_CASES = tuple(f"structured_{kind}" for kind in STRUCTURED_KINDS)
CASE_NAMES = tuple(EDGE_SHAPES) + ("dense_16x16",) + STRUCTURED_CASES


@functools.lru_cache(maxsize=None)
def case(name, rows):
    """The case `name` laid out for slabs of `rows` columns."""
    assert rows in SLAB_HEIGHTS, rows
    if name in ("flat1", "flat2"):
        return flat_case(int(name[4]))
    if name == "dense_16x16":       # the smallest served shape
        return Case(name, np.ones((16, 16), dtype=bool), np.arange(16), "identity")
    if name.startswith("structured_"):
        return structured_case(name[len("structured_"):], rows)
    m, n_of, order, last, seed = EDGE_SHAPES[name]
    return designed_case(name, m, n_of(rows), rows, order, last, seed)


# ---------------------------------------------------------------------------
# instances and runs
# ---------------------------------------------------------------------------
def instances():
    """The 35 instances launch_typed can build: (body, in, out, KV, slab rows, ACC)."""
    out = [("stationary", "float32", "float32", kv, SLAB_ROWS[64 * kv], acc)
           for kv in (1, 2, 4, 8) for acc in (False, True)]
    out += [("stationary", "float32", "float32", 4, 80, False)]
    out += [("quad", "float32", "float32", 1, 256, acc) for acc in (False, True)]
    for t in ("float16", "bfloat16"):
        out += [("quad", t, "float32", kv, SLAB_ROWS[64 * kv], acc) for kv in (1, 2, 4) for acc in (False, True)]
        out += [("quad", t, "float32", 4, 64, acc) for acc in (False, True)]
        out += [("quad", t, "float32", 4, 80, False)]
        out += [("quad", t, t, kv, SLAB_ROWS[64 * kv], False) for kv in (1, 2, 4)]
    return out


WALK = 1 << 20              # SPUTNIK_HIP_SDDMM_DEBUG bits 20..29 = 1: walk from 100 workgroups on
WALK_TARGET = 100
STATIONARY_AT_64 = 8        # the knob's bit that keeps float32 at width 64 off the quad kernel
BASE_KNOBS = {"SPUTNIK_HIP_SDDMM_KERNEL": "tiled", "SPUTNIK_HIP_SDDMM_FLAT": "0"}


class Config:
    """One way of calling: storage types, k, plain or summed, knobs -- and what it launches:
    the family, panel width, slab rows, passes (plain) or panels side by side on grid z (summed),
    and the instances that run (the first pass and, with more passes, the accumulating one)."""

    def __init__(self, in_type, out_type, k, family, width, rows, summed=False, debug=0, slab=0, flat=0):
        self.in_type, self.out_type, self.k, self.family = in_type, out_type, k, family
        self.width, self.rows, self.summed, self.debug, self.slab = width, rows, summed, debug, slab
        self.flat = flat    # SPUTNIK_HIP_SDDMM_FLAT: 0 off, 1 the 256 x 128 tiles, 2 the 128 x 64 ones
        kdim = min(width, 256) if in_type != "float32" else width   # (half: passes of at most 256)
        self.kv = kdim // 64
        self.passes = 1 if summed else k // kdim
        self.panels_on_z = k // kdim if summed else 1
        self.instances = [(family, in_type, out_type, self.kv, rows, False)]
        if self.passes > 1:
            self.instances.append((family, in_type, out_type, self.kv, rows, True))
        self.name = (f"{in_type}_{out_type}_{'sum' if summed else 'plain'}_k{k}_{family}"
                     f"{kdim}x{rows}" + ("_knob8" if debug else "") + (f"_flat{flat}" if flat else ""))

    def knobs(self, walked):
        env = dict(BASE_KNOBS, SPUTNIK_HIP_SDDMM_FLAT=str(self.flat))
        debug = self.debug | (WALK if walked else 0)
        if debug:
            env["SPUTNIK_HIP_SDDMM_DEBUG"] = str(debug)
        if self.slab:
            env["SPUTNIK_HIP_SDDMM_SLAB"] = str(self.slab)
        return env

    def slabs(self, n):
        return ceil_div(n, self.rows)

    def grid_y(self, n, row_blocks, replicas, walked):
        """launch_rows_y under the knob (test shapes stay far below the unforced threshold)."""
        per_y = self.slabs(n) * replicas * self.panels_on_z
        if not walked or per_y * row_blocks <= WALK_TARGET:
            return row_blocks
        return max(1, min(row_blocks, ceil_div(WALK_TARGET, per_y)))

    def replicas_for(self, n, grid_y):
        """Fewest replicas that put the walked grid y at `grid_y`."""
        for replicas in range(1, 200):
            if self.grid_y(n, 1 << 20, replicas, True) == grid_y:
                return replicas
        raise AssertionError((self.name, n, grid_y))


def configs():
    out = []
    # float32: the stationary kernel at width 64 through the knob's bit (one pass, three passes)
    # and through the summed form; its other widths at one pass and at an accumulating one; the
    # 80-row slabs of the summed form; the quad kernel
    out += [Config("float32", "float32", 64, "stationary", 64, 256, debug=STATIONARY_AT_64),
            Config("float32", "float32", 192, "stationary", 64, 256, debug=STATIONARY_AT_64),
            Config("float32", "float32", 192, "stationary", 64, 256, summed=True)]
    for width, k_acc in ((128, 384), (256, 768), (512, 1024)):
        out += [Config("float32", "float32", width, "stationary", width, SLAB_ROWS[width]),
                Config("float32", "float32", k_acc, "stationary", width, SLAB_ROWS[width])]
    out += [Config("float32", "float32", 512, "stationary", 256, 80, summed=True, slab=80)]
    out += [Config("float32", "float32", 64, "quad", 64, 256), Config("float32", "float32", 192, "quad", 64, 256)]
    for t in ("float16", "bfloat16"):
        for width, k_acc in ((64, 192), (128, 384), (256, 768)):
            out += [Config(t, "float32", width, "quad", width, SLAB_ROWS[width]),
                    Config(t, "float32", k_acc, "quad", width, SLAB_ROWS[width])]
        out += [Config(t, "float32", 512, "quad", 512, 64)]             # two passes of 256 on 64-row slabs
        out += [Config(t, "float32", 512, "quad", 256, 80, summed=True, slab=80)]
        out += [Config(t, t, width, "quad", width, SLAB_ROWS[width]) for width in (64, 128, 256)]
    return out


class Run:
    """(config, case) with the replica count and, when walked, the grid y it means to reach."""

    def __init__(self, config, case_name, replicas, walked_y=None):
        self.config, self.case_name, self.replicas, self.walked_y = config, case_name, replicas, walked_y
        self.id = f"{config.name}-{case_name}-r{replicas}" + (f"-y{walked_y}" if walked_y else "")

    @property
    def case(self):
        return case(self.case_name, self.config.rows)

    def launch_shape(self, walked):
        """What capi.sddmm_launch_shape must answer under config.knobs(walked)."""
        c, config = self.case, self.config
        if config.family == "flat":     # (its grid is its plan's: the query reports the family and k)
            return dict(family="flat", panel_width=config.k, slab_rows=0, passes=1, accumulates=False,
                        grid_x=0, grid_y=0, grid_z=0, row_blocks=0)
        return dict(family=config.family, panel_width=64 * config.kv, slab_rows=config.rows,
                    passes=config.passes, accumulates=config.passes > 1, grid_x=config.slabs(c.n),
                    grid_y=config.grid_y(c.n, c.row_blocks, self.replicas, walked),
                    grid_z=self.replicas * config.panels_on_z, row_blocks=c.row_blocks)


# grid y of the walked run of a case: no divisor of the block count, below it, and small enough
# that some workgroup walks two blocks (6 blocks on y = 5: workgroup 0 takes blocks 0 and 5)
WALKED_Y = {"edges_1283x313_identity_last1": 5, "edges_523x313_by_length_last2": 2,
            "edges_779x313_permuted_last33": 3}


def runs():
    """Every config takes every edge case -- the three of several row blocks walked, each with
    the replica count that puts grid y where WALKED_Y says -- and one structured kind in turn
    (walked on y = 2 of 3 blocks).  Grid y = 1 and y = 2 of six blocks once per kernel body."""
    out = []
    for j, config in enumerate(configs()):
        for name in WALKED_EDGE_CASES:
            c = case(name, config.rows)
            out.append(Run(config, name, config.replicas_for(c.n, WALKED_Y[name]), WALKED_Y[name]))
        out += [Run(config, name, 2) for name in SMALL_CASES]
        kind = STRUCTURED_CASES[j % len(STRUCTURED_CASES)]
        out.append(Run(config, kind, config.replicas_for(STRUCTURED_SHAPE[1], 2), 2))
    by_name = {config.name: config for config in configs()}
    for name in ("float32_float32_plain_k128_stationary128x128", "float32_float32_plain_k192_quad64x256",
                 "float16_float32_plain_k192_quad64x256"):
        config = by_name[name]
        for y in (1, 2):
            out.append(Run(config, "edges_1283x313_identity_last1", config.replicas_for(N_EDGES, y), y))
    return out


def largest_operand_bytes(run):
    c, config = run.case, run.config
    elem = 4 if config.in_type == "float32" else 2
    return run.replicas * max(c.m, c.n) * config.k * elem


# ---------------------------------------------------------------------------
# the pair-flat kernel (sddmm_flat.hip): planned masks, rows of 128 or 256 bytes
# ---------------------------------------------------------------------------
# SPUTNIK_HIP_SDDMM_FLAT -> tile (row block x slab), kCap (steps of a round) and compute waves
FLAT_GEOMETRIES = {1: dict(block=256, slab=128, cap=112, compute_waves=15),
                   2: dict(block=128, slab=64, cap=56, compute_waves=7)}
FLAT_STEP = 16          # pair descriptors per step
FLAT_SHAPE = (523, 313)
FLAT_CORNER = "corner"  # a tile whose only entry is column n - 1


def flat_targets(geometry):
    """Steps of one (row block, slab) tile, in turn over the tiles: none, one, fewer than the
    compute waves, one round less one / exactly / plus one, two rounds plus one."""
    g = FLAT_GEOMETRIES[geometry]
    return (0, 1, g["compute_waves"] - 1, g["cap"] - 1, g["cap"], g["cap"] + 1, 2 * g["cap"] + 1)


def flat_tile_targets(geometry):
    """[blocks, slabs] the target of every tile of FLAT_SHAPE; the last tile is the corner."""
    g = FLAT_GEOMETRIES[geometry]
    m, n = FLAT_SHAPE
    blocks, slabs = ceil_div(m, g["block"]), ceil_div(n, g["slab"])
    targets = flat_targets(geometry)
    out = [[targets[(b * slabs + s) % len(targets)] for s in range(slabs)] for b in range(blocks)]
    out[-1][-1] = FLAT_CORNER
    return out


def flat_descriptors(c, geometry):
    """[blocks, slabs] pair descriptors per tile, counted as the kernel's plan counts them
    (sddmm_flat_count_kernel): a row is walked in STORAGE order, (p, p + 1) is a pair when both
    columns lie in one slab, else p goes alone -- the reading taken here of "the step count of
    a tile": steps = ceil(descriptors / 16)."""
    g = FLAT_GEOMETRIES[geometry]
    block, slab = g["block"], g["slab"]
    blocks, slabs = ceil_div(c.m, block), ceil_div(c.n, slab)
    slots = blocks * block
    out = np.zeros((blocks, slabs), dtype=np.int64)
    singles = np.zeros((blocks, slabs), dtype=np.int64)
    for slot in range(slots):
        entry = dealt_index(slot, slots, block)
        if entry >= c.m:
            continue
        row = int(c.row_indices[entry])
        p, p1 = int(c.row_offsets[row]), int(c.row_offsets[row + 1])
        while p < p1:
            s0 = int(c.column_indices[p]) // slab
            pair = p + 1 < p1 and int(c.column_indices[p + 1]) // slab == s0
            out[slot // block, s0] += 1
            singles[slot // block, s0] += 0 if pair else 1
            p += 2 if pair else 1
    return out, singles


def flat_steps(c, geometry):
    return -(-flat_descriptors(c, geometry)[0] // FLAT_STEP)


@functools.lru_cache(maxsize=None)
def flat_case(geometry):
    """523 x 313 under the identity order, every tile of the geometry filled to its target: a
    tile of T steps holds 16 T - 5 descriptors dealt evenly over the block's rows, every other
    row with an odd number of entries there (its last descriptor is a single); rows 5 and 6
    reversed (the pair-flat kernel needs no ascending columns)."""
    g = FLAT_GEOMETRIES[geometry]
    m, n = FLAT_SHAPE
    rng = np.random.default_rng(40 + geometry)
    blocks, slabs = ceil_div(m, g["block"]), ceil_div(n, g["slab"])
    dense = np.zeros((m, n), dtype=bool)
    targets = flat_tile_targets(geometry)
    for b in range(blocks):
        rows = [j * blocks + b for j in range(g["block"]) if j * blocks + b < m]   # (identity order)
        for s in range(slabs):
            lo, hi = s * g["slab"], min((s + 1) * g["slab"], n)
            if targets[b][s] == FLAT_CORNER:
                dense[rows[-1], n - 1] = True
                continue
            if targets[b][s] == 0:
                continue
            descriptors = FLAT_STEP * targets[b][s] - 5
            for i, row in enumerate(rows):
                d = descriptors // len(rows) + (1 if i < descriptors % len(rows) else 0)
                count = 2 * d - (1 if i % 2 == 1 and d > 0 else 0)
                assert count <= hi - lo, (geometry, b, s, count)
                dense[row, rng.choice(np.arange(lo, hi), size=count, replace=False)] = True
    return Case(f"flat{geometry}_{m}x{n}", dense, np.arange(m), "identity", reversed_rows=(5, 6))


def flat_configs():
    """(storage, k) the pair-flat kernel serves, both geometries; planned calls only."""
    out = []
    for flat in (1, 2):
        out += [Config("float32", "float32", 64, "flat", 64, 256, flat=flat),
                Config("float16", "float32", 64, "flat", 64, 256, flat=flat),
                Config("float16", "float16", 128, "flat", 128, 128, flat=flat),
                Config("bfloat16", "bfloat16", 64, "flat", 64, 256, flat=flat),
                Config("bfloat16", "float32", 128, "flat", 128, 128, flat=flat)]
    return out


def flat_runs():
    return [Run(config, f"flat{config.flat}", 3) for config in flat_configs()]


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def operands(run, seed=0, integers=False):
    """(lhs [R, m, k], rhs [R, n, k]) float32: uniform in (-1, 1), or small integers (|x| <= 4,
    exact in every storage type, as are their products and sums at these k)."""
    c, config = run.case, run.config
    rng = np.random.default_rng(1000 + seed)
    if integers:
        lhs = rng.integers(-4, 5, size=(run.replicas, c.m, config.k)).astype(np.float32)
        rhs = rng.integers(-4, 5, size=(run.replicas, c.n, config.k)).astype(np.float32)
    else:
        lhs = rng.uniform(-1, 1, size=(run.replicas, c.m, config.k)).astype(np.float32)
        rhs = rng.uniform(-1, 1, size=(run.replicas, c.n, config.k)).astype(np.float32)
    return lhs, rhs
