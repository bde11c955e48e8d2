"""Named CSR patterns for the transpose (csrc/transpose.hip), one per piece of launch code that
a uniform random mask does not reach, and the reference they are held to.  numpy only, explicit
seeds, no dense m x n array for the large cases: a pattern is a set of linear indices
row * n + column.

Every case states the route it means to reach (what capi.csr_transpose_route must answer) and
the promises that make it reach the code behind that route (row lengths, column counts); the
CPU tests check both, the GPU tests run the kernels.
"""
import functools

import numpy as np

CANARY_INT = -7777777          # never a row id, an offset or a source index
CANARY_FLOAT = -12345.0        # the values are drawn from (1, 2)
GUARD = 16                     # elements behind every output that must keep the canary


class Case:
    """One topology: m, n, row_offsets [m + 1] and column_indices [nnz] (int32), the route it
    means to reach and its promises (checked by tests/test_transpose_cases_cpu.py)."""

    def __init__(self, name, m, n, row_offsets, column_indices, route, promises=None):
        self.name, self.m, self.n = name, m, n
        self.row_offsets = np.ascontiguousarray(row_offsets, dtype=np.int32)
        self.column_indices = np.ascontiguousarray(column_indices, dtype=np.int32)
        self.route = route
        self.promises = promises or {}
        assert self.row_offsets.shape == (m + 1,) and self.row_offsets[0] == 0
        assert self.row_offsets[-1] == len(self.column_indices)

    @property
    def nnz(self):
        return len(self.column_indices)

    @property
    def row_lengths(self):
        return np.diff(self.row_offsets.astype(np.int64))

    @property
    def column_counts(self):
        return np.bincount(self.column_indices, minlength=self.n)

    def values(self, replicas=1, seed=0):
        """[replicas, nnz] float32 in (1, 2): no two alike within a replica as far as float32
        allows, never the canary."""
        rng = np.random.default_rng(1000 + seed)
        return (1.0 + rng.random((replicas, self.nnz))).astype(np.float32)


def reference(row_offsets, column_indices, n):
    """(out_row_offsets [n + 1], out_column_indices [nnz], permutation [nnz]) of the stable
    transpose: output slot i holds source entry permutation[i]; values_t = values[..., perm]."""
    row_offsets = np.asarray(row_offsets, np.int64)
    column_indices = np.asarray(column_indices, np.int64)
    rows = np.repeat(np.arange(len(row_offsets) - 1), np.diff(row_offsets))
    perm = np.argsort(column_indices, kind="stable")
    out_ro = np.concatenate(([0], np.cumsum(np.bincount(column_indices, minlength=n))))
    return out_ro.astype(np.int32), rows[perm].astype(np.int32), perm.astype(np.int32)


def case_reference(case):
    return reference(case.row_offsets, case.column_indices, case.n)


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------
def _linear(rows, cols, n):
    return np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64)


def _random_linear(m, n, count, rng, columns=None):
    """`count` distinct linear indices drawn uniformly (from the given columns only, if any)."""
    width = n if columns is None else len(columns)
    assert count <= m * width
    found = np.zeros(0, np.int64)
    while len(found) < count:
        draw = rng.integers(0, m * width, size=int((count - len(found)) * 1.2) + 16)
        found = np.union1d(found, draw)
    found = np.sort(rng.permutation(found)[:count])
    if columns is None:
        return found
    return _linear(found // width, np.asarray(columns, np.int64)[found % width], n)


def _csr(m, n, linear, shuffle_rows=(), seed=0):
    """CSR of a set of linear indices, columns ascending inside a row except in `shuffle_rows`
    (order inside a row is free for the transpose)."""
    linear = np.unique(np.asarray(linear, np.int64))
    rows, cols = linear // n, (linear % n).astype(np.int32)
    row_offsets = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=m)))).astype(np.int32)
    rng = np.random.default_rng(77 + seed)
    for r in shuffle_rows:
        a, b = int(row_offsets[r]), int(row_offsets[r + 1])
        cols[a:b] = cols[a:b][rng.permutation(b - a)]
    return row_offsets, cols


def _rows_of_lengths(n, lengths, rng):
    """Linear indices of rows with the given {row: length}, columns drawn without replacement."""
    return np.concatenate([_linear(r, rng.choice(n, size=k, replace=False), n)
                           for r, k in lengths.items()] + [np.zeros(0, np.int64)])


GROUPED = {"path": "grouped", "ranges": 1, "parts": -1, "long_rank_launch": -1}
WIDE = {"path": "wide", "groups": -1, "long_rank_launch": -1}
SPARSE = {"path": "sparse", "chunks": -1, "ranges": -1, "groups": -1, "parts": -1,
          "scan_chunks_per_group": -1}


# ---------------------------------------------------------------------------
# grouped tables (n <= 8192)
# ---------------------------------------------------------------------------
LONG_ROWS = {31: 1100, 3: 513, 4: 512, 5: 511, 6: 1, 7: 0, 33: 1100, 36: 600, 39: 513}


def _long_rows():
    """Rows past the mask kernel's first 8 x 64 entries: its "rest" loop, in row 31 (the last
    bit of a chunk's masks) and in the ragged second chunk; every row's columns shuffled, so
    what lies past the 512th entry is not just the high columns."""
    m, n = 40, 1100
    rng = np.random.default_rng(11)
    lengths = {r: int(rng.integers(20, 40)) for r in range(m)}
    lengths.update(LONG_ROWS)
    ro, ci = _csr(m, n, _rows_of_lengths(n, lengths, rng), shuffle_rows=range(m), seed=1)
    return Case("long_rows", m, n, ro, ci, dict(GROUPED, chunks=2, groups=8, scan_chunks_per_group=1),
                {"row_lengths": LONG_ROWS})


def _stage_overflow_linear(n, rng, rows0=0):
    """Chunk of 32 rows from rows0 dense in columns 0..255 (8192 entries in one chunk x column
    group: twice the staging area), the next chunk at density 0.05."""
    dense = _linear(np.repeat(np.arange(rows0, rows0 + 32), 256), np.tile(np.arange(256), 32), n)
    light = _random_linear(32, n, int(0.05 * 32 * n), rng) + (rows0 + 32) * n
    return np.concatenate([dense, light])


def _stage_overflow():
    m, n = 64, 300
    rng = np.random.default_rng(12)
    tail = _random_linear(32, n, 70, rng, columns=np.arange(256, n))     # chunk 0, second group
    ro, ci = _csr(m, n, np.concatenate([_stage_overflow_linear(n, rng), tail]),
                  shuffle_rows=range(0, m, 3), seed=2)
    return Case("stage_overflow", m, n, ro, ci, dict(GROUPED, chunks=2, groups=8, scan_chunks_per_group=1),
                {"chunk_group_entries": {(0, 0): 8192}, "chunk_group_at_most": {(1, 0): 4096}})


FULL_COLUMNS = (0, 255, 256, 519)


def _full_columns():
    """Columns held by every row (mask word 0xffffffff; row 31 ranks below 2^31 - 1 others) at
    both edges of a column group, a run of empty columns across the rest of a group, a chunk
    that holds nothing else between two that do."""
    m, n = 96, 520
    rng = np.random.default_rng(13)
    full = _linear(np.repeat(np.arange(m), 4), np.tile(FULL_COLUMNS, m), n)
    free = np.setdiff1d(np.concatenate([np.arange(1, 255), np.arange(512, 519)]), FULL_COLUMNS)
    top = _random_linear(32, n, 800, rng, columns=free)
    bottom = _random_linear(32, n, 800, rng, columns=free) + 64 * n
    ro, ci = _csr(m, n, np.concatenate([full, top, bottom]))
    return Case("full_columns", m, n, ro, ci, dict(GROUPED, chunks=3, groups=8, scan_chunks_per_group=1),
                {"column_counts": {c: m for c in FULL_COLUMNS}, "empty_columns": (257, 512),
                 "row_lengths": {r: 4 for r in range(32, 64)}})


def _tall_scan(m):
    """More than 8 chunks per group of the table scan (its loops from ch0 + kKeep on), the last
    group short or empty, n no multiple of the scan block's 64 columns.  Ten times the entries
    that keep the shape on the tables."""
    n = 70
    chunks = -(-m // 32)
    rng = np.random.default_rng(14 + m)
    count = 10 * -(-chunks * n // 8)
    ro, ci = _csr(m, n, _random_linear(m, n, count, rng))
    per_group = -(-chunks // 16)
    return Case(f"tall_scan_{m}", m, n, ro, ci,
                dict(GROUPED, chunks=chunks, groups=8, scan_chunks_per_group=per_group),
                {"nnz": count})


def _widest_grouped():
    """n = 8192: 32 column groups, the slot bases of the last group summed over 7936 earlier
    columns; entries in columns 0 and 8191 and around every multiple of 256."""
    m, n = 64, 8192
    rng = np.random.default_rng(15)
    edges = np.unique(np.clip(np.concatenate([np.arange(0, n + 1, 256) + d for d in (-1, 0, 1)]), 0, n - 1))
    held = _random_linear(m, n, m * len(edges) // 2, rng, columns=edges)
    ends = _linear(np.repeat(np.arange(0, m, 2), 2), np.tile([0, n - 1], m // 2), n)
    others = _random_linear(m, n, 600, rng)
    ro, ci = _csr(m, n, np.concatenate([held, ends, others]))
    return Case("widest_grouped", m, n, ro, ci, dict(GROUPED, chunks=2, groups=32, scan_chunks_per_group=1),
                {"held_columns": (0, n - 1, 255, 256, 257, 7935, 7936, 7937)})


# ---------------------------------------------------------------------------
# wide tables (n > 8192): totals scan + plain scatter
# ---------------------------------------------------------------------------
def _wide(name, m, n, parts, long_rows, seed):
    """Just over the entries that keep the shape on the tables, a few rows longer than the
    8 x 64 entries of one batch, entries in the first and last column of every range."""
    chunks, ranges = -(-m // 32), -(-n // 8192)
    rng = np.random.default_rng(seed)
    count = -(-chunks * n // 8) + 64
    ends = np.unique(np.concatenate([[r * 8192, min(n, (r + 1) * 8192) - 1] for r in range(ranges)]))
    edge = _linear(np.repeat(np.arange(0, m, 7), len(ends)), np.tile(ends, len(range(0, m, 7))), n)
    long_ = _rows_of_lengths(n, long_rows, rng)
    fixed = np.union1d(edge, long_)
    linear = np.union1d(fixed, _random_linear(m, n, count, rng))
    ro, ci = _csr(m, n, linear, shuffle_rows=list(long_rows), seed=seed)
    return Case(name, m, n, ro, ci,
                dict(WIDE, chunks=chunks, ranges=ranges, parts=parts,
                     scan_chunks_per_group=-(-chunks // 16)),
                {"held_columns": tuple(int(c) for c in ends), "min_row_lengths": long_rows})


def _range_of_one():
    """n = 8193: the second column range is one column wide."""
    m, n = 64, 8193
    rng = np.random.default_rng(21)
    last = _linear(np.arange(0, m, 2), n - 1, n)
    ro, ci = _csr(m, n, np.union1d(last, _random_linear(m, n, 3000, rng)))
    return Case("range_of_one", m, n, ro, ci,
                dict(WIDE, chunks=2, ranges=2, parts=8, scan_chunks_per_group=1),
                {"held_columns": (n - 1,), "min_column_counts": {n - 1: m // 2}})


# ---------------------------------------------------------------------------
# O(n + nnz)
# ---------------------------------------------------------------------------
def _tiny(count):
    """64 x 400: 99 entries take the O(n + nnz) path (2 * 400 > 8 * 99), 100 the tables."""
    m, n = 64, 400
    rng = np.random.default_rng(31)
    linear = _random_linear(m, n, 100, rng)
    ro, ci = _csr(m, n, linear[rng.permutation(100)[:count]])
    route = dict(SPARSE, long_rank_launch=0) if count < 100 else \
        dict(GROUPED, chunks=2, groups=8, scan_chunks_per_group=1)
    return Case(f"tiny_{count}", m, n, ro, ci, route, {"nnz": count})


RANK_COLUMNS = {5: 2049, 4095: 2048, 700: 130, 701: 65, 0: 64, 1234: 1}


def _ranked(name, column_counts, others, long_rank_launch, seed):
    m = n = 4096
    rng = np.random.default_rng(seed)
    held = np.concatenate([_linear(rng.choice(m, size=k, replace=False), c, n)
                           for c, k in column_counts.items()])
    free = np.setdiff1d(np.arange(n), list(column_counts))
    ro, ci = _csr(m, n, np.concatenate([held, _random_linear(m, n, others, rng, columns=free)]))
    return Case(name, m, n, ro, ci, dict(SPARSE, long_rank_launch=long_rank_launch),
                {"column_counts": column_counts, "nnz": sum(column_counts.values()) + others})


def _rank_boundaries():
    """Output rows of exactly 2049 (bitmap kernel), 2048, 130, 65 (the lane-strided all-pairs
    loop), 64 and 1 entries among 8000 others."""
    return _ranked("rank_boundaries", RANK_COLUMNS, 8000, 1, 32)


def _no_bitmap():
    """At most 2048 entries in all: the bitmap kernel is not launched."""
    return _ranked("no_bitmap", {700: 130, 701: 65, 0: 64, 1234: 1}, 1788, 0, 33)


BUILDERS = {
    "long_rows": _long_rows,
    "stage_overflow": _stage_overflow,
    "full_columns": _full_columns,
    "tall_scan_4100": lambda: _tall_scan(4100),
    "tall_scan_9000": lambda: _tall_scan(9000),
    "widest_grouped": _widest_grouped,
    "range_of_one": _range_of_one,
    "parts_4": lambda: _wide("parts_4", 2048, 8200, 4, {5: 600, 31: 513, 2047: 1000}, 22),
    "parts_2": lambda: _wide("parts_2", 4105, 8200, 2, {15: 600, 16: 513, 4104: 1000}, 23),
    "parts_1": lambda: _wide("parts_1", 5472, 16400, 1, {0: 9000, 2741: 513, 5471: 700}, 24),
    "tiny_99": lambda: _tiny(99),
    "tiny_100": lambda: _tiny(100),
    "rank_boundaries": _rank_boundaries,
    "no_bitmap": _no_bitmap,
}
CASE_NAMES = tuple(BUILDERS)
LARGE_CASES = ("parts_4", "parts_2", "parts_1")   # no dense m x n array for these


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case, built once per process.  Treat its arrays as read-only."""
    c = BUILDERS[name]()
    assert c.name == name
    c.row_offsets.setflags(write=False)
    c.column_indices.setflags(write=False)
    return c


# ---------------------------------------------------------------------------
# many masks: one batch of m x n masks, flat layout
# ---------------------------------------------------------------------------
class Batch:
    """`masks` topologies of m x n: row_offsets [masks * (m + 1)] (each from 0), column_indices
    concatenated, nonzeros [masks]."""

    def __init__(self, name, m, n, cases):
        self.name, self.m, self.n, self.cases = name, m, n, cases
        self.masks = len(cases)
        self.nonzeros = [c.nnz for c in cases]
        self.row_offsets = np.concatenate([c.row_offsets for c in cases]).astype(np.int32)
        self.column_indices = np.concatenate([c.column_indices for c in cases]).astype(np.int32)

    @property
    def largest(self):
        return max(self.nonzeros)

    def reference(self):
        """(out_row_offsets [masks * (n + 1)], out_column_indices, permutation: per mask, each
        mask's source indices from 0)."""
        refs = [case_reference(c) for c in self.cases]
        return tuple(np.concatenate([r[i] for r in refs]) for i in range(3))

    def values(self, heads, width, seed=0):
        """[masks * heads, width] float32 in (1, 2) (the padding too: it must not move)."""
        rng = np.random.default_rng(2000 + seed)
        return (1.0 + rng.random((self.masks * heads, width))).astype(np.float32)


def _mixed_batch():
    """A mask with a chunk x group over the staging area, an empty one, one with rows past 512
    entries (n = 1100) and a sparse one."""
    m, n = 64, 1100
    rng = np.random.default_rng(41)
    ro, ci = _csr(m, n, _stage_overflow_linear(n, rng), shuffle_rows=range(1, m, 3), seed=5)
    overflow = Case("overflow", m, n, ro, ci, None)
    empty = Case("empty", m, n, np.zeros(m + 1, np.int32), np.zeros(0, np.int32), None)
    lengths = {r: int(rng.integers(5, 40)) for r in range(m)}
    lengths.update({31: 1100, 32: 513, 40: 512, 41: 511, 63: 700, 50: 0})
    ro, ci = _csr(m, n, _rows_of_lengths(n, lengths, rng), shuffle_rows=range(m), seed=6)
    long_ = Case("long", m, n, ro, ci, None)
    ro, ci = _csr(m, n, _random_linear(m, n, 700, rng))
    sparse = Case("sparse", m, n, ro, ci, None)
    return Batch("mixed", m, n, [overflow, empty, long_, sparse])


def _wide_batch():
    """n > 8192: mask after mask."""
    rng = np.random.default_rng(42)
    m, n = 64, 8193
    ro, ci = _csr(m, n, np.union1d(_linear(np.arange(1, m, 2), n - 1, n), _random_linear(m, n, 2500, rng)))
    return Batch("wide", m, n, [case("range_of_one"), Case("second", m, n, ro, ci, None)])


def _sparse_batch():
    """The largest mask on the O(n + nnz) path: mask after mask."""
    rng = np.random.default_rng(43)
    m, n = 64, 400
    ro, ci = _csr(m, n, _random_linear(m, n, 40, rng))
    return Batch("sparse", m, n, [Case("first", m, n, ro, ci, None), case("tiny_99")])


BATCH_BUILDERS = {"mixed": _mixed_batch, "wide": _wide_batch, "sparse": _sparse_batch}


@functools.lru_cache(maxsize=None)
def batch(name):
    return BATCH_BUILDERS[name]()


def many_region_bytes(workspace_bytes_of_largest):
    """Bytes of one mask's tables in the many-mask workspace: the single-mask workspace of the
    largest mask rounded up to 256 (include/sputnik_hip.h: "a region of tables per mask")."""
    return -(-workspace_bytes_of_largest // 256) * 256
