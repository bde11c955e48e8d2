"""CPU: the named masks of tests/attention_cases.py reach the kernel edges they are built for,
the numpy model of the staged forward's plan agrees with a brute-force recount, and the
(instance x case) list of tests/test_gpu_attention_instances.py gives every one of the 30 fused
attention kernel instances its staged, gathered, long-row and dropout cases."""
import numpy as np
import pytest

import attention_cases as A


def counts_of(name):
    return A.case(name).chunk_counts


# ---------------------------------------------------------------------------
# per (row, chunk) counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", A.CHUNK_COUNTS)
def test_every_chunk_count_in_the_first_and_in_a_later_chunk(count):
    cc = counts_of("edges_127x257_identity")
    assert (cc[:, 0] == count).any(), f"edges_127x257_identity: no row with {count} entries in chunk 0"
    assert (cc[:, 1] == count).any(), f"edges_127x257_identity: no row with {count} entries in chunk 1"
    # by-length order on two blocks too (n = 256: two full chunks)
    cc = counts_of("edges_129x256_by_length")
    assert (cc[:, 0] == count).any() and (cc[:, 1] == count).any()


def longest_sets(name):
    """(rows of the set, chunk) of every four-group set whose `longest` passes 32."""
    c = A.case(name)
    cc = c.chunk_counts
    found = []
    for rows in A.wave_sets(c.row_indices, c.m):
        real = rows[rows >= 0]
        for chunk in range(cc.shape[1]):
            if len(real) and cc[real, chunk].max() > A.PREFETCHED:
                found.append((rows, chunk))
    return c, cc, found


def test_longest_loop_partners():
    """A row with more than 32 entries in a chunk shares its `longest` with a row of 1-3
    entries there, a row with none there but some elsewhere, a row with no entry at all, and a
    padding slot."""
    c, cc, found = longest_sets("edges_127x257_identity")
    assert c.m % A.BM != 0
    kinds = set()
    for rows, chunk in found:
        for r in rows:
            if r < 0:
                kinds.add("padding")
            elif 1 <= cc[r, chunk] <= 3:
                kinds.add("short")
            elif cc[r, chunk] == 0 and cc[r].sum() > 0:
                kinds.add("elsewhere")
            elif cc[r].sum() == 0:
                kinds.add("empty")
    assert kinds == {"padding", "short", "elsewhere", "empty"}, kinds
    # the same set holds the long row, a short one, one with entries elsewhere and the padding
    rows = A.wave_sets(c.row_indices, c.m)[-1]
    assert list(rows) == [124, 125, 126, -1]
    assert cc[124, 0] == 40 and cc[125, 0] == 0 and cc[125, 2] == 1 and cc[126, 0] == 1   # (one key in chunk 2)
    # and in the other orders and block counts a long row still meets a shorter partner
    for name in ("edges_129x256_by_length", "edges_260x255_permuted"):
        c, cc, found = longest_sets(name)
        assert any((cc[rows[rows >= 0], chunk] <= A.PREFETCHED).any() or (rows < 0).any()
                   for rows, chunk in found), name


# ---------------------------------------------------------------------------
# chunk and row-block geometry
# ---------------------------------------------------------------------------
def test_chunk_geometry():
    assert {A.case(n).n for n in A.EDGE_CASES} >= {64, 128, 129, 255, 256, 257}
    assert {A.case(n).m for n in A.EDGE_CASES} >= {1, 127, 128, 129, 260}
    widths = {A.case(n).n - (A.ceil_div(A.case(n).n, A.BK) - 1) * A.BK for n in A.EDGE_CASES}
    assert widths >= {1, 127, 128}, widths           # keys of the last chunk
    assert {A.ceil_div(A.case(n).n, A.BK) for n in A.EDGE_CASES} == {1, 2, 3}
    for name in ("edges_127x257_identity", "edges_129x256_by_length", "edges_260x255_permuted"):
        c = A.case(name)
        for column in (127, 128, c.n - 1):
            assert c.dense[:, column].any(), f"{name}: no entry in column {column}"
        cc = c.chunk_counts
        assert ((cc[:, -1] > 0) & (cc[:, :-1].sum(1) == 0)).any(), f"{name}: no row only in the last chunk"
    cc = counts_of("edges_127x257_identity")
    assert ((cc[:, 0] > 0) & (cc[:, 1] == 0) & (cc[:, 2] > 0)).any(), "no row with a gap chunk"


@pytest.mark.parametrize("name", [n for n in A.EDGE_CASES if n.startswith("edges_") or n == "one_row_1x64"])
def test_last_entry_clamps_or_last_row_is_empty(name):
    c = A.case(name)
    lengths = np.diff(c.row_offsets)
    if "last_row_empty" in name:
        assert lengths[-1] == 0 and c.nnz > 0
    else:
        assert lengths[-1] == 1, f"{name}: the last entry of column_indices is not a row of its own"


def test_row_orders():
    orders = {A.case(n).order for n in A.EDGE_CASES}
    assert orders == {"by_length", "identity", "permuted"}
    for name in A.CASE_NAMES:
        c = A.case(name)
        assert sorted(c.row_indices) == list(range(c.m))
        lengths = np.diff(c.row_offsets)
        if c.order == "by_length":
            assert (np.diff(lengths[c.row_indices]) <= 0).all()
        assert c.m <= 300 and c.n <= 300
    assert (A.case("edges_260x255_permuted").row_indices != np.arange(260)).any()


def test_order_cases_gather_the_blocks_they_name():
    c = A.case("one_block_gathers_129x256")
    blocks = A.block_rows(c.row_indices, c.m)
    assert len(blocks) == 2 and c.unsorted_rows == (10, 20)
    assert {10, 20} <= set(blocks[0]) and not set(c.unsorted_rows) & set(blocks[1])
    assert list(c.gathered) == [True, False]
    a, b = c.row_offsets[10], c.row_offsets[11]
    assert (np.diff(c.column_indices[a:b]) < 0).all()                 # reversed
    a, b = c.row_offsets[20], c.row_offsets[21]
    assert (np.diff(c.column_indices[a:b]) < 0).sum() == 1            # one swapped pair
    for name in ("every_block_gathers_129x256", "every_block_gathers_260x64"):
        assert A.case(name).gathered.all() and len(A.case(name).gathered) > 1, name
    for name in A.CASE_NAMES:
        c = A.case(name)
        if not c.unsorted_rows:
            assert not c.gathered.any(), name


# ---------------------------------------------------------------------------
# the row-group kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.ROWGROUP_CASES)
def test_rowgroup_counts_in_rows_and_key_columns(name):
    c = A.case(name)
    k = len(A.ROWGROUP_COUNTS)
    assert tuple(c.dense.sum(1)[:k]) == A.ROWGROUP_COUNTS, f"{name}: row counts"
    assert tuple(c.dense.sum(0)[:k]) == A.ROWGROUP_COUNTS, f"{name}: key column counts"
    assert set(A.ROWGROUP_COUNTS) >= {0, 1, 3, 4, 5, 15, 16, 17, 32, 33, 48, 49}
    # dropout in the columns kernel: a key column of >= 17 query rows whose original entries
    # are not consecutive CSR positions (consecutive slots are not consecutive entries)
    _, t_ro, _, perm = c.transposed()
    column = A.ROWGROUP_COUNTS.index(17)
    entries = perm[t_ro[column]:t_ro[column + 1]]
    assert len(entries) == 17 and (np.diff(entries) > 1).all()
    assert c.unsorted_rows, f"{name}: no reversed row"
    # a key column that only a query row of one entry sees (dK = 0 by cancellation)
    single = c.dense.sum(1) == 1
    assert c.dense[:, -1].sum() == 1 and single[np.flatnonzero(c.dense[:, -1])[0]], name


def test_structured_kinds():
    for m, n in ((260, 260), (200, 136)):
        for kind in ("causal", "band8", "band40", "global", "block_diagonal", "stride", "dense_row"):
            c = A.case(f"{kind}_{m}x{n}")
            assert (c.m, c.n) == (m, n) and c.nnz > 0
        causal = A.case(f"causal_{m}x{n}").dense
        assert causal[0].sum() == 1 and causal[-1].all()
        for width in (8, 40):
            per_row = A.case(f"band{width}_{m}x{n}").dense.sum(1)
            assert per_row.max() == width + 1 and per_row.min() >= width // 2 + 1
        g = A.case(f"global_{m}x{n}").dense
        assert g.all(1).sum() == 3 and g.all(0).sum() == 3
        d = A.case(f"dense_row_{m}x{n}").dense
        assert d.all(1).sum() == 1 and d.mean() < 0.04
        b = A.case(f"block_diagonal_{m}x{n}").dense
        assert b[:48, :48].all() and not b[:48, 48:].any()


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def brute_force_plan(c):
    """The chunk table by counting: position of the first entry with column >= c * 128."""
    rows = A.slot_rows(c.row_indices, c.m)
    nchunks = A.ceil_div(c.n, A.BK)
    table = np.zeros((nchunks + 1, len(rows)), dtype=np.int32)
    row_ok = np.ones(len(rows), dtype=np.int32)
    for slot, row in enumerate(rows):
        if row < 0:
            continue
        a, b = c.row_offsets[row], c.row_offsets[row + 1]
        cols = c.column_indices[a:b]
        row_ok[slot] = int((np.diff(cols) > 0).all() and (cols < c.n).all())
        for chunk in range(nchunks + 1):
            table[chunk, slot] = a + np.count_nonzero(cols < chunk * A.BK)
    return row_ok, table.reshape(-1)


@pytest.mark.parametrize("name", ["edges_60x128_identity", "edges_129x256_by_length",
                                  "one_block_gathers_129x256"])
def test_plan_model_against_brute_force(name):
    c = A.case(name)
    row_ok, table, defined = A.plan_model(*c.csr, c.m, c.n)
    want_ok, want_table = brute_force_plan(c)
    assert np.array_equal(row_ok, want_ok)
    slots = len(row_ok)
    ok_words = np.tile(row_ok.astype(bool), len(table) // slots)
    assert defined[ok_words].all(), "every word of an ok row is written exactly once"
    assert np.array_equal(table[ok_words], want_table[ok_words])
    # per-chunk counts follow from the table
    cc = c.chunk_counts
    t = table.reshape(-1, slots)
    for slot, row in enumerate(A.slot_rows(c.row_indices, c.m)):
        if row >= 0 and row_ok[slot]:
            assert np.array_equal(np.diff(t[:, slot]), cc[row])
        elif row < 0:
            assert row_ok[slot] == 1 and not t[:, slot].any()


def test_dealt_slots():
    rows = A.slot_rows(np.arange(260), 260)
    assert len(rows) == 384 and sorted(rows[rows >= 0]) == list(range(260))
    assert rows[1] == 3 and rows[128] == 1 and rows[87] == -1 and rows[86] == 258
    assert list(A.slot_rows(np.arange(5)[::-1], 5)[:6]) == [4, 3, 2, 1, 0, -1]


def test_many_mask_plan_model():
    b = A.batch("order_129x256")
    plan, defined = b.plan_model()
    ints = A.mask_plan_ints(256, 2)
    assert len(plan) == 2 * ints and ints % 64 == 0
    order = [plan[ints - 1], plan[2 * ints - 1]]
    assert sorted(order) == [0, 1] and b.nonzeros[order[0]] >= b.nonzeros[order[1]]
    assert np.array_equal(plan[ints:ints + 256], A.plan_model(*b.cases[1].csr, 129, 256)[0])
    for name in A.BATCHES:
        bb = A.batch(name)
        assert bb.row_offsets.shape == (len(bb.cases) * (bb.m + 1),)
        assert bb.row_offsets[bb.m + 1] == 0 and sum(bb.nonzeros) == len(bb.column_indices)


@pytest.mark.parametrize("name", ["rowgroup_90x77", "edges_127x257_identity", "one_row_1x64"])
def test_transpose_round_trip(name):
    c = A.case(name)
    t_ro, t_ci, perm = A.transpose_numpy(c.row_offsets, c.column_indices, c.m, c.n)
    assert sorted(perm) == list(range(c.nnz))
    rows = np.repeat(np.arange(c.m), np.diff(c.row_offsets))
    assert np.array_equal(t_ci, rows[perm])
    assert np.array_equal(np.repeat(np.arange(c.n), np.diff(t_ro)), c.column_indices[perm])
    back_ro, back_ci, _ = A.transpose_numpy(t_ro, t_ci, c.n, c.m)
    assert np.array_equal(back_ro, c.row_offsets)
    ascending = np.nonzero(c.dense)[1]        # (the round trip sorts the rows' columns)
    assert np.array_equal(back_ci, ascending)
    dense = np.zeros((c.n, c.m), dtype=bool)
    dense[np.repeat(np.arange(c.n), np.diff(t_ro)), t_ci] = True
    assert np.array_equal(dense, c.dense.T)


# ---------------------------------------------------------------------------
# what the GPU file runs
# ---------------------------------------------------------------------------
def test_every_forward_instance_gets_its_cases():
    runs = A.forward_runs()
    instances = A.forward_instances()
    assert len(instances) == 20 and len(set(instances)) == 20
    for inst in instances:
        _, _, many, drop = inst
        names = [name for i, name in runs if i == inst]
        cases = [c for name in names for c in (A.batch(name).cases if many else [A.case(name)])]
        assert any((~c.gathered).any() for c in cases), f"{inst}: no staged block"
        assert any(c.gathered.any() for c in cases), f"{inst}: no gathered block"
        staged_long = any((c.chunk_counts[rows[rows >= 0]] > A.PREFETCHED).any()
                          for c in cases
                          for rows, gathered in zip(A.block_rows(c.row_indices, c.m), c.gathered)
                          if not gathered)
        assert staged_long, f"{inst}: no count above 32 in a staged block"
        assert any(name in A.STRUCTURED_CASES + A.STRUCTURED_BATCHES for name in names), inst
    # the dropout instances run every one of their cases with p > 0, and each storage pair and
    # mask layout has one
    assert A.DROP_P == 0.25
    assert {i[:3] for i in instances if i[3]} == {i[:3] for i in instances if not i[3]}
    structured = {name for (t, to, many, drop), name in runs if not many and name in A.STRUCTURED_CASES}
    assert structured == set(A.STRUCTURED_CASES)
    for pair in A.STORAGE_PAIRS:
        got = {name for (t, to, many, drop), name in runs if (t, to) == pair and not many}
        assert got >= set(A.STRUCTURED_CASES), pair


def test_every_rowgroup_instance_gets_its_cases():
    runs = A.rowgroup_runs()
    instances = A.rowgroup_instances()
    assert len(instances) == 10 and len(instances) + len(A.forward_instances()) == 30
    assert {drop for _, _, drop in instances} == {False, True}
    for inst in instances:
        kernel = inst[0]
        names = [name for i, name in runs if i == inst]
        assert set(names) >= set(A.ROWGROUP_CASES), inst
        axis = 0 if kernel == "backward_columns" else 1
        assert any((A.case(name).dense.sum(axis) > 32).any() for name in names), f"{inst}: no list above 32"
        assert any(A.case(name).unsorted_rows for name in names), inst
