"""CPU: the transpose cases (tests/transpose_cases.py) are what they say they are.  Their
reference agrees with the oracles, each keeps the promises that make it reach its code, the
host-only route queries answer the route each case states, and together the cases reach every
path, every `parts`, both scan regimes, both answers on the bitmap launch and both many-mask
answers.  No kernel runs here; tests/test_gpu_transpose_paths.py runs them."""
import numpy as np
import pytest

from tests import transpose_cases as tc
from oracle import c_oracle
from oracle import sputnik_oracle as O
from torch_sputnik_amd import capi


def route_of(case):
    return capi.csr_transpose_route(case.m, case.n, case.nnz)


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_reference_agrees_with_the_oracles(name):
    case = tc.case(name)
    out_ro, out_ci, perm = tc.case_reference(case)
    values = case.values(2)
    for oracle in (O, c_oracle):
        vt, rt, ct = oracle.csr_transpose(case.m, case.n, values, case.row_offsets, case.column_indices)
        assert np.array_equal(rt, out_ro) and np.array_equal(ct, out_ci), oracle.__name__
        assert np.array_equal(vt, values[:, perm]), oracle.__name__
    if name not in tc.LARGE_CASES:   # and with the definition: the nonzeros of the dense transpose
        dense = np.zeros((case.m, case.n), bool)
        rows = np.repeat(np.arange(case.m), case.row_lengths)
        dense[rows, case.column_indices] = True
        assert dense.sum() == case.nnz, "a row stores a column twice"
        t_rows, t_cols = np.nonzero(dense.T)
        assert np.array_equal(out_ci, t_cols)
        assert np.array_equal(out_ro, np.concatenate(([0], np.cumsum(np.bincount(t_rows, minlength=case.n)))))
        assert np.array_equal(case.column_indices[perm], t_rows) and np.array_equal(rows[perm], t_cols)


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_case_is_valid_csr_and_keeps_its_promises(name):
    case = tc.case(name)
    ci, lengths, counts = case.column_indices, case.row_lengths, case.column_counts
    assert ci.min() >= 0 and ci.max() < case.n and (lengths >= 0).all()
    rows = np.repeat(np.arange(case.m, dtype=np.int64), lengths)
    assert len(np.unique(rows * case.n + ci)) == case.nnz, "a row stores a column twice"
    p = case.promises
    for row, length in p.get("row_lengths", {}).items():
        assert lengths[row] == length, (row, lengths[row])
    for row, length in p.get("min_row_lengths", {}).items():
        assert lengths[row] >= length > 512, (row, lengths[row])
    for column, count in p.get("column_counts", {}).items():
        assert counts[column] == count, (column, counts[column])
    for column, count in p.get("min_column_counts", {}).items():
        assert counts[column] >= count
    for column in p.get("held_columns", ()):
        assert counts[column] > 0, column
    if "empty_columns" in p:
        assert not counts[slice(*p["empty_columns"])].any()
    if "nnz" in p:
        assert case.nnz == p["nnz"]
    in_cell = lambda chunk, group: np.count_nonzero((rows // 32 == chunk) & (ci // 256 == group))
    for cell, count in p.get("chunk_group_entries", {}).items():
        assert in_cell(*cell) == count
    for cell, count in p.get("chunk_group_at_most", {}).items():
        assert 0 < in_cell(*cell) <= count


def test_long_rows_case_puts_its_long_rows_where_it_says():
    case = tc.case("long_rows")
    assert case.m % 32 != 0 and case.row_lengths[31] == case.n and case.row_lengths.max() > 512
    a, b = case.row_offsets[31], case.row_offsets[32]
    assert not np.array_equal(case.column_indices[a:b], np.arange(case.n)), "row 31 is in column order"
    full = tc.case("full_columns")
    assert (full.column_counts[list(tc.FULL_COLUMNS)] == full.m).all()     # mask word 0xffffffff


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_route_query_returns_the_stated_route(name):
    case = tc.case(name)
    route = route_of(case)
    assert {k: route[k] for k in case.route} == case.route
    # the workspace is sized by the same path
    tables = 4 * (2 * -(-case.m // 32) * case.n + case.n + -(-case.m // 32) * -(-case.n // 8192))
    histogram = 4 * (2 * case.n + 3 * case.nnz)
    body = histogram if route["path"] == "sparse" else tables
    assert capi.csr_transpose_workspace_bytes(case.m, case.n, case.nnz) == -(-body // 16) * 16 + 16


def test_path_boundary_is_one_condition_for_the_route_and_the_workspace():
    """chunks * n > 8 * nnz takes the O(n + nnz) path: both sides of equality, on the two tiny
    cases and on shapes around them, for the launch decision and for the workspace size."""
    assert route_of(tc.case("tiny_99"))["path"] == "sparse"
    assert route_of(tc.case("tiny_100"))["path"] == "grouped"
    for m, n in ((64, 400), (33, 8), (4096, 4096), (64, 8200), (1, 1), (4105, 8200)):
        chunks = -(-m // 32)
        edge = chunks * n // 8            # largest nnz with 8 * nnz <= chunks * n
        for nnz in (edge - 1, edge, edge + 1):
            if nnz < 1 or nnz > m * n:
                continue
            sparse = chunks * n > 8 * nnz
            route = capi.csr_transpose_route(m, n, nnz)
            assert (route["path"] == "sparse") == sparse, (m, n, nnz, route)
            body = 4 * (2 * n + 3 * nnz) if sparse else 4 * (2 * chunks * n + n + chunks * -(-n // 8192))
            assert capi.csr_transpose_workspace_bytes(m, n, nnz) == -(-body // 16) * 16 + 16, (m, n, nnz)


def test_route_query_edges():
    none = {"path": "none", "chunks": -1, "ranges": -1, "groups": -1, "parts": -1,
            "scan_chunks_per_group": -1, "long_rank_launch": -1}
    for shape in ((0, 5, 0), (5, 0, 0), (5, 5, 0), (0, 0, 0)):
        assert capi.csr_transpose_route(*shape) == none
    with pytest.raises(RuntimeError):
        capi.csr_transpose_route(-1, 5, 0)
    assert capi.csr_transpose_route(64, 8192, 4096)["groups"] == 32
    assert capi.csr_transpose_route(64, 8193, 4096)["path"] == "wide"
    assert capi.csr_transpose_route(4096, 70, 70000)["scan_chunks_per_group"] == 8
    assert capi.csr_transpose_route(4097, 70, 70000)["scan_chunks_per_group"] == 9
    assert capi.csr_transpose_route(4096, 4096, 2048)["long_rank_launch"] == 0
    assert capi.csr_transpose_route(4096, 4096, 2049)["long_rank_launch"] == 1
    # parts: the first count of workgroups per chunk and range with 512 in all, 8 at the most
    for chunks, ranges, parts in ((2, 3, 8), (63, 2, 8), (64, 2, 4), (127, 2, 4), (128, 2, 2), (255, 2, 2),
                                  (256, 2, 1), (171, 3, 1)):
        m, n = 32 * chunks, 8192 * (ranges - 1) + 8
        route = capi.csr_transpose_route(m, n, chunks * n)
        assert (route["path"], route["chunks"], route["ranges"], route["parts"]) == ("wide", chunks, ranges, parts)


def many_route(batch, heads, with_permutation, workspace_bytes):
    return capi.csr_transpose_many_mask_route(batch.masks, batch.m, batch.n, batch.nonzeros, heads,
                                              with_permutation, workspace_bytes)


def workspaces(batch):
    """(single-mask bytes of the largest mask, bytes of the regions of all masks, bytes the
    many-mask query asks for)."""
    single = capi.csr_transpose_workspace_bytes(batch.m, batch.n, batch.largest)
    regions = batch.masks * tc.many_region_bytes(single)
    full = capi.csr_transpose_many_mask_workspace_bytes(batch.masks, batch.m, batch.n, batch.largest)
    return single, regions, full


def test_many_mask_route_of_the_mixed_batch():
    batch = tc.batch("mixed")
    assert batch.nonzeros[1] == 0 and capi.csr_transpose_route(batch.m, batch.n, batch.largest)["path"] == "grouped"
    assert max(c.row_lengths.max() for c in batch.cases) == batch.n
    single, regions, full = workspaces(batch)
    assert single < regions <= full and full >= regions + 4 * sum(batch.nonzeros)
    one = lambda by: {"one_launch": True, "values_by": by}
    after = {"one_launch": False, "values_by": None}
    for perm in (False, True):
        assert many_route(batch, 0, perm, full) == one("none")
        assert many_route(batch, 1, perm, full) == one("scatter")
        assert many_route(batch, 3, perm, full) == one("gather")
        assert many_route(batch, 1, perm, regions) == one("scatter")     # the regions alone do
        assert many_route(batch, 1, perm, regions - 1) == after
        for heads in (0, 1, 3):
            assert many_route(batch, heads, perm, single) == after
            assert many_route(batch, heads, perm, 0) == after
    # several heads without a permutation output: the permutation needs room behind the regions
    total = 4 * sum(batch.nonzeros)
    assert many_route(batch, 3, True, regions) == one("gather")
    assert many_route(batch, 3, False, regions) == after
    assert many_route(batch, 3, False, regions + total - 1) == after
    assert many_route(batch, 3, False, regions + total) == one("gather")


@pytest.mark.parametrize("name,path", [("wide", "wide"), ("sparse", "sparse")])
def test_many_mask_route_falls_back(name, path):
    batch = tc.batch(name)
    assert capi.csr_transpose_route(batch.m, batch.n, batch.largest)["path"] == path
    _, _, full = workspaces(batch)
    for heads in (0, 1, 3):
        assert many_route(batch, heads, True, 4 * full) == {"one_launch": False, "values_by": None}
    one_mask = capi.csr_transpose_many_mask_route(1, 64, 300, [500], 1, True, 1 << 20)
    assert one_mask == {"one_launch": False, "values_by": None}


def test_cases_reach_every_route_together():
    routes = [route_of(tc.case(name)) for name in tc.CASE_NAMES]
    assert {r["path"] for r in routes} | {capi.csr_transpose_route(0, 4, 0)["path"]} == set(capi.TRANSPOSE_PATHS)
    assert {r["parts"] for r in routes if r["path"] == "wide"} == {1, 2, 4, 8}
    per_group = {r["scan_chunks_per_group"] for r in routes if r["path"] != "sparse"}
    assert min(per_group) <= 8 < max(per_group) and any(p > 16 for p in per_group)
    assert any(r["scan_chunks_per_group"] > 8 for r in routes if r["path"] == "grouped")
    assert any(r["scan_chunks_per_group"] > 8 for r in routes if r["path"] == "wide")
    assert {r["long_rank_launch"] for r in routes if r["path"] == "sparse"} == {0, 1}
    assert {r["ranges"] for r in routes if r["path"] == "wide"} >= {2, 3}
    assert 32 in {r["groups"] for r in routes}
    mixed = tc.batch("mixed")
    _, regions, full = workspaces(mixed)
    answers = [many_route(mixed, h, p, w) for h in (1, 3) for p in (False, True) for w in (regions, full)]
    answers += [many_route(tc.batch(b), 1, True, 1 << 24) for b in ("wide", "sparse")]
    assert {a["one_launch"] for a in answers} == {True, False}
    assert {a["values_by"] for a in answers} == {"scatter", "gather", None}
