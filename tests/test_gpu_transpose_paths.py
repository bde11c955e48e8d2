"""GPU: every launch path of the CSR transpose (csrc/transpose.hip) at the edges of its
kernels, on the named cases of tests/transpose_cases.py.

Each test first asserts the route it means to reach (capi.csr_transpose_route /
csr_transpose_many_mask_route: the functions the launches themselves take their decisions
from), then compares out_row_offsets, out_column_indices, out_values, the permutation and
values[..., perm] with the numpy reference BIT FOR BIT -- the transpose permutes and copies,
there is nothing to tolerate.  Every output is a slice of a larger buffer filled with a canary:
16 guard elements behind it (and the padding of value rows wider than the entry count) must
keep the canary, and none may be left inside.  Topologies and references are built once per
case and shared.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import transpose_cases as tc
from tests.transpose_cases import CANARY_FLOAT, CANARY_INT, GUARD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def capi():
    from torch_sputnik_amd import capi
    assert "gfx950" in capi.version()
    return capi


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def on_device(name):
    """(case, row_offsets, column_indices on the device, reference), once per case."""
    case = tc.case(name)
    return case, T(case.row_offsets), T(case.column_indices), tc.case_reference(case)


class Guarded:
    """`count` elements in front of GUARD more, all holding the canary."""

    def __init__(self, count, dtype, shape=None):
        self.canary = CANARY_FLOAT if dtype == torch.float32 else CANARY_INT
        self.count = count
        self.buffer = torch.full((count + GUARD,), self.canary, dtype=dtype, device="cuda:0")
        self.view = self.buffer[:count] if shape is None else self.buffer[:count].view(shape)

    def numpy(self, written=True):
        """The output; the guard must be untouched and (written=True) no canary left inside."""
        got = self.buffer.cpu().numpy()
        assert (got[self.count:] == self.canary).all(), "a store behind the end of an output"
        inside = got[:self.count].reshape(tuple(self.view.shape))
        if written:
            assert not (inside == self.canary).any(), "an output element was never written"
        return inside


def assert_route(capi, case):
    route = capi.csr_transpose_route(case.m, case.n, case.nnz)
    assert {k: route[k] for k in case.route} == case.route, (case.name, route)
    return route


def workspace_for(capi, case):
    nbytes = capi.csr_transpose_workspace_bytes(case.m, case.n, case.nnz)
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")


def run_single(capi, name, replicas=1, dtype=torch.float32, with_permutation=True, checked=False):
    """One call on fresh guarded outputs; returns (values on the host as stored, out_values,
    out_row_offsets, out_column_indices, permutation or None) as numpy, guards checked."""
    case, ro, ci, _ = on_device(name)
    assert_route(capi, case)
    values = T(case.values(max(replicas, 1), seed=replicas)).to(dtype)
    out_v = Guarded(max(replicas, 1) * case.nnz, torch.float32, (max(replicas, 1), case.nnz))
    out_ro = Guarded(case.n + 1, torch.int32)
    out_ci = Guarded(case.nnz, torch.int32)
    perm = Guarded(case.nnz, torch.int32) if with_permutation else None
    ws = workspace_for(capi, case)
    if dtype == torch.float32 and replicas > 0:
        capi.csr_transpose(case.m, case.n, replicas, values, ro, ci, out_v.view, out_ro.view,
                           out_ci.view, perm.view if perm else None, ws, checked=checked)
    else:
        capi.csr_transpose_typed(case.m, case.n, replicas, values, ro, ci, out_v.view, out_ro.view,
                                 out_ci.view, perm.view if perm else None, ws, checked=checked)
    torch.cuda.synchronize()
    return (values.float().cpu().numpy(), out_v.numpy(written=replicas > 0), out_ro.numpy(),
            out_ci.numpy(), perm.numpy() if perm else None)


def assert_reference(name, values, got_v, got_ro, got_ci, got_perm):
    want_ro, want_ci, want_perm = on_device(name)[3]
    assert np.array_equal(got_ro, want_ro), f"{name}: out_row_offsets"
    assert np.array_equal(got_ci, want_ci), f"{name}: out_column_indices"
    if got_perm is not None:
        assert np.array_equal(got_perm, want_perm), f"{name}: permutation"
        assert np.array_equal(values[..., got_perm], values[..., want_perm])
    if got_v is not None:
        assert np.array_equal(got_v, values[..., want_perm]), f"{name}: out_values"


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_case_bit_exact_and_repeatable(capi, name):
    first = run_single(capi, name)
    assert_reference(name, *first)
    second = run_single(capi, name)       # (the O(n + nnz) path's cursors are atomics: the order
    for a, b in zip(first, second):       # they are taken in must not show)
        assert np.array_equal(a, b), f"{name}: two calls differ"
    values, got_v, got_ro, got_ci, _ = run_single(capi, name, with_permutation=False)
    assert_reference(name, values, got_v, got_ro, got_ci, None)


@pytest.mark.parametrize("name,replicas", [
    ("stage_overflow", 3),      # direct writes of several replicas behind a full staging area
    ("long_rows", 2), ("full_columns", 3), ("widest_grouped", 2),
    ("parts_4", 3), ("range_of_one", 2), ("rank_boundaries", 2), ("tiny_99", 3)])
def test_several_replicas_share_one_permutation(capi, name, replicas):
    assert_reference(name, *run_single(capi, name, replicas=replicas))
    values, got_v, got_ro, got_ci, _ = run_single(capi, name, replicas=replicas, with_permutation=False)
    assert_reference(name, values, got_v, got_ro, got_ci, None)


@pytest.mark.parametrize("name,replicas", [("stage_overflow", 1), ("stage_overflow", 3), ("parts_4", 2),
                                           ("rank_boundaries", 2)])
def test_value_rows_wider_than_the_entry_count(capi, name, replicas):
    """Strides of nnz + 5 (in) and nnz + 7 (out): the padding of the output rows keeps the canary."""
    case, ro, ci, (want_ro, want_ci, want_perm) = on_device(name)
    assert_route(capi, case)
    nnz, in_stride, out_stride = case.nnz, case.nnz + 5, case.nnz + 7
    host = np.full((replicas, in_stride), 3.0, np.float32)
    host[:, :nnz] = case.values(replicas, seed=7)
    values = T(host)
    out_v = Guarded(replicas * out_stride, torch.float32, (replicas, out_stride))
    out_ro, out_ci, perm = Guarded(case.n + 1, torch.int32), Guarded(nnz, torch.int32), Guarded(nnz, torch.int32)
    ws = workspace_for(capi, case)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    status = capi.lib().sputnik_hip_csr_transpose(
        case.m, case.n, nnz, replicas, ptr(values), in_stride, ptr(ro), ptr(ci), ptr(out_v.view),
        out_stride, ptr(out_ro.view), ptr(out_ci.view), ptr(perm.view), ptr(ws), ws.numel(),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    got_v = out_v.numpy(written=False)
    assert np.array_equal(got_v[:, :nnz], host[:, :nnz][:, want_perm])
    assert (got_v[:, nnz:] == CANARY_FLOAT).all(), "the padding of an output row was written"
    assert np.array_equal(out_ro.numpy(), want_ro) and np.array_equal(out_ci.numpy(), want_ci)
    assert np.array_equal(perm.numpy(), want_perm)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["long_rows", "stage_overflow", "range_of_one", "parts_2", "rank_boundaries",
                                  "no_bitmap"])
def test_half_values_are_gathered_as_stored(capi, name, dtype):
    for replicas in (1, 3):
        values, got_v, got_ro, got_ci, got_perm = run_single(capi, name, replicas=replicas, dtype=dtype)
        assert values.dtype == np.float32 and not np.array_equal(values, tc.case(name).values(replicas, replicas))
        assert_reference(name, values, got_v, got_ro, got_ci, got_perm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", ["stage_overflow", "long_rows", "parts_4", "rank_boundaries"])
def test_topology_and_permutation_without_values(capi, name, dtype):
    """replicas == 0: no value is read or written (out_values keeps the canary)."""
    values, got_v, got_ro, got_ci, got_perm = run_single(capi, name, replicas=0, dtype=dtype)
    assert (got_v == CANARY_FLOAT).all()
    assert_reference(name, values, None, got_ro, got_ci, got_perm)


@pytest.mark.parametrize("name", ["long_rows", "stage_overflow", "parts_4", "rank_boundaries", "tiny_99"])
def test_torch_ops(capi, name):
    import torch_sputnik  # noqa: F401  (registers the ops)
    case, ro, ci, (want_ro, want_ci, want_perm) = on_device(name)
    assert_route(capi, case)
    ops = torch.ops.torch_sputnik
    host = case.values(2, seed=3)
    for values in (host[0], host):
        vt, rot, cit = ops.csr_transpose(case.m, case.n, T(values), ro, ci)
        assert np.array_equal(vt.cpu().numpy(), values[..., want_perm])
        assert np.array_equal(rot.cpu().numpy(), want_ro) and np.array_equal(cit.cpu().numpy(), want_ci)
        for checked in (True, False):
            vt, rot, cit, perm = ops.csr_transpose_with_permutation(case.m, case.n, T(values), ro, ci, checked)
            assert np.array_equal(vt.cpu().numpy(), values[..., want_perm])
            assert np.array_equal(rot.cpu().numpy(), want_ro) and np.array_equal(cit.cpu().numpy(), want_ci)
            assert np.array_equal(perm.cpu().numpy(), want_perm)
    half = T(host).to(torch.bfloat16)
    vt, rot, cit, perm = ops.csr_transpose_with_permutation(case.m, case.n, half, ro, ci, True)
    assert vt.dtype == torch.float32
    assert np.array_equal(vt.cpu().numpy(), half.float().cpu().numpy()[:, want_perm])
    assert np.array_equal(perm.cpu().numpy(), want_perm)


# ---------------------------------------------------------------------------
# many masks
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_on_device(name):
    batch = tc.batch(name)
    return batch, T(batch.row_offsets), T(batch.column_indices), batch.reference()


def workspace_bytes_of(capi, batch, kind):
    single = capi.csr_transpose_workspace_bytes(batch.m, batch.n, batch.largest)
    return {"single": single, "regions": batch.masks * tc.many_region_bytes(single),
            "full": capi.csr_transpose_many_mask_workspace_bytes(batch.masks, batch.m, batch.n,
                                                                 batch.largest)}[kind]


def run_many(capi, name, heads, with_permutation, workspace, want_route):
    batch, ro, ci, (want_ro, want_ci, want_perm) = batch_on_device(name)
    nbytes = workspace_bytes_of(capi, batch, workspace)
    route = capi.csr_transpose_many_mask_route(batch.masks, batch.m, batch.n, batch.nonzeros, heads,
                                               with_permutation, nbytes)
    assert route == want_route, (name, heads, with_permutation, workspace, route)
    total, width = sum(batch.nonzeros), batch.largest + 3
    replicas = batch.masks * heads
    host = batch.values(heads, width, seed=heads)
    out_v = Guarded(replicas * width, torch.float32, (replicas, width))
    out_ro = Guarded(batch.masks * (batch.n + 1), torch.int32)
    out_ci = Guarded(total, torch.int32)
    perm = Guarded(total, torch.int32) if with_permutation else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    capi.csr_transpose_many_mask(batch.masks, batch.m, batch.n, batch.nonzeros, replicas, T(host), ro, ci,
                                 out_v.view, out_ro.view, out_ci.view, perm.view if perm else None, ws)
    torch.cuda.synchronize()
    got = (out_v.numpy(written=False), out_ro.numpy(), out_ci.numpy(), perm.numpy() if perm else None)
    tag = f"{name} heads={heads} perm={with_permutation} ws={workspace}"
    assert np.array_equal(got[1], want_ro), f"{tag}: out_row_offsets"
    assert np.array_equal(got[2], want_ci), f"{tag}: out_column_indices"
    if perm:
        assert np.array_equal(got[3], want_perm), f"{tag}: permutation"
    first = 0
    for i, count in enumerate(batch.nonzeros):
        rows = slice(i * heads, (i + 1) * heads)
        source = want_perm[first:first + count]
        assert np.array_equal(got[0][rows, :count], host[rows][:, source]), f"{tag}: values of mask {i}"
        assert (got[0][rows, count:] == CANARY_FLOAT).all(), f"{tag}: padding of mask {i}"
        first += count
    return got


ONE = lambda by: {"one_launch": True, "values_by": by}
AFTER = {"one_launch": False, "values_by": None}


@pytest.mark.parametrize("workspace", ["full", "regions", "single"])
@pytest.mark.parametrize("with_permutation", [True, False], ids=["perm", "noperm"])
@pytest.mark.parametrize("heads", [1, 3])
def test_many_mask_mixed_batch(capi, heads, with_permutation, workspace):
    """A staging overflow, an empty mask, rows past 512 entries and a sparse mask in one batch.
    Several heads without a permutation output on the regions alone: the permutation has no room
    behind them, mask after mask."""
    if workspace == "single" or (workspace == "regions" and heads > 1 and not with_permutation):
        want = AFTER
    else:
        want = ONE("scatter" if heads == 1 else "gather")
    first = run_many(capi, "mixed", heads, with_permutation, workspace, want)
    second = run_many(capi, "mixed", heads, with_permutation, workspace, want)
    for a, b in zip(first, second):
        assert a is None or np.array_equal(a, b)


@pytest.mark.parametrize("name", ["wide", "sparse"])
@pytest.mark.parametrize("heads", [1, 3])
def test_many_mask_falls_back_to_mask_after_mask(capi, name, heads):
    """n > 8192; the largest mask on the O(n + nnz) path."""
    for with_permutation in (True, False):
        run_many(capi, name, heads, with_permutation, "full", AFTER)


@pytest.mark.parametrize("name", ["mixed", "wide", "sparse"])
def test_many_mask_torch_op(capi, name):
    """The op takes no permutation and allocates the full workspace: one launch per phase with
    the values in the scatter (one head) or one gather (two) on the grouped batch, mask after
    mask on the wide and the O(n + nnz) one."""
    import torch_sputnik  # noqa: F401
    batch, ro, ci, (want_ro, want_ci, want_perm) = batch_on_device(name)
    for heads in (1, 2):
        route = capi.csr_transpose_many_mask_route(batch.masks, batch.m, batch.n, batch.nonzeros, heads,
                                                   False, workspace_bytes_of(capi, batch, "full"))
        want = ONE("scatter" if heads == 1 else "gather") if name == "mixed" else AFTER
        assert route == want, (name, heads, route)
        width = batch.largest
        host = batch.values(heads, width, seed=9)
        vt, rot, cit = torch.ops.torch_sputnik.csr_transpose_many_mask(
            batch.masks, batch.m, batch.n, torch.tensor(batch.nonzeros), T(host), ro, ci)
        assert np.array_equal(rot.cpu().numpy().reshape(-1), want_ro)
        assert np.array_equal(cit.cpu().numpy(), want_ci)
        got, first = vt.cpu().numpy(), 0
        for i, count in enumerate(batch.nonzeros):
            rows = slice(i * heads, (i + 1) * heads)
            assert np.array_equal(got[rows, :count], host[rows][:, want_perm[first:first + count]])
            assert (got[rows, count:] == 0).all()
            first += count


# ---------------------------------------------------------------------------
# detection at the new edges (patterns the kernels handle in bounds by design: an entry whose
# column lies outside [0, n) is skipped, a repeated column lands on its twin's slot)
# ---------------------------------------------------------------------------
def checked_call(capi, name, column_indices=None, dtype=torch.float32, checked=True, gathered=False):
    """One call of a case with (possibly bad) column indices on canary-filled outputs; returns
    whether the entry raised.  Whatever the pattern: nothing is stored behind an output, and
    where the permutation kept its canary -- a slot no entry took -- out_values kept its own: no
    value was moved through a slot that is no source index.  A bad pattern leaves at least one
    such slot, a valid one none.  `gathered`: the values of this call move through the
    permutation (the O(n + nnz) path; half values behind the asynchronous entry), so every
    other element is values[permutation] exactly."""
    case, ro, ci, _ = on_device(name)
    out_v = Guarded(case.nnz, torch.float32)
    out_ro, out_ci = Guarded(case.n + 1, torch.int32), Guarded(case.nnz, torch.int32)
    perm = Guarded(case.nnz, torch.int32)
    values = T(case.values(1)[0]).to(dtype)
    entry = capi.csr_transpose if dtype == torch.float32 else capi.csr_transpose_typed
    raised = False
    try:
        entry(case.m, case.n, 1, values, ro, ci if column_indices is None else T(column_indices),
              out_v.view, out_ro.view, out_ci.view, perm.view, workspace_for(capi, case), checked=checked)
    except RuntimeError:
        raised = True
    torch.cuda.synchronize()
    out_ro.numpy(written=False), out_ci.numpy(written=False)
    got_v, got_perm = out_v.numpy(written=False), perm.numpy(written=False)
    unwritten = got_perm == CANARY_INT
    assert unwritten.any() == (column_indices is not None), int(unwritten.sum())
    assert (got_v[unwritten] == CANARY_FLOAT).all(), "a value moved through a slot that is no source index"
    if gathered:
        source = got_perm[~unwritten]
        assert ((source >= 0) & (source < case.nnz)).all()
        assert np.array_equal(got_v[~unwritten], values.float().cpu().numpy()[source])
    return raised


def test_bad_entry_past_the_512th_of_a_long_row_is_detected(capi):
    case = tc.case("long_rows")
    assert_route(capi, case)
    a = int(case.row_offsets[31])
    assert case.row_lengths[31] > 700
    for position, wrong in ((700, int(case.column_indices[a + 3])), (513, case.n), (1099, case.n + 9)):
        bad = case.column_indices.copy()
        bad[a + position] = wrong
        assert checked_call(capi, "long_rows", bad)
    assert not checked_call(capi, "long_rows")             # a valid pattern passes afterwards


def test_column_out_of_range_on_a_two_range_matrix_is_detected(capi):
    case = tc.case("range_of_one")
    assert_route(capi, case)
    for position, wrong in ((0, case.n), (case.nnz - 1, case.n + 100), (case.nnz // 2, -1)):
        bad = case.column_indices.copy()
        bad[position] = wrong
        assert checked_call(capi, "range_of_one", bad)
    assert not checked_call(capi, "range_of_one")


def test_bad_entry_on_the_histogram_path_is_detected(capi):
    """The O(n + nnz) path leaves the permutation slots of a bad entry unwritten (here: the
    canary, no source index); its value move goes through the permutation and must neither read
    nor store through them -- out_values keeps its canary exactly there."""
    case = tc.case("rank_boundaries")
    assert_route(capi, case)
    row = int(np.argmax(case.row_lengths >= 2))
    a = int(case.row_offsets[row])
    rows = np.repeat(np.arange(case.m), case.row_lengths)
    in_long = np.flatnonzero((case.column_indices == 5) & (case.row_lengths[rows] >= 2))[0]   # column of 2049
    other = in_long + 1 if rows[in_long + 1] == rows[in_long] else in_long - 1
    for position, wrong in ((a + 1, int(case.column_indices[a])), (a, case.n), (case.nnz - 1, -2), (other, 5)):
        bad = case.column_indices.copy()
        bad[position] = wrong
        assert checked_call(capi, "rank_boundaries", bad, gathered=True)
        assert not checked_call(capi, "rank_boundaries", bad, checked=False, gathered=True)
    assert not checked_call(capi, "rank_boundaries", gathered=True)


@pytest.mark.parametrize("name", ["long_rows", "range_of_one", "rank_boundaries"])
def test_half_gather_does_not_follow_unwritten_permutation_slots(capi, name):
    """float16 values move through the permutation in a gather of their own.  The asynchronous
    entry launches it whatever the pattern: a slot a bad entry left unwritten is not followed,
    and out_values keeps its canary exactly at those slots."""
    case = tc.case(name)
    assert_route(capi, case)
    bad = case.column_indices.copy()
    bad[case.nnz // 2] = case.n
    assert not checked_call(capi, name, bad, dtype=torch.float16, checked=False, gathered=True)
    assert checked_call(capi, name, bad, dtype=torch.float16, checked=True)      # (no gather behind a refusal)
    assert not checked_call(capi, name, dtype=torch.float16, checked=True, gathered=True)


def test_many_mask_gather_does_not_follow_unwritten_permutation_slots(capi):
    """Three heads: ONE gather moves the values of all masks through the permutation.  A column
    = n past the 512th entry of a long row of one mask leaves a slot of that mask's permutation
    unwritten: the gather follows none, out_values keeps its canary there in every head, and the
    other masks come out bit exact."""
    batch, ro, _, (want_ro, want_ci, want_perm) = batch_on_device("mixed")
    heads, which = 3, 2
    nbytes = workspace_bytes_of(capi, batch, "full")
    assert capi.csr_transpose_many_mask_route(batch.masks, batch.m, batch.n, batch.nonzeros, heads, True,
                                              nbytes) == ONE("gather")
    starts = np.concatenate([[0], np.cumsum(batch.nonzeros)])
    long_ = batch.cases[which]
    assert long_.row_lengths[31] > 700
    bad = batch.column_indices.copy()
    bad[starts[which] + int(long_.row_offsets[31]) + 700] = batch.n
    total, width, replicas = int(starts[-1]), batch.largest + 3, batch.masks * heads
    host = batch.values(heads, width, seed=5)
    out_v = Guarded(replicas * width, torch.float32, (replicas, width))
    out_ro, out_ci = Guarded(batch.masks * (batch.n + 1), torch.int32), Guarded(total, torch.int32)
    perm = Guarded(total, torch.int32)
    capi.csr_transpose_many_mask(batch.masks, batch.m, batch.n, batch.nonzeros, replicas, T(host), ro, T(bad),
                                 out_v.view, out_ro.view, out_ci.view, perm.view,
                                 torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    got_v, got_perm = out_v.numpy(written=False), perm.numpy(written=False)
    got_ro, got_ci = out_ro.numpy(written=False), out_ci.numpy(written=False)
    for i, count in enumerate(batch.nonzeros):
        entries, rows = slice(starts[i], starts[i + 1]), slice(i * heads, (i + 1) * heads)
        source = got_perm[entries]
        unwritten = source == CANARY_INT
        assert unwritten.any() == (i == which), (i, int(unwritten.sum()))
        assert ((source[~unwritten] >= 0) & (source[~unwritten] < count)).all()
        assert (got_v[rows, :count][:, unwritten] == CANARY_FLOAT).all(), \
            f"mask {i}: a value moved through a slot that is no source index"
        assert np.array_equal(got_v[rows, :count][:, ~unwritten], host[rows][:, source[~unwritten]])
        assert (got_v[rows, count:] == CANARY_FLOAT).all(), f"mask {i}: padding"
        if i != which:
            assert np.array_equal(source, want_perm[entries])
            assert np.array_equal(got_ci[entries], want_ci[entries])
            offsets = slice(i * (batch.n + 1), (i + 1) * (batch.n + 1))
            assert np.array_equal(got_ro[offsets], want_ro[offsets])
