"""GPU: structured masks through every single-mask SpMM and SDDMM kernel route, against the
float64 oracle on the same inputs.

The other SpMM / SDDMM tests build uniform random masks, which give every wave, chunk, slab and
tile about the same few entries.  The LDS kernels go wrong on structure: chunk tables cut at
slab and K-chunk boundaries, the flat stream's column groups and tail windows, row slots dealt
in runs, SDDMM's 16-entry windows, matrix-core tiles without an entry.  Here every route runs
every kind of helpers.STRUCTURED_KINDS (causal, band, global columns, heavy rows, the partial
last chunk, block diagonal, stride, alternating, corner, and uniform as the control).

Every case names the route it means to reach (ROUTES below: knobs, shape, expected kernel) and
asserts it with the library's host-only queries BEFORE it launches; a mismatch fails.  The
same table is walked without a GPU by tests/test_host_logic.py, and printed by
tools/structured_mask_routes.py (profiles/structured_mask_routes.txt).

Inputs: operands and values uniform in (-1, 1); outputs pre-filled with NaN, every element
must have been written; rows of empty mask rows are exactly 0.  Bounds are the project's:
rel_err < 1e-4 (float32), half_err < 1e-4 (half output, one rounding taken off), the oracle
on the operands as stored.

NOT REACHED, by shape rules only (no mask kind is excluded anywhere):
  route                               why the shapes here cannot reach it
  256-column SpMM, 256-row tile       taken from 192 tiles of 256 x 256 per call (choose_instance,
                                      spmm_tiled.hip): m = 203 x n = 512 gives 2.  The 128-row
                                      tile (from 96) IS reached under SPMM_MEDIUM=1.
  512-column SpMM, 128-row tile       taken from 192 tiles per call: 2 x replicas here
                                      (both tiles, in both forms, run at their edges in
                                      tests/test_gpu_spmm_instances.py, which takes the replica
                                      count it needs: 96 replicas of 203 rows, 17 of 1283)
  tiled SDDMM, k % 64 != 0            no panel width divides k: the row-wave kernel serves it
  half SDDMM, half OUTPUT, k = 512    two passes of 256 would round twice: float32 output only
  half pair-flat SDDMM, k >= 256      its rows are 128 or 256 bytes: k = 64 / 128 in half
  float32 pair-flat SDDMM, k >= 128   the same rule: k = 64 in float32
  summed SDDMM, half, 512-wide panel  sddmm_tiled_sum_half_served: panels of at most 256
  matrix-core routes, 256-row tile    the output needs 256 rows: those routes run at m = 267
                                      (summed SDDMM 267 x 192 x 300, left_spmm 267 x 192 x 136)
  typed SpMM panel kernel, 1 replica  sputnik_hip_spmm_typed takes it from nnz * n * replicas
                                      >= 2^22, whatever the knob: the typed routes run 3 and 4
                                      replicas, the panel one at n = 264 and nnz >= 32 m
  typed SpMM on widened copies        from nnz * n * replicas >= 2^28: not a small shape

NOT ASSERTED here (the variant rests on the knob alone; the name asserted is that of the kernel
family): the long- / short-segment form and the tile (small / medium) of the 256-column SpMM
kernel, the panel width and the number of accumulating panels of the plain SDDMM kernels.  Both
are observable since -- capi.spmm_launch_shape reports the tile, the form, kBatch, the grid and
the K split, capi.sddmm_launch_shape the panel and the passes -- and are asserted, instance by
instance, by tests/test_gpu_spmm_instances.py and tests/test_gpu_sddmm_instances.py.  The flat
kernel's loop IS named (spmm_flat_kernel<0 / 1 / 2>) and asserted.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import sputnik_oracle as O
from helpers import STRUCTURED_KINDS, half_err, rel_err, rounded, structured_csr

gpu = pytest.mark.gpu

TOL = 1e-4
KNOBS = ("SPMM_KERNEL", "SPMM_SPARSE", "SPMM_MEDIUM", "SDDMM_KERNEL", "SDDMM_PANEL", "SDDMM_SLAB",
         "SDDMM_FLAT", "MFMA_TILE")
HALF_TYPES = (torch.float16, torch.bfloat16)
M = 203          # a partial last group of 8 rows, a partial second 128-row block
K_SPMM = 500     # the last 32-column chunk holds 20 columns (the last 64-column chunk 52)
N_SDDMM = 300    # ragged against slabs of 256, 128 and 64 rows: 44 columns in the last one

# (order, replicas, shared values, shuffle every n-th row's columns, planned)
SPMM_FORMS = (("descending", 1, False, 0, False), ("descending", 3, False, 0, True),
              ("identity", 3, True, 0, False), ("identity", 1, False, 3, False))
# (order, replicas, shuffle, planned)
SDDMM_FORMS = (("descending", 1, 0), ("descending", 3, 0), ("identity", 3, 3))
# (order, replicas, shared values, shuffle): the typed SpMM's panel kernel needs nnz * n * replicas >= 2^22
SPMM_HALF_FORMS = (("descending", 3, False, 0), ("descending", 4, False, 0), ("identity", 3, True, 0),
                   ("identity", 4, False, 3))


class Route:
    """One kernel route: the knobs that force it, the shape, and what the query must say."""

    def __init__(self, op, name, knobs, m, k, n, expect, min_mean_row, chunk, dtype=torch.float32,
                 planned=False, out_half=False, mixed=False, loops=None):
        self.op, self.name, self.knobs = op, name, dict(knobs)
        # the panel kernel is taken where the DEVICE offers 128 KiB of LDS per workgroup: a host
        # without a device is told "row gather" (walk_routes asserts exactly that there)
        self.needs_device = expect == "spmm_panel64_kernel"
        self.m, self.k, self.n = m, k, n
        self.expect, self.min_mean_row, self.chunk = expect, min_mean_row, chunk
        self.dtype, self.planned, self.out_half, self.mixed, self.loops = dtype, planned, out_half, mixed, loops

    @property
    def id(self):
        return f"{self.op}-{self.name}"

    @property
    def mask_shape(self):   # SpMM: the sparse operand is m x k; SDDMM: the mask is m x n
        return (self.m, self.k) if self.op.startswith("spmm") else (self.m, self.n)

    def mask(self, kind, order="descending", shuffle=0):
        rows, cols = self.mask_shape
        seed = sum(map(ord, kind + self.name)) + shuffle
        return structured_csr(kind, rows, cols, self.min_mean_row, np.random.default_rng(seed), order=order,
                              shuffle_every=shuffle, chunk=self.chunk)

    def set_knobs(self, capi, monkeypatch, loop=None):
        """The library's own knobs for this route (`loop`: one of the flat kernel's three)."""
        for knob in KNOBS:
            monkeypatch.delenv("SPUTNIK_HIP_" + knob, raising=False)
        for knob, value in self.knobs.items():
            monkeypatch.setenv("SPUTNIK_HIP_" + knob, str(value))
        if loop is not None:
            monkeypatch.setenv("SPUTNIK_HIP_SPMM_SPARSE", str(loop))
        capi.reload_options()

    def reported(self, capi, nnz, replicas, shared=False):
        """What the library's host-only query says this call takes (knobs already set)."""
        m, k, n = self.m, self.k, self.n
        if self.op == "spmm":
            return capi.spmm_kernel_name(m, k, n, nnz, replicas)
        if self.op == "spmm_half":   # (spmm_typed has a dispatch of its own)
            return capi.spmm_typed_kernel_name(m, k, n, nnz, replicas, self.dtype, 0 if shared else nnz,
                                               self.dtype)
        if self.op == "spmm_mfma":
            code = capi.TYPE_CODES[self.dtype]
            served = capi.lib().sputnik_hip_left_spmm_half_tiles_workspace_bytes(m, k, n, nnz, replicas, code,
                                                                                 code, code) > 0
            rows = capi.left_spmm_half_tiles_tile_rows(m, n, replicas)
            return f"spmm_mfma rows{rows}" if served else "not served"
        if self.op == "sddmm":
            return capi.sddmm_kernel_name(m, k, n, nnz, replicas, 4 if self.dtype == torch.float32 else 2,
                                          planned=self.planned)
        route = capi.sddmm_sum_route(m, k, n, nnz, replicas, self.dtype, planned=self.planned, mixed=self.mixed)
        if route["kernel"] == "tiled":
            return f"tiled w{route['panel_width']} x{route['panels']} rows{route['slab_rows']}"
        if route["kernel"] == "mfma":
            return f"mfma rows{route['slab_rows']}"
        return route["kernel"]

    def assert_reached(self, capi, nnz, replicas, kind="", have_device=True, loop=None, shared=False):
        got = self.reported(capi, nnz, replicas, shared)
        expect = self.expect if have_device or not self.needs_device else "spmm_rowgather_kernel"
        if loop is not None:   # the flat kernel's three loops are three instances: 2 / 3 / 4 -> <0> / <1> / <2>
            expect = f"{expect}<{loop - 2}>"
        assert got.startswith(expect), \
            f"{self.id} / {kind}: meant to reach {expect!r}, the library reports {got!r} " \
            f"(nnz {nnz}, {replicas} replicas, knobs {self.knobs})"
        return got


def _spmm(name, knobs, n, expect, min_mean_row, loops=None):
    return Route("spmm", name, knobs, M, K_SPMM, n, expect, min_mean_row, 32, loops=loops)


def _sddmm(name, knobs, k, expect, dtype=torch.float32, planned=False, out_half=False):
    # (chunk 64: the last 44 columns are the partial last slab of 256, 128 and 64 rows alike)
    return Route("sddmm", name, knobs, M, k, N_SDDMM, expect, 4, 64, dtype=dtype, planned=planned,
                 out_half=out_half)


def _sum(name, knobs, m, k, expect, dtype=torch.float32, planned=False, mixed=False):
    return Route("sddmm_sum", name, knobs, m, k, N_SDDMM, expect, 4, 64, dtype=dtype, planned=planned,
                 mixed=mixed)


def _dt(dtype):
    return {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[dtype]


TILE256 = "spmm_tiled_kernel<TileConfig<256"
SPMM_ROUTES = [
    _spmm("gather", {"SPMM_KERNEL": "gather"}, 72, "spmm_rowgather_kernel", 4),
    _spmm("panel", {"SPMM_KERNEL": "panel"}, 72, "spmm_panel64_kernel", 4),
    _spmm("tiled64", {"SPMM_KERNEL": "narrow"}, 72, "spmm_tiled64_kernel", 4),
    _spmm("tiled256_long", {"SPMM_KERNEL": "wide", "SPMM_SPARSE": 0}, 512, TILE256, 16),
    _spmm("tiled256_short", {"SPMM_KERNEL": "wide", "SPMM_SPARSE": 1}, 512, TILE256, 16),
    _spmm("tiled256_medium_tile", {"SPMM_KERNEL": "wide", "SPMM_MEDIUM": 1}, 512, TILE256, 16),
    _spmm("tiled512", {"SPMM_KERNEL": "wide512"}, 512, "spmm_tiled_kernel<TileConfig<512", 16),
    _spmm("flat", {"SPMM_KERNEL": "flat"}, 512, "spmm_flat_kernel", 16, loops=(2, 3, 4)),
]
SPMM_HALF_ROUTES = [   # (panel: n = 4 * 64 + 8 and nnz >= 32 m, so that 3 replicas of EVERY kind pass 2^22)
    Route("spmm_half", f"{name}_{_dt(dt)}", {"SPMM_KERNEL": name}, M, K_SPMM, n, expect, mean, 32, dtype=dt)
    for name, expect, n, mean in (("panel", "spmm_panel64_kernel", 264, 32), ("gather", "spmm_rowgather_kernel", 72, 4))
    for dt in HALF_TYPES
]
SPMM_MFMA_ROUTES = [   # the smallest ragged shape of test_left_spmm_half_tiles_vs_oracle; 256-row tiles need m >= 256
    Route("spmm_mfma", f"tile{tile}_{_dt(dt)}", {"SPMM_KERNEL": "mfma", "MFMA_TILE": tile}, m, 192, 136,
          f"spmm_mfma rows{tile}", 16, 64, dtype=dt)
    for tile, m in ((128, 200), (256, 267)) for dt in HALF_TYPES
]
TILED = {"SDDMM_KERNEL": "tiled"}
SDDMM_ROUTES = [
    _sddmm("rowwave_k64", {"SDDMM_KERNEL": "wave"}, 64, "sddmm_rowwave_kernel"),
    _sddmm("rowwave_k100", {"SDDMM_KERNEL": "wave"}, 100, "sddmm_rowwave_kernel"),
    _sddmm("quad_k64", TILED, 64, "sddmm_quad_kernel"),
    _sddmm("stationary_k128", TILED, 128, "sddmm_stationary_kernel"),
    _sddmm("stationary_k256", TILED, 256, "sddmm_stationary_kernel"),
    _sddmm("stationary_k512", TILED, 512, "sddmm_stationary_kernel"),
    _sddmm("stationary_k1024_two_panels", TILED, 1024, "sddmm_stationary_kernel"),
    _sddmm("quad_k320_five_panels", TILED, 320, "sddmm_quad_kernel"),
    _sddmm("stationary_k512_panel128", dict(TILED, SDDMM_PANEL=128), 512, "sddmm_stationary_kernel"),
    _sddmm("pair_flat_k64", TILED, 64, "sddmm_flat_kernel", planned=True),
    _sddmm("planned_quad_k64", dict(TILED, SDDMM_FLAT=0), 64, "sddmm_quad_kernel", planned=True),
]
SDDMM_HALF_ROUTES = [
    _sddmm(f"quad_k{k}_{_dt(dt)}_{'half' if out_half else 'f32'}_out", TILED, k, "sddmm_quad_kernel", dtype=dt,
           out_half=out_half)
    for k in (64, 128, 256, 512) for dt in HALF_TYPES for out_half in (False, True)
    if not (out_half and k == 512)   # (two passes: no half output, see the table above)
] + [
    _sddmm(f"pair_flat_k{k}_{_dt(dt)}", TILED, k, "sddmm_flat_kernel", dtype=dt, planned=True)
    for k in (64, 128) for dt in HALF_TYPES
]
SUM_TYPES = (torch.float32,) + HALF_TYPES
SDDMM_SUM_ROUTES = [
    _sum(f"rowwave_{_dt(dt)}", {"SDDMM_KERNEL": "wave"}, M, 128, "rowwave", dtype=dt) for dt in SUM_TYPES
] + [
    _sum(f"tiled_w128_{_dt(dt)}{'_planned' if planned else ''}", TILED, M, 384, "tiled w128 x3 rows128", dtype=dt,
         planned=planned)
    for dt in SUM_TYPES for planned in (False, True)
] + [
    _sum(f"tiled_w256_rows{rows}_{_dt(dt)}{'_planned' if planned else ''}", dict(TILED, SDDMM_SLAB=rows), M, 512,
         f"tiled w256 x2 rows{rows}", dtype=dt, planned=planned)
    for rows in (80, 128) for dt in SUM_TYPES for planned in (False, True)
] + [
    _sum(f"mfma_tile{tile}_{_dt(dt)}{'_mixed' if mixed else ''}{'_planned' if planned else ''}",
         {"SDDMM_KERNEL": "mfma", "MFMA_TILE": tile}, 267, 192, f"mfma rows{tile}", dtype=dt, planned=planned,
         mixed=mixed)
    for tile in (128, 256) for dt in HALF_TYPES for mixed in (False, True) for planned in (False, True)
]
ALL_ROUTES = (SPMM_ROUTES + SPMM_HALF_ROUTES + SPMM_MFMA_ROUTES + SDDMM_ROUTES + SDDMM_HALF_ROUTES +
              SDDMM_SUM_ROUTES)


def replica_counts(route):
    if route.op == "spmm":
        return sorted({f[1] for f in SPMM_FORMS})
    if route.op == "sddmm_sum":
        return [3]
    if route.op == "spmm_half":
        return sorted({f[1] for f in SPMM_HALF_FORMS})
    return [1, 3]


def walk_routes(capi, monkeypatch, routes=None):
    """Every (route, kind, replica count) of this file: asserts the route on the host alone and
    yields (route id, kind, nnz, nnz / rows, replicas, reported).  The knobs are left cleared."""
    have_device = torch.cuda.is_available()
    try:
        for route in (ALL_ROUTES if routes is None else routes):
            for kind in STRUCTURED_KINDS:
                _, ro, ci = route.mask(kind)
                for loop in route.loops or (None,):
                    route.set_knobs(capi, monkeypatch, loop)
                    for replicas in replica_counts(route):
                        got = route.assert_reached(capi, len(ci), replicas, kind, have_device, loop)
                        yield (route.id + (f"-loop{loop}" if loop else ""), kind, len(ci),
                               len(ci) / (len(ro) - 1), replicas, got)
    finally:
        for knob in KNOBS:
            monkeypatch.delenv("SPUTNIK_HIP_" + knob, raising=False)
        capi.reload_options()


def ids(routes):
    return [r.id for r in routes]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def capi():
    from torch_sputnik_amd import capi
    assert "gfx950" in capi.version()
    return capi


@pytest.fixture
def knobs(monkeypatch):
    """The library's own knobs, set per route with monkeypatch.setenv + capi.reload_options()
    (Route.set_knobs); cleared and re-read afterwards."""
    from torch_sputnik_amd import capi as _capi
    yield monkeypatch
    for knob in KNOBS:
        monkeypatch.delenv("SPUTNIK_HIP_" + knob, raising=False)
    _capi.reload_options()


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def uniform(rng, shape):
    return rng.uniform(-1, 1, size=shape).astype(np.float32)


def empty_rows(ro):
    return np.flatnonzero(np.diff(ro) == 0)


# ----------------------------------------------------------------------------
# SpMM, float32: row gather, panel, 64-column, 256-column (long / short segments, medium tile),
# 512-column, flat (three loops, bit for bit alike)
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", STRUCTURED_KINDS)
@pytest.mark.parametrize("route", SPMM_ROUTES, ids=ids(SPMM_ROUTES))
def test_spmm_structured(capi, dev, knobs, route, kind):
    m, k, n = route.m, route.k, route.n
    for order, replicas, shared, shuffle, planned in SPMM_FORMS:
        ri, ro, ci = route.mask(kind, order, shuffle)
        nnz = len(ci)
        rng = np.random.default_rng(nnz + replicas)
        v = uniform(rng, (nnz,) if shared or replicas == 1 else (replicas, nnz))
        b = uniform(rng, (replicas, k, n))
        want = c_oracle.spmm(m, k, v, ro, ci, b)
        topo = (T(ri, dev), T(ro, dev), T(ci, dev))
        tv, tb = T(v, dev), T(b, dev)
        stride = 0 if shared or replicas == 1 else nnz
        outs = []
        for loop in route.loops or (None,):
            route.set_knobs(capi, knobs, loop)
            name = route.assert_reached(capi, nnz, replicas, kind, loop=loop)
            what = f"{route.id} {kind} {order} x{replicas} shared={shared} shuffle={shuffle} planned={planned} [{name}]"
            ws = torch.empty(capi.spmm_workspace_bytes(m, k, n, nnz) + 16, dtype=torch.uint8, device=dev)
            out = torch.full((replicas, m, n), float("nan"), device=dev)
            if planned:
                capi.spmm_plan(m, k, n, *topo, ws)
                capi.spmm_batched_planned(m, k, n, replicas, topo[0], tv, stride, topo[1], topo[2], tb, out, ws)
            else:
                capi.spmm_batched(m, k, n, replicas, topo[0], tv, stride, topo[1], topo[2], tb, out, ws)
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), f"{what}: some output elements were never written"
            err = rel_err(got, want)
            assert err < TOL, f"{what}: rel_err {err:.3g}"
            assert np.all(got[:, empty_rows(ro)] == 0), f"{what}: an empty row is not exactly 0"
            outs.append(out)
        for other in outs[1:]:   # the flat loops sum every element in the same (CSR) order
            assert torch.equal(outs[0], other), f"{route.id} {kind}: the flat loops differ in bits"


# ----------------------------------------------------------------------------
# SpMM, half storage: the typed route (panel / row gather on half operands)
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", STRUCTURED_KINDS)
@pytest.mark.parametrize("route", SPMM_HALF_ROUTES, ids=ids(SPMM_HALF_ROUTES))
def test_spmm_half_structured(capi, dev, knobs, route, kind):
    m, k, n = route.m, route.k, route.n
    for order, replicas, shared, shuffle in SPMM_HALF_FORMS:
        ri, ro, ci = route.mask(kind, order, shuffle)
        nnz = len(ci)
        rng = np.random.default_rng(nnz + replicas)
        v, v32 = rounded(uniform(rng, (replicas, nnz)), route.dtype, dev)
        b, b32 = rounded(uniform(rng, (replicas, k, n)), route.dtype, dev)
        route.set_knobs(capi, knobs)
        name = route.assert_reached(capi, nnz, replicas, kind, shared=shared)
        what = f"{route.id} {kind} {order} x{replicas} shared={shared} shuffle={shuffle} [{name}]"
        out = torch.full((replicas, m, n), float("nan"), device=dev)
        topo = (T(ri, dev), T(ro, dev), T(ci, dev))
        if shared:
            capi.spmm_typed(m, k, n, replicas, topo[0], v[0].contiguous(), 0, topo[1], topo[2], b, out)
            want = c_oracle.spmm(m, k, v32[0], ro, ci, b32)
        else:
            capi.spmm_typed(m, k, n, replicas, topo[0], v, nnz, topo[1], topo[2], b, out)
            want = c_oracle.spmm(m, k, v32, ro, ci, b32)
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"{what}: some output elements were never written"
        err = rel_err(got, want)
        assert err < TOL, f"{what}: rel_err {err:.3g}"
        assert np.all(got[:, empty_rows(ro)] == 0), f"{what}: an empty row is not exactly 0"


# ----------------------------------------------------------------------------
# SpMM on the matrix cores (left_spmm, half tiles): criterion of test_left_spmm_half_tiles_vs_oracle
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", STRUCTURED_KINDS)
@pytest.mark.parametrize("route", SPMM_MFMA_ROUTES, ids=ids(SPMM_MFMA_ROUTES))
def test_left_spmm_half_tiles_structured(capi, dev, knobs, route, kind):
    m, k, n = route.m, route.k, route.n
    for order, replicas, shuffle in SDDMM_FORMS:
        ri, ro, ci = route.mask(kind, order, shuffle)
        nnz = len(ci)
        rng = np.random.default_rng(nnz + replicas)
        v, v32 = rounded(uniform(rng, (nnz,)), route.dtype, dev)
        b, b32 = rounded(uniform(rng, (replicas, k, n)), route.dtype, dev)
        want = O.left_spmm(m, k, v32, ri, ro, ci, b32)
        route.set_knobs(capi, knobs)
        route.assert_reached(capi, nnz, replicas, kind)
        what = f"{route.id} {kind} {order} x{replicas} shuffle={shuffle}"
        ws_bytes = capi.left_spmm_half_tiles_workspace_bytes(m, k, n, nnz, replicas, v, b, route.dtype)
        assert ws_bytes > 0, f"{what}: the matrix-core route does not serve the call"
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.full((replicas, m, n + 8), float("nan"), device=dev)[:, :, :n].contiguous()
        capi.left_spmm_half_tiles(m, k, n, replicas, T(ro, dev), T(ci, dev), v, b, route.dtype, out, ws)
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"{what}: some output elements were never written"
        err = rel_err(got, want)
        assert err < TOL, f"{what}: rel_err {err:.3g}"
        assert np.all(got[:, empty_rows(ro)] == 0), f"{what}: an empty row is not exactly 0"


# ----------------------------------------------------------------------------
# SDDMM, plain: float32 (row-wave, quad, stationary at every panel width, the accumulating
# launches, pair-flat) and half (quad with float32 / half output, pair-flat)
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", STRUCTURED_KINDS)
@pytest.mark.parametrize("route", SDDMM_ROUTES + SDDMM_HALF_ROUTES, ids=ids(SDDMM_ROUTES + SDDMM_HALF_ROUTES))
def test_sddmm_structured(capi, dev, knobs, route, kind):
    m, k, n = route.m, route.k, route.n
    for order, replicas, shuffle in SDDMM_FORMS:
        ri, ro, ci = route.mask(kind, order, shuffle)
        nnz = len(ci)
        rng = np.random.default_rng(nnz + replicas)
        lhs, lhs32 = rounded(uniform(rng, (replicas, m, k)), route.dtype, dev)
        rhs, rhs32 = rounded(uniform(rng, (replicas, n, k)), route.dtype, dev)
        want = c_oracle.sddmm(m, n, ro, ci, lhs32, rhs32)
        route.set_knobs(capi, knobs)
        name = route.assert_reached(capi, nnz, replicas, kind)
        what = f"{route.id} {kind} {order} x{replicas} shuffle={shuffle} [{name}]"
        topo = (T(ri, dev), T(ro, dev), T(ci, dev))
        ws = torch.empty(capi.sddmm_workspace_bytes(m, k, n, nnz) + 16, dtype=torch.uint8, device=dev)
        out = torch.full((replicas, nnz), float("nan"), device=dev,
                         dtype=route.dtype if route.out_half else torch.float32)
        if route.planned:
            capi.sddmm_plan(m, k, n, *topo, ws)
        capi.sddmm_typed(m, k, n, replicas, *topo, lhs, rhs, out, ws, planned=route.planned)
        got = out.float().cpu().numpy()
        assert not np.isnan(got).any(), f"{what}: an entry was never written"
        err = half_err(got, want, route.dtype, ro) if route.out_half else rel_err(got, want, ro)
        assert err < TOL, f"{what}: error {err:.3g}"


# ----------------------------------------------------------------------------
# SDDMM summed over the replicas (the weight gradient of SparseLinear): row-wave partials,
# tiled partials (128-wide; 256-wide on 80- and 128-row slabs), the matrix cores (half, mixed)
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", STRUCTURED_KINDS)
@pytest.mark.parametrize("route", SDDMM_SUM_ROUTES, ids=ids(SDDMM_SUM_ROUTES))
def test_sddmm_sum_structured(capi, dev, knobs, route, kind):
    m, k, n = route.m, route.k, route.n
    for order, replicas, shuffle in SDDMM_FORMS[1:]:
        ri, ro, ci = route.mask(kind, order, shuffle)
        nnz = len(ci)
        rng = np.random.default_rng(nnz + replicas)
        if route.mixed:   # the float32 operand keeps its full mantissa
            lhs32 = uniform(rng, (replicas, m, k))
            lhs = T(lhs32, dev)
        else:
            lhs, lhs32 = rounded(uniform(rng, (replicas, m, k)), route.dtype, dev)
        rhs, rhs32 = rounded(uniform(rng, (replicas, n, k)), route.dtype, dev)
        want = c_oracle.sddmm(m, n, ro, ci, lhs32, rhs32).astype(np.float64).sum(axis=0)
        route.set_knobs(capi, knobs)
        name = route.assert_reached(capi, nnz, replicas, kind)
        what = f"{route.id} {kind} {order} x{replicas} shuffle={shuffle} [{name}]"
        topo = (T(ri, dev), T(ro, dev), T(ci, dev))
        ws = torch.empty(capi.sddmm_sum_workspace_bytes(m, k, n, nnz) + 16, dtype=torch.uint8, device=dev)
        scratch_bytes = (capi.sddmm_sum_mixed_scratch_bytes(m, k, n, nnz, replicas, lhs, rhs) if route.mixed
                         else capi.sddmm_sum_scratch_bytes(m, k, n, nnz, replicas))
        scratch = torch.empty(scratch_bytes + 16, dtype=torch.uint8, device=dev)
        out = torch.full((nnz,), float("nan"), device=dev)
        if route.planned:
            capi.sddmm_sum_plan(m, k, n, *topo, ws)
        call = capi.sddmm_sum_mixed if route.mixed else capi.sddmm_sum_typed
        call(m, k, n, replicas, *topo, lhs, rhs, out, ws, scratch, planned=route.planned)
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"{what}: an entry was never written"
        # one row of `replicas * k` products per entry: the tolerance scales as for one long row
        err = rel_err(got[None, :], want[None, :].astype(np.float32), ro)
        assert err < TOL, f"{what}: rel_err {err:.3g}"



@gpu
def test_panel_knob_reaches_the_panel_kernel_where_a_device_offers_its_lds(capi, dev, monkeypatch):
    """The knob enumeration of tests/test_host_logic.py cannot ask a host without a device about
    the panel kernel (it is taken where the device offers 128 KiB of LDS per workgroup): here,
    with one, at least one static shape of every test parametrized over `spmm_kernel` must
    reach it under the "panel" knob."""
    from test_host_logic import knob_fall_through
    counts = knob_fall_through(monkeypatch)
    panel = {test: reached for (test, knob), (reached, _, _) in counts.items() if knob == "panel"}
    assert panel and all(reached >= 1 for reached in panel.values()), panel
