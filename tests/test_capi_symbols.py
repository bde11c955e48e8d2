"""CPU: the C-ABI library loads and exports every symbol include/sputnik_hip.h
declares; the ctypes signature table covers exactly that set.  No compute."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(REPO, "include", "sputnik_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sputnik_hip_\w+)\s*\(", text)))


def test_header_declares_the_surface():
    names = declared_symbols()
    for must in ("sputnik_hip_spmm", "sputnik_hip_spmm_batched", "sputnik_hip_sddmm",
                 "sputnik_hip_sddmm_batched", "sputnik_hip_sparse_softmax",
                 "sputnik_hip_sparse_softmax_batched", "sputnik_hip_csr_transpose",
                 "sputnik_hip_csr_transpose_workspace_bytes", "sputnik_hip_spmm_workspace_bytes"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from torch_sputnik_amd import _native
    lib = ctypes.CDLL(_native.KERNEL_LIB)
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in sputnik_hip.h but not exported"


def test_ctypes_table_matches_header():
    from torch_sputnik_amd import capi
    assert sorted(capi.SIGNATURES) == declared_symbols()
    capi.lib()  # binds every signature; AttributeError on a missing symbol
    assert "gfx950" in capi.version()


def test_workspace_queries_are_host_only():
    from torch_sputnik_amd import capi
    assert capi.spmm_workspace_bytes(4096, 4096, 4096, 1677724) > 0
    assert capi.spmm_workspace_bytes(64, 64, 64, 2048) > 0       # 64-column tiled kernel
    assert capi.spmm_workspace_bytes(72, 64, 72, 464) > 0        # n = 64 + 8: partial column tile
    assert capi.spmm_workspace_bytes(72, 64, 70, 464) > 0        # any n >= 64 stays on the 64-column kernel
    assert capi.spmm_workspace_bytes(72, 64, 7, 464) == 0        # narrower than a tile: row-gather kernel
    assert capi.sddmm_workspace_bytes(1024, 64, 1024, 104860) > 0
    assert capi.sddmm_workspace_bytes(72, 72, 72, 500) == 0
    assert capi.csr_transpose_workspace_bytes(2048, 2048, 838864) >= 4 * 2048
    assert capi.csr_transpose_workspace_bytes(0, 0, 0) == 0


def test_sddmm_launch_query_is_host_only():
    """sputnik_hip_sddmm_launch_shape runs the launch path without a device and reports the
    instance and the grid: the row-wave kernel below the tiled route's shapes, and the LDS
    kernels' family, panel, slab, passes and grid at config 3's shape (1024 x 64 x 1024)."""
    import torch
    from torch_sputnik_amd import capi
    assert "sputnik_hip_sddmm_launch_shape" in declared_symbols()
    assert set(capi.SDDMM_FAMILIES) == {"rowwave", "flat", "quad", "stationary", "mfma"}
    assert capi.sddmm_launch_shape(72, 72, 72, 500, 1)["family"] == "rowwave"
    shape = capi.sddmm_launch_shape(1024, 64, 1024, 104860, 64)
    assert shape == dict(family="quad", panel_width=64, slab_rows=256, passes=1, accumulates=False,
                         grid_x=4, grid_y=4, grid_z=64, row_blocks=4)
    assert capi.sddmm_launch_shape(1024, 64, 1024, 104860, 64, planned=True)["family"] == "flat"
    half = capi.sddmm_launch_shape(1024, 512, 1024, 104860, 8, torch.float16)
    assert (half["family"], half["panel_width"], half["slab_rows"], half["passes"], half["accumulates"]) == \
        ("quad", 256, 64, 2, True)


def test_spmm_launch_query_is_host_only():
    """sputnik_hip_spmm_launch_shape runs the launch path without a device and reports the
    family and, for the LDS-tiled kernels, the instance, the grid and the workspace offsets:
    the row gather below the tiled routes' shapes, the flat-stream kernel at the headline shape,
    the 256-column kernel on 128-row tiles for 16 replicas of 2048 x 2048 x 256."""
    from torch_sputnik_amd import capi
    assert "sputnik_hip_spmm_launch_shape" in declared_symbols()
    assert set(capi.SPMM_FAMILIES) == {"rowgather", "panel", "narrow64", "wide256", "wide512", "flat"}
    assert capi.spmm_launch_shape(72, 64, 7, 464, 1)["family"] == "rowgather"
    assert capi.spmm_launch_shape(4096, 4096, 4096, 1677724, 1)["family"] == "flat"
    shape = capi.spmm_launch_shape(2048, 2048, 256, 838860, 16)
    bytes_ = capi.spmm_workspace_bytes(2048, 2048, 256, 838860)
    assert shape == dict(family="wide256", tile_cols=256, tile_rows=128, waves=16, rows_per_wave=8, chunk=64,
                         sparse=True, batch=8, grid_x=16, grid_y=16, slots=2048, nchunks=32, n_tiles=1,
                         ksplits=1, workspace_bytes=bytes_, row_ok_offset=0, table_offset=8192,
                         partials_offset=-1)


def test_ops_registered_without_cpu_kernels():
    """The product registers HIP kernels only: CPU tensors must raise."""
    import pytest
    import torch
    import torch_sputnik
    for name in ("spmm", "left_spmm", "left_replicated_spmm", "sddmm", "sparse_softmax",
                 "csr_transpose"):
        assert callable(getattr(torch_sputnik, name))
    has_cpu = torch._C._dispatch_has_kernel_for_dispatch_key("torch_sputnik::spmm", "CPU")
    if not has_cpu:  # (another test module may have installed the oracle backend)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch_sputnik.spmm(2, 2, torch.ones(2), torch.arange(2, dtype=torch.int32),
                               torch.tensor([0, 1, 2], dtype=torch.int32),
                               torch.tensor([0, 1], dtype=torch.int32), torch.ones(2, 2))
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torch_sputnik::spmm", "CUDA")
