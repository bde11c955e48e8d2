"""CPU: the host side of the device topology build (csrc/topology.hip).

The two host-only queries answer without a device and change instance where DESIGN.md says;
invalid sizes are rejected; CPU tensors keep the torch path whether the device build is
enabled or not; and the reference semantics the kernels must reproduce (torch's ``x != 0``
on -0.0, NaN, inf and denormals; an all-zero mask) are pinned on the CPU."""
import pytest
import torch

from torch_sputnik_amd import capi, functional, topology

INT_MAX = 2 ** 31 - 1


@pytest.mark.parametrize("element_bytes", [1, 2, 4, 8])
def test_build_query_instances_and_boundaries(element_bytes):
    """elements_per_lane = one 16-byte load; rows_per_wave halves above n = 4, 8, 16 and 32
    times elements_per_lane; four waves per workgroup; the grid is masks x
    row blocks."""
    v = 16 // element_bytes
    changes = {}
    previous = None
    for n in range(0, 64 * v + 2):
        shape = capi.dense_to_csr_launch_shape(3, 100, n, element_bytes)
        assert shape["elements_per_lane"] == v
        assert shape["rows_per_workgroup"] == 4 * shape["rows_per_wave"]
        assert shape["grid"] == 3 * -(-100 // shape["rows_per_workgroup"])
        if previous is not None and shape["rows_per_wave"] != previous:
            changes[n - 1] = (previous, shape["rows_per_wave"])   # the last n of the old instance
        previous = shape["rows_per_wave"]
    assert changes == {4 * v: (16, 8), 8 * v: (8, 4), 16 * v: (4, 2), 32 * v: (2, 1)}
    assert capi.dense_to_csr_launch_shape(0, 0, 0, element_bytes)["grid"] == 0
    assert capi.dense_to_csr_launch_shape(8, 1024, 1024, element_bytes)["rows_per_wave"] == 1


def test_build_query_rejects_invalid_arguments():
    for args in ((-1, 4, 4, 1), (1, -4, 4, 1), (1, 4, -4, 1), (1, 4, 4, 3), (1, 4, 4, 0),
                 (1, 4, 4, 16), (1, 65536, 32768, 1),          # m * n = 2^31: beyond int32 offsets
                 (INT_MAX, INT_MAX, 1, 1)):                     # more workgroups than a grid holds
        with pytest.raises(RuntimeError):
            capi.dense_to_csr_launch_shape(*args)
    assert capi.dense_to_csr_launch_shape(1, 65536, 32767, 8)["rows_per_wave"] == 1


def test_build_entries_reject_invalid_arguments_without_a_launch():
    """The entries ask the same function first: a rejected size returns before any pointer is
    touched or anything is launched."""
    lib = capi.lib()
    invalid = -1   # SPUTNIK_HIP_INVALID_ARGUMENT
    assert lib.sputnik_hip_dense_to_csr_count(1, 4, 4, None, 3, 0, 0, 4, None, None, None, None) == invalid
    assert lib.sputnik_hip_dense_to_csr_count(1, -4, 4, None, 1, 0, 0, 4, None, None, None, None) == invalid
    assert lib.sputnik_hip_dense_to_csr_count(1, 65536, 32768, None, 1, 0, 0, 4, None, None, None, None) == invalid
    assert lib.sputnik_hip_dense_to_csr_fill(1, 4, 4, None, 5, 0, 0, 4, None, None, None, None, None) == invalid
    assert lib.sputnik_hip_dense_to_csr_fill(-1, 4, 4, None, 4, 0, 0, 4, None, None, None, None, None) == invalid
    assert lib.sputnik_hip_csr_row_order(1, -1, 4, None, None, None) == invalid
    assert lib.sputnik_hip_csr_row_order(1, 16385, 4, None, None, None) == invalid


def test_row_order_query_limit_and_instances():
    small = capi.csr_row_order_route(1, 1, 0)
    assert small == dict(served=True, capacity=2048, threads=256, sort_size=1)
    assert capi.csr_row_order_route(8, 1024, 1024) == dict(served=True, capacity=2048, threads=256,
                                                         sort_size=1024)
    assert capi.csr_row_order_route(8, 1025, 1024)["sort_size"] == 2048
    assert capi.csr_row_order_route(1, 2048, 7)["capacity"] == 2048
    large = capi.csr_row_order_route(1, 2049, 7)
    assert large == dict(served=True, capacity=16384, threads=1024, sort_size=4096)
    limit = large["capacity"]
    assert capi.csr_row_order_route(3, limit, INT_MAX) == dict(served=True, capacity=16384, threads=1024,
                                                               sort_size=16384)
    assert capi.csr_row_order_route(3, limit + 1, 4) == dict(served=False, capacity=-1, threads=-1,
                                                             sort_size=-1)
    assert capi.csr_row_order_route(0, 0, 0)["served"]
    for args in ((-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        with pytest.raises(RuntimeError):
            capi.csr_row_order_route(*args)


def _all_outputs(mask3d, matrix):
    out = list(topology.dense_to_sparse_3d(mask3d))
    out += list(topology.dense_to_sparse(matrix))
    offsets = out[1]
    out.append(topology.diffsort(offsets[0]))
    out.append(functional.diffsort_many_mask(offsets, offsets.size(0)))
    return out


def test_cpu_tensors_keep_the_torch_path():
    generator = torch.Generator().manual_seed(5)
    mask = (torch.rand(3, 1, 9, 13, generator=generator) < 0.4).to(torch.int64)
    matrix = torch.randn(7, 11, generator=generator) * (torch.rand(7, 11, generator=generator) < 0.5)
    assert topology.enable_device_build(False) is False
    try:
        want = _all_outputs(mask, matrix)
    finally:
        assert topology.enable_device_build() is True
    got = _all_outputs(mask, matrix)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.device.type == "cpu" and torch.equal(g, w)
        else:
            assert g == w and isinstance(g, list)
    import torch_sputnik_amd
    assert torch_sputnik_amd.enable_device_build is topology.enable_device_build


def test_reference_edge_semantics():
    """What the kernels must reproduce, as torch computes it on the CPU."""
    x = torch.tensor([[0., -0., float("nan")], [1e-45, float("inf"), 0.]])
    values, row_indices, row_offsets, column_indices = topology.dense_to_sparse(x)
    assert column_indices.tolist() == [2, 0, 1] and row_offsets.tolist() == [0, 1, 3]
    assert row_indices.tolist() == [0, 1]
    assert values.view(torch.int32).tolist() == x[[0, 1, 1], [2, 0, 1]].view(torch.int32).tolist()
    assert all(t.dtype == torch.int32 for t in (row_indices, row_offsets, column_indices))
    _, row_indices, row_offsets, column_indices = topology.dense_to_sparse(x.to(torch.float16))
    assert column_indices.tolist() == [2, 1] and row_offsets.tolist() == [0, 1, 2]   # 1e-45 rounds to 0
    assert row_indices.tolist() == [0, 1]
    row_indices, row_offsets, column_indices, nonzeros = topology.dense_to_sparse_3d(x[None])
    assert column_indices.tolist() == [2, 0, 1] and row_offsets.tolist() == [[0, 1, 3]] and nonzeros == [3]

    row_indices, row_offsets, column_indices, nonzeros = topology.dense_to_sparse_3d(
        torch.zeros(1, 1, 4, 4, dtype=torch.bool))
    assert column_indices.shape == (0,) and column_indices.dtype == torch.int32
    assert row_offsets.tolist() == [[0] * 5] and row_indices.tolist() == [[0, 1, 2, 3]]
    assert nonzeros == [0]
