"""GPU: the device topology build (csrc/topology.hip; ops.dense_to_csr, ops.row_order and the
four routed functions of topology / functional) against the torch path on the CPU copy of the
same input.  Everything is an integer or a bit copy: every comparison is exact.

Instance parameters (rows per wave, elements per lane, rows per workgroup, the row-order
limit) come from the host queries the launches themselves decide by, not from constants."""
import pytest
import torch

from torch_sputnik_amd import capi, functional, ops, topology
from torch_sputnik_amd.modules import SparseCoreAttention

pytestmark = pytest.mark.gpu

W = 64
DTYPES = [torch.bool, torch.int8, torch.int16, torch.float16, torch.bfloat16, torch.int32,
          torch.float32, torch.int64, torch.float64]
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def reference_3d(dense):
    """The torch path on the CPU copy (CPU tensors never take the device build)."""
    return topology.dense_to_sparse_3d(dense.cpu())


def check_3d(got, want):
    for g, w, name in zip(got[:3], want[:3], ("row_indices", "row_offsets", "column_indices")):
        assert g.dtype == torch.int32 and g.is_cuda, name
        assert g.shape == w.shape and torch.equal(g.cpu(), w), name
    assert isinstance(got[3], list) and got[3] == want[3]


def specials(dtype):
    """-0.0 (no entry), NaN, +-inf and the smallest denormal (entries) of a floating type."""
    denormal = torch.ones(1, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)
    return torch.cat([torch.tensor([-0.0, float("nan"), float("inf"), -float("inf")], dtype=dtype), denormal])


def make_masks(b, m, n, dtype, generator, densities):
    """[b, m, n]: mask i random at densities[i] (None: no entry at all, 1: full); mask 0 also
    gets an empty row, a full row, a row holding only the last column and one holding only
    column 0 (as many of them as m has rows).  Floating types carry the special values."""
    x = torch.zeros(b, m, n, dtype=torch.float64)
    for i, density in enumerate(densities):
        if density is not None:
            x[i] = (torch.rand(m, n, generator=generator) < density).to(torch.float64)
    rows = iter(range(m - 1, -1, -1))   # from the last row down: m = 1 gets the empty row
    for kind in ("empty", "full", "last", "first"):
        r = next(rows, None)
        if r is None:
            break
        x[0, r] = 1.0 if kind == "full" else 0.0
        if kind == "last":
            x[0, r, n - 1] = 1.0
        if kind == "first":
            x[0, r, 0] = 1.0
    if not dtype.is_floating_point:
        return x.to(dtype) if dtype == torch.bool else (x * 3).to(dtype)
    x = (x * (torch.rand(b, m, n, generator=generator, dtype=torch.float64) + 0.5)).to(dtype)
    flat = x[0].reshape(-1)   # (a view: the first elements of mask 0; its special rows are the last ones)
    for j, special in enumerate(specials(dtype)):
        flat[j::7][:5] = special
    return x


def boundaries(element_bytes):
    """Every n that is the last of a rows-per-wave instance, read from the query."""
    v = capi.dense_to_csr_launch_shape(1, 1, 1, element_bytes)["elements_per_lane"]
    found, previous = [], None
    for n in range(1, W * v + 2):
        rows = capi.dense_to_csr_launch_shape(1, 1, n, element_bytes)["rows_per_wave"]
        if previous is not None and rows != previous:
            found.append(n - 1)
        previous = rows
    assert len(found) == 4 and previous == 1   # 16 -> 8 -> 4 -> 2 -> 1 rows per wave
    return v, found


def shapes(element_bytes):
    v, found = boundaries(element_bytes)
    widths = {1, W - 1, W, W + 1, W * v - 1, W * v, W * v + 1, 2 * W * v + 3}
    for n in found:
        widths |= {n, n + 1}
    for n in sorted(widths):
        r = capi.dense_to_csr_launch_shape(1, 1, n, element_bytes)["rows_per_workgroup"]
        for m in sorted({1, r - 1, r, r + 1}):
            yield m, n


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_count_and_fill_every_instance(dtype):
    generator = torch.Generator().manual_seed(1234)
    element_bytes = torch.empty(0, dtype=dtype).element_size()
    for m, n in shapes(element_bytes):
        for b, densities in ((1, (0.05,)), (1, (0.5,)), (3, (0.05, None, 1)), (3, (0.5, 0.05, 0.5))):
            host = make_masks(b, m, n, dtype, generator, densities)
            want = reference_3d(host)
            out = ops.dense_to_csr(host.cuda(), False)
            assert out[3].dtype == torch.int64 and out[3].device.type == "cpu"
            got = (out[0], out[1], out[2], out[3].tolist())
            try:
                check_3d(got, want)
            except AssertionError as error:
                raise AssertionError(f"b={b} m={m} n={n} densities={densities}: {error}") from error
            check_3d(topology.dense_to_sparse_3d(host.cuda()), want)


def test_views():
    generator = torch.Generator().manual_seed(77)
    s = 70
    host = (torch.rand(3, 1, s, s, generator=generator) < 0.3).to(torch.int64)
    device = host.cuda()
    check_3d(topology.dense_to_sparse_3d(device), reference_3d(host))                 # [b, 1, s, s]
    one = device[:1, 0]
    expanded = one.expand(4, s, s)                                                    # batch stride 0
    assert expanded.stride(0) == 0
    check_3d(topology.dense_to_sparse_3d(expanded), reference_3d(expanded))
    rows = device[:, 0, ::2, :]                                                       # row-strided
    assert rows.stride(1) == 2 * s and not rows.is_contiguous()
    check_3d(topology.dense_to_sparse_3d(rows), reference_3d(rows))
    columns = device[:, 0, :, ::2]                                                    # last stride 2: copied
    assert columns.stride(2) == 2
    check_3d(topology.dense_to_sparse_3d(columns), reference_3d(columns))
    sliced = device[:, 0].to(torch.bool)[:, 1:, 3:]                                   # row starts off the wide load
    assert sliced.stride(2) == 1 and sliced.storage_offset() % 16 != 0
    check_3d(topology.dense_to_sparse_3d(sliced), reference_3d(sliced))
    single = topology.dense_to_sparse_3d(device[:1])                                  # b = 1 keeps its batch dimension
    assert single[0].shape == (1, s) and single[1].shape == (1, s + 1) and len(single[3]) == 1
    check_3d(single, reference_3d(host[:1]))
    with pytest.raises(ValueError):
        topology.dense_to_sparse_3d(device[0, 0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16],
                         ids=lambda d: str(d).split(".")[-1])
def test_dense_to_sparse_with_values(dtype):
    generator = torch.Generator().manual_seed(99)
    bits = BITS[torch.empty(0, dtype=dtype).element_size()]
    for m, n in ((1, 1), (5, 3), (33, 129), (70, 515), (3, 0), (0, 3)):
        host = make_masks(1, m, n, dtype, generator, (0.4,))[0] if m * n else torch.zeros(m, n, dtype=dtype)
        want = topology.dense_to_sparse(host)
        weight = host.cuda().requires_grad_()
        got = topology.dense_to_sparse(weight)
        out = ops.dense_to_csr(host.cuda(), True)
        for g, w, name in zip(got, want, ("values", "row_indices", "row_offsets", "column_indices")):
            assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (name, m, n)
            if name == "values":
                assert not g.requires_grad and (g.numel() == 0 or g.data_ptr() != weight.data_ptr())
                assert torch.equal(g.view(bits).cpu(), w.view(bits)), (name, m, n)
                assert torch.equal(out[4].view(bits).cpu(), w.view(bits))
            else:
                assert torch.equal(g.cpu(), w), (name, m, n)
        assert out[3].tolist() == [want[3].numel()]


def offsets_of(lengths):
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    zero = torch.zeros(lengths.shape[:-1] + (1,), dtype=torch.int64)
    return torch.cat([zero, lengths.cumsum(-1)], -1).to(torch.int32)


def check_order(offsets):
    """ops.row_order and the routed diffsort against torch.argsort on the CPU."""
    per_mask = offsets.reshape(-1, offsets.size(-1))
    want = torch.stack([topology.diffsort(o) for o in per_mask]).reshape(offsets.shape[:-1] + (-1,))
    got = ops.row_order(offsets.cuda())
    assert got.dtype == torch.int32 and got.shape == want.shape and torch.equal(got.cpu(), want)
    return want


def test_row_order_cases():
    for m in (1, 2, W, W + 1):
        identity = check_order(offsets_of([5] * m))                         # all equal
        assert identity.tolist() == list(range(m))
        reversal = check_order(offsets_of(list(range(m, 0, -1))))           # strictly descending
        assert reversal.tolist() == list(range(m - 1, -1, -1))
        ties = check_order(offsets_of([7 if r % 2 == 0 else 2 for r in range(m)]))   # two lengths interleaved
        assert ties.tolist() == list(range(1, m, 2)) + list(range(0, m, 2))
    generator = torch.Generator().manual_seed(3)
    n = 37
    mask = (torch.rand(3, 50, n, generator=generator) < 0.3)
    mask[1, 20] = True                                                      # a length equal to n
    _, row_offsets, _, _ = topology.dense_to_sparse_3d(mask)
    assert int((row_offsets[1, 21] - row_offsets[1, 20])) == n
    want = check_order(row_offsets)                                         # b = 3, different offsets per mask
    assert not torch.equal(want[0], want[1])
    flat = functional.diffsort_many_mask(row_offsets.cuda(), 3)
    assert flat.shape == (150,) and torch.equal(flat.cpu(), want.reshape(-1))
    assert torch.equal(topology.diffsort(row_offsets[2].cuda()).cpu(), want[2])


def test_row_order_at_the_instance_limits():
    small = capi.csr_row_order_route(1, 1, 0)["capacity"]
    limit = capi.csr_row_order_route(1, small + 1, 0)["capacity"]
    assert capi.csr_row_order_route(1, limit, 0)["served"] and not capi.csr_row_order_route(1, limit + 1, 0)["served"]
    generator = torch.Generator().manual_seed(8)
    for m in (small, small + 1, limit, limit + 1):
        lengths = torch.zeros(2, m, dtype=torch.int64)
        where = torch.randint(0, m, (2, 9), generator=generator)
        lengths.scatter_(1, where, torch.randint(1, 4, (2, 9), generator=generator))   # a few entries
        offsets = offsets_of(lengths)
        want = torch.stack([topology.diffsort(o) for o in offsets])
        if m <= limit:
            assert torch.equal(ops.row_order(offsets.cuda()).cpu(), want)
        else:
            with pytest.raises(RuntimeError):
                ops.row_order(offsets.cuda())
        # the routed functions serve every m: beyond the limit through torch.argsort
        assert torch.equal(topology.diffsort(offsets[0].cuda()).cpu(), want[0])
        assert torch.equal(functional.diffsort_many_mask(offsets.cuda(), 2).cpu(), want.reshape(-1))
    # a mask of limit + 1 rows takes the torch path as a whole and still matches
    tall = torch.zeros(1, limit + 1, 5, dtype=torch.bool)
    tall[0, ::1000, 2] = True
    check_3d(topology.dense_to_sparse_3d(tall.cuda()), reference_3d(tall))


def test_row_order_of_transposed_offsets():
    generator = torch.Generator().manual_seed(21)
    b, m, n = 3, 40, 90
    mask = torch.rand(b, m, n, generator=generator) < 0.2
    _, row_offsets, column_indices, nonzeros = topology.dense_to_sparse_3d(mask.cuda())
    values = torch.zeros(b, max(nonzeros), device="cuda")
    _, row_offsets_t, _ = ops.csr_transpose_many_mask(b, m, n, nonzeros, values, row_offsets, column_indices)
    assert row_offsets_t.shape == (b, n + 1)
    got = functional.diffsort_many_mask(row_offsets_t, b)
    want = reference_3d(mask.transpose(1, 2))
    assert torch.equal(row_offsets_t.cpu(), want[1])
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want[0].reshape(-1))


def graph_nodes_and_edges(raw_graph):
    """Nodes and (from, to) edges of a captured hipGraph, asked of the HIP runtime (host only)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")   # (the runtime torch has already loaded)
    handle = ctypes.c_void_p(int(raw_graph))
    count = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(count)) == 0
    nodes = (ctypes.c_void_p * max(count.value, 1))()
    assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(count)) == 0
    edge_count = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(handle, None, None, ctypes.byref(edge_count)) == 0
    sources = (ctypes.c_void_p * max(edge_count.value, 1))()
    targets = (ctypes.c_void_p * max(edge_count.value, 1))()
    if edge_count.value:
        assert hip.hipGraphGetEdges(handle, sources, targets, ctypes.byref(edge_count)) == 0
    return ([nodes[i] for i in range(count.value)],
            [(sources[i], targets[i]) for i in range(edge_count.value)])


def test_row_order_in_a_graph():
    """One launch, no synchronisation, no host knowledge of the data: the op is captured on a
    side stream and replayed on other offsets written into the same tensor."""
    generator = torch.Generator().manual_seed(31)
    masks = torch.rand(2, 3, 100, 60, generator=generator) < 0.25
    first, second = (reference_3d(x) for x in masks)
    static = first[1].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.row_order(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)   # (the captured graph stays open to the queries below)
    with torch.cuda.graph(graph):
        out = ops.row_order(static)
    nodes, edges = graph_nodes_and_edges(graph.raw_cuda_graph())
    # a single chain, no parallel branches: n nodes, n - 1 edges, no node with two successors or
    # two predecessors (here: the one kernel)
    assert len(nodes) >= 1 and len(edges) == len(nodes) - 1
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), first[0])
    static.copy_(second[1])
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first[0], second[0]) and torch.equal(out.cpu(), second[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_attention_with_a_dynamic_mask(dtype):
    generator = torch.Generator().manual_seed(41)
    b, heads, s, d = 2, 2, 72, 64
    q, k, v = (torch.randn(b, s, heads, d, generator=generator).to(dtype).cuda() for _ in range(3))
    mask = (torch.rand(b, 1, s, s, generator=generator) < 0.3).to(torch.int64)
    mask[:, 0, torch.arange(s), torch.arange(s)] = 1
    module = SparseCoreAttention(s, heads * d, heads).cuda().eval()
    row_indices, row_offsets, column_indices, nonzeros = topology.dense_to_sparse_3d(mask)
    moved = (row_indices.cuda(), row_offsets.cuda(), column_indices.cuda(), nonzeros)
    with torch.no_grad():
        want = module(q, k, v, topology=moved)
        got = module(q, k, v, mask.cuda())
    bits = BITS[got.element_size()]
    assert got.dtype == want.dtype and torch.equal(got.view(bits), want.view(bits))
