"""CPU: global magnitude pruning without a device -- the torch path of
topology.prune_csr_global against a plain Python restatement (a list of (key, layer, index)
sorted by key descending, then layer, then index; the first K taken), and
topology.prune_layers_to on CPU modules.  Everything is an integer or a bit copy: every
comparison is exact, but for the one forward pass, whose bound is worked out where it is used."""
import ctypes

import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {2: torch.int16, 4: torch.int32}
ids = dict(ids=lambda d: str(d).split(".")[-1])


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()])


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def key_of(values, i):
    """the rule, restated on one Python integer: the bit pattern without the sign"""
    width = values.element_size() * 8
    return (int(bits_of(values)[i]) & ((1 << width) - 1)) & ((1 << (width - 1)) - 1)


def pattern(lengths, n, generator):
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    columns = [torch.sort(torch.randperm(n, generator=generator)[:int(length)]).values for length in lengths]
    row_offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    column_indices = torch.cat(columns + [torch.zeros(0, dtype=torch.int64)]).to(torch.int32)
    return row_offsets, column_indices


def specials(dtype):
    """NaN, +-inf, +-0, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.5, -0.5], dtype=dtype),
                      from_bits([1], dtype)])


def layer_of(lengths, n, dtype, generator, special_at=None):
    """(values, row_offsets, column_indices, n): values of few distinct magnitudes, mixed signs;
    ``special_at``: the special values from that entry on, every third entry"""
    row_offsets, column_indices = pattern(lengths, n, generator)
    nnz = column_indices.numel()
    values = ((torch.randn(nnz, generator=generator) / 0.25).round() * 0.25).to(dtype)
    if special_at is not None:
        s = specials(dtype)
        values[special_at::3][: s.numel()] = s[: values[special_at::3].numel()]
    return values, row_offsets, column_indices, n


def by_sort(layers, total):
    """per layer the kept entry indices, ascending: the rule as one Python sort.  Layers of one
    dtype rank by their own bits, mixed dtypes as float32."""
    mixed = len({layer[0].dtype for layer in layers}) > 1
    values = [layer[0].float() if mixed else layer[0] for layer in layers]
    entries = [(-key_of(v, i), l, i) for l, v in enumerate(values) for i in range(v.numel())]
    kept = [[] for _ in layers]
    for _, l, i in sorted(entries)[:total]:
        kept[l].append(i)
    return [sorted(k) for k in kept]


def check_against_sort(layers, total):
    results = topology.prune_csr_global(layers, total)
    wants = by_sort(layers, total)
    assert len(results) == len(layers) and sum(len(w) for w in wants) == total
    for (values, row_offsets, column_indices, _), result, want in zip(layers, results, wants):
        row_indices, new_offsets, new_columns, new_values, source = result
        m = row_offsets.numel() - 1
        assert source.dtype == torch.int64 and source.tolist() == want
        assert new_columns.dtype == torch.int32 and torch.equal(new_columns, column_indices[want])
        assert new_values.dtype == values.dtype and torch.equal(bits_of(new_values), bits_of(values)[want])
        rows = torch.bucketize(torch.tensor(want, dtype=torch.int64), row_offsets[1:].to(torch.int64), right=True)
        want_offsets = torch.zeros(m + 1, dtype=torch.int32)
        want_offsets[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0)
        assert new_offsets.dtype == torch.int32 and torch.equal(new_offsets, want_offsets)
        lengths = new_offsets[1:] - new_offsets[:-1]
        assert row_indices.dtype == torch.int32
        assert torch.equal(row_indices, torch.argsort(lengths, stable=True).to(torch.int32))
    return results


def some_layers(dtype, generator):
    """three layers of different shapes: an empty row, a full row, short rows"""
    return [layer_of((2, 0, 9, 5, 13), 13, dtype, generator, special_at=1),
            layer_of((7, 7, 0), 7, dtype, generator),
            layer_of((1, 30, 4, 0, 0, 11), 30, dtype, generator, special_at=0)]


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_against_the_sort(dtype):
    generator = torch.Generator().manual_seed(51)
    layers = some_layers(dtype, generator)
    entries = sum(layer[0].numel() for layer in layers)
    for K in (0, 1, 5, entries // 3, entries // 2, entries - 1, entries):
        results = check_against_sort(layers, K)
        assert sum(r[4].numel() for r in results) == K
        assert all(int(r[1][-1]) == r[4].numel() for r in results)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_one_layer_is_prune_csr(dtype):
    generator = torch.Generator().manual_seed(52)
    layer = layer_of((2, 0, 9, 5, 13, 1), 13, dtype, generator, special_at=1)
    nnz = layer[0].numel()
    for K in (0, 1, nnz // 2, nnz - 1, nnz):
        (got,) = topology.prune_csr_global([layer], K)
        want = topology.prune_csr(*layer, total=K)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(bits_of(g) if g.is_floating_point() else g,
                                                      bits_of(w) if w.is_floating_point() else w)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_tie_quota_crosses_a_layer_boundary(dtype):
    """all magnitudes equal across three layers: the first K entries in layer order"""
    generator = torch.Generator().manual_seed(53)
    layers = []
    for lengths, n in (((3, 0, 4), 5), ((2, 6, 1), 6), ((5, 5), 5)):
        row_offsets, column_indices = pattern(lengths, n, generator)
        values = torch.where(torch.arange(column_indices.numel()) % 2 == 0, 1.5, -1.5).to(dtype)
        layers.append((values, row_offsets, column_indices, n))
    sizes = [layer[0].numel() for layer in layers]
    assert sizes == [7, 9, 10]
    for K in (7 + 4, 7, 7 + 9, 7 + 9 + 1, 3):               # inside the second layer first
        results = check_against_sort(layers, K)
        left = K
        for size, result in zip(sizes, results):
            assert result[4].tolist() == list(range(min(size, left)))
            left -= min(size, left)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_special_values_over_the_layers(dtype):
    """NaN, +-inf, +-0, the smallest denormal and x / -x, each in another layer than its partner"""
    generator = torch.Generator().manual_seed(54)
    s = specials(dtype)      # nan inf -inf 0 -0 x -x denormal
    spread = ([s[0], s[2], s[3], s[5]], [s[1], s[4], s[7]], [s[6], s[1], s[0], s[3]])
    layers = []
    for lengths, n, chosen in (((2, 3, 0, 2), 4, spread[0]), ((4, 1), 4, spread[1]), ((0, 3, 3), 3, spread[2])):
        values, row_offsets, column_indices, _ = layer_of(lengths, n, dtype, generator)
        at = torch.randperm(values.numel(), generator=generator)[: len(chosen)]
        values[at] = torch.stack(chosen)
        layers.append((values, row_offsets, column_indices, n))
    entries = sum(layer[0].numel() for layer in layers)
    for K in range(entries + 1):
        check_against_sort(layers, K)
    results = topology.prune_csr_global(layers, 2)            # the two NaN, above the three inf
    assert [r[4].numel() for r in results] == [1, 0, 1]
    assert all(torch.isnan(r[3]).all() for r in results)
    results = topology.prune_csr_global(layers, 5)
    assert all(bool((torch.isnan(r[3]) | torch.isinf(r[3])).all()) for r in results)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_empty_layers_and_empty_rows(dtype):
    generator = torch.Generator().manual_seed(55)
    layers = [layer_of((0, 0, 0), 4, dtype, generator),               # rows but no entry
              layer_of((0, 5, 0, 0, 2), 5, dtype, generator),
              layer_of((), 3, dtype, generator),                      # no row
              layer_of((3,), 3, dtype, generator)]
    for K in (0, 1, 4, 9, 10):
        results = check_against_sort(layers, K)
        assert results[0][4].numel() == results[2][4].numel() == 0
        assert results[0][0].tolist() == [0, 1, 2] and results[2][1].tolist() == [0]
    assert topology.prune_csr_global([], 0) == []
    emptied = topology.prune_csr_global([(torch.tensor([0.25, -0.25]), torch.tensor([0, 2], dtype=torch.int32),
                                          torch.tensor([0, 1], dtype=torch.int32), 2),
                                         (torch.tensor([1.0, -2.0, 3.0]), torch.tensor([0, 1, 3], dtype=torch.int32),
                                          torch.tensor([0, 0, 1], dtype=torch.int32), 2)], 3)
    assert emptied[0][4].numel() == 0 and emptied[0][1].tolist() == [0, 0]      # a layer may end empty
    assert emptied[1][4].tolist() == [0, 1, 2]


def test_mixed_dtypes_rank_as_float():
    generator = torch.Generator().manual_seed(56)
    layers = [layer_of((2, 0, 9, 5), 13, torch.float32, generator, special_at=1),
              layer_of((7, 7, 0), 7, torch.float16, generator, special_at=0),
              layer_of((1, 12, 4), 30, torch.bfloat16, generator, special_at=2)]
    entries = sum(layer[0].numel() for layer in layers)
    for K in (0, 1, entries // 3, entries // 2, entries - 1, entries):
        results = check_against_sort(layers, K)
        assert [r[3].dtype for r in results] == [torch.float32, torch.float16, torch.bfloat16]
    wide = [(layers[0][0].double(),) + layers[0][1:], layers[1]]
    got = topology.prune_csr_global(wide, 20)
    want = topology.prune_csr_global([layers[0], layers[1]], 20)
    assert got[0][3].dtype == torch.float64
    assert all(torch.equal(g[4], w[4]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))


def test_argument_errors():
    generator = torch.Generator().manual_seed(57)
    layers = some_layers(torch.float32, generator)
    entries = sum(layer[0].numel() for layer in layers)
    values, row_offsets, column_indices = ([layer[i] for layer in layers] for i in range(3))
    for bad in (-1, entries + 1, None):
        with pytest.raises(ValueError):
            topology.prune_csr_global(layers, bad)
        with pytest.raises(ValueError):
            ops.csr_topk_global(values, row_offsets, column_indices, bad)
    with pytest.raises(ValueError):
        ops.csr_topk_global(values, row_offsets[:-1], column_indices, 1)          # lists of unequal length
    with pytest.raises(ValueError):
        ops.csr_topk_global(values, row_offsets, column_indices + [column_indices[0]], 1)
    with pytest.raises(ValueError):
        topology.prune_csr_global([layers[0], layers[1][:3]], 1)                  # a layer without its n
    elsewhere = torch.empty(layers[1][0].numel(), device="meta")
    with pytest.raises(ValueError):                                               # tensors on different devices
        topology.prune_csr_global([layers[0], (elsewhere,) + layers[1][1:]], 1)
    with pytest.raises(ValueError):
        ops.csr_topk_global([values[0], elsewhere], row_offsets[:2], column_indices[:2], 1)
    with pytest.raises(ValueError):
        topology.prune_csr_global([layers[0][:1] + (layers[0][1].to("meta"),) + layers[0][2:]], 1)
    with pytest.raises(ValueError):
        topology.prune_csr_global([(layers[0][0], layers[0][1].long()) + layers[0][2:]], 1)
    with pytest.raises(ValueError):
        topology.prune_csr_global([(layers[0][0][:-1],) + layers[0][1:]], 1)
    with pytest.raises(ValueError):
        ops.csr_topk_global([v.double() for v in values], row_offsets, column_indices, 1)
    with pytest.raises(ValueError):
        ops.csr_topk_global([values[0], values[1].half()], row_offsets[:2], column_indices[:2], 1)   # mixed dtypes
    with pytest.raises(RuntimeError):
        ops.csr_topk_global(values, row_offsets, column_indices, 1)               # CPU tensors: device only
    assert ops.csr_topk_global([], [], [], 0) == []


def test_launch_shape_query_is_host_only():
    limit = 16384
    for value_bytes in (2, 4):
        shape = capi.csr_topk_global_launch_shape([limit, 3, 0], [100, 7, 0], value_bytes)
        assert shape["served"] and shape["digit_passes"] == value_bytes
        assert shape["elements_per_workgroup"] == 8 * 256 * (16 // value_bytes)
        c = shape["layers_per_launch"]
        assert c >= 2 and shape["digit_launches"] == 1
        for layers, launches in ((c - 1, 1), (c, 1), (c + 1, 2), (2 * c + 1, 3)):
            assert capi.csr_topk_global_launch_shape([2] * layers, [3] * layers, value_bytes)["digit_launches"] == launches
    beyond = capi.csr_topk_global_launch_shape([3, limit + 1], [7, 100], 4)
    assert not beyond["served"] and beyond["layers_per_launch"] == -1
    many = capi.csr_topk_global_launch_shape([3, 3], [2 ** 30, 2 ** 30], 4)       # sum nnz above INT_MAX
    assert not many["served"]
    assert capi.csr_topk_global_launch_shape([3, 3], [2 ** 30, 2 ** 30 - 1], 4)["served"]
    assert capi.csr_topk_global_launch_shape([], [], 4)["served"]
    for args in (([-1], [4], 4), ([4], [-1], 4), ([4], [4], 8), ([4], [4], 1)):
        with pytest.raises(RuntimeError):
            capi.csr_topk_global_launch_shape(*args)
    with pytest.raises(ValueError):
        capi.csr_topk_global_launch_shape([4, 4], [4], 4)


def test_c_abi_rejects_bad_arguments_without_a_device():
    lib = capi.lib()
    invalid = -1   # SPUTNIK_HIP_INVALID_ARGUMENT
    buffer = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buffer) + 15) // 16 * 16          # host memory: every call is rejected before a launch
    big = 1 << 20

    def ints(*xs):
        return (ctypes.c_int * len(xs))(*xs)

    def i64s(*xs):
        return (ctypes.c_int64 * len(xs))(*xs)

    def ptrs(*xs):
        return (ctypes.c_void_p * len(xs))(*xs)

    rows, nnz, good = ints(4, 2), ints(16, 3), ptrs(p, p)
    #   layers rows nnz offsets values vb count ws bytes out_offsets out_nonzeros
    select = (
        (2, rows, nnz, good, good, 8, 5, p, big, good, p),                 # value width
        (2, rows, nnz, good, good, 1, 5, p, big, good, p),
        (-1, rows, nnz, good, good, 4, 5, p, big, good, p),                # negative layers
        (2, None, nnz, good, good, 4, 5, p, big, good, p),                 # no rows
        (2, rows, None, good, good, 4, 5, p, big, good, p),                # no nonzeros
        (2, ints(4, -1), nnz, good, good, 4, 5, p, big, good, p),          # negative m
        (2, rows, ints(16, -1), good, good, 4, 5, p, big, good, p),        # negative nnz
        (2, ints(4, 16385), nnz, good, good, 4, 5, p, big, good, p),       # beyond the row order
        (2, rows, ints(2 ** 30, 2 ** 30), good, good, 4, 5, p, big, good, p),    # entries beyond int32
        (2, rows, nnz, good, good, 4, -1, p, big, good, p),                # negative count
        (2, rows, nnz, good, good, 4, 20, p, big, good, p),                # count above the entries
        (2, rows, nnz, None, good, 4, 5, p, big, good, p),                 # no offsets list
        (2, rows, nnz, ptrs(p, None), good, 4, 5, p, big, good, p),        # a layer without offsets
        (2, rows, nnz, ptrs(p + 2, p), good, 4, 5, p, big, good, p),       # misaligned offsets
        (2, rows, nnz, good, None, 4, 5, p, big, good, p),                 # no values list
        (2, rows, nnz, good, ptrs(None, p), 4, 5, p, big, good, p),        # a layer without values
        (2, rows, nnz, good, ptrs(p, p + 2), 4, 5, p, big, good, p),       # misaligned values
        (2, rows, nnz, good, good, 4, 5, None, big, good, p),              # no workspace
        (2, rows, nnz, good, good, 4, 5, p + 2, big, good, p),             # misaligned workspace
        (2, rows, nnz, good, good, 4, 5, p, 4 * (4 * 256 + 2 + 12) - 1, good, p),      # workspace too small
        (2, rows, nnz, good, good, 4, 5, p, big, None, p),                 # no out offsets list
        (2, rows, nnz, good, good, 4, 5, p, big, ptrs(None, p), p),        # a layer without out offsets
        (2, rows, nnz, good, good, 4, 5, p, big, good, None),              # no out_nonzeros
        (2, rows, nnz, good, good, 4, 5, p, big, good, p + 2),             # misaligned out_nonzeros
    )
    for call in select:
        assert lib.sputnik_hip_csr_topk_global_select(*call, None) == invalid, call
    capacity = i64s(4, 1)
    #   layers rows nnz offsets columns values vb ws bytes capacity row_indices offsets columns values source
    fill = (
        (2, rows, nnz, good, good, good, 8, p, big, capacity, good, good, good, good, good),      # value width
        (2, ints(4, 16385), nnz, good, good, good, 4, p, big, capacity, good, good, good, good, good),
        (2, rows, nnz, good, good, good, 4, p, big, None, good, good, good, good, good),          # no capacities
        (2, rows, nnz, good, good, good, 4, p, big, i64s(4, -1), good, good, good, good, good),   # negative capacity
        (2, rows, nnz, good, good, good, 4, p, big, i64s(17, 1), good, good, good, good, good),   # above nnz_l
        (2, rows, nnz, None, good, good, 4, p, big, capacity, good, good, good, good, good),
        (2, rows, nnz, good, ptrs(p, None), good, 4, p, big, capacity, good, good, good, good, good),
        (2, rows, nnz, good, good, ptrs(p + 2, p), 4, p, big, capacity, good, good, good, good, good),
        (2, rows, nnz, good, good, good, 4, None, big, capacity, good, good, good, good, good),   # no workspace
        (2, rows, nnz, good, good, good, 4, p, 64, capacity, good, good, good, good, good),       # too small
        (2, rows, nnz, good, good, good, 4, p, big, capacity, ptrs(p, None), good, good, good, good),
        (2, rows, nnz, good, good, good, 4, p, big, capacity, good, ptrs(None, p), good, good, good),
        (2, rows, nnz, good, good, good, 4, p, big, capacity, good, good, ptrs(p, None), good, good),
        (2, rows, nnz, good, good, good, 2, p, big, capacity, good, good, good, ptrs(p + 1, p), good),
        (2, rows, nnz, good, good, good, 4, p, big, capacity, good, good, good, good, ptrs(p + 4, p)),
        (2, rows, nnz, good, good, good, 4, p, big, capacity, good, good, good, good, None),
    )
    for call in fill:
        assert lib.sputnik_hip_csr_topk_global_fill(*call, None) == invalid, call
    assert lib.sputnik_hip_csr_topk_global_workspace_bytes(2, rows) == 4 * (4 * 256 + 2 + 12)
    assert lib.sputnik_hip_csr_topk_global_workspace_bytes(0, None) == 4 * (4 * 256 + 2)
    assert lib.sputnik_hip_csr_topk_global_workspace_bytes(2, ints(4, -1)) == 0
    assert lib.sputnik_hip_csr_topk_global_select(0, None, None, None, None, 4, 0, None, 0, None, None, None) == 0


# ---- the modules ----

SHAPES = ((12, 20), (8, 6), (5, 30))          # (out, in) of the three layers
BATCH, SEQ = 2, 3


def cpu_layers(seed, dtype=torch.float32, density=0.5):
    generator = torch.Generator().manual_seed(seed)
    layers = []
    for i, (out_f, in_f) in enumerate(SHAPES):
        w = ((torch.randn(out_f, in_f, generator=generator) * (i + 1) / 0.5).round() * 0.5).to(dtype)    # many ties
        layers.append(SparseLinear.from_dense(w, density=density))
    return layers, generator


def as_csr_layers(modules):
    return [(m.values.detach(), m.row_offsets, m.column_indices, m.input_features) for m in modules]


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), **ids)
def test_prune_layers_to_on_cpu(dtype):
    positions = sum(o * i for o, i in SHAPES)
    for kwargs, K in ((dict(density=0.25), round(0.25 * positions)), (dict(nonzeros=40), 40), (dict(nonzeros=0), 0)):
        modules, _ = cpu_layers(61, dtype)
        modules[1].values.requires_grad_(False)
        for module in modules:
            module.values.grad = torch.zeros_like(module.values) if module.values.requires_grad else None
            module.dense_grad = torch.zeros(1)
        markers = [module.dense_grad for module in modules]
        olds = [(m.values, m.row_indices, m.row_offsets, m.column_indices) for m in modules]
        copies = [[t.detach().clone() for t in old] for old in olds]
        wants = topology.prune_csr_global(as_csr_layers(modules), K)
        sources = topology.prune_layers_to(modules, **kwargs)
        assert len(sources) == len(modules) and sum(s.numel() for s in sources) == K
        for module, old, copy, want, source, marker in zip(modules, olds, copies, wants, sources, markers):
            assert torch.equal(source, want[4])
            assert torch.equal(module.row_indices, want[0]) and torch.equal(module.row_offsets, want[1])
            assert torch.equal(module.column_indices, want[2])
            assert torch.equal(bits_of(module.values.detach()), bits_of(want[3]))
            assert isinstance(module.values, torch.nn.Parameter) and module.values is not old[0]
            assert module.values.requires_grad == old[0].requires_grad and module.values.grad is None
            assert module.values.dtype == dtype and module.dense_grad is marker
            assert all(torch.equal(t.detach(), c) for t, c in zip(old, copy))       # the old arrays are not written to
            assert dict(module.named_parameters())["values"] is module.values
            # the registry: the new index tensors are static, the old ones are not any more
            assert functional._is_static(module.row_indices, module.row_offsets, module.column_indices)
            assert not any(functional._is_static(t) for t in old[1:])


def test_prune_layers_to_replaces_a_layer_that_keeps_everything():
    """every listed layer gets new tensors, also one whose entries all stay"""
    modules, _ = cpu_layers(62)
    with torch.no_grad():
        modules[0].values.mul_(1000.0).add_(torch.sign(modules[0].values) * 1000.0)     # far above the others
    old = modules[0].values
    nnz = [m.values.numel() for m in modules]
    sources = topology.prune_layers_to(modules, nonzeros=nnz[0] + 5)
    assert torch.equal(sources[0], torch.arange(nnz[0])) and modules[0].values is not old
    assert torch.equal(modules[0].values.detach(), old.detach())
    assert sources[1].numel() + sources[2].numel() == 5


def test_prune_layers_to_at_or_above_nnz_is_a_no_op():
    modules, _ = cpu_layers(63)
    parameters = [m.values for m in modules]
    indices = [(m.row_indices, m.row_offsets, m.column_indices) for m in modules]
    entries = sum(p.numel() for p in parameters)
    positions = sum(o * i for o, i in SHAPES)
    for kwargs in (dict(nonzeros=entries), dict(nonzeros=entries + 1), dict(density=1.0), dict(nonzeros=positions)):
        sources = topology.prune_layers_to(modules, **kwargs)
        for module, parameter, index, source in zip(modules, parameters, indices, sources):
            assert module.values is parameter and torch.equal(source, torch.arange(parameter.numel()))
            assert all(a is b for a, b in zip(index, (module.row_indices, module.row_offsets, module.column_indices)))
    for bad in (dict(), dict(density=0.5, nonzeros=3), dict(density=1.5), dict(density=-0.1), dict(nonzeros=-1),
                dict(nonzeros=positions + 1)):
        with pytest.raises(ValueError):
            topology.prune_layers_to(modules, **bad)
    assert all(m.values is p for m, p in zip(modules, parameters))


@pytest.mark.parametrize("which", ("sgd", "adam"))
def test_prune_layers_to_carries_the_optimizer_state(which):
    modules, generator = cpu_layers(64)
    parameters = [m.values for m in modules]
    if which == "sgd":
        optimizer = torch.optim.SGD(parameters, lr=0.1, momentum=0.9)
    else:
        optimizer = torch.optim.Adam([{"params": parameters[:1]}, {"params": parameters[1:], "lr": 0.01}])

    def one_step():
        for module in modules:
            module.values.grad = torch.randn(module.values.numel(), generator=generator)
        optimizer.step()
        for module in modules:
            module.values.grad = None

    one_step()
    before = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizer.state[p].items()} for p in parameters]
    assert all(any(torch.is_tensor(v) and v.shape == p.shape for v in b.values()) for b, p in zip(before, parameters))
    sources = topology.prune_layers_to(modules, density=0.2, optimizer=optimizer)
    held = [p for group in optimizer.param_groups for p in group["params"]]
    assert len(held) == len(modules) and all(h is m.values for h, m in zip(held, modules))
    if which == "adam":
        assert optimizer.param_groups[1]["lr"] == 0.01 and len(optimizer.param_groups[1]["params"]) == 2
    for module, old, was, source in zip(modules, parameters, before, sources):
        new = module.values
        assert new is not old and old not in optimizer.state and source.numel() == new.numel() < old.numel()
        state = optimizer.state[new]
        assert set(state) == set(was)
        for name, t in was.items():
            if torch.is_tensor(t) and t.shape == old.shape:
                assert torch.equal(state[name].view(torch.int32), t.view(torch.int32)[source]), name    # bit for bit
            elif torch.is_tensor(t):
                assert torch.equal(state[name], t), name        # step
            else:
                assert state[name] == t, name
    kept = [m.values.detach().clone() for m in modules]
    one_step()                                                  # the carried optimizer trains the new Parameters
    assert all(not torch.equal(m.values.detach(), k) for m, k in zip(modules, kept))


def test_forward_after_the_step(cpu_ops):
    """The pruned CPU layer's forward (the oracle answers the ops) against the dense float64
    product of the kept entries.  Both sum the same out * in products exactly representable
    in float64; the layer accumulates in float32, so an output of IN terms is within
    IN * 2**-23 * sum |w x| of it (one rounding of the product and one of the running sum per
    term, 2**-24 each)."""
    modules, generator = cpu_layers(65)
    topology.prune_layers_to(modules, density=0.2)
    for module, (out_f, in_f) in zip(modules, SHAPES):
        x = torch.randn(BATCH, SEQ, in_f, generator=generator)
        with torch.no_grad():
            y = module(x)
        assert tuple(y.shape) == (BATCH, out_f, SEQ)
        lengths = (module.row_offsets[1:] - module.row_offsets[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(out_f), lengths)
        dense = torch.zeros(out_f, in_f, dtype=torch.float64)
        dense[rows, module.column_indices.to(torch.int64)] = module.values.detach().double()
        want = torch.matmul(dense, x.double().transpose(1, 2))
        bound = in_f * 2.0 ** -23 * torch.matmul(dense.abs(), x.double().abs().transpose(1, 2))
        assert bool(((y.double() - want).abs() <= bound).all())
        assert module.values.numel() == 0 or bool((y != 0).any())
