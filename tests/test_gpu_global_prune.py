"""GPU: one top-k across the entries of several CSR patterns (csrc/topology.hip;
ops.csr_topk_global, topology.prune_csr_global, topology.prune_layers_to) against the torch path
on the CPU copies of the same input.  Everything is an integer or a bit copy: every comparison
is exact.

The sizes at which the launches change -- the entries one workgroup of the flat walk covers, the
layers one digit launch takes -- come from the host query the launches themselves decide by."""
import pytest
import torch

from torch_sputnik_amd import SparseLinear, capi, functional, ops, topology

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {2: torch.int16, 4: torch.int32}
NAMES = ("row_indices", "row_offsets", "column_indices", "values", "source")
ids = dict(ids=lambda d: str(d).split(".")[-1])


def width(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def bits_of(t):
    return t.contiguous().view(BITS[t.element_size()]) if t.is_floating_point() else t


def from_bits(patterns, dtype):
    return torch.tensor(patterns, dtype=BITS[width(dtype)]).view(dtype)


def query(dtype, rows=(1,), nonzeros=(1,)):
    return capi.csr_topk_global_launch_shape(list(rows), list(nonzeros), width(dtype))


def csr(lengths, n, generator):
    """row_offsets and ascending random columns for rows of these lengths"""
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    row_offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int32)
    row_offsets[1:] = torch.cumsum(lengths, 0)
    columns = [torch.sort(torch.randperm(n, generator=generator)[:int(length)]).values for length in lengths]
    return row_offsets, torch.cat(columns + [torch.zeros(0, dtype=torch.int64)]).to(torch.int32)


def split(nnz, m):
    """m row lengths of sum nnz: an empty row among them (m >= 2), the last one the longest"""
    if m == 1:
        return [nnz]
    share = nnz // (2 * (m - 1))
    lengths = [share] * (m - 1)
    lengths[0] = 0
    return lengths + [nnz - sum(lengths)]


def specials(dtype):
    """NaN, +-inf, +-0, the smallest denormal and an x / -x pair"""
    return torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 0.375, -0.375],
                                   dtype=dtype), from_bits([1], dtype)])


def quantised(count, dtype, generator, quantum=0.125, special=True):
    """few distinct magnitudes (many ties, signs mixed), the special values among them"""
    x = ((torch.randn(count, generator=generator) / quantum).round() * quantum).to(dtype)
    if special:
        s = specials(dtype)
        x[1::5][: s.numel()] = s[: x[1::5].numel()]
    return x


def random_layer(lengths, n, dtype, generator, special=True):
    row_offsets, column_indices = csr(lengths, n, generator)
    return quantised(column_indices.numel(), dtype, generator, special=special), row_offsets, column_indices, n


def same(got, want, where=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, where, g.shape, w.shape)
        assert torch.equal(bits_of(g).cpu(), bits_of(w).cpu()), (name, where)


def on_device(layers, lead=0):
    """the three lists of ops.csr_topk_global on the GPU; ``lead``: every values tensor is a view
    that starts so many elements into its buffer"""
    values = []
    for layer in layers:
        buffer = torch.zeros(layer[0].numel() + lead, dtype=layer[0].dtype, device="cuda")
        buffer[lead:] = layer[0].cuda()
        values.append(buffer[lead:])
    return values, [layer[1].cuda() for layer in layers], [layer[2].cuda() for layer in layers]


def check(layers, total, device=None, want=None, note=""):
    """ops.csr_topk_global on the device copies against the torch path on the CPU tensors.
    Returns the device result."""
    want = topology.prune_csr_global(layers, total) if want is None else want
    got = ops.csr_topk_global(*(on_device(layers) if device is None else device), total)
    assert len(got) == len(want) == len(layers)
    for l, (g, w) in enumerate(zip(got, want)):
        assert all(t.is_cuda for t in g)
        assert g[4].dtype == torch.int64 and all(g[i].dtype == torch.int32 for i in (0, 1, 2))
        same(g, w, f"layer {l} of {len(layers)} total={total} {layers[l][0].dtype} {note}")
    assert sum(g[4].numel() for g in got) == total
    return got


def counts_for(entries):
    return sorted({1, entries // 3, entries // 2 + 1, entries - 1} & set(range(entries + 1)))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_layer_sizes_around_the_workgroup_boundary(dtype):
    """nnz in {0, 1, E - 1, E, E + 1, 2E + 3} mixed in one call: a layer takes no workgroup, one
    whose last pieces stick out, exactly full ones, and one more for a few entries."""
    generator = torch.Generator().manual_seed(3001)
    shape = query(dtype)
    e = shape["elements_per_workgroup"]
    assert shape["served"] and shape["digit_passes"] == width(dtype) and e >= 2
    sizes = (e + 1, 0, 1, 2 * e + 3, e - 1, e)
    layers = [random_layer(split(nnz, m), max(nnz, 1), dtype, generator) for nnz, m in zip(sizes, (3, 2, 1, 4, 2, 3))]
    assert [layer[0].numel() for layer in layers] == list(sizes)
    entries = sum(sizes)
    device = on_device(layers)
    for K in counts_for(entries):
        check(layers, K, device)
    order = [3, 1, 5, 0, 2, 4]                                  # the long layer first, another neighbourhood
    check([layers[i] for i in order], entries // 4)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), **ids)
def test_layer_counts_around_the_argument_table(dtype):
    """L in {1, 2, C - 1, C, C + 1, 2C + 1} layers of 1 to 8 entries.  With all magnitudes equal
    the kept entries are the first K in layer order: K ends inside the first chunk of layers and
    inside the last, so the quota crosses every launch of a digit pass.  Then random values."""
    generator = torch.Generator().manual_seed(3002)
    c = query(dtype)["layers_per_launch"]
    assert c >= 3
    for count in sorted({1, 2, c - 1, c, c + 1, 2 * c + 1}):
        assert query(dtype, [2] * count, [3] * count)["digit_launches"] == -(-count // c)
        equal, random = [], []
        for l in range(count):
            lengths = split(1 + (5 * l + 3) % 8, 1 + l % 3)
            n = max(lengths)
            row_offsets, column_indices = csr(lengths, n, generator)
            nnz = column_indices.numel()
            equal.append((torch.where(torch.arange(nnz) % 2 == 0, 0.75, -0.75).to(dtype), row_offsets, column_indices, n))
            random.append((quantised(nnz, dtype, generator, special=l % 7 == 0), row_offsets, column_indices, n))
        sizes = [layer[0].numel() for layer in equal]
        entries = sum(sizes)
        assert all(1 <= s <= 8 for s in sizes)
        last_chunk = sum(sizes[:(count - 1) // c * c])          # the entries in front of the last launch's layers
        for K in sorted({min(2, entries), last_chunk + 1, entries - 1}):
            got = check(equal, K, note="all equal")
            left = K
            for size, g in zip(sizes, got):
                assert g[4].tolist() == list(range(min(size, left)))
                left -= min(size, left)
        device = on_device(random)
        for K in sorted({1, entries // 2, entries - 1} & set(range(entries + 1))):
            check(random, K, device)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_value_views_with_a_lead(dtype):
    """values that start 1 and 3 elements into their buffer: no layer starts on a 16-byte
    boundary, the pieces of the flat walk are laid out from the address rounded down"""
    generator = torch.Generator().manual_seed(3003)
    e = query(dtype)["elements_per_workgroup"]
    layers = [random_layer(split(nnz, m), nnz, dtype, generator) for nnz, m in ((e + 1, 3), (e - 2, 2), (e, 1), (37, 4))]
    entries = sum(layer[0].numel() for layer in layers)
    wants = {K: topology.prune_csr_global(layers, K) for K in (entries // 3, entries - 5)}
    for lead in (1, 3):
        device = on_device(layers, lead)
        assert all(v.data_ptr() % 16 == lead * width(dtype) for v in device[0])
        for K, want in wants.items():
            check(layers, K, device, want, note=f"lead {lead}")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_layers_of_very_different_row_lengths(dtype):
    """3 x 4 at mean 1 next to 2 x 600 at mean 300: the rows launches differ in their group
    width; each layer has an empty row and a full row"""
    generator = torch.Generator().manual_seed(3004)
    layers = [random_layer((4, 0, 0), 4, dtype, generator, special=False), random_layer((0, 600), 600, dtype, generator)]
    lanes = [capi.csr_topk_launch_shape(layer[1].numel() - 1, layer[3], layer[0].numel(), width(dtype), True)
             ["group_lanes"] for layer in layers]
    assert lanes[0] < lanes[1]
    device = on_device(layers)
    for K in (1, 4, 5, 200, 603):
        check(layers, K, device)
    check(layers[::-1], 300)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_all_values_equal(dtype):
    """three layers of one magnitude, K inside the second: the tie quota crosses a layer boundary
    and ends in the middle of a row"""
    generator = torch.Generator().manual_seed(3005)
    layers = []
    for lengths, n in (((30, 0, 41), 50), ((20, 65, 1, 90), 90), ((50, 50), 50)):
        row_offsets, column_indices = csr(lengths, n, generator)
        values = torch.where(torch.arange(column_indices.numel()) % 3 == 0, -2.5, 2.5).to(dtype)
        layers.append((values, row_offsets, column_indices, n))
    sizes = [layer[0].numel() for layer in layers]
    device = on_device(layers)
    for K in (sizes[0] + 47, sizes[0], sizes[0] + 1, sizes[0] + sizes[1], sizes[0] + sizes[1] + 1, 7):
        got = check(layers, K, device)
        left = K
        for size, g in zip(sizes, got):
            assert torch.equal(g[4].cpu(), torch.arange(min(size, left)))
            left -= min(size, left)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_special_values(dtype):
    """NaN, +-inf, +-0, the smallest denormal and x / -x, each in another layer than its partner"""
    generator = torch.Generator().manual_seed(3006)
    s = specials(dtype)      # nan inf -inf 0 -0 x -x denormal
    layers = []
    for lengths, n, chosen in (((2, 3, 0, 2), 4, (s[0], s[2], s[3], s[5])), ((4, 1), 4, (s[1], s[4], s[7])),
                               ((0, 3, 3), 3, (s[6], s[1], s[0], s[3]))):
        values, row_offsets, column_indices, _ = random_layer(lengths, n, dtype, generator, special=False)
        values[torch.randperm(values.numel(), generator=generator)[: len(chosen)]] = torch.stack(chosen)
        layers.append((values, row_offsets, column_indices, n))
    entries = sum(layer[0].numel() for layer in layers)
    device = on_device(layers)
    for K in range(entries + 1):
        check(layers, K, device)
    got = check(layers, 2, device)
    assert [g[4].numel() for g in got] == [1, 0, 1] and all(bool(torch.isnan(g[3]).all()) for g in got)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_count_edges_and_empty_layers(dtype):
    generator = torch.Generator().manual_seed(3007)
    layers = [random_layer((0, 0, 0), 4, dtype, generator), random_layer((0, 5, 0, 0, 2), 5, dtype, generator),
              random_layer((), 3, dtype, generator), random_layer((300, 7, 0, 120), 300, dtype, generator)]
    entries = sum(layer[0].numel() for layer in layers)
    device = on_device(layers)
    for K in (0, 1, entries - 1, entries):
        got = check(layers, K, device)
        assert got[0][4].numel() == got[2][4].numel() == 0 and got[2][1].tolist() == [0]
    for layer in (layers[3], layers[0], layers[2]):             # one layer: ops.csr_topk in total mode
        nnz = layer[0].numel()
        for K in sorted({0, nnz // 2, nnz}):
            (got,) = check([layer], K)
            same(got, ops.csr_topk(*(t.cuda() for t in layer[:3]), total=K))
    assert ops.csr_topk_global([], [], [], 0) == []


def test_two_calls_back_to_back():
    """the same inputs with another K, no synchronisation in between: the bins and the running
    tie count of a call start clean"""
    generator = torch.Generator().manual_seed(3008)
    layers = [random_layer([110] * 60, 1100, torch.float32, generator), random_layer([3, 0, 700], 700, torch.float32, generator),
              random_layer([40] * 9, 64, torch.float32, generator)]
    entries = sum(layer[0].numel() for layer in layers)
    device = on_device(layers)
    first = ops.csr_topk_global(*device, entries // 2)
    second = ops.csr_topk_global(*device, entries // 7)
    third = ops.csr_topk_global(*device, entries // 2)
    for got, K in ((first, entries // 2), (second, entries // 7), (third, entries // 2)):
        for g, w in zip(got, topology.prune_csr_global(layers, K)):
            same(g, w, f"total={K}")


def test_beyond_the_row_limit_falls_back():
    """a layer of 16385 rows of one entry each next to a normal layer: the op refuses, and
    topology.prune_csr_global answers by the torch path on the device tensors"""
    generator = torch.Generator().manual_seed(3009)
    limit = 16384
    m = limit + 1
    tall = (quantised(m, torch.float32, generator), torch.arange(m + 1, dtype=torch.int32),
            torch.zeros(m, dtype=torch.int32), 1)
    layers = [tall, random_layer((9, 0, 30, 12), 30, torch.float32, generator)]
    sizes = [layer[0].numel() for layer in layers]
    assert not query(torch.float32, [m, 4], sizes)["served"] and query(torch.float32, [limit, 4], sizes)["served"]
    device = on_device(layers)
    with pytest.raises(RuntimeError):
        ops.csr_topk_global(*device, limit // 2)
    on_gpu = [(v, ro, ci, layer[3]) for v, ro, ci, layer in zip(*device, layers)]
    for K in (limit // 2, sum(sizes) - 3):
        got = topology.prune_csr_global(on_gpu, K)
        for g, w in zip(got, topology.prune_csr_global(layers, K)):
            assert all(t.is_cuda for t in g)
            same(g, w)


def test_prune_csr_global_routes():
    generator = torch.Generator().manual_seed(3010)
    layers = [random_layer(torch.randint(0, 91, (70,), generator=generator), 90, torch.float32, generator, special=False),
              random_layer(torch.randint(0, 40, (33,), generator=generator), 64, torch.float32, generator, special=False)]
    K = sum(layer[0].numel() for layer in layers) // 3
    want = topology.prune_csr_global(layers, K)
    device = on_device(layers)
    on_gpu = [(v.requires_grad_(), ro, ci, layer[3]) for v, ro, ci, layer in zip(*device, layers)]
    results = [topology.prune_csr_global(on_gpu, K)]
    topology.enable_device_build(False)
    try:
        results.append(topology.prune_csr_global(on_gpu, K))
    finally:
        topology.enable_device_build(True)
    halves = [(on_gpu[0][0].detach().half(),) + on_gpu[0][1:], on_gpu[1]]         # mixed dtypes: the torch path
    mixed = topology.prune_csr_global(halves, K)
    mixed_want = topology.prune_csr_global([(layers[0][0].half(),) + layers[0][1:], layers[1]], K)
    for got, wanted in ((results[0], want), (results[1], want), (mixed, mixed_want)):
        for g, w in zip(got, wanted):
            assert all(t.is_cuda for t in g) and not g[3].requires_grad
            same(g, w)


# ---- the modules ----

SHAPES = ((64, 96), (32, 64), (96, 32))       # (out, in)
BATCH, SEQ = 2, 8


def explicit_module(out_f, in_f, values, row_indices, row_offsets, column_indices):
    """A GPU SparseLinear on a given pattern"""
    module = SparseLinear(in_f, out_f).cuda()
    module.values = torch.nn.Parameter(values.detach().clone().cuda())
    module.row_indices, module.row_offsets, module.column_indices = (
        row_indices.clone().cuda(), row_offsets.clone().cuda(), column_indices.clone().cuda())
    functional.register_static_topology(module.row_indices, module.row_offsets, module.column_indices)
    return module


def forward_backward(module, x_host):
    x = x_host.cuda().requires_grad_()
    module.values.grad = None
    y = module(x)
    y.backward(torch.ones_like(y) * 0.5)
    return y.detach(), module.values.grad.clone(), x.grad.clone()


def test_prune_layers_to_on_gpu_modules():
    """The same integers and value bits as the same call on CPU copies; the Adam state carried;
    a forward and backward of a pruned layer.  tests/test_gpu_csr_prune.py has no comparison
    with a dense float64 product after prune_to, so the forward (and the backward) on the float32
    vector route is compared bit for bit with a module built from the CPU modules' result."""
    generator = torch.Generator().manual_seed(3011)
    weights = [torch.randn(o, i, generator=generator) * (l + 1) for l, (o, i) in enumerate(SHAPES)]
    modules = [SparseLinear.from_dense(w.cuda(), density=0.5) for w in weights]
    inputs = [torch.randn(BATCH, SEQ, i, generator=generator) for _, i in SHAPES]
    for module, x_host in zip(modules, inputs):
        forward_backward(module, x_host)          # plans, transposed topology and images of the OLD patterns exist
    optimizer = torch.optim.Adam([m.values for m in modules], lr=0.1)
    optimizer.step()
    olds = [m.values for m in modules]
    old_states = [{name: t.clone() for name, t in optimizer.state[old].items()} for old in olds]
    twins = []
    for module, (o, i) in zip(modules, SHAPES):
        twin = SparseLinear(i, o)
        twin.values = torch.nn.Parameter(module.values.detach().cpu())
        twin.row_offsets, twin.column_indices = module.row_offsets.cpu(), module.column_indices.cpu()
        twin.row_indices = topology.diffsort(twin.row_offsets)
        twins.append(twin)

    sources = topology.prune_layers_to(modules, density=0.2, optimizer=optimizer)
    twin_sources = topology.prune_layers_to(twins, density=0.2)

    assert sum(m.values.numel() for m in modules) == round(0.2 * sum(o * i for o, i in SHAPES))
    for module, twin, old, source, twin_source in zip(modules, twins, olds, sources, twin_sources):
        assert source.is_cuda and torch.equal(source.cpu(), twin_source)
        for name in ("row_indices", "row_offsets", "column_indices"):
            assert torch.equal(getattr(module, name).cpu(), getattr(twin, name)), name
        assert torch.equal(module.values.detach().view(torch.int32).cpu(), twin.values.detach().view(torch.int32))
        assert module.values is not old and isinstance(module.values, torch.nn.Parameter)
        assert module.values.requires_grad and module.values.grad is None
    for module, old, was, source in zip(modules, olds, old_states, sources):
        state = optimizer.state[module.values]
        assert old not in optimizer.state and torch.equal(state["step"], was["step"])
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(state[name].view(torch.int32), was[name].view(torch.int32)[source]), name
    held = [p for group in optimizer.param_groups for p in group["params"]]
    assert all(h is m.values for h, m in zip(held, modules))
    for module, twin, x_host, (o, i) in zip(modules, twins, inputs, SHAPES):
        fresh = explicit_module(o, i, twin.values, twin.row_indices, twin.row_offsets, twin.column_indices)
        got, want = forward_backward(module, x_host), forward_backward(fresh, x_host)
        for g, w_, name in zip(got, want, ("forward", "values.grad", "input.grad")):
            assert torch.equal(g, w_), name
    before = [m.values.detach().clone() for m in modules]
    optimizer.step()                              # the carried Adam trains the new Parameters
    assert all(not torch.equal(m.values.detach(), b) for m, b in zip(modules, before))
