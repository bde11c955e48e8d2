"""CPU: the host side above the C ABI -- autograd.Functions, nn.Modules and
topology helpers -- with torch.ops.torch_sputnik.* answered by the oracle
(tests-only CPU backend).  Gradients are compared with dense autograd in
float64 and with the fixtures produced by the reference's own modules."""
import numpy as np
import pytest
import torch

from oracle import sputnik_oracle as O
from helpers import make_csr, rel_err

TOL = 2e-5  # float32 tensors between the ops


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def test_diffsort_and_dense_to_sparse(cpu_ops):
    tsa = cpu_ops
    ro = torch.tensor([0, 1, 4, 4, 6, 11, 12], dtype=torch.int32)
    assert tsa.diffsort(ro).tolist() == [2, 0, 5, 3, 1, 4]      # SURVEY.md quirk Q1 probe
    assert tsa.diffsort(ro).dtype == torch.int32
    dense, vals, _, ro_np, ci_np = make_csr(9, 7, 0.6, seed=1)
    v, ri, ro_t, ci_t = tsa.dense_to_sparse(T(dense))
    assert np.array_equal(v.numpy(), vals) and np.array_equal(ro_t.numpy(), ro_np)
    assert np.array_equal(ci_t.numpy(), ci_np)
    assert ro_t.dtype == ci_t.dtype == ri.dtype == torch.int32
    assert sorted(ri.tolist()) == list(range(9))


def test_generate_mask_counts(cpu_ops):
    mask = cpu_ops.generate_mask(1024, 1024, sparsity=0.9, generator=np.random.default_rng(0))
    assert int(mask.sum()) == 104860          # config 3's nnz
    assert mask.shape == (1024, 1024)


def test_spmm_function_matches_golden(cpu_ops, golden):
    g = golden("autograd_spmm")
    v = T(g["values"]).requires_grad_(True)
    d = T(g["dense"]).requires_grad_(True)
    out = cpu_ops.Spmm.apply(int(g["m"]), int(g["k"]), v, T(g["row_indices"]), T(g["row_offsets"]),
                             T(g["column_indices"]), d)
    out.backward(T(g["grad_out"]))
    assert rel_err(out.detach().numpy(), g["out"]) < TOL
    assert rel_err(v.grad.numpy(), g["grad_values"]) < TOL
    assert rel_err(d.grad.numpy(), g["grad_dense"]) < TOL


def test_sddmm_function_matches_golden(cpu_ops, golden):
    g = golden("autograd_sddmm")
    l = T(g["lhs"]).requires_grad_(True)
    r = T(g["rhs"]).requires_grad_(True)
    out = cpu_ops.Sddmm.apply(int(g["m"]), int(g["n"]), T(g["row_indices"]), T(g["row_offsets"]),
                              T(g["column_indices"]), l, r)
    out.backward(T(g["grad_out"]))
    assert rel_err(out.detach().numpy(), g["out"]) < TOL
    assert rel_err(l.grad.numpy(), g["grad_lhs"]) < TOL
    assert rel_err(r.grad.numpy(), g["grad_rhs"]) < TOL


def test_sparse_linear_matches_golden(cpu_ops, golden):
    g = golden("autograd_sparse_linear")
    layer = cpu_ops.SparseLinear(int(g["in_features"]), int(g["out_features"]))
    with torch.no_grad():
        layer.weight.copy_(T(g["weight"]))
    layer.setup_sparse_tensors()
    x = T(g["x"]).requires_grad_(True)
    y = layer(x)
    assert tuple(y.shape) == (int(g["batch"]), int(g["out_features"]), int(g["seq"]))
    y.backward(T(g["grad_out"]))
    assert rel_err(y.detach().numpy(), g["y"]) < TOL
    assert rel_err(x.grad.numpy(), g["grad_x"]) < TOL
    assert rel_err(layer.values.grad.numpy(), g["grad_values"]) < TOL
    assert "values" in layer.state_dict()       # nn.Parameter, as in the reference
    assert "row_offsets" not in layer.state_dict()


def test_batched_backward_extension(cpu_ops):
    """3-D Spmm backward (impossible in the reference: its csr_transpose is 1-D only)."""
    dense_a, vals, ri, ro, ci = make_csr(12, 10, 0.6, seed=2)
    rng = np.random.default_rng(3)
    r = 3
    v3 = rng.uniform(-1, 1, (r, len(vals))).astype(np.float32)
    b = rng.uniform(-1, 1, (r, 10, 6)).astype(np.float32)
    v = T(v3).requires_grad_(True)
    d = T(b).requires_grad_(True)
    out = cpu_ops.Spmm.apply(12, 10, v, T(ri), T(ro), T(ci), d)
    out.sum().backward()
    a = torch.zeros(r, 12, 10, dtype=torch.float64)
    rows = np.repeat(np.arange(12), np.diff(ro))
    a[:, rows, ci.astype(np.int64)] = T(v3).double()
    a.requires_grad_(True)
    dd = T(b).double().requires_grad_(True)
    torch.matmul(a, dd).sum().backward()
    assert rel_err(d.grad.numpy(), dd.grad.numpy()) < TOL
    assert rel_err(v.grad.numpy(), a.grad.numpy()[:, rows, ci.astype(np.int64)]) < TOL


def test_transpose_cache_gives_same_gradients(cpu_ops):
    from torch_sputnik_amd import functional
    dense_a, vals, ri, ro, ci = make_csr(15, 11, 0.7, seed=4)
    b = np.random.default_rng(5).uniform(-1, 1, (11, 8)).astype(np.float32)
    topo = (T(ri), T(ro), T(ci))

    def grads():
        v = T(vals).requires_grad_(True)
        d = T(b).requires_grad_(True)
        cpu_ops.Spmm.apply(15, 11, v, *topo, d).square().sum().backward()
        return v.grad.clone(), d.grad.clone()

    functional.enable_transpose_cache(False)     # the reference's per-call transpose
    try:
        base = grads()
        cache = functional.enable_transpose_cache(True)
        first, second = grads(), grads()
        assert len(cache._entries) == 1
    finally:
        functional.enable_transpose_cache(functional.TRANSPOSE_CACHE_DEFAULT)
    for got in (first, second):
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


def test_default_caches_serve_registered_topologies_only(cpu_ops):
    """by default nothing is remembered about arbitrary index tensors
    (the reference's per-call behaviour, modules/spmm.py:59-64); a pattern that
    its owner registered as static is cached, and its entries die with it."""
    import gc
    from torch_sputnik_amd import functional
    dense_a, vals, ri, ro, ci = make_csr(15, 11, 0.7, seed=4)
    b = np.random.default_rng(5).uniform(-1, 1, (11, 8)).astype(np.float32)

    def grads(topo):
        v = T(vals).requires_grad_(True)
        d = T(b).requires_grad_(True)
        cpu_ops.Spmm.apply(15, 11, v, *topo, d).square().sum().backward()
        return v.grad.clone(), d.grad.clone()

    functional.enable_transpose_cache(functional.TRANSPOSE_CACHE_DEFAULT)
    functional.enable_plan_cache(functional.PLAN_CACHE_DEFAULT)
    cache = functional._cache
    assert cache.scope == "static"
    topo = (T(ri), T(ro), T(ci))
    base = grads(topo)
    assert len(cache) == 0, "an unregistered pattern was cached"
    functional.register_static_topology(*topo)
    first, second = grads(topo), grads(topo)
    assert len(cache) == 1
    for got in (first, second):
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    # an in-place write changes the key (version counter): a new entry, not a stale hit
    topo[2].add_(0)
    grads(topo)
    assert len(cache) == 2
    # the owner drops the pattern: registration and entries go with it
    del topo
    gc.collect()
    assert len(cache) == 0 and not functional._static


def test_unregistered_pattern_never_takes_the_synchronising_transpose(cpu_ops, monkeypatch):
    """the transpose that also returns the permutation waits for the
    stream when `checked`; that is for results a cache KEEPS.  A pattern no cache serves
    must get the reference's asynchronous per-call transpose (modules/spmm.py:59-62) --
    no host round trip in every backward, legal inside a stream capture."""
    from torch_sputnik_amd import functional, ops
    dense_a, vals, ri, ro, ci = make_csr(15, 11, 0.7, seed=4)
    b = np.random.default_rng(5).uniform(-1, 1, (11, 8)).astype(np.float32)
    calls = []
    real = ops.csr_transpose_with_permutation

    def spy(m, n, values, row_offsets, column_indices, checked=True):
        calls.append(bool(checked))
        return real(m, n, values, row_offsets, column_indices, checked)

    monkeypatch.setattr(ops, "csr_transpose_with_permutation", spy)
    functional.enable_transpose_cache(functional.TRANSPOSE_CACHE_DEFAULT)

    def backward(topo):
        v = T(vals).requires_grad_(True)
        d = T(b).requires_grad_(True)
        cpu_ops.Spmm.apply(15, 11, v, *topo, d).square().sum().backward()
        lhs = T(np.ones((15, 4), np.float32)).requires_grad_(True)
        rhs = T(np.ones((11, 4), np.float32)).requires_grad_(True)
        cpu_ops.Sddmm.apply(15, 11, *topo, lhs, rhs).sum().backward()

    topo = (T(ri), T(ro), T(ci))
    backward(topo)
    assert True not in calls, "an unregistered pattern took the checked (synchronising) transpose"
    functional.register_static_topology(*topo)
    backward(topo)
    backward(topo)
    assert calls.count(True) == 1, "a registered pattern is checked once, when it is cached"
    functional.unregister_static_topology(*topo)


def test_cache_is_bounded_by_bytes():
    from torch_sputnik_amd import functional
    lru = functional._Lru(capacity=100, max_bytes=4096)
    for i in range(10):
        lru.put(i, (torch.zeros(256, dtype=torch.float32),))   # 1 KiB each
    assert len(lru) == 4 and lru.bytes == 4096
    assert lru.get(0) is None and lru.get(9) is not None
    lru.forget("nothing")
    lru.clear()
    assert lru.bytes == 0


def test_sparse_softmax_backward(cpu_ops):
    mask, vals, ri, ro, ci = make_csr(10, 14, 0.6, seed=6, round_to=1, empty_rows=(3,))
    x = T((vals * 4 - 2).astype(np.float32)).requires_grad_(True)
    w = T(np.random.default_rng(7).uniform(-1, 1, len(vals)).astype(np.float32))
    y = cpu_ops.SparseSoftmax.apply(x, T(ri), T(ro), T(ci))
    (y * w).sum().backward()
    # dense reference: masked softmax in float64
    xd = torch.full((10, 14), float("-inf"), dtype=torch.float64)
    rows = np.repeat(np.arange(10), np.diff(ro))
    xs = T((vals * 4 - 2).astype(np.float32)).double().requires_grad_(True)
    xd = xd.index_put((T(rows), T(ci.astype(np.int64))), xs)
    keep = torch.tensor([r != 3 for r in range(10)])
    yd = torch.softmax(xd[keep], dim=-1)
    wd = torch.zeros(10, 14, dtype=torch.float64).index_put((T(rows), T(ci.astype(np.int64))), w.double())
    (yd * wd[keep]).sum().backward()
    assert rel_err(x.grad.numpy(), xs.grad.numpy()) < 1e-4


def test_sparse_attention_matches_dense(cpu_ops):
    torch.manual_seed(0)
    heads, emb, seq, batch = 2, 8, 12, 2
    attn = cpu_ops.SparseAttention(heads, emb, max_sequence_length=seq, device="cpu",
                                   sparsity=0.5, mask_generator=np.random.default_rng(1))
    ws = []
    for lin in attn.linears:
        w = torch.randn(emb, emb) * (torch.rand(emb, emb) > 0.4)
        with torch.no_grad():
            lin.weight.copy_(w)
        lin.setup_sparse_tensors()
        ws.append(w.double())
    q, k, v = (torch.randn(batch, seq, emb) for _ in range(3))
    out = attn(q, k, v, None)                       # [batch, seq, emb]
    assert tuple(out.shape) == (batch, seq, emb)
    # `fused_training` (rounds 1-3) is an alias of `low_memory_training`
    assert attn.low_memory_training is False and attn.fused_training is False
    attn.fused_training = True
    assert attn.low_memory_training is True
    attn.low_memory_training = False
    assert cpu_ops.SparseAttention(heads, emb, max_sequence_length=seq, device="cpu", sparsity=0.5,
                                   mask_generator=np.random.default_rng(1),
                                   fused_training=True).low_memory_training is True

    def proj(x, w):                                 # SparseLinear then the module's reshapes
        y = torch.matmul(x.double(), w.t())         # [b, s, e]
        return y.view(batch, seq, heads, emb // heads).transpose(1, 2)
    qd, kd, vd = proj(q, ws[0]), proj(k, ws[1]), proj(v, ws[2])
    scores = torch.matmul(qd, kd.transpose(-2, -1)) / (emb // heads) ** 0.5
    scores = scores.masked_fill(attn.mask2d == 0, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    probs = torch.nan_to_num(probs)                 # rows without any mask entry
    ctx = torch.matmul(probs, vd).transpose(1, 2).reshape(batch, seq, emb)
    want = torch.matmul(ctx, ws[3].t())
    assert rel_err(out.detach().numpy(), want.numpy()) < 1e-4


def test_sparse_softmax_route_reports_the_launch_decisions(monkeypatch):
    """sputnik_hip_sparse_softmax_route is host only: the class by mean row length and storage
    type, two rows per group once m * replicas fills the chip, nontemporal stores for a forward
    output of 128 MiB per grid slice, and the developer knobs."""
    from torch_sputnik_amd import capi
    for name in ("SPUTNIK_HIP_SOFTMAX_RPG", "SPUTNIK_HIP_SOFTMAX_DEPTH", "SPUTNIK_HIP_SOFTMAX_NT"):
        monkeypatch.delenv(name, raising=False)
    capi.reload_options()
    try:
        def route(*args, **kw):
            r = capi.sparse_softmax_route(*args, **kw)
            return ((r["lanes_per_row"], r["base_pieces"], r["pieces"]), r["rows_per_group"], r["depth"],
                    r["nontemporal"])
        # config 3's mask (1024 x 1024 at density 0.1): mean 102, need 102 + 23 + 3
        assert route(1024, 104858, 64) == ((16, 2, 3), 2, 1, 0)
        assert route(1024, 104858, 512) == ((16, 2, 3), 2, 1, 2)         # 215 MB out
        assert route(1024, 104858, 512, backward=True) == ((16, 2, 3), 2, 1, 0)
        assert route(1024, 104858, 64, torch.float16) == ((16, 1, 2), 2, 1, 0)
        assert route(1024, 104858, 3) == ((16, 2, 3), 1, 1, 0)
        # class boundaries (need = mean + ceil(sqrt(5 mean)) + 3 against 64 / 128 / 192 / 256 / 512)
        wants = [(40, (16, 1, 2)), (100, (16, 2, 3)), (150, (16, 3, 4)), (200, (32, 2, 4)),
                 (400, (32, 4, 4)), (600, (64, 4, 4))]
        for mean, cls in wants:
            assert route(10, 10 * mean, 1)[0] == cls, mean
        for mean, cls in [(100, (16, 1, 2)), (200, (16, 2, 3)), (400, (32, 2, 3)), (600, (64, 2, 2))]:
            assert route(10, 10 * mean, 1, torch.bfloat16)[0] == cls, mean
        # the 128 MiB threshold is per grid slice of at most 65535 replicas
        assert route(1, 512, 65536)[3] == 0 and route(1, 513, 65536)[3] == 2
        monkeypatch.setenv("SPUTNIK_HIP_SOFTMAX_RPG", "40")
        monkeypatch.setenv("SPUTNIK_HIP_SOFTMAX_NT", "3")
        capi.reload_options()
        assert route(1024, 104858, 3) == ((16, 2, 3), 16, 1, 3)
        monkeypatch.setenv("SPUTNIK_HIP_SOFTMAX_DEPTH", "3")
        capi.reload_options()
        assert route(1024, 104858, 3) == ((16, 2, 3), 16, 3, 0)
        with pytest.raises(RuntimeError):
            capi.sparse_softmax_route(0, 10, 1)
    finally:
        for name in ("SPUTNIK_HIP_SOFTMAX_RPG", "SPUTNIK_HIP_SOFTMAX_DEPTH", "SPUTNIK_HIP_SOFTMAX_NT"):
            monkeypatch.delenv(name, raising=False)
        capi.reload_options()


def test_sddmm_sum_route_reports_the_summed_decision(monkeypatch):
    """sputnik_hip_sddmm_sum_route is host only and says what sddmm_sum_exec / _half decide:
    matrix cores, tiled partial vectors of some panel width and slab rows, the row-wave
    kernel, or -- one replica of one panel -- the plain product."""
    from torch_sputnik_amd import capi
    knobs = ("SPUTNIK_HIP_SDDMM_KERNEL", "SPUTNIK_HIP_SDDMM_PANEL", "SPUTNIK_HIP_SDDMM_SLAB",
             "SPUTNIK_HIP_MFMA_TILE")
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    capi.reload_options()
    try:
        def route(*args, **kw):
            r = capi.sddmm_sum_route(*args, **kw)
            return r["kernel"], r["panel_width"], r["panels"], r["slab_rows"], r["splits"]
        # config 5's weight gradient (2048^2 at density 0.2, batch 8, seq 512): float32 on
        # 256-wide panels of 80-row slabs, half operands on the matrix cores
        nnz = 838864
        assert route(2048, 512, 2048, nnz, 8) == ("tiled", 256, 2, 80, 1)
        assert route(2048, 512, 2048, nnz, 8, torch.float16)[0] == "mfma"
        assert route(2048, 512, 2048, nnz, 8, torch.bfloat16, mixed=True)[0] == "mfma"
        # the attention projections (512^2 x 1024 at 0.1): few workgroups keep 128-row slabs
        assert route(512, 1024, 512, 26216, 8) == ("tiled", 256, 4, 128, 1)
        # small, or k no multiple of 64: per-replica products of the row-wave kernel
        assert route(100, 40, 60, 3000, 5) == ("rowwave", 0, 1, 0, 1)
        assert route(33, 100, 47, 600, 4, torch.float16) == ("rowwave", 0, 1, 0, 1)
        # one replica of one panel is the plain product
        assert route(64, 64, 64, 4096, 1)[0] == "plain"
        # more (replica, panel) pairs than a grid dimension holds: the row-wave kernel
        assert route(2048, 512, 2048, nnz, 40000)[0] == "rowwave"
        # the knobs of the tests
        monkeypatch.setenv("SPUTNIK_HIP_SDDMM_KERNEL", "tiled")
        monkeypatch.setenv("SPUTNIK_HIP_SDDMM_SLAB", "80")
        capi.reload_options()
        assert route(203, 512, 300, 812, 3) == ("tiled", 256, 2, 80, 1)
        assert route(203, 384, 300, 812, 3, torch.bfloat16) == ("tiled", 128, 3, 128, 1)
        assert route(203, 100, 300, 812, 3) == ("rowwave", 0, 1, 0, 1)
        monkeypatch.setenv("SPUTNIK_HIP_SDDMM_KERNEL", "wave")
        capi.reload_options()
        assert route(2048, 512, 2048, nnz, 8, torch.float16) == ("rowwave", 0, 1, 0, 1)
        monkeypatch.setenv("SPUTNIK_HIP_SDDMM_KERNEL", "mfma")
        monkeypatch.setenv("SPUTNIK_HIP_MFMA_TILE", "256")
        capi.reload_options()
        kernel, _, _, rows, splits = route(267, 192, 300, 1068, 3, torch.float16)
        assert (kernel, rows) == ("mfma", 256) and 1 <= splits <= 8
        assert route(203, 192, 300, 812, 3, torch.float16)[3] == 128      # fewer than 256 rows
        assert route(267, 192, 300, 1068, 3)[0] != "mfma"                   # float32 pairs never
        with pytest.raises(RuntimeError):
            capi.sddmm_sum_route(267, 100, 300, 1068, 3, torch.float16, mixed=True)   # k % 64
        with pytest.raises(RuntimeError):
            capi.sddmm_sum_route(0, 64, 64, 10, 1)
    finally:
        for name in knobs:
            monkeypatch.delenv(name, raising=False)
        capi.reload_options()


def test_structured_masks_keep_their_promises():
    """helpers.structured_csr: every kind reaches the asked mean row, is deterministic, and has
    the shape its kernel edge needs (tests/test_gpu_structured_masks.py)."""
    from helpers import STRUCTURED_KINDS, structured_csr, structured_mask
    for m, n, mean, chunk in ((203, 500, 16, 32), (203, 300, 4, 64), (200, 192, 16, 64), (267, 300, 4, 64)):
        for kind in STRUCTURED_KINDS:
            mask = structured_mask(kind, m, n, mean, np.random.default_rng(1), chunk=chunk)
            assert mask.shape == (m, n) and mask.sum() >= mean * m, (kind, m, n)
            for order in ("descending", "identity"):
                a = structured_csr(kind, m, n, mean, np.random.default_rng(1), order=order, chunk=chunk)
                b = structured_csr(kind, m, n, mean, np.random.default_rng(1), order=order, chunk=chunk)
                assert all(np.array_equal(x, y) and x.dtype == np.int32 for x, y in zip(a, b))
                ri, ro, ci = a
                assert sorted(ri.tolist()) == list(range(m)) and ro[-1] == len(ci) == mask.sum()
                lengths = np.diff(ro)
                if order == "descending":
                    assert np.all(np.diff(lengths[ri]) <= 0)
                else:
                    assert np.array_equal(ri, np.arange(m))
            lengths = mask.sum(axis=1)
            if kind == "causal":
                assert lengths[0] == 1 and lengths[1] <= 3 and lengths[-1] == n and np.all(np.diff(lengths) >= 0)
            if kind.startswith("heavy_rows"):
                full = np.flatnonzero(lengths)
                assert np.all(lengths[full] == n) and np.array_equal(full, np.arange(full[0], full[-1] + 1))
                edge = {"heavy_rows_wave": 8, "heavy_rows_block": 128}.get(kind)
                if edge:   # rows on both sides of a multiple of 8 / of 128
                    assert full[0] // edge != full[-1] // edge
                    assert kind != "heavy_rows_wave" or (full[-1] // 8 * 8) % 128 != 0
            if kind == "last_chunk":
                assert np.all(lengths == lengths[0]) and np.all(mask[:, n - lengths[0]:])
                assert lengths[0] == (n % chunk if n % chunk >= mean else mean)
            if kind == "global_columns_per_chunk":
                held = np.flatnonzero(mask[0])
                assert held[-1] == n - 1 and np.all(mask == mask[0])
                assert len(set(held // chunk)) == min(len(held), -(-n // chunk))
            if kind == "global_columns_one_chunk":
                assert np.array_equal(np.flatnonzero(mask[0]), np.arange(mean)) and mean <= chunk
            if kind == "stride":      # no two rows of a group of 8 share a column
                for r0 in range(0, m - 7, 8):
                    assert mask[r0:r0 + 8].sum(axis=0).max() == 1
            if kind == "alternating":
                assert np.all(lengths[0::2] == n) and np.all(lengths[1::2] == 1)
                assert len(set(np.nonzero(mask[1::2])[1][:8])) == 8
            if kind == "corner":
                rows, cols = np.nonzero(mask)
                assert rows.max() < 128 and cols.max() < 128 and mask[:rows.max() + 1, :cols.max() + 1].all()
            if kind == "block_diagonal":
                assert mask[-1, -1] and mask[m - 1, (n - 1) // 64 * 64:].all() and lengths.max() <= 64
    shuffled = structured_csr("band", 203, 500, 16, np.random.default_rng(2), shuffle_every=3)
    plain = structured_csr("band", 203, 500, 16, np.random.default_rng(2))
    assert not np.array_equal(shuffled[2], plain[2])
    for r in range(203):
        a, b = plain[1][r], plain[1][r + 1]
        assert sorted(shuffled[2][a:b]) == list(plain[2][a:b])
        assert r % 3 == 0 or np.array_equal(shuffled[2][a:b], plain[2][a:b])


def test_structured_mask_cases_reach_their_routes_on_the_host(monkeypatch):
    """The case table of tests/test_gpu_structured_masks.py, walked without a GPU: every
    (route, kind, replica count) reports the route it means to reach (the name and route
    queries are host only), no kind is excluded from any route, every LDS and matrix-core
    route sees every kind, and every summed route has a kind with nnz % 4 != 0."""
    import test_gpu_structured_masks as S
    from helpers import STRUCTURED_KINDS
    from torch_sputnik_amd import capi
    seen, odd = {}, set()
    for route, kind, nnz, mean, replicas, reported in S.walk_routes(capi, monkeypatch):
        seen.setdefault(route, set()).add(kind)
        if nnz % 4:
            odd.add(route)
    assert len(seen) == len(S.ALL_ROUTES) + 2       # (the flat route walks its three loops)
    assert any(r[5] == "spmm_flat_kernel<2>" for r in S.walk_routes(capi, monkeypatch, S.SPMM_ROUTES[-1:]))
    for route, kinds in seen.items():
        assert kinds == set(STRUCTURED_KINDS), route
        assert not route.startswith("sddmm_sum") or route in odd, route


# Knob of the `spmm_kernel` / `sddmm_kernel` fixtures -> what the name query says when reached.
SPMM_KNOB_ROUTES = {"wide": "spmm_tiled_kernel<TileConfig<256", "wide512": "spmm_tiled_kernel<TileConfig<512",
                    "flat": "spmm_flat_kernel", "narrow": "spmm_tiled64_kernel", "gather": "spmm_rowgather_kernel",
                    "panel": "spmm_panel64_kernel"}
SDDMM_KNOB_ROUTES = {"tiled": ("sddmm_quad_kernel", "sddmm_stationary_kernel"), "wave": ("sddmm_rowwave_kernel",)}


def _params(test):
    """argvalues of a test function's static parametrizations, outermost decorator last."""
    return [list(mark.args[1]) for mark in test.pytestmark if mark.name == "parametrize"]


def knob_fall_through(monkeypatch, report=None):
    """For the tests parametrized over the `spmm_kernel` / `sddmm_kernel` fixtures: per test and
    knob, (shapes that reach the knob's route, shapes in all) -- the rest runs another kernel
    under the knob's label (a kernel that does not apply to a shape falls through)."""
    import test_gpu_parity as P
    import test_gpu_extensions as E
    import test_gpu_half as H
    from torch_sputnik_amd import capi

    def nnz_of(*args, **kw):
        return len(make_csr(*args, **kw)[4])
    spmm_tests = {
        "test_spmm_capi_vs_oracle": [(m, k, n, nnz_of(m, k, s, seed=m * 7 + n, empty_rows=e, order=o), 1)
                                     for m, k, n, s, o, e in P.SPMM_SHAPES],
        "test_spmm_tiled_stress": [(m, k, n, nnz_of(m, k, s, seed=3 * m + k + n, round_to=1,
                                                    empty_rows=(m - 1,) if s > 0.5 else ()), 1)
                                   for m, k, n, s in P.STRESS],
        "test_spmm_partial_column_tiles": [(m, k, n, nnz_of(m, k, s, seed=m + n, round_to=1, empty_rows=(m // 3,)), r)
                                           for m, k, n, s, r in P.TAIL_SHAPES],
        "test_spmm_batched_capi": [(m, k, n, nnz_of(m, k, 0.85, seed=21), r)
                                   for r, _, m, k, n in _params(P.test_spmm_batched_capi)[0]],
        "test_spmm_unsorted_columns": [(m, k, n, nnz_of(m, k, 0.8, seed=23), 1)
                                       for m, k, n in _params(P.test_spmm_unsorted_columns)[0]],
        "test_spmm_bias_capi_vs_oracle": [(m, k, n, nnz_of(m, k, s, seed=m + n + relu, order="ascending"), r)
                                          for m, k, n, s, r in E.BIAS_SHAPES for relu in (0, 1)],
        "test_spmm_bias_unsorted_columns_take_the_fallback_epilogue": [
            (256, k, n, nnz_of(256, k, 0.7, seed=21), 1)
            for k, n in _params(E.test_spmm_bias_unsorted_columns_take_the_fallback_epilogue)[0]],
    }
    sddmm_tests = {
        "test_sddmm_capi_vs_oracle": [(m, k, n, nnz_of(m, n, s, seed=m + k + n, round_to=1, empty_rows=(m // 2,)), r, 4)
                                      for m, k, n, s, r in P.SDDMM_SHAPES],
        "test_sddmm_half_capi_vs_oracle": [(m, k, n, nnz_of(m, n, s, seed=m + k + n, round_to=1,
                                                            empty_rows=(m // 2,)), r, 2)
                                           for m, k, n, s, r in H.SDDMM_SHAPES],
        "test_sddmm_half_output": [(m, k, n, nnz_of(m, n, s, seed=m + k + n, round_to=1), r, 2)
                                   for m, k, n, s, r in _params(H.test_sddmm_half_output)[0]],
    }
    # the summed form has its own decision: "tiled" must give tiled partial vectors (or the
    # plain product on an LDS kernel), "wave" the row-wave kernel
    sum_shapes = [(m, k, n, nnz_of(m, n, s, seed=m + k + n, round_to=1 if m == 33 else 4, empty_rows=(m // 2,)), r)
                  for m, k, n, s, r in P.SDDMM_SUM_SHAPES]
    counts = {}
    knobs = ("SPUTNIK_HIP_SPMM_KERNEL", "SPUTNIK_HIP_SDDMM_KERNEL")
    try:
        for knob, expect in SPMM_KNOB_ROUTES.items():
            monkeypatch.setenv("SPUTNIK_HIP_SPMM_KERNEL", knob)
            capi.reload_options()
            for test, shapes in spmm_tests.items():
                names = [capi.spmm_kernel_name(*shape) for shape in shapes]
                counts[test, knob] = (sum(name.startswith(expect) for name in names), len(shapes),
                                      sum(name == "spmm_rowgather_kernel" for name in names))
        monkeypatch.delenv("SPUTNIK_HIP_SPMM_KERNEL")
        for knob, expect in SDDMM_KNOB_ROUTES.items():
            monkeypatch.setenv("SPUTNIK_HIP_SDDMM_KERNEL", knob)
            capi.reload_options()
            for test, shapes in sddmm_tests.items():
                names = [capi.sddmm_kernel_name(*shape) for shape in shapes]
                counts[test, knob] = (sum(name in expect for name in names), len(shapes),
                                      sum(name == "sddmm_rowwave_kernel" for name in names))
            got = [capi.sddmm_sum_route(*shape) for shape in sum_shapes]
            on_lds = [r["kernel"] == "tiled" or (r["kernel"] == "plain" and r["panel_width"] > 0) for r in got]
            counts["test_sddmm_sum_capi_vs_oracle", knob] = (
                sum(on_lds) if knob == "tiled" else sum(not x for x in on_lds), len(got), sum(not x for x in on_lds))
    finally:
        for name in knobs:
            monkeypatch.delenv(name, raising=False)
        capi.reload_options()
    return counts


def test_every_forced_knob_reaches_its_route_in_every_test(monkeypatch):
    """The `spmm_kernel` / `sddmm_kernel` fixtures force a route, but a kernel that does not
    apply to a shape falls through to the next one: per test and knob at least one of the
    test's static shapes must really reach the kernel the knob names (DESIGN.md has the
    counts).  The panel kernel is taken where the DEVICE offers its 128 KiB of LDS, so a host
    without a device cannot be asked about it."""
    counts = knob_fall_through(monkeypatch)
    print("\ntest, knob: shapes that reach the knob's route / shapes (of which on the row gather / row-wave)")
    for (test, knob), (reached, shapes, gather) in counts.items():
        print(f"{test:<58} {knob:<8} {reached:>2} / {shapes:<2} ({gather})")
        if knob == "panel" and not torch.cuda.is_available():
            continue
        assert reached >= 1, f"no shape of {test} reaches the route of knob {knob!r}"
