"""GPU: the argument checks of the topology ops of the binding itself (csrc/torch_binding.cpp),
reached through ``torch.ops.torch_sputnik.*`` directly -- ``ops.py`` turns the same inputs away
before the binding sees them, so nothing else exercises these checks.  Every bad input is a
host-side rejection before any launch: a RuntimeError.  One good call per op equals the torch path
of ``topology.*`` on the CPU copy of the same input bit for bit.

The pattern is 4 x 8 with 6 entries (row lengths 2, 0, 3, 1).

Two inputs of the list are accepted by the binding, as documented, and are asserted as such:
``csr_topk`` takes any ``per_row >= 0`` (it does not know the matrix width: a row keeps
``min(len_r, per_row)``), and ``dense_to_csr`` reads every real dtype, float64 included."""
import pytest
import torch

from torch_sputnik_amd import ops, topology

pytestmark = pytest.mark.gpu

M, N, NNZ = 4, 8, 6
T = torch.ops.torch_sputnik
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module")
def host():
    """The pattern, its values, a second layer's values, drop counts and dense scores on the CPU."""
    return dict(
        values=torch.tensor([0.5, -2.0, 1.5, -0.25, 3.0, -1.0]),
        other=torch.tensor([-0.75, 4.0, 0.125, 2.5, -1.25, 0.0625]),
        row_offsets=torch.tensor([0, 2, 2, 5, 6], dtype=torch.int32),
        column_indices=torch.tensor([1, 5, 0, 3, 7, 4], dtype=torch.int32),
        drop_counts=torch.tensor([1, 0, 2, 1], dtype=torch.int32),
        scores=((torch.arange(M * N, dtype=torch.float32) * 7) % 32 - 15.5).reshape(M, N))


@pytest.fixture(scope="module")
def dev(host):
    return {name: t.cuda() for name, t in host.items()}


def rejects(op, *args, what, **kwargs):
    with pytest.raises(RuntimeError):
        op(*args, **kwargs)
        pytest.fail(f"accepted {what}")


def same(got, want, what):
    got, want = list(got), list(want)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        bits = _BITS[w.element_size()]
        assert torch.equal(g.cpu().contiguous().view(bits), w.contiguous().view(bits)), (what, i, g, w)


def csr_cases(dev, with_scores):
    """The bad inputs every op over (values, row_offsets, column_indices[, scores]) shares, as
    (values, row_offsets, column_indices, scores)"""
    v, ro, ci, sc = dev["values"], dev["row_offsets"], dev["column_indices"], dev["scores"]
    yield (v, ro.cpu(), ci, sc), "row_offsets on the CPU"
    yield (v, ro, ci.cpu(), sc), "column_indices on the CPU"
    yield (v, ro.long(), ci, sc), "int64 row_offsets"
    yield (v, ro, ci.long(), sc), "int64 column_indices"
    yield (v, ro, ci[:-1], sc), "column_indices one short"
    yield (v[:-1], ro, ci, sc), "values one short"
    yield (v.reshape(1, NNZ), ro, ci, sc), "2-D values"
    yield (v.reshape(2, 3), ro, ci, sc), "2-D values"
    yield (v.double(), ro, ci, sc), "float64 values"
    yield (v.to(torch.int32), ro, ci, sc), "int32 values"
    yield (v, ro.reshape(1, M + 1), ci, sc), "2-D row_offsets"
    if with_scores:
        yield (v, ro, ci, sc.cpu()), "scores on the CPU"
        yield (v, ro, ci, sc.double()), "float64 scores"
        yield (v, ro, ci, sc.reshape(-1)), "1-D scores"
        yield (v, ro, ci, sc.reshape(1, M, N)), "3-D scores"
        yield (v, ro[:-1], ci, sc), "row_offsets one short of [m + 1]"
        yield (v, ro, ci, sc[:-1]), "scores one row short"


def test_topk_to_csr(host, dev):
    sc = dev["scores"]
    for args, what in (((sc.double(), 3, -1, None), "float64 scores"),
                       ((sc.reshape(-1), 3, -1, None), "1-D scores"),
                       ((sc.reshape(1, M, N), 3, -1, None), "3-D scores"),
                       ((sc.cpu(), 3, -1, None), "scores on the CPU"),
                       ((sc, 3, -1, sc.cpu()), "values_from on the CPU"),
                       ((sc, 3, -1, sc[:-1]), "values_from of another shape"),
                       ((sc, 3, -1, sc.double()), "8-byte values_from"),
                       ((sc, 3, 6, None), "both per_row and total"),
                       ((sc, -1, -1, None), "neither per_row nor total"),
                       ((sc, N + 1, -1, None), "per_row above n"),
                       ((sc, -1, M * N + 1, None), "total above m * n")):
        rejects(T.topk_to_csr, *args, what=what)
    same(T.topk_to_csr(sc, 3, -1, None), topology.topk_to_csr(host["scores"], per_row=3), "per_row")
    same(T.topk_to_csr(sc, -1, NNZ, None), topology.topk_to_csr(host["scores"], total=NNZ), "total")
    half = host["scores"].to(torch.float16)
    same(T.topk_to_csr(sc, -1, NNZ, half.cuda()), topology.topk_to_csr(host["scores"], total=NNZ, values_from=half),
         "values_from")


def test_csr_regrow(host, dev):
    dc = dev["drop_counts"]

    def call(v, ro, ci, sc, drop_counts=dc):
        return T.csr_regrow(v, ro, ci, drop_counts, sc)

    for args, what in csr_cases(dev, True):
        rejects(call, *args, what=what)
    good = (dev["values"], dev["row_offsets"], dev["column_indices"], dev["scores"])
    for drop_counts, what in ((dc.cpu(), "drop_counts on the CPU"), (dc.long(), "int64 drop_counts"),
                              (dc[:-1], "drop_counts one short"), (dc.reshape(2, 2), "2-D drop_counts")):
        rejects(call, *good, drop_counts, what=what)
    same(call(*good), topology.regrow_per_row(host["values"], host["row_offsets"], host["column_indices"],
                                              host["drop_counts"], host["scores"]), "csr_regrow")


def test_csr_regrow_total(host, dev):
    def call(v, ro, ci, sc, drop=3):
        return T.csr_regrow_total(v, ro, ci, drop, sc)

    for args, what in csr_cases(dev, True):
        rejects(call, *args, what=what)
    good = (dev["values"], dev["row_offsets"], dev["column_indices"], dev["scores"])
    rejects(call, *good, -1, what="drop below 0")
    rejects(call, *good, NNZ + 1, what="drop above nnz")
    for drop in (0, 3, NNZ):
        same(call(*good, drop), topology.regrow_total(host["values"], host["row_offsets"], host["column_indices"],
                                                      drop, host["scores"]), f"csr_regrow_total drop {drop}")


def test_csr_topk(host, dev):
    def call(v, ro, ci, sc=None, per_row=-1, total=4):
        return T.csr_topk(v, ro, ci, per_row, total)

    for args, what in csr_cases(dev, False):
        rejects(call, *args, what=what)
    good = (dev["values"], dev["row_offsets"], dev["column_indices"])
    rejects(call, good[0], good[1][:0], good[2], what="empty row_offsets")
    rejects(call, *good, None, 2, 4, what="both per_row and total")
    rejects(call, *good, None, -1, -1, what="neither per_row nor total")
    rejects(call, *good, None, -1, NNZ + 1, what="total above nnz")
    on_host = (host["values"], host["row_offsets"], host["column_indices"], N)
    same(call(*good), topology.prune_csr(*on_host, total=4), "total")
    same(call(*good, None, 2, -1), topology.prune_csr(*on_host, per_row=2), "per_row")
    # the op does not know n: per_row above it is taken, every row keeps what it has
    same(call(*good, None, N + 1, -1), topology.prune_csr(*on_host, per_row=N), "per_row above n")


def test_csr_topk_global(host, dev):
    other = dev["other"]

    def call(v, ro, ci, sc=None, total=7):
        return T.csr_topk_global([other, v], [dev["row_offsets"], ro], [dev["column_indices"], ci], total)

    for args, what in csr_cases(dev, False):
        rejects(call, *args, what=what)
    v, ro, ci = dev["values"], dev["row_offsets"], dev["column_indices"]
    rejects(call, v.to(torch.float16), ro, ci, what="two dtypes")
    rejects(T.csr_topk_global, [v.double(), other], [ro, ro], [ci, ci], 7, what="float64 values in the first layer")
    rejects(T.csr_topk_global, [v, other], [ro], [ci, ci], 7, what="lists of different lengths")
    rejects(call, v, ro, ci, None, -1, what="total below 0")
    rejects(call, v, ro, ci, None, 2 * NNZ + 1, what="total above the entries of all layers")
    want = topology.prune_csr_global([(host["other"], host["row_offsets"], host["column_indices"], N),
                                      (host["values"], host["row_offsets"], host["column_indices"], N)], 7)
    same(call(v, ro, ci), [t for layer in want for t in layer], "csr_topk_global")


def test_random_csr(dev):
    device = dev["values"].device
    state = torch.tensor([1234, 8], dtype=torch.int64)
    scale, mask = ops.random_value_scale(1.0), ops.RANDOM_KEY_MASK

    def call(m=M, n=N, per_row=-1, total=NNZ, dtype=torch.float32, where=device, rng_state=state.cuda(), key_mask=mask):
        return T.random_csr(m, n, per_row, total, dtype, scale, where, rng_state, key_mask)

    for kwargs, what in ((dict(where=torch.device("cpu")), "a CPU device"),
                         (dict(rng_state=state), "rng_state on the CPU"),
                         (dict(rng_state=state.cuda().to(torch.int32)), "int32 rng_state"),
                         (dict(rng_state=torch.zeros(3, dtype=torch.int64, device=device)), "rng_state [3]"),
                         (dict(dtype=torch.float64), "float64 values"),
                         (dict(per_row=3), "both per_row and total"),
                         (dict(total=-1), "neither per_row nor total"),
                         (dict(per_row=N + 1, total=-1), "per_row above n"),
                         (dict(total=M * N + 1), "total above m * n"),
                         (dict(m=-1), "m below 0"),
                         (dict(key_mask=-1), "key_mask below 0"),
                         (dict(key_mask=mask + 1), "key_mask above 0x7fffffff")):
        rejects(call, what=what, **kwargs)
    for per_row, dtype in ((False, torch.float32), (True, torch.bfloat16)):
        count = 3 if per_row else NNZ
        got = call(per_row=count if per_row else -1, total=-1 if per_row else count, dtype=dtype)
        values, row_indices, row_offsets, column_indices = topology.random_csr(
            M, N, nonzeros=count, per_row=per_row, dtype=dtype, bound=1.0, device="cpu", rng_state=state)
        same(got, (row_indices, row_offsets, column_indices, values, state), f"random_csr per_row={per_row}")


def test_dense_to_csr(host, dev):
    dense = torch.zeros(M, N)
    rows = torch.repeat_interleave(torch.arange(M), torch.tensor([2, 0, 3, 1]))
    dense[rows, host["column_indices"].long()] = host["values"]
    on_device = dense.cuda()
    for args, what in (((dense, True), "a dense matrix on the CPU"),
                       ((on_device.reshape(-1), False), "a 1-D tensor"),
                       ((on_device.reshape(1, 1, 1, M, N), False), "a 5-D tensor"),
                       ((on_device.reshape(1, 2, 2, N), False), "[b, 2, m, n]"),
                       ((on_device.reshape(1, M, N), True), "values of a 3-D tensor"),
                       ((on_device.to(torch.complex64), False), "a complex tensor")):
        rejects(T.dense_to_csr, *args, what=what)
    for dtype in (torch.float32, torch.float64):        # every real dtype is read, float64 too
        values, row_indices, row_offsets, column_indices = topology.dense_to_sparse(dense.to(dtype))
        assert torch.equal(column_indices, host["column_indices"]) and torch.equal(row_offsets, host["row_offsets"])
        got = T.dense_to_csr(on_device.to(dtype), True)
        same(got[:3] + got[4:], (row_indices, row_offsets, column_indices, values), f"dense_to_csr {dtype}")
        assert got[3].tolist() == [NNZ]
    nonzeros = T.dense_to_csr(on_device.reshape(1, 1, M, N), False)[3]
    assert not nonzeros.is_cuda and nonzeros.dtype == torch.int64 and nonzeros.tolist() == [NNZ]
