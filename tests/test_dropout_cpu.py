"""CPU: the attention-dropout contract restated in numpy (tests/philox_ref.py) against
known-answer vectors, the p rules, the C ABI's argument check, and modules in eval() mode
(no dropout, no new op reached)."""
import numpy as np
import pytest
import torch

import philox_ref as P


def words(key, counter):
    return [int(w) for w in P.philox4x32_10(key, counter)]


def test_philox_known_answers():
    assert words((0, 0), (0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert words((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    ones = 0xFFFFFFFF
    assert words((ones, ones), (ones, ones, ones, ones)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_threshold_and_scale_rules():
    assert P.threshold(0.0) == 2 ** 32 - 1
    assert P.threshold(0.5) == 2 ** 31
    assert P.threshold(0.1) == int(np.floor(0.9 * 2 ** 32))
    assert P.threshold(1 - 2 ** -40) == 0
    assert P.keep_scale(0.1) == np.float32(1 / 0.9)
    assert P.keep_scale(0.5) == np.float32(2.0)


def test_mask_layout_is_replica_and_entry():
    seed, offset, p = 0x1234_5678_9ABC_DEF0, 40, 0.3
    mask = P.keep_mask(seed, offset, 3, 13, p)
    c = offset // 4
    for r in range(3):
        for e in range(13):
            w = words((seed & 0xFFFFFFFF, seed >> 32), (c & 0xFFFFFFFF, c >> 32, e >> 2, r))[e & 3]
            assert mask[r, e] == (w < P.threshold(p))
    # a many-mask array is the same function of its [replicas, max(nonzeros)] columns: a
    # narrower mask is a prefix of the wider one
    assert np.array_equal(P.keep_mask(seed, offset, 3, 7, p), mask[:, :7])
    # one mask, [nnz] values: replica 0
    assert np.array_equal(P.keep_mask(seed, offset, 1, 13, p)[0], mask[0])


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan")])
def test_p_outside_unit_interval_is_rejected(p):
    from torch_sputnik_amd import capi, functional, modules, ops
    with pytest.raises(ValueError):
        ops.check_dropout_p(p)
    with pytest.raises(ValueError):
        functional.sparse_dropout(torch.zeros(4), p)
    with pytest.raises(ValueError):
        modules.SparseCoreAttention(8, 16, 2, attention_dropout=p)
    # the C ABI checks p before it touches anything
    fn = capi.lib().sputnik_hip_sparse_dropout_typed
    assert fn(0, 0, 0, 0, None, 0, None, 0, p, capi.PhiloxState(), None, None) == -1


def test_eval_module_ignores_attention_dropout(cpu_ops, monkeypatch):
    from torch_sputnik_amd import ops
    from torch_sputnik_amd.modules import SparseAttention, SparseCoreAttention

    def forbidden(*args, **kwargs):
        raise AssertionError("a dropout op was reached in eval()")

    for name in ("sparse_dropout", "sparse_attention_dropout", "sparse_attention_heads_dropout",
                 "sparse_attention_many_mask_dropout", "sparse_attention_heads_many_mask_dropout"):
        monkeypatch.setattr(ops, name, forbidden)

    def attention(**kw):
        torch.manual_seed(0)
        layer = SparseAttention(num_heads=2, embedding_size=16, max_sequence_length=24,
                                device=torch.device("cpu"), sparsity=0.6,
                                mask_generator=np.random.default_rng(5), **kw)
        for i, lin in enumerate(layer.linears):
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(
                    np.random.default_rng(i).uniform(-1, 1, (16, 16)).astype(np.float32)))
            lin.setup_sparse_tensors()
        return layer.eval()

    x = torch.rand(2, 24, 16)
    for fused in (True, False):
        plain, dropped = attention(), attention(attention_dropout=0.1)
        plain.fused_inference = dropped.fused_inference = fused
        with torch.no_grad():
            assert torch.equal(plain(x, x, x), dropped(x, x, x))

    mask = torch.rand(2, 1, 12, 12) < 0.5
    q, k, v = (torch.rand(2, 12, 2, 8) for _ in range(3))
    core = SparseCoreAttention(12, 16, 2).eval()
    core_dropped = SparseCoreAttention(12, 16, 2, attention_dropout=0.1).eval()
    assert torch.equal(core(q, k, v, mask), core_dropped(q, k, v, mask))
