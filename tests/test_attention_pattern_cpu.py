"""CPU: topology.AttentionPattern -- the rule in torch (dense_mask) against a plain-Python
double loop of the table in include/sputnik_hip.h ("Attention patterns"), the random blocks
against tests/philox_ref.py; the torch path of build against dense_to_sparse(dense_mask), slab
boundaries included; the argument contract; and the host-only launch-shape query over the
shapes tests/test_gpu_attention_pattern.py runs.  Everything is an integer: comparisons are
exact."""
import itertools

import numpy as np
import pytest
import torch

from tests import attention_pattern_cases as C
from torch_sputnik_amd import capi, ops, topology
from torch_sputnik_amd.topology import AttentionPattern

M, N = 29, 37
STATE = torch.tensor(C.RNG_STATE, dtype=torch.int64)


def same_mask(arguments, m, n, offset, rng_state=None):
    pattern = AttentionPattern(**arguments)
    got = pattern.dense_mask(m, n, offset=offset, rng_state=rng_state)
    assert got.dtype == torch.bool and tuple(got.shape) == (m, n)
    want = C.brute_mask(m, n, offset=offset, rng_state=None if rng_state is None else rng_state.tolist(), **arguments)
    wrong = np.argwhere(got.numpy() != want)
    assert wrong.size == 0, f"{arguments} at offset {offset}: first difference at {wrong[0]}"
    return got


def test_dense_mask_is_the_table():
    """every combination of the deterministic components at 29 x 37"""
    count = 0
    for offset, window, dilation, block, summary, tokens, global_rows, causal in itertools.product(
            (0, -3, 8), (None, 2, (3, 1)), (1, 3), (0, 4), (None, (8, 2)), (None, [0, 5, 36]), (True, False),
            (False, True)):
        if window is None and block == 0 and summary is None and tokens is None:
            continue
        if (window is None and dilation != 1) or (tokens is None and not global_rows):
            continue        # (the argument changes nothing)
        same_mask(dict(window=window, dilation=dilation, block=block, summary=summary, global_tokens=tokens,
                       global_rows=global_rows, causal=causal), M, N, offset)
        count += 1
    assert count == 3 * 2 * (5 * 2 * 2 * 3 - 1)


@pytest.mark.parametrize("tokens", [0, 4, 37, [36], torch.tensor([5, 0, 5], dtype=torch.int32), []])
def test_global_token_forms(tokens):
    mask = same_mask(dict(global_tokens=tokens.tolist() if torch.is_tensor(tokens) else tokens), M, N, 3)
    pattern = AttentionPattern(global_tokens=tokens)
    assert torch.equal(pattern.dense_mask(M, N, offset=3), mask)


@pytest.mark.parametrize("rb", [1, 4])
@pytest.mark.parametrize("offset", [0, -3])
def test_random_blocks_are_the_philox_keys(rb, offset):
    mask = same_mask(dict(random_blocks=(rb, 0.3)), M, N, offset, STATE)
    assert 0 < int(mask.sum()) < M * N
    same_mask(dict(random_blocks=(rb, 0.3), window=(2, 2), causal=True), M, N, offset, STATE)


def test_probability_zero_and_one():
    window = AttentionPattern(window=1).dense_mask(M, N)
    assert torch.equal(AttentionPattern(window=1, random_blocks=(4, 0.0)).dense_mask(M, N, rng_state=STATE), window)
    assert not AttentionPattern(random_blocks=(1, 0.0)).dense_mask(M, N, rng_state=STATE).any()
    assert AttentionPattern(random_blocks=(4, 1.0)).dense_mask(M, N, rng_state=STATE).all()
    causal = AttentionPattern(random_blocks=(4, 1.0), causal=True).dense_mask(M, N, rng_state=STATE)
    assert torch.equal(causal, torch.ones(M, N, dtype=torch.bool).tril())


def test_rng_state_reproduces_and_offset_changes():
    pattern = AttentionPattern(random_blocks=(2, 0.4))
    first = pattern.build(M, N, rng_state=STATE)
    again = pattern.build(M, N, rng_state=STATE.clone())
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    moved = pattern.build(M, N, rng_state=STATE + torch.tensor([0, 4]))
    assert not torch.equal(first[2], moved[2])
    # without a state a CPU build draws one and returns it; that state reproduces the build
    torch.manual_seed(3)
    drawn = pattern.build(M, N, return_rng_state=True)
    assert drawn[3].dtype == torch.int64 and drawn[3].numel() == 2 and int(drawn[3][1]) % 4 == 0
    replay = pattern.build(M, N, rng_state=drawn[3])
    assert all(torch.equal(a, b) for a, b in zip(drawn[:3], replay))
    # no random blocks: no state, and torch's generator is left alone
    before = torch.get_rng_state()
    assert AttentionPattern(window=2).build(M, N, return_rng_state=True)[3] is None
    assert torch.equal(torch.get_rng_state(), before)


def assert_build_is_dense_to_sparse(pattern, m, n, offset, rng_state=None):
    mask = pattern.dense_mask(m, n, offset=offset, rng_state=rng_state)
    _, row_indices, row_offsets, column_indices = topology.dense_to_sparse(mask.to(torch.float32))
    got = pattern.build(m, n, offset=offset, rng_state=rng_state)
    for name, a, b in zip(("row_indices", "row_offsets", "column_indices"), got,
                          (row_indices, row_offsets, column_indices)):
        assert a.dtype == torch.int32 and torch.equal(a, b), f"{name} of {pattern} at {m} x {n}, offset {offset}"
    assert int(got[1][m]) == got[2].numel()


@pytest.mark.parametrize("slab", [2 ** 24, 12 * N, 5 * N, 1])
def test_build_equals_dense_to_sparse(slab, monkeypatch):
    """the torch path in slabs of 29, 12, 5 and 1 rows (a slab boundary inside a block row of the
    random blocks, and inside the run of empty rows of the causal pattern)"""
    monkeypatch.setattr(topology, "_PATTERN_SLAB", slab)
    for name, arguments in C.rules(N).items():
        for offset in (0, -5, N - M):
            assert_build_is_dense_to_sparse(AttentionPattern(**arguments), M, N, offset, STATE)
    assert_build_is_dense_to_sparse(AttentionPattern(window=1), 0, N, 0)
    assert_build_is_dense_to_sparse(AttentionPattern(window=1), M, 0, 0)


def test_counted_example():
    """(203, 300, offset -5, window (7, 0), causal): 5 empty rows and 1556 entries"""
    row_indices, row_offsets, column_indices = AttentionPattern(window=(7, 0), causal=True).build(203, 300, offset=-5)
    lengths = row_offsets[1:] - row_offsets[:-1]
    assert int((lengths == 0).sum()) == 5 and column_indices.numel() == 1556
    assert row_indices[:5].tolist() == [0, 1, 2, 3, 4]


def test_fallback_beyond_the_device_rows(monkeypatch):
    """more rows than the device path serves, without an [m, n] image: 20000 x 64 in slabs of
    4096 rows"""
    monkeypatch.setattr(topology, "_PATTERN_SLAB", 4096 * 64)
    m, n = 20000, 64
    assert not capi.attention_pattern_launch_shape(m, n, 0)["served"]
    row_indices, row_offsets, column_indices = AttentionPattern(block=8, causal=True).build(m, n, offset=n - m)
    lengths = (row_offsets[1:] - row_offsets[:-1]).tolist()
    assert lengths[:m - n] == [0] * (m - n) and lengths[m - n:] == [1 + i % 8 for i in range(n)]
    assert column_indices[-8:].tolist() == list(range(56, 64)) and row_indices.numel() == m


BAD = [
    (dict(), "at least one"),
    (dict(window=-1), "window"),
    (dict(window=(1, 2, 3)), "window"),
    (dict(window=1.5), "window"),
    (dict(window=(1, -2)), "window"),
    (dict(window=1, dilation=0), "dilation"),
    (dict(block=-4), "block"),
    (dict(block=True), "block"),
    (dict(summary=(4, 5)), "summary"),
    (dict(summary=(4, 0)), "summary"),
    (dict(summary=(0, 0)), "summary"),
    (dict(summary=4), "summary"),
    (dict(global_tokens=-1), "global_tokens"),
    (dict(global_tokens=[0, -2]), "global_tokens"),
    (dict(global_tokens=torch.tensor([0.5])), "global_tokens"),
    (dict(global_tokens=torch.zeros(2, 2, dtype=torch.int64)), "global_tokens"),
    (dict(random_blocks=(0, 0.5)), "random_blocks"),
    (dict(random_blocks=(4, 1.5)), "random_blocks"),
    (dict(random_blocks=(4, -0.1)), "random_blocks"),
    (dict(random_blocks=0.5), "random_blocks"),
]


@pytest.mark.parametrize("arguments,word", BAD, ids=[str(i) for i in range(len(BAD))])
def test_contract_of_the_rule(arguments, word):
    with pytest.raises(ValueError, match=word) as raised:
        AttentionPattern(**arguments)
    assert "AttentionPattern" in str(raised.value)
    with pytest.raises(ValueError, match="attention_pattern_csr.*" + word):   # before the device is looked at
        ops.attention_pattern_csr(4, 4, device="cpu", **arguments)


def test_contract_of_a_build():
    with pytest.raises(ValueError, match="global_tokens"):      # positions against n
        AttentionPattern(global_tokens=[37]).build(M, N)
    with pytest.raises(ValueError, match="global_tokens"):
        AttentionPattern(global_tokens=38).dense_mask(M, N)
    AttentionPattern(global_tokens=[36]).build(M, N)
    pattern = AttentionPattern(random_blocks=(4, 0.5))
    with pytest.raises(ValueError, match="rng_state"):
        pattern.build(M, N, rng_state=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="rng_state"):
        pattern.build(M, N, rng_state=torch.tensor([1.0, 4.0]))
    with pytest.raises(ValueError, match="multiple of 4"):
        pattern.build(M, N, rng_state=torch.tensor([1, 6]))
    with pytest.raises(ValueError, match="rng_state"):
        pattern.dense_mask(M, N)
    for sizes in ((-1, 4), (4, -1), (4.0, 4)):
        with pytest.raises(ValueError, match="AttentionPattern.build"):
            AttentionPattern(window=1).build(*sizes)
    with pytest.raises(ValueError, match="offset"):
        AttentionPattern(window=1).build(4, 4, offset=0.5)
    with pytest.raises(RuntimeError, match="GPU devices only"):
        ops.attention_pattern_csr(4, 4, window=1, device="cpu")


def test_launch_shape_walk():
    """every rows_per_wave instance is reached over the widths the GPU file runs, and its shapes
    hold a partial last step and a partial last workgroup"""
    reached, partial_step, partial_group = set(), False, False
    for n in C.WIDTHS:
        for m in C.ROWS:
            shape = capi.attention_pattern_launch_shape(m, n, 0)
            assert shape["served"] and shape["columns_per_lane"] == 4 and shape["launches"] == 4
            rows_per_wave = shape["rows_per_wave"]
            span = 64 // rows_per_wave * 4
            assert rows_per_wave == 16 or n > span // 2        # the most rows whose lanes cover n ...
            assert rows_per_wave == 1 or n <= span             # ... in one step
            assert shape["rows_per_workgroup"] == 4 * rows_per_wave
            assert shape["grid"] == -(-m // shape["rows_per_workgroup"])
            reached.add(rows_per_wave)
            partial_step |= n % span != 0
            partial_group |= m % shape["rows_per_workgroup"] != 0
    assert reached == {16, 8, 4, 2, 1}
    assert {capi.attention_pattern_launch_shape(5, n, 0)["rows_per_wave"] for n in
            (1, 3, 16, 17, 63, 64, 65, 255, 256, 257, 300)} == {16, 8, 4, 2, 1}
    assert partial_step and partial_group


def test_launch_shape_limits():
    served = lambda *a: capi.attention_pattern_launch_shape(*a)["served"]   # noqa: E731
    assert served(16384, 1024, 0) and not served(16385, 1024, 0)
    assert served(16384, 131071, 0) and not served(16384, 131072, 0)        # m * n against INT_MAX
    assert served(8, 8, 2 ** 30 - 1) and not served(8, 8, 2 ** 30) and not served(8, 8, -2 ** 30)
    assert served(0, 5, 0) and served(5, 0, 0)
    assert not served(2 ** 31, 1, 0) and not served(1, 1, 2 ** 63)
    with pytest.raises(RuntimeError):
        capi.attention_pattern_launch_shape(-1, 4, 0)
    unserved = capi.attention_pattern_launch_shape(16385, 4, 0)
    assert unserved == dict(served=False, rows_per_wave=-1, columns_per_lane=-1, rows_per_workgroup=-1, grid=-1,
                            launches=-1)


def test_module_takes_its_topology_from_the_pattern():
    """construction and set_pattern on the CPU (the kernels are exercised in the GPU file); without
    a pattern the constructor draws the same random mask from the same generator calls"""
    from torch_sputnik_amd import SparseAttention, functional
    cpu = torch.device("cpu")
    pattern = AttentionPattern(window=(16, 0), global_tokens=4, causal=True)
    module = SparseAttention(2, 128, max_sequence_length=128, device=cpu, pattern=pattern)
    assert module.mask2d is None and module.pattern is pattern and module.pattern_rng_state is None
    want = pattern.build(128)
    topology_of = lambda m: (m.row_indices, m.row_offsets, m.column_indices)   # noqa: E731
    assert all(torch.equal(a, b) for a, b in zip(topology_of(module), want))
    assert functional._is_static(*topology_of(module))
    old = topology_of(module)
    second = AttentionPattern(block=32, random_blocks=(8, 0.2))
    assert module.set_pattern(second, rng_state=STATE) is module
    assert torch.equal(module.pattern_rng_state, STATE) and module.pattern is second
    assert all(torch.equal(a, b) for a, b in zip(topology_of(module), second.build(128, rng_state=STATE)))
    assert functional._is_static(*topology_of(module)) and not functional._is_static(*old)
    with pytest.raises(TypeError, match="AttentionPattern"):
        module.set_pattern("window")
    plain = SparseAttention(2, 128, max_sequence_length=64, device=cpu, mask_generator=np.random.default_rng(3))
    mask = topology.generate_mask(64, 64, cpu, sparsity=0.9, generator=np.random.default_rng(3))
    assert plain.pattern is None and torch.equal(plain.mask2d, mask)
    assert torch.equal(plain.column_indices, topology.dense_to_sparse(mask)[3])
