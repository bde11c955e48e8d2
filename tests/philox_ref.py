"""numpy restatement of the attention-dropout contract (csrc/philox.h, sputnik_hip.h
"Attention dropout"), for the tests: Philox4x32-10, the keep threshold and scale, and the
(replica, entry) layout of the keep masks."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, counter):
    """key (k0, k1), counter (c0, c1, c2, c3): scalars or broadcastable uint32 arrays ->
    the four output words, uint32 arrays."""
    k0, k1 = (np.asarray(k, dtype=np.uint32) for k in key)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & LO).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & LO).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = k0 + W0, k1 + W1
    return c0, c1, c2, c3


def threshold(p):
    return min(math.floor((1.0 - p) * 4294967296.0), 4294967295)


def keep_scale(p):
    return np.float32(1.0 / (1.0 - p))


def keep_mask(seed, offset, replicas, width, p):
    """bool [replicas, width]: entry (r, e) kept."""
    seed, offset = int(seed), int(offset)
    assert offset % 4 == 0
    c = offset // 4
    r = np.arange(replicas, dtype=np.uint64)[:, None]
    e = np.arange(width, dtype=np.uint64)[None, :]
    words = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32),
                          (c & 0xFFFFFFFF, c >> 32, (e >> np.uint64(2)).astype(np.uint32),
                           r.astype(np.uint32)))
    stacked = np.stack(words)   # [4, replicas, width]
    word = np.take_along_axis(stacked, (e & np.uint64(3)).astype(np.int64)[None].repeat(replicas, 1), 0)[0]
    return word.astype(np.uint64) < np.uint64(threshold(p))


def keep_mask_of(rng_state, replicas, width, p):
    """keep_mask from an rng_state tensor {seed, offset} (any device)."""
    seed, offset = (int(v) for v in rng_state.cpu().tolist())
    return keep_mask(seed & 0xFFFFFFFFFFFFFFFF, offset, replicas, width, p)
