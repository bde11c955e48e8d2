"""The shapes and rules the attention-pattern tests share (tests/test_attention_pattern_cpu.py,
tests/test_gpu_attention_pattern.py), and the rule of include/sputnik_hip.h, "Attention
patterns", as a plain-Python double loop."""
import numpy as np

from tests import philox_ref

ROWS = (1, 5, 127, 128, 129, 203)
WIDTHS = (1, 3, 16, 17, 63, 64, 65, 255, 256, 257, 300, 1000)
RNG_STATE = (0x123456789abcdef, 8)     # {seed, offset} of the random blocks


def offsets(m, n):
    return (0, -5, n - m)


def rules(n):
    """name -> AttentionPattern arguments at width n: each component alone, both dilations, both
    forms of the flags, a global row, and all together"""
    ends = sorted({0, n - 1})
    return {
        "window": dict(window=(3, 2)),
        "window_dilated": dict(window=(2, 3), dilation=3),
        "causal_window": dict(window=(7, 0), causal=True),
        "block": dict(block=5),
        "summary": dict(summary=(8, 2)),
        "global_ends": dict(global_tokens=ends),
        "global_count": dict(global_tokens=min(3, n), global_rows=False),
        "random_1": dict(random_blocks=(1, 0.3)),
        "random_4": dict(random_blocks=(4, 0.3)),
        "random_64": dict(random_blocks=(64, 0.5)),
        "all": dict(window=(2, 1), dilation=3, block=4, summary=(16, 1), global_tokens=ends,
                    random_blocks=(4, 0.1), causal=True),
    }


def random_key(seed, rng_offset, block_row, block_column):
    """key(R, C) of the random component"""
    seed, block = int(seed) & 0xffffffffffffffff, (int(rng_offset) & 0xffffffffffffffff) // 4
    words = philox_ref.philox4x32_10((seed & 0xffffffff, seed >> 32),
                                     (block & 0xffffffff, block >> 32, block_column >> 2, block_row))
    return int(words[block_column & 3]) & 0x7fffffff


def brute_mask(m, n, offset=0, window=None, dilation=1, block=0, global_tokens=None, global_rows=True, summary=None,
               random_blocks=None, causal=False, rng_state=None):
    """bool [m, n] (numpy): the table of the rule, entry by entry"""
    if isinstance(window, int):
        window = (window, window)
    flags = None
    if global_tokens is not None:
        flags = set(range(global_tokens)) if isinstance(global_tokens, int) else {int(g) for g in global_tokens}
    keys = {}
    mask = np.zeros((m, n), dtype=bool)
    for r in range(m):
        p = r + offset
        for c in range(n):
            d = c - p
            keep = False
            if window is not None:
                keep |= -window[0] * dilation <= d <= window[1] * dilation and d % dilation == 0
            if block > 0:
                keep |= c // block == p // block
            if summary is not None:
                keep |= c % summary[0] >= summary[0] - summary[1]
            if flags is not None:
                keep |= c in flags or (global_rows and 0 <= p < n and p in flags)
            if random_blocks is not None:
                rb, probability = random_blocks
                at = (r // rb, c // rb)
                if at not in keys:
                    keys[at] = random_key(rng_state[0], rng_state[1], *at)
                keep |= keys[at] < round(probability * 2 ** 31)
            mask[r, c] = keep and (not causal or d <= 0)
    return mask
