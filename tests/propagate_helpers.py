"""Shared inputs of the signal-propagation tests (plain numpy, no GPU):
seeded records with tombstones and the weights that matter to the rule, and
x planes with the values that matter."""
from __future__ import annotations

import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
# NaN, +-inf, not summable (200, 128), the edge of summable, denormals, zeros, small terms
SPECIAL_W = np.array([np.nan, np.inf, -np.inf, 200.0, -200.0, 128.0, -128.0, 127.99999, -127.99999, 1e-40, -1e-40, -0.0,
                      0.0, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -24), 15.9, -0.75], dtype=F32)
SPECIAL_X = np.array([0, 1, -1, I32_MIN, I32_MAX, 1 << 30, -(1 << 30), 65535, -65537], dtype=np.int32)


def records(n, seed, n_nrn, dead=0.1):
    """Seeded records: uniform src / dst, weights in [-1, 1] with the special
    values on a third of them, the fraction ``dead`` of the records tombstones."""
    from abnn_amd import SYN_DTYPE

    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"] = rng.integers(0, n_nrn, n, dtype=np.uint32)
    syn["dst"] = rng.integers(0, n_nrn, n, dtype=np.uint32)
    syn["w"] = rng.uniform(-1.0, 1.0, n).astype(F32)
    sp = rng.random(n) < 0.33
    syn["w"][sp] = rng.choice(SPECIAL_W, int(sp.sum()))
    gone = rng.random(n) < dead
    syn["src"][gone] = NONE
    syn["dst"][gone] = NONE
    return syn


def plane(n_nrn, seed, zero_fraction=0.3):
    """A seeded x: any int32, the special values on four tenths, ``zero_fraction`` zeros."""
    rng = np.random.default_rng(seed)
    x = rng.integers(I32_MIN, I32_MAX, n_nrn, dtype=np.int64).astype(np.int32)
    sp = rng.random(n_nrn) < 0.4
    x[sp] = rng.choice(SPECIAL_X, int(sp.sum()))
    x[rng.random(n_nrn) < zero_fraction] = 0
    return x


def one_hot(n_nrn, at, value=1 << 30):
    x = np.zeros(n_nrn, dtype=np.int32)
    x[at] = value
    return x
