"""Record pairs and configs shared by the snapshot tests (test_snapshot_abi.py on
the CPU, test_snapshot_gpu.py on the device): every class of the diff's rule
and the special weight pairs, over 1000 neurons (the 256 / 256 / 488 brain)."""
import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
N_NRN = 1000
SYN = np.dtype([("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")])
SIZES = (0, 1, 2, 3, 4095, 4096, 4097, 8193)
UNEQUAL = ((4097, 4099), (4099, 4096))
# name -> snapshot.config(bins, lo, hi, src, dst)
CONFIGS = {
    "no range": (64, -0.05, 0.05, None, None),
    "dst range": (64, -0.05, 0.05, None, (256, 256)),
    "src range": (64, -0.05, 0.05, (0, 500), None),
    "both": (32, -1.0, 1.0, (100, 600), (300, 600)),
    "1 bin": (1, -0.01, 0.01, None, None),
    "4096 bins": (4096, -0.05, 0.05, None, None),
}


def _bits(*u):
    return np.array(u, dtype=np.uint32).view(F32)


# (then, now) weights: NaN against a NaN of another payload and against a number,
# +0 against -0, inf against inf (equal bits: same) and against -inf (d = -inf)
# and a number, denormals, the summable limit from both sides
SPECIAL_PAIRS = np.stack([
    _bits(0x7FC00000, 0x7FC00001, 0x00000000, 0x80000000, 0x7F800000, 0x7F800000, 0xFF800000, 0x7F800000),
    _bits(0x7FC00001, 0x3F000000, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7F800000, 0x3F000000)], axis=1)
SPECIAL_PAIRS = np.concatenate([SPECIAL_PAIRS, np.array(
    [(1e-40, 2e-40), (1e-40, 0.0), (-1e-40, 1e-40), (127.99999, 128.0), (128.0, 127.99999), (127.99999, -127.99999),
     (0.5, np.nan), (-128.0, 0.25), (0.25, 0.25000003), (3e38, -3e38)], dtype=F32)])


def records(n, seed):
    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN)
    syn["src"] = rng.integers(0, N_NRN, n, dtype=np.uint32)
    syn["dst"] = rng.integers(0, N_NRN, n, dtype=np.uint32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    return syn


def pair(n_then, n_now, seed):
    """(then, now): `now` is `then` after learning-sized weight changes on 40 %
    of the records, with records killed, revived, dead on both sides and
    rewired, and the special weight pairs at the first, a middle and the last
    compared index (one of them at each index of a tiny array)."""
    rng = np.random.default_rng(seed + 1000)
    base = records(max(n_then, n_now), seed)
    a, b = base[:n_then].copy(), base[:n_now].copy()
    c = min(n_then, n_now)
    move = rng.random(c) < 0.4
    b["w"][:c][move] = (b["w"][:c][move] + rng.normal(0.0, 0.01, int(move.sum())).astype(F32)).astype(F32)
    for x, first, step in ((b, 1, 17), (a, 3, 19), (a, 5, 23), (b, 5, 23)):  # killed, revived, dead on both sides
        x["src"][first:c:step] = NONE
        x["dst"][first:c:step] = NONE
    live = (a["dst"][:c] != NONE) & (b["dst"][:c] != NONE)
    k = np.flatnonzero(live)[7::29]  # rewired: another dst, another src
    b["dst"][k] = (b["dst"][k] + 1) % N_NRN
    k = np.flatnonzero(live)[11::31]
    b["src"][k] = (b["src"][k] + 999) % N_NRN
    m = len(SPECIAL_PAIRS)
    if c >= 3 * m:
        spots = [(at + j, j) for at in (0, c // 2 - m // 2, c - m) for j in range(m)]
    else:
        spots = [(i, (seed + i) % m) for i in range(c)]
    for i, j in spots:
        a[i] = b[i] = base[i]
        a["w"][i], b["w"][i] = SPECIAL_PAIRS[j]
    return a, b


def invariants(d):
    """The four invariants of abnn.h on a decoded result."""
    assert d["compared"] == min(d["n_then"], d["n_now"]) == d["dead_both"] + d["killed"] + d["revived"] + d["rewired"] + d["paired"]
    assert d["born"] == d["n_now"] - d["compared"] and d["gone"] == d["n_then"] - d["compared"]
    assert d["selected"] == d["same"] + d["changed"] and d["selected"] <= d["paired"]
    assert d["changed"] == d["up"] + d["down"] + d["zero"] + d["nan"]
    assert d["up"] + d["down"] + d["zero"] == d["under"] + d["over"] + int(d["counts"].sum())
    assert d["not_summable"] <= d["changed"] and abs(d["net"]) <= d["abs"]
