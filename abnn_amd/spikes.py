"""The spike recorder's host side (abnn.h abnn_spikes_*): the
config, the numpy view of a pass entry, the per-pass rule restated in numpy
(the test reference: it never calls the library) and the split of a raster
into its passes."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._lib import SpikesConfig

# abnn_spike_pass, 32 bytes
SPIKE_PASS_DTYPE = np.dtype([("pass_index", "<u8"), ("now", "<u8"), ("offset", "<u8"),
                             ("count", "<u4"), ("epoch", "<u4")])
assert SPIKE_PASS_DTYPE.itemsize == 32

INFO_FIELDS = ("passes_seen", "spikes_seen", "selected_seen", "passes_recorded", "spikes_recorded",
               "passes_dropped", "spikes_dropped")


def config(raster: int, passes: int, neurons: Optional[Sequence[int]] = None, counts: bool = False) -> SpikesConfig:
    """abnn_spikes_config: ``raster`` spikes and ``passes`` pass entries held;
    ``neurons`` = (first, count) or None for every neuron; ``counts`` keeps the
    per-neuron spike counts.  Nothing is checked here: abnn_spikes_start does."""
    first, count = (0, 0) if neurons is None else (int(neurons[0]), int(neurons[1]))
    return SpikesConfig(int(raster), int(passes), first, count, 1 if counts else 0)


def reference(lists, meta, cfg: SpikesConfig, n_neuron: Optional[int] = None, clears=()) -> dict:
    """The per-pass rule of abnn.h over given per-pass spike lists.

    ``lists[k]`` is pass k's list L (dst in budget order), ``meta[k]`` its
    (pass_index, now, epoch).  ``clears`` maps a position k to keep_counts: an
    abnn_spikes_clear(keep_counts) before pass k (k == len(lists): after the
    last one); a dict, or pairs.  Returns what Brain.spikes() returns -- info,
    passes (SPIKE_PASS_DTYPE), raster (u32; empty without a raster) -- and
    counts (u32 over the selected neurons; ``n_neuron`` of them when no range is
    set; None with counts off)."""
    clears = dict(clears)
    ranged = cfg.count != 0
    first = cfg.first if ranged else 0
    info = dict.fromkeys(INFO_FIELDS, 0)
    n_counts = (cfg.count if ranged else n_neuron) if cfg.counts else None
    if cfg.counts and n_counts is None:
        raise ValueError("counts over every neuron need n_neuron")
    counts = np.zeros(n_counts, dtype=np.uint32) if cfg.counts else None
    entries, raster, dropped = [], [], False

    def clear(keep_counts):
        nonlocal dropped
        entries.clear()
        raster.clear()
        dropped = False
        for k in ("passes_recorded", "spikes_recorded", "passes_dropped", "spikes_dropped"):
            info[k] = 0
        if counts is not None and not keep_counts:
            counts[:] = 0

    for k, (L, m) in enumerate(zip(lists, meta)):
        if k in clears:
            clear(clears[k])
        L = np.asarray(L, dtype=np.uint32)
        S = L[(L >= first) & (L.astype(np.uint64) < first + cfg.count)] if ranged else L
        info["passes_seen"] += 1
        info["spikes_seen"] += int(L.size)
        info["selected_seen"] += int(S.size)
        if counts is not None:
            np.add.at(counts, (S - np.uint32(first)).astype(np.int64), np.uint32(1))
        room = cfg.raster_capacity == 0 or info["spikes_recorded"] + S.size <= cfg.raster_capacity
        if not dropped and info["passes_recorded"] < cfg.pass_capacity and room:
            entries.append((int(m[0]), int(m[1]), info["spikes_recorded"], int(S.size), int(m[2]) & 0xFFFFFFFF))
            if cfg.raster_capacity:
                raster.append(S)
            info["passes_recorded"] += 1
            info["spikes_recorded"] += int(S.size)
        else:
            dropped = True
            info["passes_dropped"] += 1
            info["spikes_dropped"] += int(S.size)
    if len(lists) in clears:
        clear(clears[len(lists)])
    return {"info": info, "passes": np.array(entries, dtype=SPIKE_PASS_DTYPE),
            "raster": np.concatenate(raster).astype(np.uint32) if raster else np.zeros(0, dtype=np.uint32),
            "counts": counts}


def split(passes: np.ndarray, raster: np.ndarray) -> list:
    """The raster cut into one u32 array per recorded pass (views)."""
    return [raster[int(p["offset"]):int(p["offset"]) + int(p["count"])] for p in passes]
