"""Python mirror of the device-resident learning loop (abnn.h ``abnn_engine_*``).

``LearnEngine`` is the reference's per-pass driver (``BrainEngine::run_one_pass``,
brain-engine.cpp:108-190; include/abnn/engine.hpp) with its state on the GPU:
``run`` enqueues whole learning passes -- input injection, teacher forcing, the
traversal, the output read, the rate filter and the windowed loss -> reward --
and returns at once; ``state``, ``rates`` and ``trace`` wait for them.  All
compute runs in the HIP library; this module only hands it the stimulus frames.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import census as _census
from ._lib import EngineConfig, EngineState, call
from .brain import Brain, _stream_ptr


def default_engine_config(**overrides) -> EngineConfig:
    c = EngineConfig()
    _lib.load().abnn_default_engine_config(C.byref(c))
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise KeyError(k)
        setattr(c, k, v)
    return c


class LearnEngine:
    """One learning driver over one (unsharded) :class:`Brain`.  Close it before the brain."""

    def __init__(self, brain: Brain, *, config: Optional[EngineConfig] = None, **config_overrides):
        if config is None:
            config = default_engine_config(**config_overrides)
        elif config_overrides:
            raise TypeError("pass either config= or keyword overrides, not both")
        self._brain = brain  # keeps the handle alive
        self._config = config
        self._n_in, self._n_out = brain.n_input(), brain.n_output()
        h = C.c_void_p()
        call("abnn_engine_create", brain._h, C.byref(config), C.byref(h))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            call("abnn_engine_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def config(self) -> EngineConfig:
        return self._config

    def run(self, in_frames, expected_frames, stream=None) -> int:
        """Enqueue one learning pass per frame: ``in_frames`` is passes x n_input,
        ``expected_frames`` passes x n_output (float32; copied before the call
        returns).  Does not wait, not even for an earlier call's passes."""
        xin = np.ascontiguousarray(in_frames, dtype=np.float32).reshape(-1, self._n_in)
        xex = np.ascontiguousarray(expected_frames, dtype=np.float32).reshape(-1, self._n_out)
        if len(xin) != len(xex):
            raise ValueError("one input frame and one expected frame per pass")
        call("abnn_engine_run", self._h, xin.ctypes.data, xex.ctypes.data, len(xin), _stream_ptr(stream))
        return len(xin)

    def state(self) -> dict:
        s = EngineState()
        call("abnn_engine_get_state", self._h, C.byref(s))
        return s.as_dict()

    def rates(self) -> dict:
        """The output-spike EWMA, the last pass's normalised rates, the spike counts."""
        rate = np.empty(self._n_out, np.float32)
        smooth = np.empty(self._n_out, np.float32)
        window = np.empty(self._n_out, np.uint32)
        call("abnn_engine_get_rates", self._h, rate.ctypes.data, smooth.ctypes.data, window.ctypes.data,
             self._n_out)
        return {"rate": rate, "smooth": smooth, "spike_window": window}

    def set_census(self, bins: Optional[int] = None, lo: float = 0.0, hi: float = 1.0, src=None, dst=None, *,
                   every: int = 1, capacity: int = 1) -> None:
        """A synapse census (Brain.census's arguments) after every ``every``-th
        step inside the loop, kept in a device ring of ``capacity`` results;
        ``set_census(None)`` turns it off.  Restarts the ring."""
        if bins is None:
            call("abnn_engine_set_census", self._h, None, 0, 0)
            self._census_cfg = None
            return
        cfg = _census.config(bins, lo, hi, src, dst)
        call("abnn_engine_set_census", self._h, C.byref(cfg), int(every), int(capacity))
        self._census_cfg = cfg

    def census_count(self) -> int:
        """Censuses taken since set_census (host count, no synchronisation)."""
        return int(_lib.load().abnn_engine_census_count(self._h))

    def census_trace(self, first: int, n: int) -> tuple[np.ndarray, list]:
        """Snapshots [first, first + n) since set_census: the step counts they
        were taken at (np.uint64) and the results as dicts (Brain.census's)."""
        cfg = getattr(self, "_census_cfg", None)
        words = _census.n_words(cfg) if cfg is not None else 1
        out = np.zeros((n, words), np.uint64)
        steps = np.zeros(n, np.uint64)
        call("abnn_engine_read_census", self._h, int(first), int(n), out.ctypes.data, steps.ctypes.data)
        return steps, [_census.decode(row, cfg) for row in out]

    def trace(self, first_step: int, n: int) -> tuple[np.ndarray, np.ndarray]:
        """Output spikes (n x n_output uint8) and normalised rates (float32) of
        steps [first_step, first_step + n); the last ``trace_passes`` steps are held."""
        out = np.empty((n, self._n_out), np.uint8)
        smooth = np.empty((n, self._n_out), np.float32)
        call("abnn_engine_read_trace", self._h, int(first_step), int(n), out.ctypes.data, smooth.ctypes.data)
        return out, smooth
