"""Python mirror of the reference host class ``Brain`` over the C-ABI.

Reference: abnn/src/core/brain/brain.h:24-83 and brain.cpp:21-178.  Method
names follow the reference (``encode_traversal``, ``inject_inputs``,
``read_outputs``, ``save``/``load``, ``n_input()`` ...); Metal types are
replaced by the HIP engine behind ``libabnn_hip.so``.  All compute runs in the
HIP library -- this module only moves small host arrays and pointers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib
from . import census as _census
from . import components as _components
from . import corr as _corr
from . import degree as _degree
from . import edit as _edit
from . import hops as _hops
from . import matrix as _matrix
from . import propagate as _propagate
from . import reorder as _reorder
from . import select as _select
from . import spikes as _spikes
from ._lib import Dims, Params, Scalars, State, Stats, call

# SynapsePacked {u32 src, u32 dst, f32 w, f32 pad} (brain.metal:11, brain.h:21)
SYN_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")])


def visited_events(events_per_pass: int, n_syn: int, mode: int = 0) -> int:
    """Sweep: min(roundup(EVENTS,256), nSyn) -- brain.cpp:116-118 with
    brain.metal:60-61.  Random mode: exactly EVENTS picks (README §4)."""
    if mode == _lib.MODE_RANDOM:
        return int(events_per_pass) if int(n_syn) else 0
    grid = (int(events_per_pass) + 255) // 256 * 256
    return min(grid, int(n_syn))


def _stream_ptr(stream) -> Optional[int]:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return int(getattr(stream, "cuda_stream"))  # torch.cuda.Stream


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


class Brain:
    """One traversal engine on one GPU (optionally one synapse shard)."""

    def __init__(self, n_input: int, n_output: int, n_hidden: int, n_syn: int,
                 events_per_pass: int, *, params: Optional[Params] = None, device: int = 0,
                 syn_offset: int = 0, global_events: int = 0, syn_capacity: int = 0,
                 **param_overrides):
        self._lib = _lib.load()
        if params is None:
            params = _lib.default_params(**param_overrides)
        elif param_overrides:
            raise TypeError("pass either params= or keyword overrides, not both")
        self._dims = Dims(n_input, n_output, n_hidden, n_syn, events_per_pass, syn_offset,
                          global_events, syn_capacity)
        self._params = params
        h = C.c_void_p()
        call("abnn_brain_create", C.byref(self._dims), C.byref(params), int(device), C.byref(h))
        self._h = h
        self.device = int(device)

    # ---- lifetime -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            call("abnn_brain_destroy", self._h)
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

    # ---- getters (brain.h:48-52) --------------------------------------------------------------
    def n_input(self) -> int:
        return int(self._dims.n_input)

    def n_output(self) -> int:
        return int(self._dims.n_output)

    def n_hidden(self) -> int:
        return int(self._dims.n_hidden)

    def n_neuron(self) -> int:
        return int(self._lib.abnn_n_neuron(self._h))

    def n_syn(self) -> int:
        """Current record count (structural updates change it)."""
        return int(self.dims.n_syn)

    @property
    def dims(self) -> Dims:
        d = Dims()
        call("abnn_get_dims", self._h, C.byref(d))
        return d

    @property
    def params(self) -> Params:
        return self._params

    def visited_events(self) -> int:
        return visited_events(self._dims.events_per_pass, self.n_syn(), self._params.mode)

    def state_ptrs(self) -> dict:
        """Borrowed device pointers (brain.h:54-58); ``synapses`` is opaque."""
        s = State()
        call("abnn_state_ptrs", self._h, C.byref(s))
        return {k: int(getattr(s, k) or 0) for k, _ in State._fields_}

    def synapse_layout(self) -> dict:
        """The device record layout behind state_ptrs()['synapses'] (versioned apart from the ABI)."""
        lay = _lib.Layout()
        call("abnn_synapse_layout", self._h, C.byref(lay))
        arrays = {lay.arrays[i].name.decode(): (int(lay.arrays[i].ptr or 0), int(lay.arrays[i].bytes),
                                                int(lay.arrays[i].elem_bytes)) for i in range(lay.n_arrays)}
        return {"version": int(lay.version), "arrays": arrays}

    def budget(self) -> int:
        """Spike budget left by the last pass (bufBudget_, brain.h:58)."""
        v = C.c_uint32()
        call("abnn_get_budget", self._h, C.byref(v))
        return int(v.value)

    def structural_updates(self) -> int:
        """Structural updates run so far (host count, no synchronisation)."""
        return int(self._lib.abnn_structural_updates(self._h))

    def renormalisations(self) -> int:
        """Renormalisations run so far (host count, no synchronisation)."""
        return int(self._lib.abnn_renormalisations(self._h))

    # ---- synapses ------------------------------------------------------------------------------
    def upload_synapses(self, syn: np.ndarray, first: int = 0) -> None:
        syn = np.ascontiguousarray(syn, dtype=SYN_DTYPE)
        call("abnn_upload_synapses", self._h, first, _ptr(syn), syn.shape[0])

    def download_synapses(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.n_syn() - first if n is None else n
        out = np.empty(n, dtype=SYN_DTYPE)
        call("abnn_download_synapses", self._h, first, _ptr(out), n)
        return out

    def build_random_graph(self, seed: int = 1) -> None:
        """build_random_graph recipe (brain-engine.cpp:31-53), generated on the GPU."""
        call("abnn_generate_synapses", self._h, seed)

    def build_graph(self, spec: _lib.GraphSpec) -> None:
        """Fill this handle's records from a graph spec on the GPU
        (abnn_build_graph; abnn_amd.graph builds specs): local
        record k becomes global record syn_offset + k of the spec.  The neuron
        state and the scalars are untouched."""
        call("abnn_build_graph", self._h, C.byref(spec))

    def checksum(self) -> int:
        v = C.c_uint64()
        call("abnn_checksum_synapses", self._h, C.byref(v))
        return int(v.value)

    def census(self, bins: int, lo: float, hi: float, src=None, dst=None) -> dict:
        """Synapse census on the device (abnn_census): counts of
        this handle's records, tombstones and selected records, and a
        ``bins``-bin histogram over [lo, hi) of the selected weights.  ``src``
        / ``dst`` are (first, count) neuron ranges, None = any.  Returns
        records, tombstones, live, selected, under, over, nan, min, max, counts
        (np.uint64) and edges (census.decode)."""
        cfg = _census.config(bins, lo, hi, src, dst)
        words = int(self._lib.abnn_census_words(C.byref(cfg)))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_census", self._h, C.byref(cfg), _ptr(out), words)  # an invalid config fails here
        return _census.decode(out, cfg)

    def census_enqueue(self, cfg: _lib.CensusConfig, out_ptr: int, stream=None) -> None:
        """Enqueue a census into device memory at ``out_ptr`` (abnn_census_words(cfg)
        u64) on ``stream``; nothing synchronises.  Decode with census.decode."""
        call("abnn_census_enqueue", self._h, C.byref(cfg), int(out_ptr), _stream_ptr(stream))

    def degrees(self, neurons=None, what=("out", "in", "out_w", "in_w")) -> dict:
        """Neuron degree census on the device (abnn_degree): per
        neuron of ``neurons`` = (first, count) (None: every neuron) the live
        records that leave it (``out``) and enter it (``in``), np.uint64, and
        their weights' sums in 2**-24 fixed point (``out_w`` / ``in_w``,
        np.int64), for the planes named in ``what``; the definition is in
        abnn.h.  Returns the header counts and the planes (degree.decode)."""
        cfg = _degree.config(neurons, what)
        n_nrn = self.n_neuron()
        words = int(self._lib.abnn_degree_words(C.byref(cfg), n_nrn))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_degree", self._h, C.byref(cfg), _ptr(out), words)  # an invalid config fails here
        return _degree.decode(out, cfg, n_nrn)

    def degrees_enqueue(self, cfg: _lib.DegreeConfig, out_ptr: int, stream=None) -> None:
        """Enqueue a degree census into device memory at ``out_ptr``
        (abnn_degree_words(cfg, N_NRN) u64) on ``stream``; nothing synchronises.
        Decode with degree.decode."""
        call("abnn_degree_enqueue", self._h, C.byref(cfg), int(out_ptr), _stream_ptr(stream))

    def select(self, src=None, dst=None, weights=None, any: bool = False, capacity: Optional[int] = None) -> dict:
        """Synapse select on the device (abnn_select): this
        handle's records that match, in record order.  ``src`` / ``dst`` are
        (first, count) neuron ranges (None = not set), ``weights`` = (w_lo,
        w_hi) keeps w_lo <= w < w_hi, ``any`` matches either set range instead
        of both; the rule is in abnn.h.  At most ``capacity`` matches are
        returned; None first counts (capacity 0) and then selects exactly the
        matches.  Returns records, tombstones, matched, written, syn_offset,
        capacity, ``index`` (np.uint64, global) and ``syn`` (SYN_DTYPE), both
        trimmed to written (select.decode)."""
        cfg = _select.config(src, dst, weights, any)
        if capacity is None:
            capacity = self._select(cfg, 0)["matched"]
        return self._select(cfg, int(capacity))

    def _select(self, cfg: _lib.SelectConfig, capacity: int) -> dict:
        words = int(self._lib.abnn_select_words(C.byref(cfg), capacity))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_select", self._h, C.byref(cfg), capacity, _ptr(out), words)  # an invalid config fails here
        return _select.decode(out, capacity)

    def select_enqueue(self, cfg: _lib.SelectConfig, capacity: int, out_ptr: int, stream=None) -> None:
        """Enqueue a select into device memory at ``out_ptr``
        (abnn_select_words(cfg, capacity) u64) on ``stream``; nothing
        synchronises after the handle's first select.  Plane entries at and
        past ``written`` are not written.  Decode with select.decode."""
        call("abnn_select_enqueue", self._h, C.byref(cfg), int(capacity), int(out_ptr), _stream_ptr(stream))

    def edit(self, op, *, src=None, dst=None, weights=None, any: bool = False, a: float = 0.0, b: float = 0.0,
             clamp=None, seed: int = 0, plane=None) -> dict:
        """Synapse edit on the device (abnn_edit): this handle's
        records that match (the select's ``src`` / ``dst`` / ``weights`` /
        ``any``) get a new weight by ``op`` (edit.OPS: set b; affine w * a + b;
        scale_dst / scale_src w * plane[key - first]; draw uniform in [a, b]
        from ``seed``; kill: the pruning tombstone), then ``clamp`` = (c_lo,
        c_hi); the rule is in abnn.h.  ``plane``: the float32 factors of a
        scale op, one per neuron of its range (every neuron when the range is
        not set).  Returns records, tombstones, matched, changed, killed and
        nonfinite (edit.decode)."""
        cfg = _edit.config(op, src, dst, weights, any, a, b, clamp, seed)
        out = np.zeros(_lib.EDIT_HEADER_WORDS, dtype=np.uint64)
        if plane is not None:
            plane = np.ascontiguousarray(plane, dtype=np.float32)
        call("abnn_edit", self._h, C.byref(cfg), None if plane is None else _ptr(plane),
             0 if plane is None else plane.shape[0], _ptr(out))  # an invalid config fails here
        return _edit.decode(out)

    def edit_enqueue(self, cfg: _lib.EditConfig, plane_ptr: Optional[int], out_ptr: int, stream=None) -> None:
        """Enqueue an edit on ``stream``: the header into device memory at
        ``out_ptr`` (8 u64), a scale op's factors from device memory at
        ``plane_ptr`` (None otherwise); nothing synchronises.  Decode with
        edit.decode."""
        call("abnn_edit_enqueue", self._h, C.byref(cfg), int(plane_ptr) if plane_ptr else None, int(out_ptr),
             _stream_ptr(stream))

    def reorder(self, key=None, descending: bool = False, seed: int = 0, origin: bool = False, perm=None) -> dict:
        """Record reorder on the device (abnn_reorder): this
        handle's records put into the stable order of ``key`` ('src', 'dst',
        'w'; ``descending`` inverts it), shuffled ('random', by ``seed``),
        compacted ('none': only the tombstones move) or permuted by ``perm``
        (np.uint32, record k becomes the old record perm[k]; an invalid perm
        moves nothing).  Tombstones end up last except under ``perm``; the rule
        is in abnn.h.  Returns records, tombstones, moved, invalid, syn_offset
        and, with ``origin``, the permutation (reorder.decode)."""
        if perm is not None:
            if key not in (None, "perm", _lib.REORDER_PERM):
                raise ValueError("reorder: perm goes with no other key")
            key = "perm"
            perm = np.ascontiguousarray(perm, dtype=np.uint32)
            if perm.shape != (self.n_syn(),):
                raise ValueError("reorder: perm must hold n_syn entries")
        elif key is None:
            raise ValueError("reorder: a key or a perm")
        cfg = _reorder.config(key, descending, seed, origin)
        words = int(self._lib.abnn_reorder_words(C.byref(cfg), self.n_syn()))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_reorder", self._h, C.byref(cfg), None if perm is None else _ptr(perm), _ptr(out), words)  # an invalid config fails here
        return _reorder.decode(out[:words], cfg)

    def reorder_enqueue(self, cfg: _lib.ReorderConfig, perm_ptr: Optional[int], out_ptr: int, stream=None) -> None:
        """Enqueue a reorder on ``stream``: the result into device memory at
        ``out_ptr`` (abnn_reorder_words(cfg, n_syn) u64), a perm's n_syn u32
        from device memory at ``perm_ptr`` (None otherwise); nothing
        synchronises after the handle's first reorder.  Decode with
        reorder.decode."""
        call("abnn_reorder_enqueue", self._h, C.byref(cfg), int(perm_ptr) if perm_ptr else None, int(out_ptr),
             _stream_ptr(stream))

    def reorder_release(self) -> None:
        """Free the reorder's device scratch (28 bytes per record of capacity)."""
        call("abnn_reorder_release", self._h)

    def edit_factors_enqueue(self, strength_ptr: int, count: int, target: float, f_lo: float, f_hi: float,
                             plane_ptr: int, stream=None) -> None:
        """Enqueue the factors of synaptic scaling on ``stream``: ``count``
        int64 fixed-point strength words in device memory at ``strength_ptr``
        (a degree census's in_w / out_w plane) into float32 factors at
        ``plane_ptr``: target / strength, clamped to [f_lo, f_hi], 1 where the
        strength is not positive (edit.factors restates it)."""
        call("abnn_edit_factors_enqueue", self._h, int(strength_ptr), int(count), float(target), float(f_lo),
             float(f_hi), int(plane_ptr), _stream_ptr(stream))

    def scale_inputs(self, target: float, neurons=None, limits=(0.5, 2.0)) -> dict:
        """Homeostatic synaptic scaling on the device: every incoming weight
        of each neuron of ``neurons`` = (first, count) (None: every neuron) is
        multiplied by the neuron's factor target / (its summed input), clamped
        to ``limits`` -- the degree census's in_w plane, the factors and the
        scale_dst edit enqueued on one stream, one synchronise at the end.
        Returns the edit's header and ``factors`` (np.float32, one per neuron)."""
        import torch

        dev = torch.device("cuda", self.device)
        n_nrn = self.n_neuron()
        dcfg = _degree.config(neurons, ("in_w",))
        words = _degree.n_words(dcfg, n_nrn)
        if not words:
            raise ValueError("scale_inputs: invalid neuron range")
        m = words - _lib.DEGREE_HEADER_WORDS
        ecfg = _edit.config("scale_dst", dst=None if neurons is None else (int(neurons[0]), int(neurons[1])))
        with torch.cuda.device(dev):
            deg = torch.zeros(words, dtype=torch.int64, device=dev)
            plane = torch.zeros(m, dtype=torch.float32, device=dev)
            head = torch.zeros(_lib.EDIT_HEADER_WORDS, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev)
            self.degrees_enqueue(dcfg, deg.data_ptr(), stream)
            self.edit_factors_enqueue(deg.data_ptr() + 8 * _lib.DEGREE_HEADER_WORDS, m, target, limits[0], limits[1],
                                      plane.data_ptr(), stream)
            self.edit_enqueue(ecfg, plane.data_ptr(), head.data_ptr(), stream)
            stream.synchronize()
        out = _edit.decode(head.cpu().numpy().view(np.uint64))
        out["factors"] = plane.cpu().numpy()
        return out

    def snapshot(self, stream=None):
        """A device-side snapshot of this brain as it is now
        (abnn_snapshot_*): create, capture on ``stream`` and
        synchronise.  Returns a :class:`abnn_amd.snapshot.Snapshot`: restore()
        rolls the brain back to it, diff() says what changed since, capture()
        takes it again.  Close it before the brain."""
        from .snapshot import Snapshot

        snap = Snapshot(self)
        snap.capture(stream)
        self.synchronize(stream)
        return snap

    def hops(self, seeds, max_hops: int = 64, reverse: bool = False, weights=None) -> dict:
        """Reachability on the device (abnn_hops): the hop
        distance of every neuron from the seed range ``seeds`` = (first,
        count) over this handle's records, at most ``max_hops`` hops;
        ``reverse`` follows dst -> src (who can reach the seeds), ``weights`` =
        (w_lo, w_hi) follows only records with w_lo <= w < w_hi; the rule is
        in abnn.h.  Returns records, neurons, reached, depth, complete,
        ``levels`` (np.uint64) and ``dist`` (np.uint32, hops.UNREACHED = not
        reached) (hops.decode)."""
        cfg = _hops.config(seeds, max_hops, reverse, weights)
        n_nrn = self.n_neuron()
        words = int(self._lib.abnn_hops_words(C.byref(cfg), n_nrn))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_hops", self._h, C.byref(cfg), _ptr(out), words)  # an invalid config fails here
        return _hops.decode(out, cfg, n_nrn)

    def hops_enqueue(self, cfg: _lib.HopsConfig, out_ptr: int, stream=None) -> None:
        """Enqueue a whole search into device memory at ``out_ptr``
        (abnn_hops_words(cfg, N_NRN) u64) on ``stream``; nothing synchronises
        after the handle's first search.  Decode with hops.decode."""
        call("abnn_hops_enqueue", self._h, C.byref(cfg), int(out_ptr), _stream_ptr(stream))

    def hops_step_enqueue(self, cfg: _lib.HopsConfig, step: int, out_ptr: int, stream=None) -> None:
        """Enqueue one step (hops.BEGIN, or 0 .. max_hops) of a search in the
        device memory at ``out_ptr``: the sharded caller's path, which merges
        the ranks' planes (hops.merge_planes) between two steps."""
        call("abnn_hops_step_enqueue", self._h, C.byref(cfg), int(step), int(out_ptr), _stream_ptr(stream))

    def components(self, neurons=None, weights=None, sizes: bool = False) -> dict:
        """Connected components on the device (abnn_components):
        the weakly connected components of this handle's records over the
        neuron range ``neurons`` = (first, count) (None: every neuron);
        ``weights`` = (w_lo, w_hi) follows only records with w_lo <= w < w_hi,
        ``sizes`` also returns the per-neuron component size; the rule is in
        abnn.h.  Returns records, neurons, followed, components, largest,
        largest_label, singletons, gave_up, ``bins`` (np.uint64), ``labels``
        (np.uint32: the smallest neuron id of the component, components.NONE
        outside the range) and with ``sizes`` the plane ``sizes``
        (components.decode)."""
        n_nrn = self.n_neuron()
        cfg = _components.config(neurons, weights, sizes, n_nrn)
        words = int(self._lib.abnn_components_words(C.byref(cfg), n_nrn))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_components", self._h, C.byref(cfg), _ptr(out), words)  # an invalid config fails here
        return _components.decode(out, cfg, n_nrn)

    def components_enqueue(self, cfg: _lib.ComponentsConfig, out_ptr: int, stream=None) -> None:
        """Enqueue a whole labelling (BEGIN, LINK, FLATTEN, CLOSE) into device
        memory at ``out_ptr`` (abnn_components_words(cfg, N_NRN) u64) on
        ``stream``; nothing synchronises after the handle's first call.
        Decode with components.decode."""
        call("abnn_components_enqueue", self._h, C.byref(cfg), int(out_ptr), _stream_ptr(stream))

    def components_step_enqueue(self, cfg: _lib.ComponentsConfig, step: int, out_ptr: int, stream=None) -> None:
        """Enqueue one step (components.BEGIN / LINK / FLATTEN / CLOSE) of a
        labelling in the device memory at ``out_ptr``: the sharded caller's path."""
        call("abnn_components_step_enqueue", self._h, C.byref(cfg), int(step), int(out_ptr), _stream_ptr(stream))

    def components_merge_enqueue(self, cfg: _lib.ComponentsConfig, planes_ptr: int, n_planes: int, out_ptr: int,
                                 stream=None) -> None:
        """Enqueue the shard merge: ``planes_ptr`` is device memory holding
        ``n_planes`` label planes one after the other (each 2 * ((N_NRN + 1) //
        2) u32, as a result holds it); every neuron of the range is united
        with its label in each of them, in the plane at ``out_ptr``."""
        call("abnn_components_merge_enqueue", self._h, C.byref(cfg), int(planes_ptr), int(n_planes), int(out_ptr),
             _stream_ptr(stream))

    def _matrix_partition(self, bounds, labels, pops):
        """(P, bounds array or None, labels device pointer or None, keep-alive)
        of a matrix call.  Neither given: the built-in populations."""
        if labels is None:
            if bounds is None:
                bounds = _matrix.io_bounds(self.n_input(), self.n_output(), self.n_hidden())
            b = np.ascontiguousarray(bounds, dtype=np.uint32)
            if b.ndim != 1 or len(b) < 2 or (pops is not None and int(pops) != len(b) - 1):
                raise ValueError("matrix: bounds holds P + 1 values")
            return len(b) - 1, b, None, b
        if bounds is not None or pops is None:
            raise ValueError("matrix: labels needs pops and no bounds")
        if isinstance(labels, (int, np.integer)):
            return int(pops), None, int(labels), None
        if isinstance(labels, np.ndarray):  # uploaded
            import torch

            if labels.shape != (self.n_neuron(),):
                raise ValueError("matrix: labels must hold N_NRN entries")
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint32).view(np.int32)).to(f"cuda:{self.device}")
        if labels.element_size() != 4 or labels.numel() < self.n_neuron() or not labels.is_contiguous():
            raise ValueError("matrix: a labels tensor holds N_NRN contiguous 32-bit entries")
        return int(pops), None, int(labels.data_ptr()), labels

    def matrix(self, bounds=None, labels=None, pops: Optional[int] = None, what=("count", "w"), weights=None) -> dict:
        """Population connectivity matrix on the device (abnn_matrix,
        DESIGN.md §9): for every pair (a, b) of populations the records from a
        to b (``count``), their summed weights (``w``) and fire probabilities
        (``p``) in 2**-24 fixed point, in one pass over this handle's records.
        The partition is ``bounds`` (P + 1 ascending ids; None and no labels:
        inputs / outputs / hidden, matrix.io_bounds) or ``labels`` with
        ``pops`` = P: a plane of N_NRN u32 (a torch tensor on this device, a
        device pointer, or a numpy array that is uploaded), values >= P = no
        population.  ``weights`` = (w_lo, w_hi) counts only w_lo <= w < w_hi;
        the rule is in abnn.h.  Returns the header, ``sizes``, the planes and
        ``density`` (matrix.decode)."""
        n_pops, b, lab_ptr, keep = self._matrix_partition(bounds, labels, pops)
        cfg = _matrix.config(n_pops, what, lab_ptr is not None, weights)
        words = int(self._lib.abnn_matrix_words(C.byref(cfg)))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_matrix", self._h, C.byref(cfg), None if b is None else _ptr(b), lab_ptr, _ptr(out), words)
        del keep
        return _matrix.decode(out, cfg)  # an invalid config failed above

    def matrix_enqueue(self, cfg: _lib.MatrixConfig, out_ptr: int, bounds=None, labels_ptr: Optional[int] = None,
                       stream=None) -> None:
        """Enqueue a connectivity matrix into device memory at ``out_ptr``
        (abnn_matrix_words(cfg) u64) on ``stream``; nothing synchronises after
        the handle's first LABELS call.  ``bounds`` (host values, read during
        the call) or ``labels_ptr`` (device memory, N_NRN u32: e.g. the distance
        plane inside a hops result), whichever cfg's LABELS flag names.  Decode
        with matrix.decode."""
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint32)
        if b is not None and b.shape != (int(cfg.pops) + 1,):
            raise ValueError("matrix: bounds holds P + 1 values")
        call("abnn_matrix_enqueue", self._h, C.byref(cfg), None if b is None else _ptr(b),
             None if labels_ptr is None else int(labels_ptr), int(out_ptr), _stream_ptr(stream))

    def propagate(self, x, inputs=None, outputs=None, reverse: bool = False, fire_p: bool = False, weights=None) -> dict:
        """Signal propagation on the device (abnn_propagate):
        y[kout] += c(w) * x[kin] over this handle's records, in integers.
        ``x`` holds N_NRN int32 (propagate.to_fixed); ``inputs`` / ``outputs``
        are the (first, count) ranges x is read from and y is summed over
        (None: every neuron); ``reverse`` is the transpose, ``fire_p`` takes
        the fire probability (w*w)*base_scale for c, ``weights`` = (w_lo,
        w_hi) follows only records with w_lo <= w < w_hi; the rule is in
        abnn.h.  Returns records, tombstones, followed, skipped, nnz,
        sum_abs_x and ``y`` (np.int64, 8 fractional bits more than x)
        (propagate.decode)."""
        cfg = _propagate.config(inputs, outputs, reverse, fire_p, weights)
        n_nrn = self.n_neuron()
        x = np.ascontiguousarray(x, dtype=np.int32)
        if x.shape != (n_nrn,):
            raise ValueError("propagate: x must hold N_NRN entries")
        words = int(self._lib.abnn_propagate_words(C.byref(cfg), n_nrn))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_propagate", self._h, C.byref(cfg), _ptr(x), _ptr(out), words)  # an invalid config fails here
        return _propagate.decode(out, cfg, n_nrn)

    def propagate_enqueue(self, cfg: _lib.PropagateConfig, x_ptr: int, out_ptr: int, stream=None) -> None:
        """Enqueue a propagation of the device plane at ``x_ptr`` (N_NRN
        int32, 16-byte aligned) into device memory at ``out_ptr``
        (abnn_propagate_words(cfg, N_NRN) u64) on ``stream``; nothing
        synchronises after the handle's first propagation.  Decode with
        propagate.decode."""
        call("abnn_propagate_enqueue", self._h, C.byref(cfg), int(x_ptr), int(out_ptr), _stream_ptr(stream))

    def propagate_rescale_enqueue(self, cfg: _lib.PropagateConfig, out_ptr: int, x_ptr: int, row_ptr: Optional[int] = None,
                                  stream=None) -> None:
        """Enqueue the rescale of the result at ``out_ptr`` into the plane at
        ``x_ptr`` over the out-range, with its trace row (8 u64) at ``row_ptr``
        (None: no row)."""
        call("abnn_propagate_rescale_enqueue", self._h, C.byref(cfg), int(out_ptr), int(x_ptr),
             int(row_ptr) if row_ptr else None, _stream_ptr(stream))

    def propagate_iterate_enqueue(self, cfg: _lib.PropagateConfig, steps: int, x_ptr: int, work_ptr: int, trace_ptr: int,
                                  stream=None) -> None:
        """Enqueue ``steps`` times propagate and rescale (abnn_propagate_iterate_enqueue):
        the plane at ``x_ptr`` ends as the last rescaled one, ``trace_ptr``
        holds steps x 8 u64 (propagate.branching reads them)."""
        call("abnn_propagate_iterate_enqueue", self._h, C.byref(cfg), int(steps), int(x_ptr), int(work_ptr),
             int(trace_ptr), _stream_ptr(stream))

    def branching(self, steps: int = 16, neurons=None, fire_p: bool = True, reverse: bool = False, weights=None,
                  x0=None) -> dict:
        """The branching ratio on the device: ``steps`` power iterations of
        the fire-probability matrix (``fire_p``; else of the weights)
        restricted to ``neurons`` = (first, count) (None: every neuron), from
        ``x0`` (N_NRN int32; None: propagate.ONE >> 1 on every neuron of the
        range), all enqueued on one stream with one synchronise at the end.
        Returns propagate.branching of the trace (``ratio``, ``estimates``,
        ...) and ``x``, the last rescaled plane (np.int32, N_NRN): the
        influence vector (with ``reverse``, of the transpose)."""
        import torch

        dev = torch.device("cuda", self.device)
        n_nrn = self.n_neuron()
        cfg = _propagate.config(neurons, neurons, reverse, fire_p, weights)
        words = _propagate.n_words(cfg, n_nrn)
        if not words:
            raise ValueError("branching: invalid neuron range or weight bounds")
        if x0 is None:
            first, count = _propagate.ranges(cfg, n_nrn)[:2]
            x0 = np.zeros(n_nrn, dtype=np.int32)
            x0[first:first + count] = _propagate.ONE >> 1
        x0 = np.ascontiguousarray(x0, dtype=np.int32)
        if x0.shape != (n_nrn,):
            raise ValueError("branching: x0 must hold N_NRN entries")
        with torch.cuda.device(dev):
            x = torch.from_numpy(x0).to(dev)
            work = torch.zeros(words, dtype=torch.int64, device=dev)
            trace = torch.zeros(int(steps) * _lib.PROP_TRACE_WORDS, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev)
            self.propagate_iterate_enqueue(cfg, steps, x.data_ptr(), work.data_ptr(), trace.data_ptr(), stream)
            stream.synchronize()
        out = _propagate.branching(trace.cpu().numpy().view(np.uint64))
        out["x"] = x.cpu().numpy()
        return out

    # ---- spike recorder (abnn_spikes_*) -------------------------------------------
    def record_spikes(self, raster: int, passes: int, neurons=None, counts: bool = False) -> None:
        """Start (or restart) the spike recorder: from now on every pass this
        handle completes appends its spike list -- the dst of every spike, in
        budget order -- to device buffers of ``raster`` spikes (0: no raster)
        and ``passes`` pass entries, with no synchronise.  ``neurons`` =
        (first, count) keeps only those dst; ``counts`` keeps per-neuron counts."""
        cfg = _spikes.config(raster, passes, neurons, counts)
        self._spk = None  # a failed start leaves no recorder
        call("abnn_spikes_start", self._h, C.byref(cfg))
        self._spk = cfg

    def spikes(self) -> dict:
        """What the recorder holds (synchronises): ``info`` (abnn_spikes_info
        as a dict), ``passes`` (spikes.SPIKE_PASS_DTYPE, one per recorded
        pass) and ``raster`` (u32 dst; spikes.split cuts it into passes)."""
        info = _lib.SpikesInfo()
        call("abnn_spikes_get_info", self._h, C.byref(info))
        passes = np.zeros(int(info.passes_recorded), dtype=_spikes.SPIKE_PASS_DTYPE)
        call("abnn_spikes_read_passes", self._h, 0, passes.shape[0], _ptr(passes))
        cfg = getattr(self, "_spk", None)
        raster = np.zeros(int(info.spikes_recorded) if cfg is not None and cfg.raster_capacity else 0, dtype=np.uint32)
        call("abnn_spikes_read_raster", self._h, 0, raster.shape[0], _ptr(raster))
        return {"info": info.as_dict(), "passes": passes, "raster": raster}

    def spike_counts(self, first: Optional[int] = None, n: Optional[int] = None) -> np.ndarray:
        """Per-neuron spike counts (u32) of the absolute neuron ids [first,
        first + n); by default the whole selected range."""
        cfg = getattr(self, "_spk", None)
        lo, cnt = (cfg.first, cfg.count) if cfg is not None and cfg.count else (0, self.n_neuron())
        first = lo if first is None else int(first)
        n = lo + cnt - first if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=np.uint32)
        call("abnn_spikes_read_counts", self._h, first, n, _ptr(out))
        return out

    def clear_spikes(self, keep_counts: bool = False) -> None:
        """Empty the pass table and the raster and re-arm recording."""
        call("abnn_spikes_clear", self._h, 1 if keep_counts else 0)

    def stop_spikes(self) -> None:
        """Free the recorder (synchronises)."""
        self._spk = None
        call("abnn_spikes_stop", self._h)

    def load_spikes(self, passes: np.ndarray, raster: np.ndarray) -> None:
        """Replace what the recorder holds with a host pass table
        (spikes.SPIKE_PASS_DTYPE) and its raster (abnn_spikes_load;
        synchronises): as after a clear followed by len(passes) recorded
        passes.  Offsets, capacities and ids are checked first."""
        passes = np.ascontiguousarray(passes, dtype=_spikes.SPIKE_PASS_DTYPE)
        raster = np.ascontiguousarray(raster, dtype=np.uint32)
        call("abnn_spikes_load", self._h, _ptr(passes) if len(passes) else None, len(passes),
             _ptr(raster) if len(raster) else None, len(raster))

    # ---- spike correlograms (abnn_corr_*) -----------------------------------------
    def correlate(self, mode, a=None, b=None, max_lag: int = 16, rows=None, weights=None) -> dict:
        """A correlogram of the recorded spikes on the device (abnn_corr,
        DESIGN.md §9): ``mode`` "pop", "pairs" or "synapses"; ``a`` / ``b`` =
        (first, count) of the pre / post population (None: every neuron),
        lags -max_lag .. max_lag in table rows, ``rows`` = (first, count) of
        the rows used (None: all), ``weights`` = (w_lo, w_hi) follows only
        such records; the rule is in abnn.h.  Returns the header fields,
        ``lags`` and ``plane`` (corr.decode)."""
        cfg = _corr.config(mode, a, b, max_lag, rows, weights)
        words = int(self._lib.abnn_corr_words(C.byref(cfg)))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_corr", self._h, C.byref(cfg), _ptr(out), words)  # an invalid config fails here
        return _corr.decode(out, cfg)

    def correlate_enqueue(self, cfg: _lib.CorrConfig, out_ptr: int, stream=None) -> None:
        """Enqueue a correlogram into device memory at ``out_ptr``
        (abnn_corr_words(cfg) u64) on ``stream``; nothing synchronises after
        the handle's first one.  Decode with corr.decode."""
        call("abnn_corr_enqueue", self._h, C.byref(cfg), int(out_ptr), _stream_ptr(stream))

    # ---- neuron state ---------------------------------------------------------------------------
    def last_fired(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.n_neuron() - first if n is None else n
        out = np.empty(n, dtype=np.uint64)
        call("abnn_get_last_fired", self._h, first, _ptr(out), n)
        return out

    def set_last_fired(self, values: np.ndarray, first: int = 0) -> None:
        v = np.ascontiguousarray(values, dtype=np.uint64)
        call("abnn_set_last_fired", self._h, first, _ptr(v), v.shape[0])

    def last_visited(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.n_neuron() - first if n is None else n
        out = np.empty(n, dtype=np.uint64)
        call("abnn_get_last_visited", self._h, first, _ptr(out), n)
        return out

    def set_last_visited(self, values: np.ndarray, first: int = 0) -> None:
        v = np.ascontiguousarray(values, dtype=np.uint64)
        call("abnn_set_last_visited", self._h, first, _ptr(v), v.shape[0])

    def set_timestamps(self, idx: Sequence[int], value: int) -> None:
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        call("abnn_set_timestamps", self._h, _ptr(i), i.shape[0], int(value))

    def scalars(self) -> dict:
        s = Scalars()
        call("abnn_get_scalars", self._h, C.byref(s))
        return {"clock": int(s.clock), "reward": float(s.reward), "rbar": float(s.rbar),
                "pass_index": int(s.pass_index)}

    def set_scalars(self, clock: int, reward: float, rbar: float, pass_index: Optional[int] = None) -> None:
        if pass_index is None:
            pass_index = self.scalars()["pass_index"]
        s = Scalars(clock, reward, rbar, pass_index)
        call("abnn_set_scalars", self._h, C.byref(s))

    def set_reward(self, r: float) -> None:
        call("abnn_set_reward", self._h, float(r))

    # ---- pass-boundary hooks ------------------------------------------------------------------
    def inject_inputs(self, vals: Sequence[float], hz: float) -> None:
        """Brain::inject_inputs (brain.cpp:73-83)."""
        v = np.ascontiguousarray(vals, dtype=np.float32)
        call("abnn_inject_inputs", self._h, _ptr(v), v.shape[0], float(hz))

    def read_outputs(self) -> np.ndarray:
        """Brain::read_outputs (brain.cpp:145-157) -> bool[n_output]."""
        out = np.zeros(self.n_output(), dtype=np.uint8)
        call("abnn_read_outputs", self._h, _ptr(out), out.shape[0])
        return out.astype(bool)

    def set_auto_stimulus(self, first: int, count: int) -> None:
        call("abnn_set_auto_stimulus", self._h, int(first), int(count))

    # ---- passes --------------------------------------------------------------------------------
    def encode_traversal(self, passes: int = 1, stream=None) -> None:
        """Brain::encode_traversal + commit (brain.cpp:87-141): enqueue whole C1 passes."""
        call("abnn_traverse", self._h, int(passes), _stream_ptr(stream))

    traverse = encode_traversal

    def synchronize(self, stream=None) -> None:
        call("abnn_synchronize", self._h, _stream_ptr(stream))

    def exchange_bytes(self) -> int:
        """Bytes of this shard's exchange record (summary + local spike list, abnn.h)."""
        return int(self._lib.abnn_exchange_bytes(self._h))

    def set_global_events(self, n: int) -> None:
        """Visited events of all shards per pass (after structural updates)."""
        call("abnn_set_global_events", self._h, int(n))

    def shard_gate(self, xchg_ptr: int, stream=None) -> None:
        call("abnn_shard_gate", self._h, xchg_ptr, _stream_ptr(stream))

    def shard_apply(self, gathered_ptr: int, world: int, rank: int, stream=None) -> None:
        call("abnn_shard_apply", self._h, gathered_ptr, world, rank, _stream_ptr(stream))

    def shard_commit(self, gathered_ptr: int, world: int, stream=None) -> None:
        call("abnn_shard_commit", self._h, gathered_ptr, world, _stream_ptr(stream))

    def shard_visits_delta(self, delta_ptr: int, stream=None) -> None:
        """This shard's lastVisited merge deltas (u64 x N_NRN, device; abnn.h)."""
        call("abnn_shard_visits_delta", self._h, delta_ptr, _stream_ptr(stream))

    def shard_visits_merge(self, reduced_ptr: int, stream=None) -> None:
        """Apply the all-reduced (MAX) deltas; clears this shard's visit marks."""
        call("abnn_shard_visits_merge", self._h, reduced_ptr, _stream_ptr(stream))

    # ---- statistics / timing ------------------------------------------------------------------
    def stats(self) -> dict:
        s = Stats()
        call("abnn_get_stats", self._h, C.byref(s))
        return s.as_dict()

    def reset_stats(self) -> None:
        call("abnn_reset_stats", self._h)

    def enable_timing(self, on: bool | int = True) -> None:
        """True/1: time every gate launch; n > 1: every n-th; False/0: off."""
        call("abnn_enable_timing", self._h, int(on))

    def kernel_time(self) -> tuple[float, int]:
        ms = C.c_double()
        n = C.c_uint64()
        call("abnn_get_kernel_time", self._h, C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def kernel_times(self, cap: int = 1 << 16) -> np.ndarray:
        """The timed gate launches since the last call, one by one (ms)."""
        out = np.zeros(cap, dtype=np.float32)
        n = C.c_uint64()
        call("abnn_get_kernel_times", self._h, _ptr(out), cap, C.byref(n))
        return out[:min(int(n.value), cap)].astype(np.float64)

    # ---- persistence (brain.cpp:161-178, README §2) --------------------------------------------
    def save(self, path: str | os.PathLike) -> None:
        call("abnn_save_bnn", self._h, os.fsencode(path))

    def load(self, path: str | os.PathLike) -> None:
        call("abnn_load_bnn", self._h, os.fsencode(path))

    def save_flat(self, path: str | os.PathLike) -> None:
        call("abnn_save_flat", self._h, os.fsencode(path))

    def load_flat(self, path: str | os.PathLike) -> None:
        call("abnn_load_flat", self._h, os.fsencode(path))
