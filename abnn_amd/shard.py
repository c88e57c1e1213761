"""Synapse-shard data parallelism: one process per GPU, exchange over RCCL.

The reference is single-GPU (no NCCL/MPI anywhere).  The build
shards the synapse array in contiguous ranges across ranks, replicates the
neuron state (lastFired, lastVisited, clock, reward, rBar) and keeps schedule
C1 bit-exact with ONE exchange per pass: after the gate phase
every rank all-gathers each rank's record (include/abnn/abnn.h) -- its
summary (4 x int64: spike candidates capped at the budget, global-event-0
flag, visited events, gated events) followed by its spikes in local budget
order (max_spikes x int32).  From the gathered records every rank knows its
offset in the ordered global spike budget (apply) and the global spike list
(rank order = budget order: commit stamps it).  All stamps of a pass write the
same value ``now``, so this equals the north-star all-reduce(MAX) over
lastFired exactly, at ~10 KB per rank instead of 40 MB per pass.

``lastVisited`` feeds no decision (brain.metal:44), so it is merged lazily
(:func:`merge_visits`): unsharded it holds the LAST value written, so each
shard contributes only the neurons it visited since the previous merge
(value + 1, else 0), the contributions are all-reduced with MAX, and a
non-zero result replaces the value everywhere.  MAX picks the last writer
because the clock only moves forward between merges: one is forced after
every renormalisation (:func:`sharded_pass`), and the C-ABI refuses to move
the clock back over unmerged visits.
"""
from __future__ import annotations

from typing import Optional, Protocol

import numpy as np

from .brain import Brain, visited_events


def shard_ranges(n_syn_global: int, world: int) -> list[tuple[int, int]]:
    """Contiguous, balanced [lo, hi) synapse ranges; rank order = global tid order."""
    base, extra = divmod(int(n_syn_global), int(world))
    out, lo = [], 0
    for r in range(world):
        hi = lo + base + (1 if r < extra else 0)
        out.append((lo, hi))
        lo = hi
    return out


def global_events(n_syn_global: int, events_per_pass: int, world: int, mode: int = 0) -> int:
    """Visited events per pass over all shards (each shard sweeps, or picks
    within, its own range)."""
    return sum(visited_events(events_per_pass, hi - lo, mode) for lo, hi in shard_ranges(n_syn_global, world))


class Engine(Protocol):
    """One shard's pass phases (the GPU Brain, or a CPU stand-in in tests)."""

    def gate(self, xchg) -> None: ...

    def apply(self, gathered, world: int, rank: int) -> None: ...

    def commit(self, gathered, world: int) -> None: ...

    def tracks_visits(self) -> bool: ...

    def renormalisations(self) -> int: ...

    def visits_delta(self):
        """int64 tensor of N_NRN merge deltas (abnn_shard_visits_delta)."""

    def visits_merge(self, reduced) -> None: ...


class TorchComm:
    """torch.distributed communicator.

    backend nccl (= RCCL on ROCm): the collectives run on device tensors, ordered
    with the pass kernels through the current stream.  backend gloo (CPU tests,
    or the single-GPU rehearsal of the multi-rank bench): device tensors are
    staged through host memory."""

    def __init__(self, group=None):
        import torch.distributed as dist

        self._dist = dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.staged = dist.get_backend(group) == "gloo"

    def _run(self, fn, *tensors):
        if not (self.staged and any(t.is_cuda for t in tensors)):
            fn(*tensors)
            return
        host = [t.cpu() for t in tensors]
        fn(*host)
        for t, h in zip(tensors, host):
            t.copy_(h)

    def all_gather(self, out, inp) -> None:
        self._run(lambda o, i: self._dist.all_gather_into_tensor(o, i, group=self.group), out, inp)

    def all_reduce_max(self, t) -> None:
        self._run(lambda x: self._dist.all_reduce(x, op=self._dist.ReduceOp.MAX, group=self.group), t)

    def all_reduce_sum(self, t) -> None:
        self._run(lambda x: self._dist.all_reduce(x, op=self._dist.ReduceOp.SUM, group=self.group), t)


def merge_visits(engine: Engine, comm) -> None:
    """The lastVisited merge (abnn.h abnn_shard_visits_delta / _merge): every
    rank's deltas, one all-reduce(MAX), the merge.  Collective: every rank
    calls it at the same point."""
    if not engine.tracks_visits():
        return
    delta = engine.visits_delta()
    comm.all_reduce_max(delta)
    engine.visits_merge(delta)


def sharded_pass(engine: Engine, comm, xchg, gathered) -> None:
    """One C1 pass over all shards: gate -> all-gather of the records -> apply
    -> commit; after a renormalisation (the clock went back) the lastVisited
    merge, before the next pass stamps values below this epoch's."""
    renorms = engine.renormalisations()
    engine.gate(xchg)
    comm.all_gather(gathered, xchg)
    engine.apply(gathered, comm.world, comm.rank)
    engine.commit(gathered, comm.world)
    if engine.renormalisations() != renorms:  # every rank renormalises after the same pass
        merge_visits(engine, comm)


class _GpuEngine:
    def __init__(self, brain: Brain, stream_fn):
        self.brain = brain
        self._stream = stream_fn

    def gate(self, xchg) -> None:
        self.brain.shard_gate(xchg.data_ptr(), self._stream())

    def apply(self, gathered, world, rank) -> None:
        self.brain.shard_apply(gathered.data_ptr(), world, rank, self._stream())

    def commit(self, gathered, world) -> None:
        self.brain.shard_commit(gathered.data_ptr(), world, self._stream())

    def tracks_visits(self) -> bool:
        return bool(self.brain.params.track_visits)

    def renormalisations(self) -> int:
        return self.brain.renormalisations()

    def visits_delta(self):
        import torch

        dev = torch.device("cuda", self.brain.device)
        t = torch.empty(self.brain.n_neuron(), dtype=torch.int64, device=dev)
        self.brain.shard_visits_delta(t.data_ptr(), self._stream())
        return t

    def visits_merge(self, reduced) -> None:
        self.brain.shard_visits_merge(reduced.data_ptr(), self._stream())


class NativeComm:
    """The library's own RCCL communicator (abnn_comm, include/abnn/abnn.h):
    rank 0's unique id is broadcast over ``torch.distributed`` once, then
    every pass's all-gather is enqueued by the C-ABI itself
    (abnn_shard_traverse) -- no Python, no torch collective per pass."""

    def __init__(self, device: int, group=None):
        import ctypes as C

        import torch
        import torch.distributed as dist

        from . import _lib

        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        uid = np.zeros(_lib.COMM_ID_BYTES, dtype=np.uint8)
        if self.rank == 0:
            _lib.call("abnn_comm_unique_id", uid.ctypes.data)
        on_gpu = dist.get_backend(group) == "nccl"
        t = torch.from_numpy(uid).to(torch.device("cuda", device) if on_gpu else "cpu")
        src = dist.get_global_rank(group, 0) if group is not None else 0  # the group's rank 0
        dist.broadcast(t, src, group=group)
        uid = np.ascontiguousarray(t.cpu().numpy())
        h = C.c_void_p()
        _lib.call("abnn_comm_create", uid.ctypes.data, self.world, self.rank, int(device), C.byref(h))
        self.handle = h

    def close(self) -> None:
        from . import _lib

        if getattr(self, "handle", None) is not None and self.handle.value:
            _lib.call("abnn_comm_destroy", self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalGroup:
    """In-process communicator group (abnn_comm_group, include/abnn/abnn.h):
    ``world`` ranks in ONE process, one host thread per rank, each driving its
    shard handle through the C-ABI (abnn_shard_traverse) with the communicator
    :meth:`comm` returns.  The collectives are device copies and a reduction
    kernel between host barriers -- no RCCL: the sharded pass at world > 1 on
    one GPU (SURVEY §4 item 4's fake communicator behind the same interface).
    Ranks on one device must use one stream (torch's default stream in every
    thread does)."""

    def __init__(self, world: int):
        import ctypes as C

        from . import _lib

        self.world = int(world)
        h = C.c_void_p()
        _lib.call("abnn_comm_group_create", self.world, C.byref(h))
        self.handle = h
        self._comms: list = []

    def comm(self, rank: int, device: int = 0) -> "LocalComm":
        c = LocalComm(self, rank, device)
        self._comms.append(c)
        return c

    def close(self) -> None:
        from . import _lib

        for c in self._comms:
            c.close()
        self._comms = []
        if getattr(self, "handle", None) is not None and self.handle.value:
            _lib.call("abnn_comm_group_destroy", self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalComm:
    """Rank ``rank`` of a :class:`LocalGroup`: the ``world`` / ``rank`` of the
    shard layout and the abnn_comm handle ShardedBrain drives (native)."""

    def __init__(self, group: LocalGroup, rank: int, device: int):
        import ctypes as C

        from . import _lib

        self.world, self.rank = group.world, int(rank)
        h = C.c_void_p()
        _lib.call("abnn_comm_create_local", group.handle, self.rank, int(device), C.byref(h))
        self.handle = h

    def close(self) -> None:
        from . import _lib

        if getattr(self, "handle", None) is not None and self.handle.value:
            _lib.call("abnn_comm_destroy", self.handle)
        self.handle = None


class ShardedBrain:
    """The rank-local shard of a graph of ``n_syn_global`` synapses on GPU ``device``.

    native=True (one GPU per rank, RCCL): passes are driven by the C-ABI over
    the library's RCCL communicator (NativeComm, abnn_shard_traverse); False:
    phase by phase from Python around ``comm.all_gather`` (any backend; the
    gloo rehearsal of ranks that share a GPU).  ``comm`` a :class:`LocalComm`:
    the C-driven passes over the in-process group (one thread per rank)."""

    def __init__(self, comm, n_input: int, n_output: int, n_hidden: int, n_syn_global: int,
                 events_per_pass: int, *, device: int = 0, capacity_factor: float = 1.0,
                 native: bool = False, **param_overrides):
        import torch

        self.comm = comm
        self.world, self.rank = comm.world, comm.rank
        lo, hi = shard_ranges(n_syn_global, self.world)[self.rank]
        self.lo, self.hi = lo, hi
        self.n_syn_global = n_syn_global
        self.global_events = global_events(n_syn_global, events_per_pass, self.world,
                                           int(param_overrides.get("mode", 0)))
        cap = int((hi - lo) * capacity_factor) if capacity_factor > 1.0 else 0  # synaptogenesis headroom
        self.brain = Brain(n_input, n_output, n_hidden, hi - lo, events_per_pass, device=device,
                           syn_offset=lo, global_events=self.global_events, syn_capacity=cap,
                           **param_overrides)
        dev = torch.device("cuda", device)
        self._torch = torch
        words = self.brain.exchange_bytes() // 4
        self.xchg = torch.zeros(words, dtype=torch.int32, device=dev)
        self.gathered = torch.zeros(words * self.world, dtype=torch.int32, device=dev)
        self.engine = _GpuEngine(self.brain, lambda: torch.cuda.current_stream(dev))
        self.compact_every = int(self.brain.params.compact_every)
        self._updates = self.brain.structural_updates()
        self.native = None
        if isinstance(comm, LocalComm):
            self.native = comm  # C-driven passes over the in-process group
        elif native:
            # the RCCL communicator spans the same process group as `comm`:
            # rank_offset and the gathered records' order follow its ranks
            self.native = NativeComm(device, group=getattr(comm, "group", None))
            if (self.native.world, self.native.rank) != (self.world, self.rank):
                raise ValueError(f"native communicator is rank {self.native.rank}/{self.native.world}, "
                                 f"the shard layout rank {self.rank}/{self.world}")

    def step(self, passes: int = 1) -> None:
        if self.native is not None:
            from ._lib import call

            call("abnn_shard_traverse", self.brain._h, self.native.handle, int(passes),
                 int(self._torch.cuda.current_stream(self.xchg.device).cuda_stream))
            return
        for _ in range(passes):
            sharded_pass(self.engine, self.comm, self.xchg, self.gathered)
            # every rank runs its structural update after the same pass (the
            # pass index is replicated): re-sum the visited events after one
            if self.compact_every and self.brain.structural_updates() != self._updates:
                self._updates = self.brain.structural_updates()
                self.refresh_global_events()

    def refresh_global_events(self) -> None:
        """A structural update changed every shard's record count, and with it
        the shard's visited events: re-sum them for the clock-tick rule
        (abnn_set_global_events)."""
        t = self._torch.tensor([self.brain.visited_events()], dtype=self._torch.int64, device=self.xchg.device)
        self.comm.all_reduce_sum(t)
        self.global_events = int(t.item())
        self.brain.set_global_events(self.global_events)

    def build_graph(self, spec) -> None:
        """Brain.build_graph of this rank's slice [lo, hi) of the spec
        (abnn_build_graph is shard-aware through syn_offset; no communication).
        The spec's total must be the global record count."""
        from . import graph as _graph

        total = _graph.records(spec)
        if total == 0:
            raise ValueError("build_graph: invalid spec")
        if total != self.n_syn_global:
            raise ValueError(f"build_graph: the spec holds {total} records, the sharded graph {self.n_syn_global}")
        self.brain.build_graph(spec)

    def census(self, bins: int, lo: float, hi: float, src=None, dst=None) -> dict:
        """Brain.census over every shard's records (collective: every rank
        calls it at the same point and gets the whole graph's result): the
        local census, then counts and bins summed (all_reduce_sum) and min /
        max combined on their order keys (all_reduce_max; the minimum as the
        maximum of the inverted key)."""
        from . import census as _census

        torch = self._torch
        cfg = _census.config(bins, lo, hi, src, dst)
        local = _census.to_words(self.brain.census(bins, lo, hi, src, dst))
        h = _census.CENSUS_HEADER_WORDS
        counts = np.concatenate([local[:6], local[h:]]).astype(np.int64)
        kmin, kmax = (int(_census.order_key(int(local[i]))) for i in (6, 7))
        t_counts = torch.from_numpy(counts).to(self.xchg.device)
        t_keys = torch.tensor([0xFFFFFFFF - kmin, kmax], dtype=torch.int64, device=self.xchg.device)
        self.comm.all_reduce_sum(t_counts)
        self.comm.all_reduce_max(t_keys)
        counts = t_counts.cpu().numpy().astype(np.uint64)
        keys = np.array([0xFFFFFFFF - int(t_keys[0].item()), int(t_keys[1].item())], dtype=np.uint32)
        bits = np.where(keys >> np.uint32(31), keys ^ np.uint32(0x80000000), ~keys)  # the key's inverse
        words = np.concatenate([counts[:6], bits.astype(np.uint64), counts[6:]])
        return _census.decode(words, cfg)

    def degrees(self, neurons=None, what=("out", "in", "out_w", "in_w")) -> dict:
        """Brain.degrees over every shard's records (collective: every rank
        calls it at the same point and gets the whole graph's result): the
        local result, then the header counts and the planes summed as int64
        (all_reduce_sum; the strength planes wrap as the device's sums do)."""
        from . import degree as _degree

        torch = self._torch
        cfg = _degree.config(neurons, what)
        n_nrn = self.brain.n_neuron()
        local = _degree.to_words(self.brain.degrees(neurons, what))
        t = torch.from_numpy(local.view(np.int64).copy()).to(self.xchg.device)
        self.comm.all_reduce_sum(t)  # words 6 / 7 are zeros on every rank
        return _degree.decode(t.cpu().numpy().view(np.uint64), cfg, n_nrn)

    def select(self, src=None, dst=None, weights=None, any: bool = False, capacity: Optional[int] = None) -> dict:
        """Brain.select over every shard's records (collective: every rank
        calls it at the same point and gets the whole graph's result, indices
        global).  The local count, the header counts exchanged (all_reduce_sum
        and all_gather of every rank's matches), the local select of what the
        merged result needs from this rank, one all_gather of the planes padded
        to the largest part, then select.merge in rank order."""
        from . import select as _select

        torch, dev = self._torch, self.xchg.device
        head = self.brain.select(src, dst, weights, any, capacity=0)
        t_sum = torch.tensor([head["records"], head["tombstones"], head["matched"]], dtype=torch.int64, device=dev)
        self.comm.all_reduce_sum(t_sum)
        mine = torch.tensor([head["matched"]], dtype=torch.int64, device=dev)
        every = torch.zeros(self.world, dtype=torch.int64, device=dev)
        self.comm.all_gather(every, mine)
        matched = [int(m) for m in every.cpu().tolist()]
        capacity = int(t_sum[2].item()) if capacity is None else int(capacity)
        # what the merged result takes from each rank: the first `capacity` matches in rank order
        take, need = [], capacity
        for m in matched:
            take.append(min(m, need))
            need -= take[-1]
        local = self.brain.select(src, dst, weights, any, capacity=take[self.rank])
        pad = max(max(take), 1)
        plane = np.zeros(3 * pad, dtype=np.int64)  # index plane, then record plane
        plane[:local["written"]] = local["index"].view(np.int64)
        plane[pad:pad + 2 * local["written"]] = local["syn"].view(np.int64)
        t_in = torch.from_numpy(plane).to(dev)
        t_out = torch.zeros(self.world * 3 * pad, dtype=torch.int64, device=dev)
        self.comm.all_gather(t_out, t_in)
        planes = t_out.cpu().numpy().reshape(self.world, 3 * pad)
        parts = []
        for r in range(self.world):
            n = take[r]
            parts.append({"records": 0, "tombstones": 0, "matched": matched[r], "written": n,
                          "syn_offset": 0,  # the whole graph's
                          "index": planes[r, :n].view(np.uint64),
                          "syn": np.ascontiguousarray(planes[r, pad:pad + 2 * n]).view(_select.SYN_DTYPE)})
        out = _select.merge(parts, capacity)
        out["records"], out["tombstones"] = int(t_sum[0].item()), int(t_sum[1].item())
        return out

    def edit(self, op, **kw) -> dict:
        """Brain.edit over every shard's records (collective: every rank calls
        it at the same point with the same arguments -- a scale op's ``plane``
        included -- and edits its own shard; a draw gives every record what
        the unsharded brain would give it).  The headers are summed
        (all_reduce_sum): every rank gets the whole graph's."""
        from . import edit as _edit

        local = self.brain.edit(op, **kw)
        t = self._torch.tensor([local[k] for k in _edit.KEYS], dtype=self._torch.int64, device=self.xchg.device)
        self.comm.all_reduce_sum(t)
        return dict(zip(_edit.KEYS, (int(v) for v in t.cpu().tolist())))

    def reorder(self, key=None, descending: bool = False, seed: int = 0, origin: bool = False, perm=None) -> dict:
        """Brain.reorder of this rank's own slice (every rank calls it with the
        same arguments; ``perm`` is the rank's own, over its local indices).
        There is no global sort across shards: a key orders each slice by
        itself, and 'random' gives a record the key the unsharded brain gives
        the same global index.  Returns this rank's result."""
        return self.brain.reorder(key, descending, seed, origin, perm)

    def scale_inputs(self, target: float, neurons=None, limits=(0.5, 2.0)) -> dict:
        """Brain.scale_inputs over every shard's records (collective): a
        neuron's inputs lie on every rank, so the factors come from the merged
        in_w plane of the whole graph (:meth:`degrees`), the same on every
        rank, and each rank scales its own records.  Returns the summed header
        and ``factors``."""
        from . import edit as _edit

        deg = self.degrees(neurons, ("in_w",))
        f = _edit.factors(deg["in_w"], target, limits[0], limits[1])
        out = self.edit("scale_dst", dst=None if neurons is None else (int(neurons[0]), int(neurons[1])), plane=f)
        out["factors"] = f
        return out

    def snapshot(self):
        """Brain.snapshot of this rank's shard (every rank keeps its own;
        no communication): create, capture and synchronise."""
        return self.brain.snapshot()

    def restore(self, snap, what=("records", "state")) -> None:
        """Snapshot.restore on every rank (collective: every rank calls it at
        the same point with its own snapshot of the same moment); a records
        restore changes the shards' record counts, so the visited events are
        re-summed as after a structural update."""
        snap.restore(what)
        self._updates = self.brain.structural_updates()
        parts = (what,) if isinstance(what, str) else tuple(what)
        if "records" in parts:
            self.refresh_global_events()

    def diff(self, snap, bins: int, lo: float, hi: float, src=None, dst=None, now=None) -> dict:
        """Snapshot.diff over every shard's records (collective: every rank
        calls it at the same point with its own snapshots and gets the whole
        graph's result): every word summed as int64 (all_reduce_sum; net wraps
        as the device's sum does), the largest |d| by all_reduce_max."""
        from . import snapshot as _snapshot

        torch = self._torch
        cfg = _snapshot.config(bins, lo, hi, src, dst)
        local = _snapshot.to_words(snap.diff(bins, lo, hi, src, dst, now=now))
        t_sum = torch.from_numpy(local.view(np.int64).copy()).to(self.xchg.device)
        t_max = torch.tensor([int(local[22])], dtype=torch.int64, device=self.xchg.device)
        self.comm.all_reduce_sum(t_sum)
        self.comm.all_reduce_max(t_max)
        words = t_sum.cpu().numpy().view(np.uint64).copy()
        words[22] = int(t_max.item())
        return _snapshot.decode(words, cfg)

    def hops(self, seeds, max_hops: int = 64, reverse: bool = False, weights=None) -> dict:
        """Brain.hops over every shard's records (collective: every rank calls
        it at the same point and gets the whole graph's result).  Every rank
        holds some of the edges, so this drives the steps itself
        (hops_step_enqueue) and, between two steps, replaces every rank's
        plane with the element-wise minimum over the ranks: the comm has no
        min reduction, so the plane goes through all_reduce_max as inverted
        distances (H - d; unreached stays -1).  The merged planes are equal, so
        every rank counts the same levels[h] and skips the dead steps at the
        same point.  Word 0 (records) is summed over the ranks."""
        from . import hops as _hops

        torch, dev = self._torch, self.xchg.device
        cfg = _hops.config(seeds, max_hops, reverse, weights)
        n_nrn = self.brain.n_neuron()
        words = _hops.n_words(cfg, n_nrn)
        if not words:
            raise ValueError("hops: invalid config")
        H, at = int(cfg.max_hops), _hops.plane_offset(cfg)
        out = torch.zeros(words, dtype=torch.int64, device=dev)
        plane = out[at:].view(torch.int32)  # UNREACHED is -1; the pad entry of an odd N_NRN stays 0
        stream = torch.cuda.current_stream(dev)
        self.brain.hops_step_enqueue(cfg, _hops.BEGIN, out.data_ptr(), stream)
        for h in range(H):
            self.brain.hops_step_enqueue(cfg, h, out.data_ptr(), stream)
            if int(out[_hops.HOPS_HEADER_WORDS + h].item()) == 0:
                break  # the same on every rank: the steps up to H - 1 are dead
            inv = torch.where(plane < 0, plane, H - plane)
            self.comm.all_reduce_max(inv)
            plane.copy_(torch.where(inv < 0, inv, H - inv))
        self.brain.hops_step_enqueue(cfg, H, out.data_ptr(), stream)
        records = torch.tensor([self.brain.n_syn()], dtype=torch.int64, device=dev)
        self.comm.all_reduce_sum(records)
        got = out.cpu().numpy().view(np.uint64)
        got[0] = int(records.item())
        return _hops.decode(got, cfg, n_nrn)

    def components(self, neurons=None, weights=None, sizes: bool = False) -> dict:
        """Brain.components over every shard's records (collective: every rank
        calls it at the same point and gets the whole graph's result).  Every
        rank labels its own edges (BEGIN, LINK, FLATTEN); a rank's label plane
        is a spanning forest of that rank's connectivity, so ONE all-gather of
        the planes and their merge on every rank (components_merge_enqueue,
        then FLATTEN, CLOSE) gives the whole graph's components.  Words 0
        (records) and 2 (followed) are summed over the ranks."""
        from . import components as _comp

        torch, dev = self._torch, self.xchg.device
        n_nrn = self.brain.n_neuron()
        cfg = _comp.config(neurons, weights, sizes, n_nrn)
        words = _comp.n_words(cfg, n_nrn)
        if not words:
            raise ValueError("components: invalid config")
        pw = (n_nrn + 1) // 2
        out = torch.zeros(words, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        for step in (_comp.BEGIN, _comp.LINK, _comp.FLATTEN):
            self.brain.components_step_enqueue(cfg, step, out.data_ptr(), stream)
        mine = out[_comp.PLANE_AT:_comp.PLANE_AT + pw]
        planes = torch.empty(self.comm.world * pw, dtype=torch.int64, device=dev)
        self.comm.all_gather(planes, mine.contiguous())
        self.brain.components_merge_enqueue(cfg, planes.data_ptr(), self.comm.world, out.data_ptr(), stream)
        for step in (_comp.FLATTEN, _comp.CLOSE):
            self.brain.components_step_enqueue(cfg, step, out.data_ptr(), stream)
        own = out[torch.tensor([0, 2], device=dev)].clone()
        self.comm.all_reduce_sum(own)
        got = out.cpu().numpy().view(np.uint64)
        got[0], got[2] = int(own[0].item()), int(own[1].item())
        res = _comp.decode(got, cfg, n_nrn)
        if res["gave_up"]:
            raise RuntimeError(f"components: a bounded loop gave up, code {res['gave_up']}")
        return res

    def matrix(self, bounds=None, labels=None, pops=None, what=("count", "w"), weights=None) -> dict:
        """Brain.matrix over every shard's records (collective: every rank
        calls it at the same point with the same partition and gets the whole
        graph's result): the local result, then words 0..8 and the planes
        summed as int64 (all_reduce_sum; the sums wrap as the device's do).
        Words 9..11 and the sizes are the same on every rank and are not
        summed.  That is matrix.merge."""
        from . import matrix as _matrix

        torch = self._torch
        local = self.brain.matrix(bounds, labels, pops, what, weights)
        words = _matrix.to_words(local)
        n_pops = int(local["pops"])
        cfg = _matrix.config(n_pops, sum(bit for k, bit in (("count", 1), ("w", 2), ("p", 4)) if k in local))
        at = _matrix.SIZES_AT + n_pops
        summed = np.concatenate([words[:9], words[at:]])
        t = torch.from_numpy(summed.view(np.int64).copy()).to(self.xchg.device)
        self.comm.all_reduce_sum(t)
        got = t.cpu().numpy().view(np.uint64)
        words[:9], words[at:] = got[:9], got[9:]
        return _matrix.decode(words, cfg)

    def _propagate_merged(self, cfg, x, out, stream):
        """One collective step: this rank's propagation of the device plane
        ``x`` into ``out``, then words 0..3 and y summed over the ranks (exact:
        int64 sums that wrap as the device's do).  Words 4 and 5 describe the
        one x every rank reads and stay the rank's own."""
        self.brain.propagate_enqueue(cfg, x.data_ptr(), out.data_ptr(), stream)
        keep = out[4:6].clone()
        self.comm.all_reduce_sum(out)  # words 6 / 7 are zeros on every rank
        out[4:6] = keep

    def propagate(self, x, inputs=None, outputs=None, reverse: bool = False, fire_p: bool = False, weights=None) -> dict:
        """Brain.propagate over every shard's records (collective: every rank
        calls it at the same point with the same ``x`` and gets the whole
        graph's result): the local pass, then the record counts and y summed
        (all_reduce_sum), which is propagate.merge."""
        from . import propagate as _propagate

        torch, dev = self._torch, self.xchg.device
        cfg = _propagate.config(inputs, outputs, reverse, fire_p, weights)
        n_nrn = self.brain.n_neuron()
        words = _propagate.n_words(cfg, n_nrn)
        x = np.ascontiguousarray(x, dtype=np.int32)
        if not words or x.shape != (n_nrn,):
            raise ValueError("propagate: invalid config or x")
        t_x = torch.from_numpy(x).to(dev)
        out = torch.zeros(words, dtype=torch.int64, device=dev)
        self._propagate_merged(cfg, t_x, out, torch.cuda.current_stream(dev))
        return _propagate.decode(out.cpu().numpy().view(np.uint64), cfg, n_nrn)

    def branching(self, steps: int = 16, neurons=None, fire_p: bool = True, reverse: bool = False, weights=None,
                  x0=None) -> dict:
        """Brain.branching over every shard's records (collective).  Every
        rank holds some of the records, so this drives the steps itself: each
        rank propagates its own records, the results are summed over the ranks
        and the rescale follows the merge (the way :meth:`hops` merges between
        two steps), so every rank holds the same x and the same trace."""
        from . import propagate as _propagate

        torch, dev = self._torch, self.xchg.device
        cfg = _propagate.config(neurons, neurons, reverse, fire_p, weights)
        n_nrn = self.brain.n_neuron()
        words = _propagate.n_words(cfg, n_nrn)
        if not words or not 1 <= int(steps) <= _propagate.PROP_MAX_STEPS:
            raise ValueError("branching: invalid neuron range, weight bounds or steps")
        if x0 is None:
            first, count = _propagate.ranges(cfg, n_nrn)[:2]
            x0 = np.zeros(n_nrn, dtype=np.int32)
            x0[first:first + count] = _propagate.ONE >> 1
        x0 = np.ascontiguousarray(x0, dtype=np.int32)
        if x0.shape != (n_nrn,):
            raise ValueError("branching: x0 must hold N_NRN entries")
        x = torch.from_numpy(x0).to(dev)
        out = torch.zeros(words, dtype=torch.int64, device=dev)
        trace = torch.zeros(int(steps) * _propagate.PROP_TRACE_WORDS, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        for k in range(int(steps)):
            self._propagate_merged(cfg, x, out, stream)
            self.brain.propagate_rescale_enqueue(cfg, out.data_ptr(), x.data_ptr(),
                                                 trace.data_ptr() + 8 * _propagate.PROP_TRACE_WORDS * k, stream)
        stream.synchronize()
        res = _propagate.branching(trace.cpu().numpy().view(np.uint64))
        res["x"] = x.cpu().numpy()
        return res

    def record_spikes(self, raster: int, passes: int, neurons=None, counts: bool = False) -> None:
        """Brain.record_spikes on the local handle.  No collective: every
        rank's spike list is the merged global one, so any rank's recorder
        holds the whole network's spikes."""
        self.brain.record_spikes(raster, passes, neurons, counts)

    def spikes(self) -> dict:
        return self.brain.spikes()

    def spike_counts(self, first=None, n=None) -> np.ndarray:
        return self.brain.spike_counts(first, n)

    def load_spikes(self, passes, raster) -> None:
        self.brain.load_spikes(passes, raster)

    def correlate(self, mode, a=None, b=None, max_lag: int = 16, rows=None, weights=None) -> dict:
        """Brain.correlate over every shard's records (collective for
        "synapses": every rank calls it at the same point and gets the whole
        graph's result).  Every rank's recorder holds the whole network's
        spikes, so "pop" and "pairs" are the local result; for "synapses"
        words 4..6 and the plane are summed (all_reduce_sum)."""
        from . import corr as _corr

        local = self.brain.correlate(mode, a, b, max_lag, rows, weights)
        cfg = _corr.config(mode, a, b, max_lag, rows, weights)
        if cfg.mode != _corr.CORR_SYNAPSES:
            return local
        words = _corr.to_words(local)
        t = self._torch.from_numpy(words[4:].view(np.int64).copy()).to(self.xchg.device)
        t[3] = 0  # word 7 (K) is not a sum
        self.comm.all_reduce_sum(t)
        k = words[7]
        words[4:] = t.cpu().numpy().view(np.uint64)
        words[7] = k
        return _corr.decode(words, cfg)

    def local_events(self) -> int:
        return self.brain.visited_events()

    def sync_visits(self) -> None:
        """The lazy lastVisited merge (never read by a decision): call on every
        rank before reading or saving lastVisited."""
        if self.native is not None:
            from ._lib import call

            call("abnn_comm_sync_visits", self.brain._h, self.native.handle,
                 int(self._torch.cuda.current_stream(self.xchg.device).cuda_stream))
            return
        merge_visits(self.engine, self.comm)
        self.brain.synchronize()
