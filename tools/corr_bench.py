#!/usr/bin/env python3
"""Spike correlograms (abnn_corr_*): the SYNAPSES stream against the synapse
census and one sparse forward hop, the index build alone, PAIRS, POP, and the
route it replaces.

1. At one config (default c3, the generated graph, auto stimulus on the
   inputs), in one process: a learning run of `--warm` passes, then `--rows`
   recorded passes.  These are alternated `--reps` times, each enqueued into a
   device buffer and timed on the host clock up to a synchronise:
     census_64       abnn_census_enqueue, 64 bins (8 B per record)
     fwd_hop_inputs  a whole H = 1 search forward from the inputs (the 3-B src
                     stream with one map test): the yardstick
     syn_steady      SYNAPSES, every neuron, L = 16, over the recorded window
     index_build     the same raster loaded into a brain of eight records with
                     the same neurons: the tallies, the slabs and the fill alone
     pairs_256x256   PAIRS, the first 256 hidden neurons against the outputs, L = 16
     pop             POP, every neuron, L = 16
   Then the state is re-zeroed (lastFired, lastVisited, the clock), `--rows`
   passes are recorded again (bursts) and SYNAPSES is timed alone (syn_bursts).
2. The route this replaces, end to end at `--host-config` (default c2) over a
   window of `--host-rows` rows: Brain.spikes() + download_synapses() +
   abnn_corr_host against Brain.correlate.  Checked: the results are equal.
Writes profiles/corr_bench.json and prints it.  Needs a GPU.

    python tools/corr_bench.py [--config c3] [--reps 7] [--out profiles/corr_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _alternate(cases, reps):
    for fn in cases.values():  # warm-up
        fn()
        fn()
    rows = [{k: _timed(fn) for k, fn in cases.items()} for _ in range(reps)]
    return rows, {k: _stat([r[k] for r in rows]) for k in cases}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--host-config", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import _lib, census, corr, hops
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("corr_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    res = {"tool": "tools/corr_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "ms per call (host clock: enqueue into a device buffer, then a synchronise)"}

    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    b.set_auto_stimulus(0, wl.n_input)
    n_nrn, hidden, L = wl.n_neuron, wl.n_input + wl.n_output, 16
    b.encode_traversal(args.warm)
    b.record_spikes(raster=args.rows * int(b.params.max_spikes), passes=args.rows)
    b.encode_traversal(args.rows)
    steady = b.spikes()
    small = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, 8, 1000)  # the index build alone
    small.record_spikes(raster=args.rows * int(b.params.max_spikes), passes=args.rows)
    small.load_spikes(steady["passes"], steady["raster"])

    cfgs = {"syn": corr.config("synapses", max_lag=L), "pop": corr.config("pop", max_lag=L),
            "pairs": corr.config("pairs", (hidden, 256), (wl.n_input, min(256, wl.n_output)), L)}
    outs = {k: torch.zeros(corr.n_words(c), dtype=torch.int64, device="cuda:0") for k, c in cfgs.items()}
    hcfg = hops.config((0, wl.n_input), 1)
    hout = torch.zeros(hops.n_words(hcfg, n_nrn), dtype=torch.int64, device="cuda:0")
    cout = torch.zeros(8 + 64, dtype=torch.int64, device="cuda:0")
    ccfg = census.config(64, 0.0, 1.0)
    torch.cuda.synchronize()

    def leg(brain, k):
        def run():
            brain.correlate_enqueue(cfgs[k], outs[k].data_ptr())
            brain.synchronize()
        return run

    def census_leg():
        b.census_enqueue(ccfg, cout.data_ptr())
        b.synchronize()

    def hop_leg():
        b.hops_enqueue(hcfg, hout.data_ptr())
        b.synchronize()

    cases = {"census_64": census_leg, "fwd_hop_inputs": hop_leg, "syn_steady": leg(b, "syn"),
             "index_build": leg(small, "syn"), "pairs_256x256": leg(b, "pairs"), "pop": leg(b, "pop")}
    rows, stats = _alternate(cases, args.reps)
    leg(b, "syn")()
    d_steady = corr.decode(outs["syn"].cpu().numpy().view(np.uint64), cfgs["syn"])
    small.close()

    # re-zeroed state: bursts
    b.clear_spikes()
    b.set_last_fired(np.zeros(n_nrn, dtype=np.uint64))
    b.set_last_visited(np.zeros(n_nrn, dtype=np.uint64))
    sc = b.scalars()
    b.set_scalars(0, sc["reward"], sc["rbar"])
    b.encode_traversal(args.rows)
    bursts = b.spikes()
    rows_b, stats_b = _alternate({"syn_bursts": leg(b, "syn")}, args.reps)
    d_bursts = corr.decode(outs["syn"].cpu().numpy().view(np.uint64), cfgs["syn"])
    b.close()

    def summary(s, d):
        return {"rows": int(s["info"]["passes_recorded"]), "spikes": int(s["info"]["spikes_recorded"]),
                "spikes_per_pass": s["info"]["spikes_recorded"] / max(1, s["info"]["passes_recorded"]),
                "neurons_with_entries": int(np.unique(s["raster"]).size), "followed": d["followed"],
                "coupled": d["coupled"], "pairs": d["total"]}

    hop, cen = stats["fwd_hop_inputs"]["median"], stats["census_64"]["median"]
    res["corr"] = {"config": args.config, "workload": wl.note, "n_syn": wl.n_syn, "n_neuron": n_nrn, "max_lag": L,
                   "alternations": rows, **stats, "bursts_alternations": rows_b, **stats_b,
                   "steady": summary(steady, d_steady), "bursts": summary(bursts, d_bursts),
                   "syn_steady_over_hop_median": stats["syn_steady"]["median"] / hop,
                   "syn_steady_over_census_median": stats["syn_steady"]["median"] / cen,
                   "syn_bursts_over_hop_median": stats_b["syn_bursts"]["median"] / hop,
                   "bytes": {"src_stream": 3 * wl.n_syn, "dst_w_gather": 8 * wl.n_syn}}
    del outs

    # ---- 2. the route this replaces ----
    hw = abnn_amd.CONFIGS[args.host_config]
    b = abnn_amd.Brain(hw.n_input, hw.n_output, hw.n_hidden, hw.n_syn, hw.events)
    b.build_random_graph(1)
    b.set_auto_stimulus(0, hw.n_input)
    b.encode_traversal(args.warm)
    b.record_spikes(raster=args.host_rows * int(b.params.max_spikes), passes=args.host_rows)
    b.encode_traversal(args.host_rows)
    cfg = corr.config("synapses", max_lag=L)
    got = {}
    lib = _lib.load()

    def host_route():
        s, syn = b.spikes(), b.download_synapses()
        out = np.zeros(corr.n_words(cfg), dtype=np.uint64)
        _lib.check("abnn_corr_host", lib.abnn_corr_host(C.byref(cfg), hw.n_neuron, s["passes"].ctypes.data, len(s["passes"]),
                                                        s["raster"].ctypes.data, len(s["raster"]), syn.ctypes.data, len(syn),
                                                        out.ctypes.data))
        got["host"] = out

    def device_route():
        got["device"] = corr.to_words(b.correlate("synapses", max_lag=L))

    rows, stats = _alternate({"download_plus_host_rule": host_route, "brain_correlate": device_route}, max(args.reps, 5))
    assert np.array_equal(got["host"], got["device"])
    b.close()
    res["host_route"] = {"config": args.host_config, "n_syn": hw.n_syn, "n_neuron": hw.n_neuron, "rows": args.host_rows,
                         "unit": "ms end to end (host clock; Brain.correlate includes the copy of the result to the host)",
                         "alternations": rows, **stats,
                         "speedup_median": stats["download_plus_host_rule"]["median"] / stats["brain_correlate"]["median"]}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
