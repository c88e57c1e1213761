#!/usr/bin/env python3
"""Reachability (abnn_hops_*): a hop against the synapse census's stream, a
whole search, the dead steps of a search that completes early, and the route
it replaces.

1. At one config (default c3, the generated graph), in one process, after a
   warm-up, these are alternated `--reps` times, each enqueued into a device
   buffer and timed on the host clock up to a synchronise:
     census_64          abnn_census_enqueue, 64 bins -- the yardstick: the project's
                        reference streaming pass, 8 B per record
     fwd_hop_inputs     a whole H = 1 search forward from the 256 inputs: BEGIN, step 0
                        (frontier scan + the 3-B src stream, 65 536 hits), step 1
     fwd_step0_inputs   step 0 of it alone (BEGIN runs before, outside the clock)
     rev_hop_outputs    a whole H = 1 search in reverse from the 256 outputs (the 8-B stream)
     rev_step0_outputs  step 0 of it alone
     fwd_search_hidden  the whole H = 64 search forward from hidden neuron 512: the
                        frontier turns dense and most hits are gathers
     dead_steps         the steps depth + 2 .. 63 of that search again, after it has
                        completed: every kernel reads one word and returns
2. The route this replaces, end to end at `--host-config` (default c2):
   download_synapses() + hops.reference against Brain.hops from hidden neuron
   512.  Checked: the results are equal and the device route is faster.
Writes profiles/hops_bench.json and prints it.  Needs a GPU.

    python tools/hops_bench.py [--config c3] [--reps 7] [--out profiles/hops_bench.json]
"""
import argparse
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
    import torch

    torch.cuda.synchronize()  # the device buffers' zeros
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hops_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import census, hops
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("hops_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    res = {"tool": "tools/hops_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "ms per call (host clock: enqueue into a device buffer, then a synchronise)"}

    # ---- 1. a hop, a search and the dead steps against the census's stream ----
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    n_nrn = wl.n_neuron
    hidden = wl.n_input + wl.n_output
    cfgs = {"fwd_inputs": hops.config((0, wl.n_input), 1), "rev_outputs": hops.config((wl.n_input, wl.n_output), 1, reverse=True),
            "fwd_hidden": hops.config((hidden, 1), 64)}
    outs = {k: torch.zeros(hops.n_words(c, n_nrn), dtype=torch.int64, device="cuda:0") for k, c in cfgs.items()}
    cout = torch.zeros(8 + 64, dtype=torch.int64, device="cuda:0")
    ccfg = census.config(64, 0.0, 1.0)

    def census_leg():
        b.census_enqueue(ccfg, cout.data_ptr())
        b.synchronize()

    def search(k):
        def run():
            b.hops_enqueue(cfgs[k], outs[k].data_ptr())
            b.synchronize()
        return run

    def step0(k):
        def run():
            b.hops_step_enqueue(cfgs[k], hops.BEGIN, outs[k].data_ptr())
            b.synchronize()
            t0 = time.perf_counter()
            b.hops_step_enqueue(cfgs[k], 0, outs[k].data_ptr())
            b.synchronize()
            run.ms = (time.perf_counter() - t0) * 1e3
        return run

    search("fwd_hidden")()
    whole = hops.decode(outs["fwd_hidden"].cpu().numpy().view(np.uint64), cfgs["fwd_hidden"], n_nrn)
    assert whole["complete"] == 1 and whole["depth"] + 2 < 64, whole["depth"]
    dead = list(range(whole["depth"] + 2, 64))

    def dead_leg():  # the plane is complete: these steps find levels[h - 1] == 0
        for h in dead:
            b.hops_step_enqueue(cfgs["fwd_hidden"], h, outs["fwd_hidden"].data_ptr())
        b.synchronize()

    s_fwd, s_rev = step0("fwd_inputs"), step0("rev_outputs")
    cases = {"census_64": census_leg, "fwd_hop_inputs": search("fwd_inputs"), "fwd_step0_inputs": s_fwd,
             "rev_hop_outputs": search("rev_outputs"), "rev_step0_outputs": s_rev,
             "fwd_search_hidden": search("fwd_hidden"), "dead_steps": dead_leg}
    torch.cuda.synchronize()
    for fn in cases.values():  # warm-up
        fn()
        fn()
    rows = []
    for _ in range(args.reps):
        row = {}
        for k, fn in cases.items():
            ms = _timed(fn)
            row[k] = getattr(fn, "ms", ms)  # a step-0 leg clocks itself, after its BEGIN
        rows.append(row)
    stats = {k: _stat([r[k] for r in rows]) for k in cases}
    for k in ("fwd_inputs", "rev_outputs"):  # the step-0 legs left these buffers after step 0
        search(k)()
    fwd = hops.decode(outs["fwd_inputs"].cpu().numpy().view(np.uint64), cfgs["fwd_inputs"], n_nrn)
    rev = hops.decode(outs["rev_outputs"].cpu().numpy().view(np.uint64), cfgs["rev_outputs"], n_nrn)
    assert fwd["levels"].tolist() == [wl.n_input, wl.n_output] and rev["levels"].tolist() == [wl.n_output, wl.n_input]
    b.close()
    floor = stats["census_64"]["median"]
    res["hops"] = {"config": args.config, "workload": wl.note, "n_syn": wl.n_syn, "n_neuron": n_nrn,
                   "alternations": rows, **stats,
                   "over_census_median": {k: stats[k]["median"] / floor for k in cases if k != "census_64"},
                   "fwd_hidden_levels": [int(x) for x in whole["levels"][:whole["depth"] + 2]],
                   "fwd_hidden_reached": whole["reached"], "fwd_hidden_depth": whole["depth"],
                   "dead_steps_count": len(dead), "dead_step_us": stats["dead_steps"]["median"] * 1e3 / len(dead),
                   "bytes_per_hop": {"forward_stream": 3 * wl.n_syn, "reverse_stream": 8 * wl.n_syn,
                                     "frontier_scan": 4 * n_nrn, "bitmap": (n_nrn + 7) // 8},
                   "fwd_step0_stream_GB_per_s": 3 * wl.n_syn / (stats["fwd_step0_inputs"]["median"] * 1e-3) / 1e9,
                   "rev_step0_stream_GB_per_s": 8 * wl.n_syn / (stats["rev_step0_outputs"]["median"] * 1e-3) / 1e9,
                   "census_stream_GB_per_s": 8 * wl.n_syn / (floor * 1e-3) / 1e9}
    del outs

    # ---- 2. the route this replaces ----
    hw = abnn_amd.CONFIGS[args.host_config]
    b = abnn_amd.Brain(hw.n_input, hw.n_output, hw.n_hidden, hw.n_syn, hw.events)
    b.build_random_graph(1)
    seeds = (hw.n_input + hw.n_output, 1)
    cfg = hops.config(seeds, 64)
    got = {}

    def host_route():
        got["host"] = hops.reference(b.download_synapses(), cfg, hw.n_neuron)

    def device_route():
        got["device"] = b.hops(seeds, 64)

    rows, stats = _alternate({"download_plus_numpy": host_route, "brain_hops": device_route}, max(args.reps, 5))
    assert np.array_equal(hops.to_words(got["host"]), hops.to_words(got["device"]))
    b.close()
    res["host_route"] = {"config": args.host_config, "n_syn": hw.n_syn, "n_neuron": hw.n_neuron,
                         "unit": "ms end to end (host clock; Brain.hops includes the copy of the result to the host)",
                         "reached": got["device"]["reached"], "depth": got["device"]["depth"],
                         "alternations": rows, **stats,
                         "speedup_median": stats["download_plus_numpy"]["median"] / stats["brain_hops"]["median"],
                         "device_route_is_faster": stats["brain_hops"]["max"] < stats["download_plus_numpy"]["min"]}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
