#!/usr/bin/env python3
"""What the spike recorder's extra launch costs per pass.

At each config (default c1 and c3, the generated graph, all inputs stimulated),
in one process, after a warm-up, these are alternated `--reps` times, each a
call of `--passes` passes that ends in a synchronise, under a host clock:
  (a) abnn_traverse, recorder off
  (b) abnn_traverse, recorder on: no range, counts on
  (c) abnn_traverse, recorder on: range = the outputs, counts on
  (d) abnn_engine_run, recorder off
  (e) abnn_engine_run, recorder on as in (b)
The recorder is started (and so emptied) before every timed call of (b), (c)
and (e), outside the clock, with room for every pass: no pass is dropped, so
every launch does its full work.  The generated graph's steady state emits
about one spike per pass, so (a)-(e) time the launch on nearly empty lists;
full lists exist only in the start-up transient of a fresh state (lastFired =
0: a full budget from the fourth pass on), so
  (f) / (g) a burst of `--burst-passes` passes from a re-zeroed state (lastFired
      and the scalars rewritten by the host before every call, outside the
      clock), recorder off / on as in (b), alternated `--burst-rounds` times,
      with the spikes per pass the recorder saw.
Reported: median and [min, max] in us per
pass, and (b) - (a), (c) - (a), (e) - (d), both as differences of the medians
and as the median and [min, max] of the differences inside each alternation.
Nothing is gated.
--bench-json FILE embeds a recorded bench.py series (this commit against its
parent, alternated) under "bench_py".
Writes profiles/spike_bench.json and prints it.  Needs a GPU.

    python tools/spike_bench.py [--configs c1,c3] [--reps 5] [--out profiles/spike_bench.json]
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


def _config(abnn_amd, name, passes, reps, settle, burst_passes, burst_rounds):
    wl = abnn_amd.CONFIGS[name]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    b.set_auto_stimulus(0, wl.n_input)
    budget = int(b.params.max_spikes)
    outputs = (wl.n_input, wl.n_output)
    rng = np.random.default_rng(3)
    xin = rng.uniform(0.0, 1.0, (passes, wl.n_input)).astype(np.float32)
    xex = rng.uniform(0.0, 1.0, (passes, wl.n_output)).astype(np.float32)

    def start(neurons):
        b.record_spikes(raster=passes * budget, passes=passes, neurons=neurons, counts=True)

    def stop():
        try:
            b.stop_spikes()
        except abnn_amd.AbnnError:
            pass

    def traverse():
        b.encode_traversal(passes)
        b.synchronize()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6 / passes

    b.encode_traversal(settle)  # the start-up transient of a fresh graph
    b.synchronize()
    recorded = {}
    with abnn_amd.LearnEngine(b, trace_passes=passes) as e:
        def engine():
            e.run(xin, xex)
            e.state()  # synchronises

        def row():
            r = {}
            stop()
            r["a_traverse_off"] = timed(traverse)
            start(None)
            r["b_traverse_on"] = timed(traverse)
            recorded["b"] = b.spikes()["info"]
            start(outputs)
            r["c_traverse_on_outputs"] = timed(traverse)
            recorded["c"] = b.spikes()["info"]
            stop()
            r["d_engine_off"] = timed(engine)
            start(None)
            r["e_engine_on"] = timed(engine)
            recorded["e"] = b.spikes()["info"]
            stop()
            return r

        row()  # warm-up: every variant once
        rows = [row() for _ in range(reps)]
    # (f) / (g): full lists, from the start-up transient of a re-zeroed state
    zeros = np.zeros(wl.n_neuron, dtype=np.uint64)

    def burst_call():
        b.encode_traversal(burst_passes)
        b.synchronize()

    def burst(on):
        stop()
        b.set_last_fired(zeros)
        b.set_scalars(0, 0.0, 0.0, 0)
        if on:
            b.record_spikes(raster=burst_passes * budget, passes=burst_passes, counts=True)
        t0 = time.perf_counter()
        burst_call()
        us = (time.perf_counter() - t0) * 1e6 / burst_passes
        return (us, b.spikes()["info"]) if on else (us, None)

    burst(False), burst(True)  # warm-up
    bursts = []
    for _ in range(burst_rounds):
        off, _ = burst(False)
        on, info = burst(True)
        assert info["passes_recorded"] == burst_passes, info
        bursts.append({"f_burst_off": off, "g_burst_on": on, "spikes_per_pass": info["spikes_seen"] / burst_passes})
    stop()
    for k, info in recorded.items():
        assert info["passes_recorded"] == passes and info["passes_dropped"] == 0, (k, info)
    res = {"workload": wl.note, "passes_per_call": passes, "settle_passes": settle, "alternations": rows,
           "last_call_info": recorded}
    for k in rows[0]:
        res[k] = _stat([r[k] for r in rows])
    res["b_minus_a_us_per_pass"] = res["b_traverse_on"]["median"] - res["a_traverse_off"]["median"]
    res["c_minus_a_us_per_pass"] = res["c_traverse_on_outputs"]["median"] - res["a_traverse_off"]["median"]
    res["e_minus_d_us_per_pass"] = res["e_engine_on"]["median"] - res["d_engine_off"]["median"]
    # the same differences inside each alternation (neighbouring calls share the clocks' state)
    res["b_minus_a_each_alternation"] = _stat([r["b_traverse_on"] - r["a_traverse_off"] for r in rows])
    res["c_minus_a_each_alternation"] = _stat([r["c_traverse_on_outputs"] - r["a_traverse_off"] for r in rows])
    res["e_minus_d_each_alternation"] = _stat([r["e_engine_on"] - r["d_engine_off"] for r in rows])
    res["burst"] = {"passes_per_call": burst_passes, "rounds": burst_rounds,
                    "f_burst_off": _stat([r["f_burst_off"] for r in bursts]),
                    "g_burst_on": _stat([r["g_burst_on"] for r in bursts]),
                    "spikes_per_pass": _stat([r["spikes_per_pass"] for r in bursts]),
                    "g_minus_f_each_round": _stat([r["g_burst_on"] - r["f_burst_off"] for r in bursts])}
    res["burst"]["g_minus_f_us_per_pass"] = res["burst"]["g_burst_on"]["median"] - res["burst"]["f_burst_off"]["median"]
    b.close()
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=1000)
    ap.add_argument("--settle", type=int, default=128)
    ap.add_argument("--burst-passes", type=int, default=8)
    ap.add_argument("--burst-rounds", type=int, default=51)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spike_bench.json"))
    args = ap.parse_args()

    import abnn_amd
    from abnn_amd.build import kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("spike_bench needs a HIP device", file=sys.stderr)
        return 1
    res = {"tool": "tools/spike_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "us per pass (host clock around a call of passes_per_call passes that ends in a synchronise)",
           "yardstick": "profiles/learn_bench.json device_minus_bare_us: the learning loop's two extra launches per pass",
           "configs": {}}
    for name in args.configs.split(","):
        res["configs"][name] = _config(abnn_amd, name, args.passes, args.reps, args.settle, args.burst_passes,
                                       args.burst_rounds)
    if args.bench_json:
        with open(args.bench_json) as f:
            res["bench_py"] = json.load(f)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
