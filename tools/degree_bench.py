#!/usr/bin/env python3
"""The neuron degree census: its two paths against the synapse census's stream,
its wave aggregation under contention, and the route it replaces.

1. At one config (default c3, the generated graph), in one process, after a
   warm-up, these are alternated `--reps` times, each enqueued into a device
   buffer and timed on the host clock up to a synchronise:
     census_64        abnn_census_enqueue, 64 bins -- the stream floor (8 B per record)
     narrow_outputs   neurons (256, 256), in | in_w
     narrow_inputs    neurons (0, 256), out | out_w   (reads the src streams: 11 B per record)
     narrow_window    a 4096-neuron hidden window, all four planes (two scans)
     wide_window      an 8192-neuron hidden window, all four planes (the wide path just
                      above the crossover; against two narrow_window calls)
     wide_in          every neuron, in only
     wide_all         every neuron, all four planes
2. Contention, on brains of `--contention-records` uploaded records: uniform
   random src / dst, src sorted ascending, every record on one (src, dst);
   on the narrow path (a brain of NARROW_MAX neurons, every neuron, all four
   planes) and on the wide path (a brain of a million neurons, every neuron, all
   four planes).  Checked: each degenerate leg's median is no longer than the
   uniform leg's of the same path plus that leg's run-to-run spread (max - min).
3. The route this replaces, end to end at `--host-config` (default c2):
   download_synapses() + degree.reference against Brain.degrees of every
   neuron with all four planes.  Checked: the device route is faster.
Writes profiles/degree_bench.json and prints it.  Needs a GPU.

    python tools/degree_bench.py [--config c3] [--reps 7] [--out profiles/degree_bench.json]
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


def _uploaded_brain(abnn_amd, n_nrn, n_syn, kind, piece=1 << 24):
    """A brain of n_syn uploaded records over n_nrn neurons: one host piece,
    re-used (uniform), shifted to the piece's slice of the neurons (sorted) or
    constant (one pair)."""
    b = abnn_amd.Brain(256, 256, n_nrn - 512, n_syn, 100_000)
    rng = np.random.default_rng(7)
    buf = np.zeros(min(piece, n_syn), dtype=abnn_amd.SYN_DTYPE)
    buf["w"] = rng.uniform(0.0, 1.0, len(buf)).astype(np.float32)
    buf["dst"] = rng.integers(0, n_nrn, len(buf), dtype=np.uint32)
    pieces = (n_syn + len(buf) - 1) // len(buf)
    per = n_nrn // pieces
    base = np.sort(rng.integers(0, max(per, 1), len(buf), dtype=np.uint32))
    if kind == "uniform":
        buf["src"] = rng.integers(0, n_nrn, len(buf), dtype=np.uint32)
    elif kind == "one_pair":
        buf["src"], buf["dst"] = 7, 300
    for k, first in enumerate(range(0, n_syn, len(buf))):
        if kind == "src_sorted":
            buf["src"] = base + np.uint32(k * per)
        b.upload_synapses(buf[:min(len(buf), n_syn - first)], first)
    return b


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--host-config", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--contention-records", type=int, default=100_000_000)
    ap.add_argument("--wide-neurons", type=int, default=1_000_512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degree_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import census, degree
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("degree_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    res = {"tool": "tools/degree_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "narrow_max": degree.NARROW_MAX,
           "unit": "ms per call (host clock: enqueue into a device buffer, then a synchronise)"}

    def leg(b, out, neurons, what):
        cfg = degree.config(neurons, what)
        assert degree.n_words(cfg, b.n_neuron()) <= out.numel()

        def run():
            b.degrees_enqueue(cfg, out.data_ptr())
            b.synchronize()
        return run

    # ---- 1. the paths against the census's stream ----
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    out = torch.zeros(8 + 4 * wl.n_neuron, dtype=torch.int64, device="cuda:0")
    ccfg = census.config(64, 0.0, 1.0)

    def census_leg():
        b.census_enqueue(ccfg, out.data_ptr())
        b.synchronize()

    hidden = wl.n_input + wl.n_output + (wl.n_hidden // 2 if wl.n_hidden > 2 * 8192 else 0)
    cases = {
        "census_64": census_leg,
        "narrow_outputs": leg(b, out, (wl.n_input, wl.n_output), ("in", "in_w")),
        "narrow_inputs": leg(b, out, (0, wl.n_input), ("out", "out_w")),
        "narrow_window": leg(b, out, (hidden, degree.NARROW_MAX), 15),
        "wide_window": leg(b, out, (hidden, 2 * degree.NARROW_MAX), 15),
        "wide_in": leg(b, out, None, ("in",)),
        "wide_all": leg(b, out, None, 15),
    }
    rows, stats = _alternate(cases, args.reps)
    whole = b.degrees(None, ("in",))
    assert whole["in_total"] == wl.n_syn and whole["tombstones"] == 0
    assert (whole["in"][wl.n_input:wl.n_input + wl.n_output] == wl.n_input).all()
    b.close()
    del out
    floor = stats["census_64"]["median"]
    paths = {"config": args.config, "workload": wl.note, "n_syn": wl.n_syn, "n_neuron": wl.n_neuron,
             "alternations": rows, **stats,
             "over_census_median": {k: stats[k]["median"] / floor for k in cases if k != "census_64"}}
    for k, adds in (("wide_in", 1), ("wide_all", 4)):  # at most one atomic per record and plane (fewer: runs, zero terms)
        paths[k + "_records_per_s"] = wl.n_syn / (stats[k]["median"] * 1e-3)
        paths[k + "_u64_atomic_adds_per_s_upper"] = adds * wl.n_syn / (stats[k]["median"] * 1e-3)
    paths["wide_window_over_two_narrow_windows"] = stats["wide_window"]["median"] / (2 * stats["narrow_window"]["median"])
    res["paths"] = paths

    # ---- 2. contention ----
    cont = {"records": args.contention_records}
    for path, n_nrn in (("narrow", degree.NARROW_MAX), ("wide", args.wide_neurons)):
        brains = {kind: _uploaded_brain(abnn_amd, n_nrn, args.contention_records, kind)
                  for kind in ("uniform", "src_sorted", "one_pair")}
        out = torch.zeros(8 + 4 * n_nrn, dtype=torch.int64, device="cuda:0")
        rows, stats = _alternate({kind: leg(x, out, None, 15) for kind, x in brains.items()}, args.reps)
        one = brains["one_pair"].degrees(None, 15)
        assert one["out"][7] == args.contention_records == one["in"][300]
        for x in brains.values():
            x.close()
        del out
        spread = stats["uniform"]["max"] - stats["uniform"]["min"]
        cont[path] = {"n_neuron": n_nrn, "alternations": rows, **stats, "uniform_spread": spread,
                      "no_longer_than_uniform_plus_spread": {
                          k: stats[k]["median"] <= stats["uniform"]["median"] + spread
                          for k in ("src_sorted", "one_pair")}}
    res["contention"] = cont

    # ---- 3. the route this replaces ----
    hw = abnn_amd.CONFIGS[args.host_config]
    b = abnn_amd.Brain(hw.n_input, hw.n_output, hw.n_hidden, hw.n_syn, hw.events)
    b.build_random_graph(1)
    cfg = degree.config(None, 15)
    got = {}

    def host_route():
        got["host"] = degree.reference(b.download_synapses(), cfg, hw.n_neuron)

    def device_route():
        got["device"] = b.degrees(None, 15)

    rows, stats = _alternate({"download_plus_numpy": host_route, "brain_degrees": device_route}, max(args.reps, 5))
    assert np.array_equal(degree.to_words(got["host"]), degree.to_words(got["device"]))
    b.close()
    res["host_route"] = {"config": args.host_config, "n_syn": hw.n_syn, "n_neuron": hw.n_neuron,
                         "unit": "ms end to end (host clock; Brain.degrees includes the copy of the planes to the host)",
                         "alternations": rows, **stats,
                         "speedup_median": stats["download_plus_numpy"]["median"] / stats["brain_degrees"]["median"],
                         "device_route_is_faster": stats["brain_degrees"]["max"] < stats["download_plus_numpy"]["min"]}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
