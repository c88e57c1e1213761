#!/usr/bin/env python3
"""Signal propagation (abnn_propagate_*): a sparse and a dense step against
the project's other streaming passes, the run aggregation, a narrow out-range,
the branching ratio, the sparse / dense crossover, and the route it replaces.

1. At one config (default c3, the generated graph), in one process, after a
   warm-up, these are alternated `--reps` times, each enqueued into a device
   buffer and timed on the host clock up to a synchronise:
     census_64          abnn_census_enqueue, 64 bins -- the yardstick: 8 B per record
     hops_fwd_inputs    one forward hop of abnn_hops from the 256 inputs (the 3-B src stream)
     sparse_inputs      one step with x non-zero on the 256 inputs, every neuron out: the
                        device chooses the sparse instance (65 536 hits)
     degree_in_w        the degree census's wide in_w plane over every neuron: 1e9 u64 atomics
     dense_all          one step with x non-zero on every neuron, every neuron out (wide)
     dense_all_fire_p   the same with the fire-probability coefficient
     reverse_all        the transpose of dense_all (runs of equal src aggregate)
     narrow_outputs     x non-zero everywhere, the 256 outputs out (LDS accumulators)
     branching_16       abnn_propagate_iterate_enqueue, 16 steps over every neuron, fire_p
   and, after abnn_reorder by dst on the same handle:
     dense_all_sorted   dense_all again: a wave's 128 consecutive records share few dst
2. The crossover: x non-zero on one neuron in `f` (spread evenly), the sparse and
   the dense instance forced in turn through abnn_debug_set_propagate_path.
3. The route this replaces, end to end at `--small` (default c2):
   download_synapses() + propagate.reference against Brain.propagate.
4. With `--parent-lib PATH` (the parent commit's library, built apart):
   bench.py's pass time with that library and with this one, interleaved
   `--bench-reps` times.
Writes profiles/propagate_bench.json and prints it.  Needs a GPU.

    python tools/propagate_bench.py [--config c3] [--small c2] [--reps 7] [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
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


def _bench_pass_ms(lib_path, steps, warmup):
    env = dict(os.environ)
    if lib_path:
        env["ABNN_LIB"] = lib_path
    else:
        env.pop("ABNN_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--no-cpu-baseline", "--no-reference-layout"], capture_output=True, text=True, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(lines[-1])["ms_per_step"]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--small", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-reps", type=int, default=3)
    ap.add_argument("--no-sorted", action="store_true", help="skip the reorder by dst and its leg")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propagate_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import _lib, census, degree, hops
    from abnn_amd import propagate as P
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("propagate_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    res = {"tool": "tools/propagate_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "ms per call (host clock: enqueue into a device buffer, then a synchronise)",
           "sparse_div": P.SPARSE_DIV}

    # ---- 1. the steps against the project's other streaming passes ----
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    n_nrn = wl.n_neuron
    dev = "cuda:0"

    def plane(nonzero):  # x: ONE / 2 where `nonzero` (a bool array or a slice), else 0
        x = np.zeros(n_nrn, dtype=np.int32)
        x[nonzero] = P.ONE >> 1
        return torch.from_numpy(x).to(dev)

    x_in, x_all = plane(slice(0, wl.n_input)), plane(slice(None))
    x_it = plane(slice(None))
    every = P.config()
    cfgs = {"sparse_inputs": (every, x_in), "dense_all": (every, x_all), "dense_all_fire_p": (P.config(fire_p=True), x_all),
            "reverse_all": (P.config(reverse=True), x_all),
            "narrow_outputs": (P.config(outputs=(wl.n_input, wl.n_output)), x_all)}
    out = torch.zeros(P.n_words(every, n_nrn), dtype=torch.int64, device=dev)
    trace = torch.zeros(16 * 8, dtype=torch.int64, device=dev)
    cout = torch.zeros(8 + 64, dtype=torch.int64, device=dev)
    ccfg = census.config(64, 0.0, 1.0)
    hcfg = hops.config((0, wl.n_input), 1)
    hout = torch.zeros(hops.n_words(hcfg, n_nrn), dtype=torch.int64, device=dev)
    dcfg = degree.config(None, ("in_w",))
    dout = torch.zeros(degree.n_words(dcfg, n_nrn), dtype=torch.int64, device=dev)
    it_cfg = P.config(fire_p=True)

    def leg(fn):
        def run():
            fn()
            b.synchronize()
        return run

    def step(name):
        cfg, x = cfgs[name]
        return leg(lambda: b.propagate_enqueue(cfg, x.data_ptr(), out.data_ptr()))

    def branching():
        x_it.copy_(x_all)
        b.propagate_iterate_enqueue(it_cfg, 16, x_it.data_ptr(), out.data_ptr(), trace.data_ptr())

    cases = {"census_64": leg(lambda: b.census_enqueue(ccfg, cout.data_ptr())),
             "hops_fwd_inputs": leg(lambda: b.hops_enqueue(hcfg, hout.data_ptr())),
             "sparse_inputs": step("sparse_inputs"),
             "degree_in_w": leg(lambda: b.degrees_enqueue(dcfg, dout.data_ptr())),
             "dense_all": step("dense_all"), "dense_all_fire_p": step("dense_all_fire_p"),
             "reverse_all": step("reverse_all"), "narrow_outputs": step("narrow_outputs"),
             "branching_16": leg(branching)}
    torch.cuda.synchronize()
    rows, stats = _alternate(cases, args.reps)
    br = P.branching(trace.cpu().numpy().view(np.uint64))
    step("dense_all")()
    dense = P.decode(out.cpu().numpy().view(np.uint64), every, n_nrn)
    step("sparse_inputs")()
    sparse = P.decode(out.cpu().numpy().view(np.uint64), every, n_nrn)
    floor = stats["census_64"]["median"]
    res["steps"] = {"config": args.config, "workload": wl.note, "n_syn": wl.n_syn, "n_neuron": n_nrn,
                    "alternations": rows, **stats,
                    "over_census_median": {k: stats[k]["median"] / floor for k in cases if k != "census_64"},
                    "sparse_over_hops_hop": stats["sparse_inputs"]["median"] / stats["hops_fwd_inputs"]["median"],
                    "dense_over_degree_in_w": stats["dense_all"]["median"] / stats["degree_in_w"]["median"],
                    "sparse_followed": sparse["followed"], "dense_followed": dense["followed"],
                    "dense_followed_G_per_s": dense["followed"] / (stats["dense_all"]["median"] * 1e-3) / 1e9,
                    "branching_estimates": [float(v) for v in br["estimates"]], "branching_ratio": br["ratio"],
                    "branching_ms_per_step": stats["branching_16"]["median"] / 16}

    # ---- 2. the crossover: one neuron in f non-zero, both forward instances forced ----
    cross = []
    for f in (4096, 1024, 256, 128, 64, 32, 16, 4, 2, 1):
        x = plane(slice(0, n_nrn, f))
        t = {}
        for name, path in (("sparse", 1), ("dense", 2)):
            _lib.call("abnn_debug_set_propagate_path", b._h, path)
            run = leg(lambda: b.propagate_enqueue(every, x.data_ptr(), out.data_ptr()))
            run()
            t[name] = _stat([_timed(run) for _ in range(max(3, args.reps // 2))])["median"]
        cross.append({"one_in": f, "nnz": int((n_nrn + f - 1) // f), "sparse_ms": t["sparse"], "dense_ms": t["dense"]})
    _lib.call("abnn_debug_set_propagate_path", b._h, 0)
    faster = [c["one_in"] for c in cross if c["sparse_ms"] <= c["dense_ms"]]
    res["crossover"] = {"rows": cross, "sparse_no_slower_down_to_one_in": min(faster) if faster else None}

    # ---- the dense step over records sorted by dst ----
    if not args.no_sorted:
        b.reorder("dst")
        b.reorder_release()
        run = step("dense_all")
        run()
        res["steps"]["dense_all_sorted"] = _stat([_timed(run) for _ in range(args.reps)])
        after = P.decode(out.cpu().numpy().view(np.uint64), every, n_nrn)
        assert np.array_equal(after["y"], dense["y"]), "the order of the records changed y"
    b.close()
    del out, dout, hout, x_in, x_all, x_it

    # ---- 3. the route this replaces ----
    sw = abnn_amd.CONFIGS[args.small]
    b = abnn_amd.Brain(sw.n_input, sw.n_output, sw.n_hidden, sw.n_syn, sw.events)
    b.build_random_graph(1)
    x = np.full(sw.n_neuron, P.ONE >> 1, dtype=np.int32)
    cfg = P.config(fire_p=True)
    got = {}

    def host_route():
        got["host"] = P.reference(b.download_synapses(), cfg, sw.n_neuron, x, b.params.base_scale)

    def device_route():
        got["device"] = b.propagate(x, fire_p=True)

    rows, stats = _alternate({"download_plus_numpy": host_route, "brain_propagate": device_route}, args.small_reps)
    assert np.array_equal(P.to_words(got["host"]), P.to_words(got["device"]))
    b.close()
    res["host_route"] = {"config": args.small, "n_syn": sw.n_syn, "n_neuron": sw.n_neuron,
                         "unit": "ms end to end (host clock; Brain.propagate includes both planes' copies)",
                         "alternations": rows, **stats,
                         "speedup_median": stats["download_plus_numpy"]["median"] / stats["brain_propagate"]["median"]}

    # ---- 4. bench.py's pass against the parent commit's library ----
    if args.parent_lib:
        rows = []
        for _ in range(args.bench_reps):
            rows.append({"parent_library": _bench_pass_ms(os.path.abspath(args.parent_lib), args.bench_steps, 10),
                         "this_library": _bench_pass_ms(None, args.bench_steps, 10)})
        res["bench_pass"] = {"unit": "ms per pass (bench.py --gpus 1 ms_per_step)", "steps": args.bench_steps,
                             "alternations": rows, "parent_library_ms": _stat([r["parent_library"] for r in rows]),
                             "this_library_ms": _stat([r["this_library"] for r in rows])}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
