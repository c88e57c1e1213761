#!/usr/bin/env python3
"""Connected components (abnn_components_*): both LINK paths against the
project's other streaming passes, a fragmenting threshold, a narrow range, and
the route it replaces.

1. At one config (default c3, the generated graph), in one process, after a
   warm-up, these are alternated `--reps` times, each enqueued into a device
   buffer and timed on the host clock up to a synchronise:
     census_64            abnn_census_enqueue, 64 bins -- the yardstick: 8 B per record
     degree_in            the degree census's wide `in` plane over every neuron
     hops_hidden          a whole abnn_hops search from hidden neuron 512
     components_walk      abnn_components_enqueue over every neuron, the path at 1:
                          every followed record walks the plane
     components_settled   the same with the path at 2: the settled map
     components_auto      the same with the path at 0 (the default)
     components_sizes     the default path with the size plane
     threshold            w in [0.1998, inf): one hidden record in 500 is followed, less
                          than one per neuron, so the graph falls apart (default path)
     range_4096           the 4096 neurons from 512 on (default path)
2. The route this replaces, end to end at `--small` (default c2):
   download_synapses() + components.reference against Brain.components.
3. With `--parent-lib PATH` (the parent commit's library, built apart):
   bench.py's pass time with that library and with this one, interleaved
   `--bench-reps` times.
Writes profiles/components_bench.json (or --out) and prints it.  Needs a GPU.

    python tools/components_bench.py [--config c3] [--small c2] [--reps 7] [--parent-lib PATH]
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import _lib, census, degree, hops
    from abnn_amd import components as K
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("components_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    res = {"tool": "tools/components_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "ms per call (host clock: enqueue into a device buffer, then a synchronise)"}

    # ---- 1. both paths against the project's other streaming passes ----
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    n_nrn = wl.n_neuron
    dev = "cuda:0"
    # the generated hidden weights are uniform in [0.1, 0.2): this keeps one hidden record in 500, and the whole
    # dense input -> output block (its weights are in [0.4, 0.8))
    t_cut = 0.1998
    every = K.config(None, None, False, n_nrn)
    sized = K.config(None, None, True, n_nrn)
    cut = K.config(None, (t_cut, float("inf")), False, n_nrn)
    narrow = K.config((512, 4096), None, False, n_nrn)
    out = torch.zeros(K.n_words(sized, n_nrn), dtype=torch.int64, device=dev)
    cout = torch.zeros(8 + 64, dtype=torch.int64, device=dev)
    ccfg = census.config(64, 0.0, 1.0)
    hcfg = hops.config((512, 1), 64)
    hout = torch.zeros(hops.n_words(hcfg, n_nrn), dtype=torch.int64, device=dev)
    dcfg = degree.config(None, ("in",))
    dout = torch.zeros(degree.n_words(dcfg, n_nrn), dtype=torch.int64, device=dev)

    def leg(fn):
        def run():
            fn()
            b.synchronize()
        return run

    def comp(cfg, path):
        def run():
            _lib.call("abnn_debug_set_components_path", b._h, path)
            b.components_enqueue(cfg, out.data_ptr())
            b.synchronize()
        return run

    b.components((0, 1))  # the handle's first call allocates the scratch
    cases = {"census_64": leg(lambda: b.census_enqueue(ccfg, cout.data_ptr())),
             "degree_in": leg(lambda: b.degrees_enqueue(dcfg, dout.data_ptr())),
             "hops_hidden": leg(lambda: b.hops_enqueue(hcfg, hout.data_ptr())),
             "components_walk": comp(every, 1), "components_settled": comp(every, 2), "components_auto": comp(every, 0),
             "components_sizes": comp(sized, 0), "threshold": comp(cut, 0), "range_4096": comp(narrow, 0)}
    torch.cuda.synchronize()
    rows, stats = _alternate(cases, args.reps)
    found = {}
    for name, cfg, path in (("walk", every, 1), ("settled", every, 2), ("threshold", cut, 0), ("range_4096", narrow, 0)):
        comp(cfg, path)()
        d = K.decode(out[:K.n_words(cfg, n_nrn)].cpu().numpy().view(np.uint64), cfg, n_nrn)
        found[name] = {k: d[k] for k in ("followed", "components", "largest", "largest_label", "singletons", "gave_up")}
        found[name]["labels_crc"] = int(np.bitwise_xor.reduce(d["labels"].astype(np.uint64) * np.arange(1, n_nrn + 1, dtype=np.uint64)))
    assert found["walk"] == found["settled"], "the paths disagree"
    floor = stats["census_64"]["median"]
    hd = hops.decode(hout.cpu().numpy().view(np.uint64), hcfg, n_nrn)
    res["calls"] = {"config": args.config, "workload": wl.note, "n_syn": wl.n_syn, "n_neuron": n_nrn, "threshold_w_lo": t_cut,
                    "alternations": rows, **stats, "found": found,
                    "hops_hidden_depth": hd["depth"], "hops_hidden_reached": hd["reached"],
                    "over_census_median": {k: stats[k]["median"] / floor for k in cases if k != "census_64"},
                    "walk_over_settled": stats["components_walk"]["median"] / stats["components_settled"]["median"],
                    "settled_over_degree_in": stats["components_settled"]["median"] / stats["degree_in"]["median"],
                    "followed_G_per_s_settled": found["settled"]["followed"] / (stats["components_settled"]["median"] * 1e-3) / 1e9,
                    "followed_G_per_s_walk": found["walk"]["followed"] / (stats["components_walk"]["median"] * 1e-3) / 1e9}
    _lib.call("abnn_debug_set_components_path", b._h, 0)
    b.close()
    del out, dout, hout

    # ---- 2. the route this replaces ----
    sw = abnn_amd.CONFIGS[args.small]
    b = abnn_amd.Brain(sw.n_input, sw.n_output, sw.n_hidden, sw.n_syn, sw.events)
    b.build_random_graph(1)
    cfg = K.config(None, None, True, sw.n_neuron)
    got = {}

    def host_route():
        got["host"] = K.reference(b.download_synapses(), cfg, sw.n_neuron)

    def device_route():
        got["device"] = b.components(sizes=True)

    rows, stats = _alternate({"download_plus_numpy": host_route, "brain_components": device_route}, args.small_reps)
    assert np.array_equal(K.to_words(got["host"]), K.to_words(got["device"]))
    b.close()
    res["host_route"] = {"config": args.small, "n_syn": sw.n_syn, "n_neuron": sw.n_neuron,
                         "unit": "ms end to end (host clock; Brain.components includes the result's copy)",
                         "alternations": rows, **stats,
                         "speedup_median": stats["download_plus_numpy"]["median"] / stats["brain_components"]["median"]}

    # ---- 3. bench.py's pass against the parent commit's library ----
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
