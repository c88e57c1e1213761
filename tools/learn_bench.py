#!/usr/bin/env python3
"""Learning passes per second: the host-driven loop against the device-resident loop.

(a) abnn::BrainEngine<abnn::Brain>::run_one_pass -- the reference's driver over
    the C-ABI accessors, every pass synchronised several times;
(b) abnn::DeviceBrainEngine -- abnn_engine_run in calls of 1000 passes;
and the bare traversal (abnn_traverse alone) beside them, at config 1 and
config 3.  The three are alternated `--reps` times in one process per config
(tools/learn_bench.cpp); host clock around work that ends in a synchronise.
Writes profiles/learn_bench.json and prints it.  Needs a GPU.

    python tools/learn_bench.py [--configs c1,c3] [--reps 3] [--out profiles/learn_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=1000)
    ap.add_argument("--device-calls", type=int, default=3)
    ap.add_argument("--call", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_bench.json"))
    args = ap.parse_args()

    import abnn_amd
    from abnn_amd.build import build_hip, build_learn_bench, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("learn_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    prog = build_learn_bench()
    res = {"tool": "tools/learn_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "us per learning pass (host clock, ends in a synchronise)", "configs": {}}
    for name in args.configs.split(","):
        wl = abnn_amd.CONFIGS[name]
        r = subprocess.run([prog, str(wl.n_hidden), str(wl.n_syn), str(wl.events), str(args.host_passes),
                            str(args.device_calls), str(args.call), str(args.reps)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            return 1
        run = json.loads(r.stdout.strip().splitlines()[-1])
        reps = run["reps"]
        row = {"workload": wl.note, "host_passes_per_rep": run["host_passes"],
               "device_passes_per_rep": run["device_passes"], "call": run["call"], "alternations": reps}
        for k in ("host_us", "device_us", "bare_us"):
            v = sorted(x[k] for x in reps)
            row[k] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
        row["host_passes_per_s"] = 1e6 / row["host_us"]["median"]
        row["device_passes_per_s"] = 1e6 / row["device_us"]["median"]
        row["speedup_median"] = row["host_us"]["median"] / row["device_us"]["median"]
        row["device_minus_bare_us"] = row["device_us"]["median"] - row["bare_us"]["median"]
        row["device_no_slower_in_every_alternation"] = all(x["device_us"] <= x["host_us"] for x in reps)
        res["configs"][name] = row
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
