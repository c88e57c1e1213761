#!/usr/bin/env python3
"""The record reorder against the synapse census, which streams the same records.

At one config (default c3, the generated graph), in one process, after a
warm-up, each reorder below is alternated with the census `--reps` times; every
call is an enqueue with device buffers allocated beforehand and one
synchronise, under the host clock.  The graph is generated again before every
timed reorder, so each one starts from the same (unsorted) records:
  census        abnn_census_enqueue, 64 bins over [0, 1)  -- the yardstick: 8 B per record
  src, dst      ascending; with N_NRN < 2^24 the fourth radix pass is skipped
  w             ascending: all four radix passes
  random        a seeded shuffle: all four
  none          no tombstone in the graph: the keys pass, no radix pass, a move that moves nothing
  dst_sorted    by dst once more, over the records the timed `dst` left
  perm          PERM with the inverse of `dst`'s origin (built on the device with torch)
Then, on a second handle created with ABNN_REORDER_SKIP=0, `src` with all four
radix passes.  Then the default pass (abnn_traverse, `--pass-reps` passes per
timing) on the generated graph, after a reorder by dst and after RANDOM -- for
the record: such passes compute a different, equally legal result.  Then, at
the size of `--small` (default c2), Brain.reorder against download_synapses() +
numpy stable argsort + upload_synapses().  Every rate is given against two byte
counts per record: the model of the issue (8 B keys, 16 B per radix pass, 11 B
gathered, 22 B copied) and what this implementation moves (reorder.hip).
Writes profiles/reorder_bench.json and prints it.  Needs a GPU.

    python tools/reorder_bench.py [--config c3] [--small c2] [--reps 7] [--out profiles/reorder_bench.json]

The split into keys / radix passes / move comes from a run of its own under
the profiler, which this tool only drives and folds in:
    rocprofv3 --kernel-trace --stats -T --output-format csv -d DIR -o run -- \\
        python tools/reorder_bench.py --profile src --config c3
    python tools/reorder_bench.py --fold-stats DIR --profile src [--out profiles/reorder_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROFILE_REORDERS = 3  # reorders of a --profile run (the first is the warm-up)
GROUPS = (("keys", ("k_reorder_tombs", "k_reorder_tomb_scan", "k_reorder_keys", "k_reorder_plan")),
          ("radix", ("k_reorder_count", "k_reorder_scan", "k_reorder_scatter")),
          ("move", ("k_reorder_pack", "k_reorder_move", "k_reorder_valid")),
          ("bookkeeping", ("k_src32_sync", "k_tally_dead")))


def _stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def model_bytes(radix_passes: int, src_key: bool) -> dict:
    """Bytes per record: the issue's model, and what reorder.hip moves -- the
    tombstone count (8), the keys pass (8 or 11 read, 8 written), per radix pass
    the count (8) and the scatter (8 + 8), the packed copy (11 + 12) and the move
    (8 of origin, 12 gathered, 11 written)."""
    return {"model": 8 + 16 * radix_passes + 11 + 22,
            "implementation": 8 + (11 if src_key else 8) + 8 + 24 * radix_passes + 23 + 31}


def fold_stats(stats_dir: str, key: str, out: str) -> int:
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        print(f"no *kernel_stats.csv under {stats_dir}", file=sys.stderr)
        return 1
    kernels = {}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            kernels[row["Name"]] = {"calls": int(row["Calls"]), "total_ns": int(float(row["TotalDurationNs"]))}
    groups = {g: {"ms_per_reorder": 0.0, "kernels": {}} for g, _ in GROUPS}
    for name, k in kernels.items():
        for g, needles in GROUPS:
            if any(s in name for s in needles):
                short = name.split("(")[0].split("::")[-1]
                groups[g]["kernels"][short] = k
                groups[g]["ms_per_reorder"] += k["total_ns"] / 1e6 / PROFILE_REORDERS
    total = sum(g["ms_per_reorder"] for g in groups.values())
    split = {"source": "rocprofv3 --kernel-trace --stats, a run of its own: " + str(PROFILE_REORDERS) + " reorders by '"
                       + key + "' of the generated graph; kernel time only",
             "ms_per_reorder_total": total, "groups": groups}
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    res.setdefault("kernel_split", {})[key] = split
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(split))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--small", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-reps", type=int, default=3)
    ap.add_argument("--pass-reps", type=int, default=20)
    ap.add_argument("--profile", default=None, help="only a few reorders by this key (a run under the profiler)")
    ap.add_argument("--fold-stats", default=None, help="fold the profiler's kernel_stats.csv under this directory into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reorder_bench.json"))
    args = ap.parse_args()
    if args.fold_stats:
        return fold_stats(args.fold_stats, args.profile or "src", args.out)

    import torch

    import abnn_amd
    from abnn_amd import census, reorder
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("reorder_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    wl = abnn_amd.CONFIGS[args.config]
    n = wl.n_syn

    def make():
        b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, wl.n_input)
        return b

    b = make()
    words = reorder.n_words(reorder.config("dst", origin=True), n)
    out = torch.zeros(words, dtype=torch.int64, device="cuda:0")

    def run(cfg, perm_ptr=None):
        b.reorder_enqueue(cfg, perm_ptr, out.data_ptr())
        b.synchronize()

    if args.profile:
        cfg = reorder.config(args.profile, seed=1 if args.profile == "random" else 0)
        for _ in range(PROFILE_REORDERS):
            b.build_random_graph(1)
            run(cfg)
        b.close()
        print(json.dumps({"profiled": args.profile, "reorders": PROFILE_REORDERS}))
        return 0

    ccfg = census.config(64, 0.0, 1.0)
    cbuf = torch.zeros(census.CENSUS_HEADER_WORDS + 64, dtype=torch.int64, device="cuda:0")

    def run_census():
        b.census_enqueue(ccfg, cbuf.data_ptr())
        b.synchronize()

    cfgs = {"src": reorder.config("src"), "dst": reorder.config("dst", origin=True), "w": reorder.config("w"),
            "random": reorder.config("random", seed=1), "none": reorder.config("none")}
    passes = {"src": 3, "dst": 3, "w": 4, "random": 4, "none": 0, "dst_sorted": 3}
    inv = torch.empty(n, dtype=torch.int32, device="cuda:0")
    idx = torch.arange(n, dtype=torch.int32, device="cuda:0")

    def round_(timed: bool):
        row = {}
        for k, cfg in cfgs.items():
            b.build_random_graph(1)
            b.synchronize()
            t_c = _timed(run_census)
            t = _timed(lambda: run(cfg))
            row["census_before_" + k], row[k] = t_c, t
            if k == "dst":  # over the sorted records once more, then back by PERM with the inverse
                head = reorder.decode(out[:8].cpu().numpy().view(np.uint64), reorder.config("dst"))
                assert head["records"] == n and head["moved"] > 0.9 * n, head
                origin = out[8:].view(torch.int32)[:n]
                inv[origin.long()] = idx
                torch.cuda.synchronize()
                row["census_before_dst_sorted"] = _timed(run_census)
                row["dst_sorted"] = _timed(lambda: run(reorder.config("dst")))
                assert int(out[2].item()) == 0, "a sorted input moved"
                row["census_before_perm"] = _timed(run_census)
                row["perm"] = _timed(lambda: run(reorder.config("perm"), inv.data_ptr()))
                assert int(out[3].item()) == 0 and int(out[2].item()) == head["moved"]
        return row

    sum0 = None
    b.build_random_graph(1)
    sum0 = b.checksum()
    round_(False)  # warm-up: the scratch, every kernel
    assert b.checksum() != 0
    reps = [round_(True) for _ in range(args.reps)]
    b.build_random_graph(1)
    run(cfgs["dst"])
    run(reorder.config("perm"), inv.data_ptr())
    assert b.checksum() == sum0, "PERM with the inverse did not give the generated graph back"

    res = {"tool": "tools/reorder_bench.py", "source_sha": kernel_source_sha(), "config": args.config, "workload": wl.note,
           "n_syn": n, "n_neuron": wl.n_neuron, "reps": args.reps,
           "unit": "ms per call (host clock: an enqueue with preallocated device buffers, then one synchronise)",
           "scratch_bytes": 28 * n, "alternations": reps}
    res["census"] = _stat([r[k] for r in reps for k in r if k.startswith("census_before_")])
    for k in list(cfgs) + ["dst_sorted", "perm"]:
        res[k] = {"ms": _stat([r[k] for r in reps]), "census_ms": _stat([r["census_before_" + k] for r in reps]),
                  "over_census": _stat([r[k] / r["census_before_" + k] for r in reps])}
        if k in passes:
            by = model_bytes(passes[k], k == "src")
            res[k]["radix_passes"] = passes[k]
            res[k]["bytes_per_record"] = by
            res[k]["bytes_per_s"] = {m: v * n / (res[k]["ms"]["median"] * 1e-3) for m, v in by.items()}

    # the default pass on the generated graph, after a reorder by dst and after RANDOM
    def passes_ms():
        b.encode_traversal(args.pass_reps)
        b.synchronize()

    res["default_pass"] = {"unit": f"ms per abnn_traverse pass (host clock over {args.pass_reps} passes, one synchronise)",
                           "note": "for the record, not a target: a pass over reordered records visits other records first "
                                   "and computes a different, equally legal result"}
    for name, cfg in (("generated", None), ("after_dst", cfgs["dst"]), ("after_random", cfgs["random"])):
        b.build_random_graph(1)
        if cfg is not None:
            run(cfg)
        passes_ms()  # settle
        res["default_pass"][name] = _stat([_timed(passes_ms) / args.pass_reps for _ in range(args.reps)])
    b.close()

    # src with all four radix passes (ABNN_REORDER_SKIP is read when the handle is created)
    os.environ["ABNN_REORDER_SKIP"] = "0"
    b = make()
    os.environ.pop("ABNN_REORDER_SKIP", None)
    rows = []
    for i in range(args.reps + 1):
        b.build_random_graph(1)
        b.synchronize()
        rows.append(_timed(lambda: run(cfgs["src"])))
    res["src_all_four_passes"] = {"ms": _stat(rows[1:]), "radix_passes": 4,
                                  "skip_gain_ms": _stat(rows[1:])["median"] - res["src"]["ms"]["median"]}
    b.close()
    del out, inv, idx, cbuf

    # Brain.reorder against download + numpy stable argsort + upload at a size the host route can afford
    ws = abnn_amd.CONFIGS[args.small]
    with abnn_amd.Brain(ws.n_input, ws.n_output, ws.n_hidden, ws.n_syn, ws.events) as s:
        def host_route():
            syn = s.download_synapses()
            order = np.argsort(syn["dst"], kind="stable")
            s.upload_synapses(syn[order])

        s.build_random_graph(1)
        s.reorder("dst")  # warm-up: the scratch
        small = []
        for _ in range(args.small_reps):
            s.build_random_graph(1)
            row = {"download_argsort_upload": _timed(host_route)}
            want = s.checksum()
            s.build_random_graph(1)
            row["brain_reorder"] = _timed(lambda: s.reorder("dst"))
            assert s.checksum() == want, "the host route and Brain.reorder disagree"
            small.append(row)
    res["host_route"] = {"config": args.small, "n_syn": ws.n_syn, "unit": "ms per call (host clock)", "alternations": small,
                         "brain_reorder_ms": _stat([r["brain_reorder"] for r in small]),
                         "download_argsort_upload_ms": _stat([r["download_argsort_upload"] for r in small])}
    res["host_route"]["speedup"] = (res["host_route"]["download_argsort_upload_ms"]["median"]
                                    / res["host_route"]["brain_reorder_ms"]["median"])

    if os.path.exists(args.out):  # keep a kernel split folded in earlier
        with open(args.out) as f:
            old = json.load(f)
        if "kernel_split" in old:
            res["kernel_split"] = old["kernel_split"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
