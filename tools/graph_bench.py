#!/usr/bin/env python3
"""The device-side graph builder (abnn_build_graph) against the generator it
generalises and the host route it replaces.

1. Parity with the old generator, at one config (default c3): on ONE handle,
   in one process, after a warm-up, these synchronous calls are alternated
   `--reps` times and timed on the host clock (each call waits for the device
   before and after its launch):
     generate        abnn_generate_synapses (k_generate: 2-byte and 1-byte src stores)
     build_recipe    Brain.build_graph(graph.recipe(...)): the same shape, uniform weights
     build_ring_beta one small-world block, k = 200, p = 0.1, Beta(2, 8): eleven draws a
                     record -- what the arithmetic costs when the stores are the same
   and the same three on a second handle created with ABNN_GRAPH_NT=1
   (non-temporal stores), so that the two store flavours alternate in one run.
   Reported: median and range, the write rate on 11 B per record against the
   measured HBM copy ceiling (6.29 TB/s, the MI355X microarchitecture notes),
   and whether build_recipe is no slower than generate beyond the spread of
   the alternations (max - min of generate).
2. The host route, at `--host-config` (default c2): graph.reference +
   upload_synapses (what a user without the builder does) against build_graph.
Writes profiles/graph_bench.json, prints it and the README row.  Needs a GPU.

    python tools/graph_bench.py [--config c3] [--reps 7] [--out profiles/graph_bench.json]

--grid-sweep: instead, one handle per grid cap (ABNN_GRAPH_BLOCKS = 2048 ..
65536) at the config, alternating the recipe, the small-world Beta block and a
dense block (one draw per record: the store side alone) on each, the recipe
with non-temporal stores at 16384, and abnn_generate_synapses; writes
{"rows", "median"} to profiles/graph_bench_grid_sweep.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_RECORD = 11  # u16 lo + u8 hi + {dst, w}
HBM_COPY_CEILING = 6.29e12  # B/s, measured float4 copy


def _stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _alternate(cases, reps):
    for fn in cases.values():  # warm-up: code objects, first-touch of the arrays
        fn()
        fn()
    rows = [{k: _timed(fn) for k, fn in cases.items()} for _ in range(reps)]
    return rows, {k: _stat([r[k] for r in rows]) for k in cases}


def grid_sweep(args) -> int:
    import abnn_amd
    from abnn_amd import graph

    w = abnn_amd.CONFIGS[args.config]
    recipe = graph.recipe(w.n_input, w.n_output, w.n_hidden, w.n_syn, seed=1)
    ring = graph.spec([graph.small_world((w.n_input + w.n_output, w.n_hidden), 200, 0.1, graph.beta(2, 8),
                                         count=w.n_syn)], 1)
    dense = graph.spec([graph.dense((0, 4096), (4096, 4096), graph.uniform(0.1, 0.2), count=w.n_syn)], 1)
    cases, brains = {}, []
    for blocks in (2048, 8192, 16384, 32768, 65536):
        for nt in ((0, 1) if blocks == 16384 else (0,)):
            os.environ["ABNN_GRAPH_BLOCKS"], os.environ["ABNN_GRAPH_NT"] = str(blocks), str(nt)  # read at create
            b = abnn_amd.Brain(w.n_input, w.n_output, w.n_hidden, w.n_syn, w.events)
            brains.append(b)
            cases[f"recipe_{blocks}_nt{nt}"] = lambda b=b: b.build_graph(recipe)
            if nt == 0:
                cases[f"ring_{blocks}"] = lambda b=b: b.build_graph(ring)
                cases[f"dense_{blocks}"] = lambda b=b: b.build_graph(dense)
    cases["generate"] = lambda b=brains[0]: b.build_random_graph(1)
    rows, stats = _alternate(cases, args.reps)
    res = {"rows": rows, "median": {k: v["median"] for k, v in stats.items()}}
    out = args.out if args.out.endswith("sweep.json") else os.path.join(ROOT, "profiles", "graph_bench_grid_sweep.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["median"], indent=1))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--host-config", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_bench.json"))
    ap.add_argument("--grid-sweep", action="store_true")
    args = ap.parse_args()

    import abnn_amd
    from abnn_amd import graph
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("graph_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    if args.grid_sweep:
        return grid_sweep(args)
    res = {"tool": "tools/graph_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "ms per synchronous call (host clock)", "bytes_per_record": BYTES_PER_RECORD,
           "hbm_copy_ceiling_TBps": HBM_COPY_CEILING / 1e12}

    # ---- 1. parity with abnn_generate_synapses, the compute-bound block ---------------------------
    w = abnn_amd.CONFIGS[args.config]
    recipe = graph.recipe(w.n_input, w.n_output, w.n_hidden, w.n_syn, seed=1)
    hid = (w.n_input + w.n_output, w.n_hidden)
    ring = graph.spec([graph.small_world(hid, 200, 0.1, graph.beta(2, 8), count=w.n_syn)], 1)
    assert graph.records(recipe) == w.n_syn == graph.records(ring)
    cases, brains = {}, []
    for nt in (0, 1):
        os.environ["ABNN_GRAPH_NT"] = str(nt)  # read at create
        b = abnn_amd.Brain(w.n_input, w.n_output, w.n_hidden, w.n_syn, w.events)
        brains.append(b)
        tag = "_nt" if nt else ""
        cases["generate" + tag] = lambda b=b: b.build_random_graph(1)
        cases["build_recipe" + tag] = lambda b=b: b.build_graph(recipe)
        cases["build_ring_beta" + tag] = lambda b=b: b.build_graph(ring)
    del os.environ["ABNN_GRAPH_NT"]
    rows, stats = _alternate(cases, args.reps)
    checks = {}
    for b in brains:  # the two store flavours write the same records
        b.build_graph(recipe)
        checks.setdefault("recipe", []).append(b.checksum())
        b.build_graph(ring)
        checks.setdefault("ring", []).append(b.checksum())
    for b in brains:
        b.close()
    par = {"config": w.name, "workload": w.note, "n_syn": w.n_syn, "n_neuron": w.n_neuron, "alternations": rows}
    par.update(stats)
    par["write_TBps_median"] = {k: w.n_syn * BYTES_PER_RECORD / (v["median"] * 1e-3) / 1e12 for k, v in stats.items()}
    par["share_of_hbm_copy_ceiling"] = {k: v * 1e12 / HBM_COPY_CEILING for k, v in par["write_TBps_median"].items()}
    par["records_per_s_median"] = {k: w.n_syn / (v["median"] * 1e-3) for k, v in stats.items()}
    spread = stats["generate"]["max"] - stats["generate"]["min"]
    par["generate_spread"] = spread
    par["build_recipe_no_slower_than_generate_plus_spread"] = {
        k: stats[k]["median"] <= stats["generate"]["median"] + spread for k in ("build_recipe", "build_recipe_nt")}
    par["ring_beta_over_recipe_median"] = {
        "plain": stats["build_ring_beta"]["median"] / stats["build_recipe"]["median"],
        "nt": stats["build_ring_beta_nt"]["median"] / stats["build_recipe_nt"]["median"]}
    par["nt_over_plain_median"] = {k: stats[k + "_nt"]["median"] / stats[k]["median"]
                                   for k in ("generate", "build_recipe", "build_ring_beta")}
    par["checksums_equal_for_both_store_flavours"] = all(len(set(v)) == 1 for v in checks.values())
    res["parity"] = par

    # ---- 2. the host route -------------------------------------------------------------------------
    h = abnn_amd.CONFIGS[args.host_config]
    hspec = graph.recipe(h.n_input, h.n_output, h.n_hidden, h.n_syn, seed=1)
    with abnn_amd.Brain(h.n_input, h.n_output, h.n_hidden, h.n_syn, h.events) as b:
        def host_route():
            b.upload_synapses(graph.reference(hspec))

        hrows, hstats = _alternate({"reference_plus_upload": host_route, "build_graph": lambda: b.build_graph(hspec)},
                                   min(args.reps, 3))
        host_sum = (host_route(), b.checksum())[1]
        b.build_graph(hspec)
        dev_sum = b.checksum()
    res["host_route"] = {"config": h.name, "n_syn": h.n_syn, "n_neuron": h.n_neuron,
                         "unit": "ms end to end (host clock)", "alternations": hrows, **hstats,
                         "speedup_median": hstats["reference_plus_upload"]["median"] / hstats["build_graph"]["median"],
                         "same_checksum": host_sum == dev_sum}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    s = stats
    print(f"| graph builder ({w.name}, {w.n_syn:,} records) | generate {s['generate']['median']:.2f} ms "
          f"| build_graph(recipe) {s['build_recipe']['median']:.2f} ms "
          f"({par['write_TBps_median']['build_recipe']:.2f} TB/s) "
          f"| small-world k=200 Beta(2,8) {s['build_ring_beta']['median']:.2f} ms |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
