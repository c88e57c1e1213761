#!/usr/bin/env python3
"""Population connectivity matrix (abnn_matrix_*): every kernel path against the
project's nearest streaming passes, the contention cases, and the routes it
replaces.

1. At one config (default c3, the generated graph), in one process, after a
   warm-up, these are alternated `--reps` times, each enqueued into a device
   buffer and timed on the host clock up to a synchronise:
     census_src_range     abnn_census_enqueue, 64 bins, a src range -- the yardstick: the
                          same 11 B per record
     census_nine          the nine range-restricted censuses (src range x dst range of
                          inputs / outputs / hidden) the P = 3 matrix replaces
     io_count_w           the built-in populations (matrix.io_bounds), COUNT | W: nearly
                          every record in ONE cell, run aggregation (the default path)
     io_all               ... with all three planes
     io_count_w_atomic    ... COUNT | W with one LDS atomic per record (aggregation off)
     io_count             ... COUNT alone: the scatter carries no 64-bit sum
     p1_count_w           one population over every neuron, COUNT | W: no bounds search at all
     p64_count_w          64 equal-width populations, COUNT | W: the cells spread
     p64_all              ... all three planes (two scans: the planes do not fit one LDS)
     p64_count_w_atomic   ... COUNT | W, aggregation off
     hops_packed          LABELS: the distance plane of a hops search from the inputs
                          (P = 8 layers), COUNT | W, through the packed byte plane
     hops_direct          ... gathering the u32 plane directly
     edit_scale_dst       abnn_edit SCALE_DST over every neuron: one f32 gather per record
                          from an N_NRN plane, the nearest measured neighbour of the gathers
2. The route this replaces, end to end at `--small` (default c2):
   download_synapses() + matrix.reference against Brain.matrix.
3. With `--parent-lib PATH` (the parent commit's library, built apart):
   bench.py's pass time with that library and with this one, interleaved
   `--bench-reps` times.
Writes profiles/matrix_bench.json (or --out) and prints it.  Needs a GPU.

    python tools/matrix_bench.py [--config c3] [--small c2] [--reps 7] [--parent-lib PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import _lib, census, edit, hops
    from abnn_amd import matrix as M
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("matrix_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    res = {"tool": "tools/matrix_bench.py", "source_sha": kernel_source_sha(), "reps": args.reps,
           "unit": "ms per call (host clock: enqueue into a device buffer, then a synchronise)"}

    # ---- 1. every path against the nearest streaming passes ----
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    n_nrn = wl.n_neuron
    dev = "cuda:0"
    io = M.io_bounds(wl.n_input, wl.n_output, wl.n_hidden)
    wide = (np.arange(65, dtype=np.uint64) * n_nrn // 64).astype(np.uint32)
    pops = [(int(io[j]), int(io[j + 1] - io[j])) for j in range(3)]
    ccfg = census.config(64, 0.0, 1.0, src=pops[2])
    nine = [census.config(64, 0.0, 1.0, src=s, dst=d) for s in pops for d in pops]
    couts = [torch.zeros(census.CENSUS_HEADER_WORDS + 64, dtype=torch.int64, device=dev) for _ in nine]
    hcfg = hops.config((0, wl.n_input), 6)
    hout = torch.zeros(hops.n_words(hcfg, n_nrn), dtype=torch.int64, device=dev)
    b.hops_enqueue(hcfg, hout.data_ptr())
    b.synchronize()
    layers_ptr = hout.data_ptr() + 8 * hops.plane_offset(hcfg)
    ecfg = edit.config("scale_dst")
    ehead = torch.zeros(8, dtype=torch.int64, device=dev)
    up = torch.from_numpy(np.random.default_rng(1).uniform(1.0, 1.25, n_nrn).astype(np.float32)).to(dev)
    down = (1.0 / up).contiguous()  # alternated with `up`: the weights stay where they are, give or take a rounding
    flip = [0]
    cw, every = ("count", "w"), ("count", "w", "p")
    mcfg = {"io_count_w": (M.config(3, cw), io, None, 0), "io_all": (M.config(3, every), io, None, 0),
            "io_count_w_atomic": (M.config(3, cw), io, None, 3),
            "io_count": (M.config(3, ("count",)), io, None, 0),
            "p1_count_w": (M.config(1, cw), np.array([0, n_nrn], dtype=np.uint32), None, 0),
            "p64_count_w": (M.config(64, cw), wide, None, 0), "p64_all": (M.config(64, every), wide, None, 0),
            "p64_count_w_atomic": (M.config(64, cw), wide, None, 3),
            "hops_packed": (M.config(8, cw, labels=True), None, layers_ptr, 1),
            "hops_direct": (M.config(8, cw, labels=True), None, layers_ptr, 2)}
    mout = torch.zeros(M.n_words(M.config(64, every)), dtype=torch.int64, device=dev)

    def leg(fn):
        def run():
            fn()
            b.synchronize()
        return run

    def mat(name):
        cfg, bounds, labels_ptr, path = mcfg[name]

        def run():
            _lib.call("abnn_debug_set_matrix_path", b._h, path)
            b.matrix_enqueue(cfg, mout.data_ptr(), bounds=bounds, labels_ptr=labels_ptr)
            b.synchronize()
        return run

    def run_nine():
        for c, o in zip(nine, couts):
            b.census_enqueue(c, o.data_ptr())
        b.synchronize()

    def run_edit():
        b.edit_enqueue(ecfg, (up if flip[0] % 2 == 0 else down).data_ptr(), ehead.data_ptr())
        flip[0] += 1
        b.synchronize()

    b.matrix(labels=hout[hops.plane_offset(hcfg):].view(torch.int32), pops=8)  # the first LABELS call allocates the scratch
    cases = {"census_src_range": leg(lambda: b.census_enqueue(ccfg, couts[0].data_ptr())), "census_nine": run_nine,
             **{k: mat(k) for k in mcfg}, "edit_scale_dst": run_edit}
    torch.cuda.synchronize()
    rows, stats = _alternate(cases, args.reps)
    found, partitions = {}, {}
    ramp = lambda n: np.arange(1, n + 1, dtype=np.uint64)  # noqa: E731
    for name, (cfg, _, _, _) in mcfg.items():
        mat(name)()
        d = M.decode(mout[:M.n_words(cfg)].cpu().numpy().view(np.uint64), cfg)
        part = name.split("_")[0]  # io / p64 / hops: the header and the sizes are recorded once per partition
        head = [int(d[k]) for k in M._HEAD_KEYS]
        partitions.setdefault(part, {"header": head, "sizes": [int(x) for x in d["sizes"]]})
        assert partitions[part]["header"][:7] == head[:7] and partitions[part]["sizes"] == [int(x) for x in d["sizes"]]
        found[name] = {"counted": d["counted"], "count_max_cell_share": float(d["count"].max() / max(1, d["counted"])),
                       "count_crc": int(np.bitwise_xor.reduce(d["count"].reshape(-1) * ramp(cfg.pops ** 2))),
                       "w_crc": int(np.bitwise_xor.reduce(d["w"].view(np.uint64).reshape(-1) * ramp(cfg.pops ** 2))) if "w" in d else None}
    for x, y in (("io_count_w", "io_count_w_atomic"), ("p64_count_w", "p64_count_w_atomic"), ("hops_packed", "hops_direct")):
        assert found[x] == found[y], f"the paths disagree: {x} / {y}"
    cen = [census.decode(o.cpu().numpy().view(np.uint64), c) for c, o in zip(nine, couts)]
    mat("io_count_w")()
    d = M.decode(mout[:M.n_words(mcfg["io_count_w"][0])].cpu().numpy().view(np.uint64), mcfg["io_count_w"][0])
    assert [c["selected"] for c in cen] == [int(x) for x in d["count"].reshape(-1)], "the nine censuses disagree with the matrix"
    floor = stats["census_src_range"]["median"]
    res["calls"] = {"config": args.config, "workload": wl.note, "n_syn": wl.n_syn, "n_neuron": n_nrn,
                    "hops_layers": partitions["hops"]["sizes"],
                    "alternations": rows, **stats, "partitions": partitions, "found": found,
                    "over_census_src_range_median": {k: stats[k]["median"] / floor for k in cases if k != "census_src_range"},
                    "nine_censuses_over_io_count_w": stats["census_nine"]["median"] / stats["io_count_w"]["median"],
                    "atomic_over_runs_one_cell": stats["io_count_w_atomic"]["median"] / stats["io_count_w"]["median"],
                    "atomic_over_runs_spread_cells": stats["p64_count_w_atomic"]["median"] / stats["p64_count_w"]["median"],
                    "direct_over_packed": stats["hops_direct"]["median"] / stats["hops_packed"]["median"],
                    "packed_over_edit_scale_dst": stats["hops_packed"]["median"] / stats["edit_scale_dst"]["median"]}
    _lib.call("abnn_debug_set_matrix_path", b._h, 0)
    b.close()
    del mout, hout, up, down

    # ---- 2. the route this replaces ----
    sw = abnn_amd.CONFIGS[args.small]
    b = abnn_amd.Brain(sw.n_input, sw.n_output, sw.n_hidden, sw.n_syn, sw.events)
    b.build_random_graph(1)
    sio = M.io_bounds(sw.n_input, sw.n_output, sw.n_hidden)
    scfg = M.config(3, every)
    got = {}

    def host_route():
        got["host"] = M.reference(b.download_synapses(), scfg, sw.n_neuron, b.params.base_scale, bounds=sio)

    def device_route():
        got["device"] = b.matrix(what=every)

    rows, stats = _alternate({"download_plus_numpy": host_route, "brain_matrix": device_route}, args.small_reps)
    assert np.array_equal(M.to_words(got["host"]), M.to_words(got["device"]))
    b.close()
    res["host_route"] = {"config": args.small, "n_syn": sw.n_syn, "n_neuron": sw.n_neuron,
                         "unit": "ms end to end (host clock; Brain.matrix includes the result's copy)",
                         "alternations": rows, **stats,
                         "speedup_median": stats["download_plus_numpy"]["median"] / stats["brain_matrix"]["median"]}

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
