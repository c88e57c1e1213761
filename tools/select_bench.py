#!/usr/bin/env python3
"""The synapse select against the synapse census, which streams the same records.

At one config (default c3, the generated graph), in one process, after a
warm-up, each select below is alternated with the census `--reps` times; every
call is an enqueue into a device buffer allocated beforehand and one
synchronise, under the host clock:
  census   abnn_census_enqueue, 64 bins over [0, 1)       -- the yardstick: 8 B per record
  (a) dst = (256, 256)                                    -- sparse, no src stream: 65 536 matches
  (b) src = (0, 256)                                      -- sparse, with the src streams (11 B per record)
  (c) ANY over a 4096-neuron hidden window
  (d) weights [0.19, +inf)
  (e) every record, capacity n_syn where the device's free memory allows, else 250M
The synchronous abnn_census (the call profiles/census_bench.json times) is
alternated too.  Then (f), at the size of `--small` (default c2): Brain.select
(count, then select) against download_synapses() plus numpy for dst = (256, 256).
Every count is checked against the census of the same ranges.  Writes
profiles/select_bench.json and prints it.  Needs a GPU.

    python tools/select_bench.py [--config c3] [--small c2] [--reps 7] [--out profiles/select_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INF = float("inf")


def _stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--small", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import census, select
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("select_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    n = wl.n_syn
    first_hidden = wl.n_input + wl.n_output
    window = (first_hidden + (wl.n_neuron - first_hidden) // 2, 4096)

    ccfg = census.config(64, 0.0, 1.0)
    cbuf = torch.zeros(census.CENSUS_HEADER_WORDS + 64, dtype=torch.int64, device="cuda:0")
    kws = {
        "a_dst_256": dict(dst=(wl.n_input, wl.n_output)),
        "b_src_256": dict(src=(0, wl.n_input)),
        "c_any_hidden_window": dict(src=window, dst=window, any=True),
        "d_weights_from_0.19": dict(weights=(0.19, INF)),
        "e_every_record": dict(),
    }
    cfgs = {k: select.config(**kw) for k, kw in kws.items()}
    counts = {k: b.select(capacity=0, **kw) for k, kw in kws.items()}  # also allocates the handle's scratch
    caps = {k: counts[k]["matched"] for k in kws}
    free, _ = torch.cuda.mem_get_info(0)
    if 24 * n + (1 << 30) > free:
        caps["e_every_record"] = min(n, 250_000_000)
    bufs = {k: torch.empty(select.n_words(cfgs[k], caps[k]), dtype=torch.int64, device="cuda:0") for k in kws}
    torch.cuda.synchronize()

    def run_census():
        b.census_enqueue(ccfg, cbuf.data_ptr())
        b.synchronize()

    def run_select(k):
        b.select_enqueue(cfgs[k], caps[k], bufs[k].data_ptr())
        b.synchronize()

    for k in kws:  # warm-up
        run_census()
        run_select(k)
        run_select(k)
    reps = []
    for _ in range(args.reps):
        row = {"census_sync_call": _timed(lambda: b.census(64, 0.0, 1.0))}
        for k in kws:
            row["census_before_" + k] = _timed(run_census)
            row[k] = _timed(lambda: run_select(k))
        reps.append(row)

    res = {"tool": "tools/select_bench.py", "source_sha": kernel_source_sha(), "config": args.config,
           "workload": wl.note, "n_syn": n, "tile": select.TILE, "reps": args.reps,
           "unit": "ms per call (host clock: an enqueue into a preallocated device buffer, then one synchronise)",
           "alternations": reps, "census_sync_call": _stat([r["census_sync_call"] for r in reps])}
    every_census = [r["census_before_" + k] for r in reps for k in kws]
    res["census"] = _stat(every_census)
    for k, kw in kws.items():
        head = dict(zip(("records", "tombstones", "matched", "written"), bufs[k][:4].cpu().tolist()))
        sel = b.census(64, -1.0, 2.0, src=kw.get("src"), dst=kw.get("dst"))["selected"] if not (
            kw.get("any") or kw.get("weights")) else None
        assert head["records"] == n and head["matched"] == counts[k]["matched"], (k, head)
        assert head["written"] == min(head["matched"], caps[k]), (k, head)
        assert sel is None or sel == head["matched"], (k, sel, head)
        yard = [r["census_before_" + k] for r in reps]
        ratio = [r[k] / r["census_before_" + k] for r in reps]
        res[k] = {"config": {kk: list(v) if isinstance(v, tuple) else v for kk, v in kw.items()},
                  "matched": head["matched"], "capacity": caps[k], "written": head["written"],
                  "ms": _stat([r[k] for r in reps]), "census_ms": _stat(yard), "over_census": _stat(ratio),
                  "minus_census_us": _stat([(r[k] - r["census_before_" + k]) * 1e3 for r in reps])}
    a = res["a_dst_256"]
    assert a["matched"] == wl.n_input * wl.n_output, a
    # the first and the last written entry of the dense select are the brain's records
    e_cap = caps["e_every_record"]
    if e_cap:
        w = bufs["e_every_record"]
        idx = w[8:8 + e_cap][[0, e_cap - 1]].cpu().numpy().view(np.uint64)
        assert idx.tolist() == [0, e_cap - 1], idx
        for j, at in ((0, 0), (e_cap - 1, e_cap - 1)):
            rec = w[8 + e_cap + 2 * j:8 + e_cap + 2 * j + 2].cpu().numpy().view(np.uint32)
            assert np.array_equal(rec, b.download_synapses(at, 1).view(np.uint32)), at
    res["e_every_record"]["bytes_read_plus_written_per_s"] = \
        (8.0 * n + (8.0 * n if e_cap else 0) + 24.0 * e_cap) / (res["e_every_record"]["ms"]["median"] * 1e-3)
    res["a_dst_256"]["stream_bytes_per_s"] = 8.0 * n / (a["ms"]["median"] * 1e-3)
    del bufs, cbuf
    b.close()

    # (f) Brain.select against download_synapses() + numpy at a size the host route can afford
    ws = abnn_amd.CONFIGS[args.small]
    with abnn_amd.Brain(ws.n_input, ws.n_output, ws.n_hidden, ws.n_syn, ws.events) as s:
        s.build_random_graph(1)
        kw = dict(dst=(ws.n_input, ws.n_output))
        cfg = select.config(**kw)

        def host_route():
            syn = s.download_synapses()
            at = np.flatnonzero(select.matches(syn, cfg))
            return at, syn[at]

        got = s.select(**kw)  # warm-up
        at, rec = host_route()
        assert np.array_equal(got["index"], at.astype(np.uint64))
        assert np.array_equal(got["syn"].view(np.uint32), rec.view(np.uint32))
        small = [{"brain_select": _timed(lambda: s.select(**kw)), "download_numpy": _timed(host_route)}
                 for _ in range(args.small_reps)]
    res["f_host_route"] = {"config": args.small, "n_syn": ws.n_syn, "matched": int(got["matched"]),
                           "unit": "ms per call (host clock; Brain.select counts, then selects exactly the matches)",
                           "alternations": small, "brain_select_ms": _stat([r["brain_select"] for r in small]),
                           "download_numpy_ms": _stat([r["download_numpy"] for r in small])}
    res["f_host_route"]["speedup"] = (res["f_host_route"]["download_numpy_ms"]["median"]
                                      / res["f_host_route"]["brain_select_ms"]["median"])

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
