#!/usr/bin/env python3
"""Device-side snapshots: capture, restore and the diff, timed.

At one config (default c3, the generated graph), in one process, after a
warm-up; every call is an enqueue (restore: the synchronous call) and one
synchronise, under the host clock, alternated `--reps` times:
  capture            abnn_snapshot_capture_enqueue
  plain_memcpy       hipMemcpyAsync of the same bytes between two plain device buffers
  census             abnn_census_enqueue, 64 bins over [0, 1)         -- the yardstick: 8 B per record
  diff_handle        abnn_snapshot_diff_enqueue against the handle after `--passes` learning passes,
                     64 bins over [-0.05, 0.05)                        -- 22 B per record
  diff_snapshot      ... against a second snapshot of the same moment
  restore_records / restore_state / restore_both      abnn_snapshot_restore
Then, at the size of `--small` (default c2): Snapshot.diff against two
download_synapses() plus snapshot.reference, and restore("records") against
upload_synapses().  With `--parent-lib PATH` (the parent commit's library,
built apart): bench.py's pass time with that library and with this one,
interleaved `--bench-reps` times, to show the pass did not move.  Writes
profiles/snapshot_bench.json and prints it.  Needs a GPU.

    python tools/snapshot_bench.py [--config c3] [--small c2] [--reps 7] [--passes 1000] [--parent-lib PATH]
"""
import argparse
import ctypes as C
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


def _hip_runtime():
    """The HIP runtime already in the process (torch's copy when torch is installed)."""
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is not None and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            return C.CDLL(p)
    return C.CDLL("libamdhip64.so")


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
    ap.add_argument("--passes", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import Snapshot, census, snapshot
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("snapshot_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    wl = abnn_amd.CONFIGS[args.config]
    n, n_nrn = wl.n_syn, wl.n_neuron

    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    b.set_auto_stimulus(0, wl.n_input)
    b.encode_traversal(8)
    b.synchronize()
    then, now = Snapshot(b), Snapshot(b)
    pieces = [2 * n, n, 8 * n, 8 * n_nrn, 8 * n_nrn, 24]  # lo, hi, dw, lastFired, lastVisited, the scalar block
    total = sum(pieces)
    src = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    ccfg = census.config(64, 0.0, 1.0)
    cbuf = torch.zeros(census.CENSUS_HEADER_WORDS + 64, dtype=torch.int64, device="cuda:0")
    dcfg = snapshot.config(64, -0.05, 0.05)
    dbuf = torch.zeros(snapshot.n_words(dcfg), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def run_capture():
        then.capture()
        b.synchronize()

    def run_memcpy():
        at = 0
        for size in pieces:  # the capture's copies, piece for piece
            assert hip.hipMemcpyAsync(dst.data_ptr() + at, src.data_ptr() + at, size, 3, None) == 0
            at += size
        b.synchronize()

    def run_census():
        b.census_enqueue(ccfg, cbuf.data_ptr())
        b.synchronize()

    def run_diff(other=None):
        then.diff_enqueue(dcfg, dbuf.data_ptr(), now=other)
        b.synchronize()

    for fn in (run_capture, run_memcpy, run_census, run_diff):  # warm-up
        fn()
    rows = [{"capture": _timed(run_capture), "plain_memcpy": _timed(run_memcpy)} for _ in range(args.reps)]
    res = {"tool": "tools/snapshot_bench.py", "source_sha": kernel_source_sha(), "config": args.config, "workload": wl.note,
           "n_syn": n, "n_neuron": n_nrn, "reps": args.reps, "snapshot_bytes": then.info()["bytes"],
           "unit": "ms per call (host clock: an enqueue with preallocated device buffers, then one synchronise)",
           "capture": {"alternations": rows, "bytes": total, "ms": _stat([r["capture"] for r in rows]),
                       "plain_memcpy_ms": _stat([r["plain_memcpy"] for r in rows])}}
    res["capture"]["over_plain_memcpy"] = _stat([r["capture"] / r["plain_memcpy"] for r in rows])
    res["capture"]["bytes_read_plus_written_per_s"] = 2.0 * total / (res["capture"]["ms"]["median"] * 1e-3)
    del src, dst
    torch.cuda.empty_cache()

    # the diff after learning, against the census in the same alternations
    fired = b.stats()["fired"]
    b.encode_traversal(args.passes)
    b.synchronize()
    now.capture()
    b.synchronize()
    rows = []
    for _ in range(args.reps):
        rows.append({"census": _timed(run_census), "diff_handle": _timed(run_diff),
                     "census_2": _timed(run_census), "diff_snapshot": _timed(lambda: run_diff(now))})
    header = snapshot.decode(dbuf.cpu().numpy().view(np.uint64), dcfg)
    assert header["compared"] == n and header["changed"] > 0 and b.stats()["fired"] > fired
    counts = header.pop("counts")
    header.pop("edges")
    header["max_abs"] = float(header["max_abs"])
    header["bins_nonzero"] = int((counts > 0).sum())
    header["largest_bin_share"] = float(counts.max()) / max(1, int(counts.sum()))
    res["diff"] = {"learning_passes": args.passes, "alternations": rows, "header": header,
                   "census_ms": _stat([r[k] for r in rows for k in ("census", "census_2")]),
                   "diff_handle_ms": _stat([r["diff_handle"] for r in rows]),
                   "diff_snapshot_ms": _stat([r["diff_snapshot"] for r in rows]),
                   "diff_handle_over_census": _stat([r["diff_handle"] / r["census"] for r in rows]),
                   "diff_snapshot_over_census": _stat([r["diff_snapshot"] / r["census_2"] for r in rows]),
                   "byte_model_over_census": 22.0 / 8.0}
    res["diff"]["stream_bytes_per_s"] = 22.0 * n / (res["diff"]["diff_handle_ms"]["median"] * 1e-3)
    res["census_stream_bytes_per_s"] = 8.0 * n / (res["diff"]["census_ms"]["median"] * 1e-3)

    # restore: the parts and both (after each the handle is at the capture again: the copies cost the same)
    rows = []
    for _ in range(args.reps):
        rows.append({"restore_records": _timed(lambda: then.restore("records")),
                     "restore_state": _timed(lambda: then.restore("state")),
                     "restore_both": _timed(then.restore)})
    res["restore"] = {"alternations": rows, **{k + "_ms": _stat([r[k] for r in rows]) for k in rows[0]}}
    assert then.diff(8, -1.0, 1.0)["changed"] == 0
    then.close()
    now.close()
    b.close()
    del cbuf, dbuf

    # the host routes, at a size they can afford
    ws = abnn_amd.CONFIGS[args.small]
    with abnn_amd.Brain(ws.n_input, ws.n_output, ws.n_hidden, ws.n_syn, ws.events) as s:
        s.build_random_graph(1)
        s.set_auto_stimulus(0, ws.n_input)
        s.encode_traversal(8)
        scfg = snapshot.config(64, -0.05, 0.05)
        small = []
        for _ in range(args.small_reps):
            snap = s.snapshot()
            row = {"download_then": _timed(lambda: s.download_synapses())}
            a = s.download_synapses()
            s.encode_traversal(50)
            s.synchronize()
            got = {}
            row["snapshot_diff"] = _timed(lambda: got.update(d=snap.diff(64, -0.05, 0.05)))
            host = {}

            def host_route():
                host.update(d=snapshot.reference(a, s.download_synapses(), scfg))

            row["download_now_plus_numpy"] = _timed(host_route)
            row["two_downloads_plus_numpy"] = row["download_then"] + row["download_now_plus_numpy"]
            assert snapshot.to_words(got["d"]).tolist() == snapshot.to_words(host["d"]).tolist()
            row["restore_records"] = _timed(lambda: snap.restore("records"))
            row["upload_synapses"] = _timed(lambda: s.upload_synapses(a))
            snap.close()
            small.append(row)
    res["host_route"] = {"config": args.small, "n_syn": ws.n_syn, "unit": "ms per call (host clock)", "alternations": small,
                         **{k + "_ms": _stat([r[k] for r in small]) for k in small[0]}}
    res["host_route"]["diff_speedup"] = (res["host_route"]["two_downloads_plus_numpy_ms"]["median"]
                                         / res["host_route"]["snapshot_diff_ms"]["median"])
    res["host_route"]["restore_speedup"] = (res["host_route"]["upload_synapses_ms"]["median"]
                                            / res["host_route"]["restore_records_ms"]["median"])

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
