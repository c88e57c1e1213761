#!/usr/bin/env python3
"""The synapse census against the library's other streaming reduction.

At one config (default c3, the generated graph), in one process, after a
warm-up, these are alternated `--reps` times:
  (a) abnn_checksum_synapses            -- the yardstick: 11 B per record
  (b) census, 64 bins over [0, 1)       -- 8 B per record
  (c) census, 4096 bins over [0, 1)
  (d) census, 64 bins, on a second brain whose weights all hold one value
      (uploaded through abnn_upload_synapses)
  (e) census, 64 bins, src = (0, 256)   -- 11 B per record, reported only
Host clock around calls that end in a synchronise.  (b), (c), (d) are gated:
each must be no slower than (a).  Then abnn_engine_run over `--passes` passes
with a census every `--every` steps against the census off (reported only).
Writes profiles/census_bench.json and prints it.  Needs a GPU.

    python tools/census_bench.py [--config c3] [--reps 7] [--out profiles/census_bench.json]
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


def _flat_brain(abnn_amd, wl, value, piece=1 << 24):
    """A brain of the workload's size whose weights all equal `value` (src and
    dst among the hidden neurons), uploaded piece by piece from one host buffer."""
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    rng = np.random.default_rng(7)
    lo = wl.n_input + wl.n_output if wl.n_hidden else 0
    buf = np.zeros(min(piece, wl.n_syn), dtype=abnn_amd.SYN_DTYPE)
    buf["src"] = rng.integers(lo, wl.n_neuron, len(buf), dtype=np.uint32)
    buf["dst"] = rng.integers(lo, wl.n_neuron, len(buf), dtype=np.uint32)
    buf["w"] = np.float32(value)
    for first in range(0, wl.n_syn, len(buf)):
        b.upload_synapses(buf[:min(len(buf), wl.n_syn - first)], first)
    return b


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=2000)
    ap.add_argument("--every", type=int, default=1000)
    ap.add_argument("--engine-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_bench.json"))
    args = ap.parse_args()

    import abnn_amd
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("census_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    wl = abnn_amd.CONFIGS[args.config]
    b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
    b.build_random_graph(1)
    flat = _flat_brain(abnn_amd, wl, 0.15)

    cases = {
        "a_checksum": b.checksum,
        "b_census_64": lambda: b.census(64, 0.0, 1.0),
        "c_census_4096": lambda: b.census(4096, 0.0, 1.0),
        "d_census_64_one_value": lambda: flat.census(64, 0.0, 1.0),
        "e_census_64_src_range": lambda: b.census(64, 0.0, 1.0, src=(0, 256)),
    }
    for fn in cases.values():  # warm-up
        fn()
        fn()
    reps = [{k: _timed(fn) for k, fn in cases.items()} for _ in range(args.reps)]
    one = flat.census(64, 0.0, 1.0)
    assert int(one["counts"].max()) == wl.n_syn == one["selected"], "the one-value brain is not one-valued"
    whole = b.census(64, 0.0, 1.0)
    assert whole["selected"] == wl.n_syn and whole["tombstones"] == 0

    res = {"tool": "tools/census_bench.py", "source_sha": kernel_source_sha(), "config": args.config,
           "workload": wl.note, "n_syn": wl.n_syn, "reps": args.reps,
           "unit": "ms per call (host clock, ends in a synchronise)", "alternations": reps}
    for k in cases:
        res[k] = _stat([r[k] for r in reps])
    yard = res["a_checksum"]["median"]
    res["gated"] = {k: {"median_over_checksum": res[k]["median"] / yard,
                        "no_slower_than_checksum_median": res[k]["median"] <= yard,
                        "no_slower_in_every_alternation": all(r[k] <= r["a_checksum"] for r in reps)}
                    for k in ("b_census_64", "c_census_4096", "d_census_64_one_value")}
    res["reported_only"] = {"e_census_64_src_range_over_checksum": res["e_census_64_src_range"]["median"] / yard}
    bps = 8.0 * wl.n_syn / (res["b_census_64"]["median"] * 1e-3)
    res["b_stream_bytes_per_s"] = bps
    res["b_share_of_8_TBps"] = bps / 8e12
    res["a_stream_bytes_per_s"] = 11.0 * wl.n_syn / (yard * 1e-3)
    flat.close()

    # the learning loop: per-pass time with a census every `every` steps against the census off
    rng = np.random.default_rng(3)
    xin = rng.uniform(0.0, 1.0, (args.passes, wl.n_input)).astype(np.float32)
    xex = rng.uniform(0.0, 1.0, (args.passes, wl.n_output)).astype(np.float32)
    with abnn_amd.LearnEngine(b, trace_passes=max(args.passes, 1)) as e:
        def run():
            e.run(xin, xex)
            e.state()  # synchronises

        run()  # warm-up
        loop = []
        for _ in range(args.engine_reps):
            row = {}
            e.set_census(None)
            row["off_us"] = _timed(run) * 1e3 / args.passes
            e.set_census(64, 0.0, 1.0, every=args.every, capacity=4)
            row["on_us"] = _timed(run) * 1e3 / args.passes
            row["censuses"] = e.census_count()
            loop.append(row)
    res["engine"] = {"passes_per_call": args.passes, "every": args.every, "alternations": loop,
                     "unit": "us per learning pass (host clock around abnn_engine_run + a synchronise)",
                     "off_us": _stat([r["off_us"] for r in loop]), "on_us": _stat([r["on_us"] for r in loop])}
    res["engine"]["on_minus_off_us_per_pass"] = res["engine"]["on_us"]["median"] - res["engine"]["off_us"]["median"]
    res["engine"]["expected_us_per_pass"] = (args.passes // args.every) * res["b_census_64"]["median"] * 1e3 / args.passes
    b.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
