#!/usr/bin/env python3
"""The synapse edit against the synapse census, which streams the same records.

At one config (default c3, the generated graph), in one process, after a
warm-up, each edit below is alternated with the census `--reps` times; every
call is an enqueue with device buffers allocated beforehand and one
synchronise, under the host clock:
  census   abnn_census_enqueue, 64 bins over [0, 1)   -- the yardstick: 8 B per record
  (a) SET on a weight band that holds nothing         -- an edit that matches nothing: a pure read
  (b) KILL dst = the outputs                          -- 65 536 records (last of each round: the graph is rebuilt after it)
  (c) AFFINE + CLAMP over w in [0.10, 0.11)           -- about 10 % of the records; w -> 0.21 - w stays in the band
  (d) AFFINE of every record, w -> w +- 2^-20         -- 8 B read and 8 B written per record
  (e) SCALE_DST over every neuron                     -- (d) plus the gather from a plane of N_NRN floats
  (f) AFFINE with src = the inputs                    -- sparse, with the src streams (11 B per record)
  (g) Brain.scale_inputs of the outputs, end to end   -- degree census + factors + SCALE_DST + one synchronise
Then the first abnn_traverse pass after (d) against the pass after it, with the
edit's stores non-temporal (the default) and plain (ABNN_EDIT_NT=0, a second
handle).  Then, at the size of `--small` (default c2): Brain.edit against
download_synapses() + edit.reference + upload_synapses() for (c).  Every header
is checked against the census of the same brain.  Writes profiles/edit_bench.json
and prints it.  Needs a GPU.

    python tools/edit_bench.py [--config c3] [--small c2] [--reps 7] [--out profiles/edit_bench.json]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--small", default="c2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.json"))
    args = ap.parse_args()

    import torch

    import abnn_amd
    from abnn_amd import census, edit
    from abnn_amd.build import build_hip, kernel_source_sha

    if abnn_amd.device_count() == 0:
        print("edit_bench needs a HIP device", file=sys.stderr)
        return 1
    build_hip()
    wl = abnn_amd.CONFIGS[args.config]
    n, n_nrn = wl.n_syn, wl.n_neuron
    outputs = (wl.n_input, wl.n_output)

    def make():
        b = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, wl.n_input)
        return b

    b = make()
    ccfg = census.config(64, 0.0, 1.0)
    cbuf = torch.zeros(census.CENSUS_HEADER_WORDS + 64, dtype=torch.int64, device="cuda:0")
    head = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    rng = np.random.default_rng(1)
    up = torch.from_numpy(rng.uniform(1.0, 1.25, n_nrn).astype(np.float32)).to("cuda:0")
    down = (1.0 / up).contiguous()  # alternated with `up`: the weights stay where they are, give or take a rounding
    band = dict(weights=(0.10, 0.11), a=-1.0, b=0.21, clamp=(0.0, 1.0))
    cfgs = {
        "a_no_match": edit.config("set", b=0.5, weights=(5.0, 6.0)),
        "c_affine_clamp_band": edit.config("affine", **band),
        "d_affine_every_record": edit.config("affine", a=1.0, b=2.0**-20),
        "e_scale_dst_every_neuron": edit.config("scale_dst"),
        "f_affine_src_inputs": edit.config("affine", src=(0, wl.n_input), a=-1.0, b=1.2),
        "b_kill_outputs": edit.config("kill", dst=outputs),  # the last: it removes what (f) and (g) match
    }
    d_back = edit.config("affine", a=1.0, b=-2.0**-20)  # alternated with (d): the weights stay where they are
    flip = [0, 0]

    def dense(h, out_ptr):
        h.edit_enqueue(cfgs["d_affine_every_record"] if flip[1] % 2 == 0 else d_back, None, out_ptr)
        flip[1] += 1
        h.synchronize()

    def run_census():
        b.census_enqueue(ccfg, cbuf.data_ptr())
        b.synchronize()

    def run_edit(k):
        plane = None
        if k.startswith("d_"):
            return dense(b, head.data_ptr())
        if k.startswith("e_"):
            plane = (up if flip[0] % 2 == 0 else down).data_ptr()
            flip[0] += 1
        b.edit_enqueue(cfgs[k], plane, head.data_ptr())
        b.synchronize()

    def run_scale_inputs():
        return b.scale_inputs(150.0, neurons=outputs)

    for k in cfgs:  # warm-up (an even number of each, so (e) ends where it began)
        run_census()
        if not k.startswith("b_"):
            run_edit(k)
            run_edit(k)
    run_scale_inputs()
    reps, heads = [], {}
    for _ in range(args.reps):
        row = {}
        for k in cfgs:
            if k.startswith("b_"):
                row["census_before_g_scale_inputs_outputs"] = _timed(run_census)
                row["g_scale_inputs_outputs"] = _timed(run_scale_inputs)
            row["census_before_" + k] = _timed(run_census)
            row[k] = _timed(lambda: run_edit(k))
            heads[k] = edit.decode(head.cpu().numpy().view(np.uint64))
        reps.append(row)
        tomb = b.census(4, 0.0, 1.0)["tombstones"]
        assert tomb == heads["b_kill_outputs"]["killed"], (tomb, heads)
        b.build_random_graph(1)  # the lesion's records back

    res = {"tool": "tools/edit_bench.py", "source_sha": kernel_source_sha(), "config": args.config, "workload": wl.note,
           "n_syn": n, "n_neuron": n_nrn, "reps": args.reps,
           "unit": "ms per call (host clock: an enqueue with preallocated device buffers, then one synchronise)",
           "alternations": reps}
    res["census"] = _stat([r[k] for r in reps for k in r if k.startswith("census_before_")])
    for k in list(cfgs) + ["g_scale_inputs_outputs"]:
        ratio = [r[k] / r["census_before_" + k] for r in reps]
        res[k] = {"ms": _stat([r[k] for r in reps]), "census_ms": _stat([r["census_before_" + k] for r in reps]),
                  "over_census": _stat(ratio)}
        if k in heads:
            res[k]["header"] = heads[k]
            assert heads[k]["records"] == n, (k, heads[k])
    assert heads["a_no_match"]["matched"] == 0 and heads["b_kill_outputs"]["killed"] == wl.n_input * wl.n_output
    assert heads["d_affine_every_record"]["changed"] > 0.99 * (n - heads["d_affine_every_record"]["tombstones"])
    assert 0 < heads["f_affine_src_inputs"]["matched"] <= wl.n_input * wl.n_output
    res["c_affine_clamp_band"]["matched_fraction"] = heads["c_affine_clamp_band"]["matched"] / n
    for k in ("d_affine_every_record", "e_scale_dst_every_neuron"):
        res[k]["bytes_read_plus_written_per_s"] = (8.0 * n + 8.0 * heads[k]["changed"]) / (res[k]["ms"]["median"] * 1e-3)
    res["a_no_match"]["stream_bytes_per_s"] = 8.0 * n / (res["a_no_match"]["ms"]["median"] * 1e-3)
    b.close()

    # the first pass after a dense edit against the pass after it, per store flavour
    def one_pass(h):
        h.encode_traversal(1)
        h.synchronize()

    res["pass_after_dense_edit"] = {"unit": "ms per abnn_traverse pass (host clock, one synchronise)"}
    for name, nt in (("nontemporal_stores", "1"), ("plain_stores", "0")):
        os.environ["ABNN_EDIT_NT"] = nt  # read when the handle is created
        h = make()
        h.encode_traversal(8)
        h.synchronize()
        rows = []
        for _ in range(args.reps):
            t_edit = _timed(lambda: dense(h, head.data_ptr()))
            rows.append({"dense_edit": t_edit, "first_pass": _timed(lambda: one_pass(h)), "next_pass": _timed(lambda: one_pass(h)),
                         "third_pass": _timed(lambda: one_pass(h))})
        res["pass_after_dense_edit"][name] = {
            "alternations": rows, **{k + "_ms": _stat([r[k] for r in rows]) for k in rows[0]}}
        h.close()
    os.environ.pop("ABNN_EDIT_NT", None)
    del cbuf, head, up, down

    # Brain.edit against download_synapses() + numpy + upload_synapses() at a size the host route can afford
    ws = abnn_amd.CONFIGS[args.small]
    with abnn_amd.Brain(ws.n_input, ws.n_output, ws.n_hidden, ws.n_syn, ws.events) as s:
        s.build_random_graph(1)
        cfg = edit.config("affine", **band)

        def host_route():
            syn = s.download_synapses()
            new, h = edit.reference(syn, cfg, s.n_neuron())
            s.upload_synapses(new)
            return h

        want = host_route()  # warm-up; the band maps onto itself, so every repetition matches as much
        small = []
        for _ in range(args.small_reps):
            row = {"download_numpy_upload": _timed(host_route)}
            row["brain_edit"] = _timed(lambda: s.edit("affine", **band))
            small.append(row)
        assert abs(s.edit("affine", **band)["matched"] - want["matched"]) < 0.01 * want["matched"] + 10
    res["host_route"] = {"config": args.small, "n_syn": ws.n_syn, "matched": want["matched"],
                         "unit": "ms per call (host clock)", "alternations": small,
                         "brain_edit_ms": _stat([r["brain_edit"] for r in small]),
                         "download_numpy_upload_ms": _stat([r["download_numpy_upload"] for r in small])}
    res["host_route"]["speedup"] = (res["host_route"]["download_numpy_upload_ms"]["median"]
                                    / res["host_route"]["brain_edit_ms"]["median"])

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
