"""bench.py: the sample --dump-outputs takes, and one plain run at config 2
whose dumped arrays are the state an in-process Brain holds after the same
passes (settle + warm-up + timed), with none of the --full extras in the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _covered(chunks):
    return np.concatenate([np.arange(a, a + n) for a, n in chunks]) if chunks else np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize("span", [0, 1, 65_535, 65_536, 65_537, 65_536 + 30 * 32_768,
                                  65_536 + 30 * 32_768 + 1, 10_000_000, 4_000_000_000])
def test_dump_chunks_are_a_fixed_sample_inside_the_span(span):
    chunks = bench.dump_chunks(span)
    assert chunks == bench.dump_chunks(span)  # the same sample every time
    idx = _covered(chunks)
    assert idx.size == np.unique(idx).size  # no record twice
    assert np.all(np.diff(idx) > 0)  # in record order
    whole = min(span, 65_536 + 30 * 32_768)
    if span <= whole:
        assert np.array_equal(idx, np.arange(span))  # a small span is dumped whole
    else:
        assert np.array_equal(idx[:65_536], np.arange(65_536))  # the dense block always
        assert idx[-1] < span and 65_536 < idx.size <= whole
        assert 20 * idx.size <= 21_000_000  # src + dst as f64, w as f32: 20 B per record in the files


def test_dump_neurons_whole_or_fixed_sample():
    v = np.arange(1000, dtype=np.uint64) * 3
    assert np.array_equal(bench.dump_neurons(v), v.astype(np.float64))
    big = np.arange(bench.DUMP_NEURONS + 7, dtype=np.uint32)
    s = bench.dump_neurons(big)
    assert s.dtype == np.float64 and s.size == bench.DUMP_NEURONS
    assert np.all(np.diff(s) > 0) and np.array_equal(s, bench.dump_neurons(big))


@pytest.mark.gpu
def test_plain_run_dumps_the_state_after_its_last_step(gpu, tmp_path):
    import abnn_amd

    steps, warmup = 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                        "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["ms_per_step"] > 0 and out["unit"] == "events/s" and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(out["config"]["visited_events_per_pass_per_gpu"] / (out["ms_per_step"] * 1e-3))
    # what takes runs of its own is behind --full
    assert out["cpu_baseline"] is None and out["reference_layout"] is None
    assert "sampled_launches" not in out["roofline"] and "steady" not in out["roofline"]

    wl = abnn_amd.CONFIGS["c2"]
    g = abnn_amd.Brain(wl.n_input, wl.n_output, wl.n_hidden, wl.n_syn, wl.events, device=gpu)
    g.build_random_graph(1)
    g.set_auto_stimulus(0, wl.n_input)
    g.encode_traversal(bench.SETTLE_PASSES + warmup)
    g.synchronize()
    g.reset_stats()
    g.encode_traversal(steps)
    g.synchronize()
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["last_fired", "outputs", "scalars", "stats", "synapse_checksum", "synapse_dst",
                           "synapse_src", "synapse_w"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64_000_000
    assert np.array_equal(got["last_fired"], g.last_fired().astype(np.float64))
    syn = np.concatenate([g.download_synapses(a, n) for a, n in bench.dump_chunks(g.visited_events())])
    assert np.array_equal(got["synapse_w"].view(np.uint32), syn["w"].view(np.uint32))
    assert np.array_equal(got["synapse_src"], syn["src"]) and np.array_equal(got["synapse_dst"], syn["dst"])
    ck = sum(int(w) << s for w, s in zip(got["synapse_checksum"], (48, 32, 16, 0)))
    assert ck == g.checksum()
    assert np.array_equal(got["outputs"], g.read_outputs().astype(np.float32))
    sc, st = g.scalars(), g.stats()
    assert got["scalars"].tolist() == [sc["clock"], sc["reward"], sc["rbar"], sc["pass_index"], g.budget()]
    assert got["stats"].tolist() == [st[k] for k in sorted(st)]
    assert st["passes"] == steps
