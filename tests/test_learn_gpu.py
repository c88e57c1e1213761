"""The device-resident learning loop (abnn.h abnn_engine_*, learn.hip) on the GPU.

C++: abnn::DeviceBrainEngine on the GPU brain against the host driver
BrainEngine<OracleBrain> on the CPU oracle (tests/cpp/learn_test.cpp), bit for
bit: every pass's outputs and normalised rates, loss / reward at every call
boundary, the final weights, lastFired, scalars and driver state; the GPU side
runs uneven chunks with no synchronise between the calls.
Python: LearnEngine, one call against two, the error returns, and the census
inside the loop across structural updates."""
import json
import subprocess

import numpy as np
import pytest

from abnn_amd.build import build_learn_test
from test_engine import F32, _libm


def _run_case(case):
    prog = build_learn_test()
    r = subprocess.run([prog, str(case)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    return res


@pytest.mark.gpu
def test_config1_matches_the_host_driver(gpu):
    res = _run_case(1)
    assert res["passes"] == 300 and res["windows"] == 6
    assert res["spikes"] > 0 and res["teacher_stamps"] > 0 and res["reward_changes"] > 0


@pytest.mark.gpu
def test_odd_sizes_with_renormalisation(gpu):
    res = _run_case(2)
    assert res["passes"] == 130 and res["windows"] == 3
    assert res["renorms_gpu"] >= 1 and res["renorms_gpu"] == res["renorms_cpu"]
    assert res["spikes"] > 0


@pytest.mark.gpu
def test_without_the_fir(gpu):
    res = _run_case(3)
    assert res["passes"] == 90 and res["windows"] == 3 and res["spikes"] > 0


@pytest.mark.gpu
def test_more_than_one_gate_workgroup(gpu):
    res = _run_case(4)
    assert res["passes"] == 60 and res["windows"] == 2 and res["spikes"] > 0


@pytest.mark.gpu
def test_hand_back_to_the_host_paths(gpu):
    res = _run_case(5)
    assert res["passes"] == 40 and res["spikes"] > 0


@pytest.mark.gpu
def test_clock_inc_2_window_pre_7(gpu):
    """Off the default knobs (clock_inc = 2, window_pre = 7, tick_ns = 500,
    w_max = 2, renormalisation every ~25 passes).  With the clock skipping,
    read_outputs' window [now - 1, now) holds no stamp: what is asserted is
    that the device loop and the host driver agree on that (the program's
    bit-for-bit comparison), not that the trace holds spikes."""
    res = _run_case(6)
    assert res["passes"] == 120 and res["windows"] == 4
    assert res["teacher_stamps"] > 0
    assert res["renorms_gpu"] == res["renorms_cpu"] and res["renorms_cpu"] >= 1


@pytest.mark.gpu
def test_window_pre_1_with_a_large_reward_term(gpu):
    res = _run_case(7)
    assert res["passes"] == 120 and res["windows"] == 4
    assert res["spikes"] > 0 and res["reward_changes"] > 0 and res["teacher_stamps"] > 0
    assert res["renorms_gpu"] == res["renorms_cpu"] and res["renorms_cpu"] >= 1


@pytest.mark.gpu
def test_structural_updates_inside_the_loop(gpu):
    """Pruning and synaptogenesis on, an update after every 7th pass: 17 updates
    in 120 passes, in the middle of the 7-, 64- and 48-pass calls (the update's
    synchronising host part runs inside abnn_engine_run).  The program's
    bit-for-bit comparison covers n_syn and the pruned / grown counts."""
    res = _run_case(8)
    assert res["passes"] == 120 and res["windows"] == 4 and res["spikes"] > 0
    assert res["structural_updates"] == 17
    assert res["pruned"] > 0 and res["grown"] > 0


def _stimulus(frames, n_in=256, n_out=256, dt=0.0009, hz=0.5):
    """FunctionalDataset's frames (functional-dataset.cpp:24-52) as test_engine._frames
    makes them, vectorised: cos^2 input, 0.5 sin + 0.5 target, libm's cosf / sinf."""
    two_pi = 2.0 * 3.14159265358979323846
    xin, xex = np.empty((frames, n_in), F32), np.empty((frames, n_out), F32)
    phase = 0.0
    for f in range(frames):
        phase += hz * dt
        if phase > 1.0:
            phase -= 1.0
        for i in range(n_in):
            c = F32(_libm.cosf(F32(two_pi * (i / n_in + phase))))
            xin[f, i] = F32(c * c)
        for i in range(n_out):
            xex[f, i] = F32(F32(0.5) * F32(_libm.sinf(F32(two_pi * (i / n_out + phase)))) + F32(0.5))
    return xin, xex


@pytest.fixture(scope="module")
def stimulus():
    xin, xex = _stimulus(120)
    xin.setflags(write=False)
    xex.setflags(write=False)
    return xin, xex


def _brain():
    import abnn_amd

    b = abnn_amd.Brain(256, 256, 488, 10_000, 100_000)  # config 1
    b.build_random_graph(1)
    return b


@pytest.mark.gpu
def test_python_one_call_equals_two(gpu, stimulus):
    import abnn_amd

    xin, xex = stimulus
    got = []
    for split in ((60,), (30, 30)):
        b = _brain()
        with abnn_amd.LearnEngine(b, win_size=25) as e:
            at = 0
            for n in split:
                assert e.run(xin[at:at + n], xex[at:at + n]) == n
                at += n
            out, smooth = e.trace(0, 60)
            st, rates = e.state(), e.rates()
        got.append((b.checksum(), b.scalars(), b.last_fired(), out, smooth, st, rates))
        b.close()
    a, c = got
    assert a[0] == c[0] and a[1] == c[1] and np.array_equal(a[2], c[2])
    assert np.array_equal(a[3], c[3]) and np.array_equal(a[4].view(np.uint32), c[4].view(np.uint32))
    assert a[5] == c[5]
    for k in ("rate", "smooth", "spike_window"):
        assert np.array_equal(a[6][k].view(np.uint32), c[6][k].view(np.uint32)), k
    assert a[5]["step"] == 60 and a[5]["windows"] == 2 and a[5]["win_pos"] == 10 and a[5]["teach"] == 0
    assert a[3].sum() > 0 and np.array_equal(a[6]["smooth"], a[4][59])
    assert a[1]["clock"] == 60


@pytest.mark.gpu
def test_python_error_returns(gpu, stimulus):
    import abnn_amd

    xin, xex = stimulus
    b = _brain()
    with abnn_amd.LearnEngine(b, trace_passes=8, win_size=5) as e:
        with pytest.raises(abnn_amd.AbnnError) as err:
            e.run(xin[:9], xex[:9])  # passes > trace_passes
        assert err.value.status == 1
        assert e.state()["step"] == 0
        e.run(xin[:8], xex[:8])
        e.run(xin[8:12], xex[8:12])
        out, smooth = e.trace(4, 8)  # the last 8 of 12 steps are held, across the ring's wrap
        b2 = _brain()
        with abnn_amd.LearnEngine(b2, win_size=5) as e2:  # the same steps in a trace that holds them all
            e2.run(xin[:12], xex[:12])
            out2, smooth2 = e2.trace(4, 8)
        b2.close()
        assert np.array_equal(out, out2) and np.array_equal(smooth.view(np.uint32), smooth2.view(np.uint32))
        for first, n in ((3, 1), (0, 12), (12, 1), (5, 8)):  # evicted, evicted, not run yet, past the end
            with pytest.raises(abnn_amd.AbnnError) as err:
                e.trace(first, n)
            assert err.value.status == 1, (first, n)
    b.close()
    shard = abnn_amd.Brain(256, 256, 488, 10_000, 100_000, global_events=20_000)
    with pytest.raises(abnn_amd.AbnnError) as err:
        abnn_amd.LearnEngine(shard)
    assert err.value.status == 1
    shard.close()


def _plastic_brain():
    import abnn_amd

    b = abnn_amd.Brain(256, 256, 488, 10_000, 100_000, syn_capacity=12_000,  # config 1, learn_test case 8
                       w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=7)
    b.build_random_graph(1)
    return b


@pytest.mark.gpu
def test_python_census_follows_structural_updates(gpu, stimulus):
    """set_census(every=7) on a brain whose structural updates fall on the same
    steps: each census counts the records as the update of its step left them
    (live + tombstones = n_syn then), which a second handle stepped from the
    host one pass per call reports after every step; the last one, taken at
    the run's end, is Brain.census()."""
    import abnn_amd

    xin, xex = stimulus
    steps_total = 119  # 17 x 7: the last census closes the run
    b = _plastic_brain()
    with abnn_amd.LearnEngine(b, win_size=30) as e:
        e.set_census(16, 0.0, 1.0, every=7, capacity=32)
        at = 0
        for n in (1, 7, 64, 47):  # updates and censuses in the middle of the calls
            e.run(xin[at:at + n], xex[at:at + n])
            at += n
        assert at == steps_total and e.census_count() == 17
        steps, got = e.census_trace(0, 17)
        final = b.census(16, 0.0, 1.0)
    assert b.structural_updates() == 17

    h = _plastic_brain()
    sizes = []
    with abnn_amd.LearnEngine(h, win_size=30) as e:
        for k in range(steps_total):
            e.run(xin[k:k + 1], xex[k:k + 1])
            sizes.append(h.n_syn())  # host mirror, as the update of step k + 1 left it
    assert steps.tolist() == [7 * (i + 1) for i in range(17)]
    for s, c in zip(steps.tolist(), got):
        assert c["records"] == c["live"] + c["tombstones"] == sizes[s - 1], s
        assert c["tombstones"] == 0, s  # taken right after the update of its step
    assert len(set(sizes)) > 1 and b.n_syn() == h.n_syn() == sizes[-1]
    assert b.checksum() == h.checksum() and b.stats() == h.stats()
    st = b.stats()
    assert st["pruned"] > 0 and st["grown"] > 0
    last = got[-1]
    assert {k: v for k, v in last.items() if k not in ("counts", "edges")} == \
        {k: v for k, v in final.items() if k not in ("counts", "edges")}
    assert np.array_equal(last["counts"], final["counts"])
    b.close()
    h.close()
