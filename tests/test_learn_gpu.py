"""The device-resident learning loop (abnn.h abnn_engine_*, learn.hip) on the GPU.

C++: abnn::DeviceBrainEngine on the GPU brain against the host driver
BrainEngine<OracleBrain> on the CPU oracle (tests/cpp/learn_test.cpp), bit for
bit: every pass's outputs and normalised rates, loss / reward at every call
boundary, the final weights, lastFired, scalars and driver state; the GPU side
runs uneven chunks with no synchronise between the calls.
Python: LearnEngine, one call against two, and the error returns."""
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
    xin, xex = _stimulus(60)
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
