"""The GPU passes against fixtures made from the reference kernel's own text.

tests/golden/ref_case*.json are written by tests/golden/make_ref_golden.py
from `ref_pass`: the reference's kernel file compiled in place on the host
and run under schedule C1.  These tests read only those files
(and generate the graphs they name): neither the reference checkout nor
oracle/_ref/, and the oracle computes nothing here.  Every pass must
reproduce its record: SHA-256 of the 16-B records and of lastF mod 2^32, the
clock mod 2^32, the budget left, rBar's bits and a sample of weight bits.

* the buffer-index launcher (abnn_launch_traversal / abnn_launch_renormalise)
  in both pass kinds, on every case;
* the handle path (abnn_amd.Brain, the stimulus on all inputs) on the cases
  that start at clock 0: fused, two-kernel, and case 1 on the indexed pass."""
import numpy as np
import pytest

import ref_kernel_helpers as R

pytestmark = pytest.mark.gpu

RUNS = [(name, i) for name, c in R.CASES.items() for i in range(len(c["runs"]))]
HANDLE_CASES = ("case1", "case2", "case3a", "case3b", "case5", "case7")  # clock 0, no host renormalisation
HANDLE_RUNS = [(n, i) for n, i in RUNS if n in HANDLE_CASES]


def _ids(runs):
    return [f"{n}-{i}" for n, i in runs]


def _graph(g, run):
    syn = R.case_graph((g["n_hidden"], g["n_syn"], g["events"]), run["special"])
    assert len(syn) == g["n_syn"] and g["seed"] == 1
    return syn


class RawRunner:
    """tests/test_gpu_raw.py's caller-owned buffers behind the runner surface;
    the host's renormalisation decision on the clock read before the pass
    (brain.cpp:127-128)."""

    def __init__(self, g, run):
        from test_gpu_raw import RawBrain

        s = R.fixture_settings(run)
        self.r = r = RawBrain(_graph(g, run), 512 + g["n_hidden"], g["events"], s["max_spikes"])
        a = s["args"]
        r.args.a_ltp, r.args.a_ltd, r.args.w_min, r.args.w_max = a["a_ltp"], a["a_ltd"], a["w_min"], a["w_max"]
        r.set_clock(s["clock0"])
        self.renorm_thresh = s["renorm_thresh"]

    def set_reward(self, x):
        self.r.set_reward(x)

    def step(self):
        now = self.r.scalars()[0] if self.renorm_thresh != R.NEVER else 0
        self.r.one_pass()
        if now > self.renorm_thresh:
            self.r.renormalise()
        assert self.r.workspace_error() == 0

    def observe(self):
        clock, left, rbar = self.r.scalars()
        return self.r.records(), self.r.last_fired(), clock, left, R.f32_bits(rbar)


class HandleRunner:
    """abnn_amd.Brain with the stimulus on all inputs; the budget left is the
    budget less the pass's spikes (stats()["fired"])."""

    def __init__(self, g, run, fused=True):
        import abnn_amd

        s = R.fixture_settings(run)
        assert s["clock0"] == 0 and s["renorm_thresh"] == R.NEVER
        self.max_spikes = s["max_spikes"]
        self.b = b = abnn_amd.Brain(g["n_input"], g["n_output"], g["n_hidden"], g["n_syn"], g["events"],
                                    max_spikes=self.max_spikes, **s["args"])
        b.upload_synapses(_graph(g, run))
        b.set_auto_stimulus(*g["stimulus"])
        assert b._lib.abnn_debug_set_fused(b._h, int(fused)) == 0
        self.left = self.max_spikes

    def set_reward(self, x):
        self.b.set_reward(x)

    def step(self):
        before = self.b.stats()["fired"]
        self.b.encode_traversal(1)
        self.left = self.max_spikes - (self.b.stats()["fired"] - before)

    def observe(self):
        b = self.b
        sc = b.scalars()
        return (b.download_synapses().view(np.uint32).reshape(-1), (b.last_fired() & np.uint64(R.U32)).astype(np.uint32),
                sc["clock"] & R.U32, self.left, R.f32_bits(sc["rbar"]))


@pytest.mark.parametrize("kind", [0, 1], ids=["five_launches", "fused"])
@pytest.mark.parametrize("name,run", RUNS, ids=_ids(RUNS))
def test_raw_launcher_reproduces_reference_fixture(gpu, name, run, kind):
    from abnn_amd import _lib

    lib = _lib.load()
    g = R.load_fixture(name)
    assert lib.abnn_debug_raw_fused(kind) == 0
    try:
        R.check_against_fixture(RawRunner(g, g["runs"][run]), g["runs"][run], f"raw launcher (kind {kind}), {name} run {run}")
    finally:
        lib.abnn_debug_raw_fused(-1)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_kernel"])
@pytest.mark.parametrize("name,run", HANDLE_RUNS, ids=_ids(HANDLE_RUNS))
def test_handle_reproduces_reference_fixture(gpu, name, run, fused):
    g = R.load_fixture(name)
    R.check_against_fixture(HandleRunner(g, g["runs"][run], fused), g["runs"][run],
                            f"handle ({'fused' if fused else 'two-kernel'}), {name} run {run}")


def test_indexed_handle_reproduces_reference_fixture(gpu, monkeypatch):
    """Case 1 with every pass after the first on the indexed pass."""
    from test_gpu_indexed import index_state

    monkeypatch.setenv("ABNN_INDEXED", "2")
    monkeypatch.setenv("ABNN_INDEX_AFTER", "1")
    g = R.load_fixture("case1")
    h = HandleRunner(g, g["runs"][0])
    R.check_against_fixture(h, g["runs"][0], "handle (indexed), case1 run 0")
    st = index_state(h.b)
    assert st["built"] and st["indexed_passes"] == len(g["runs"][0]["passes"]) - 1, st
