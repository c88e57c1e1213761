"""Helpers of the tests that pin the oracle and the GPU passes to the reference
kernel's own text (tests/test_reference_kernel.py, tests/test_gpu_reference_golden.py,
tests/golden/make_ref_golden.py).

`oracle/_ref/libref_kernel.so` is the reference's kernel file compiled in
place as host C++ (oracle/ref_recipe/, abnn_amd/build.py: build_reference);
`ref_pass` runs one dispatch of it under schedule C1.  The host side of a
pass restates Brain::encode_traversal (brain.cpp:87-141), as
tests/test_gpu_raw.py does: every input stamped `now` (inject_inputs with
every input firing, brain.cpp:82), the budget reset (brain.cpp:90), one
dispatch, and the renormalisation dispatch where the clock read before the
pass exceeds the threshold (brain.cpp:127-128).

Runners: one pass-by-pass surface over the compiled reference kernel (`RefRunner`)
and the oracle (`OracleRunner`); the GPU file adds the launcher's and the
handle's.  `observe()` gives the state in the reference's layouts: the records
as u32 words, lastF mod 2^32, the clock mod 2^32, the budget left, rBar's
bits.  `fixture()` turns a runner's passes into the per-pass records of
tests/golden/ref_case*.json.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os

import numpy as np

import knob_helpers as K

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
U32 = 0xFFFFFFFF
NEVER = 2**64 - 1  # a renormalisation threshold no clock exceeds

# the kernel's buffer arguments as Brain::encode_traversal binds them
# (constants.h:16-19, brain.cpp:106-110) and the budget (brain.h:18)
ARGS = dict(a_ltp=0.04, a_ltd=0.02, w_min=0.001, w_max=1.0)
MAX_SPIKES = 2560

# ---- the cases (shape = n_hidden, n_syn, events over 256 + 256 + n_hidden neurons) --------------
# run keys: max_spikes, args (buffer arguments off the defaults), reward_from (reward 0.5 from that
# pass on), clock0, renorm_thresh (the host's, on the pass-start clock), special (knob_helpers'
# special weights on every third record)
_BUDGET = (9_488, 200_000, 150_000)
_ARGS_A = dict(a_ltp=0.08, w_min=0.05)
_ARGS_B = dict(w_min=0.0, w_max=2.0)
CASES = {
    # BASELINE configs[0]; events > n_syn
    "case1": dict(shape=(488, 10_000, 100_000), passes=40, runs=[dict(reward_from=15)]),
    "case2": dict(shape=_BUDGET, passes=8, runs=[dict(max_spikes=37), dict(max_spikes=0), dict(max_spikes=1)]),
    # events not a multiple of 256 (the grid rounds up, brain.cpp:116-118); 3b: fewer records than the grid
    "case3a": dict(shape=(9_488, 100_000, 54_321), passes=8, runs=[{}]),
    "case3b": dict(shape=(9_488, 3_000, 4_097), passes=8, runs=[{}]),
    # the u32 clock wraps mid-run (brain.metal:45)
    "case4": dict(shape=(9_488, 100_000, 100_000), passes=8, runs=[dict(clock0=2**32 - 4)]),
    # NaN, +-inf, 0, subnormal, negative and above-1 weights
    "case5": dict(shape=K.RAW, passes=8, runs=[dict(special=True, reward_from=4)]),
    # the clock read before pass 6 is 3 999 996: the first above the threshold, so renormalise_clock_and_times
    # runs after that pass's dispatch
    "case6": dict(shape=(9_488, 100_000, 100_000), passes=10, runs=[dict(clock0=3_999_990, renorm_thresh=3_999_995)]),
    # the aLTP / aLTD / wMin / wMax buffer arguments off the defaults, at case 2's budget and at the default one
    "case7": dict(shape=_BUDGET, passes=8, runs=[dict(max_spikes=37, args=_ARGS_A), dict(max_spikes=37, args=_ARGS_B),
                                                  dict(args=_ARGS_A), dict(args=_ARGS_B)]),
}
EXEMPT_FROM_BUSY = {("case2", 1)}  # budget 0: nothing is updated


def run_settings(run: dict) -> dict:
    """A run of CASES with every key present."""
    return dict(max_spikes=run.get("max_spikes", MAX_SPIKES), args={**ARGS, **run.get("args", {})},
                reward_from=run.get("reward_from"), clock0=run.get("clock0", 0),
                renorm_thresh=run.get("renorm_thresh", NEVER), special=bool(run.get("special", False)))


def case_graph(shape, special=False):
    """The generated graph of seed 1 over 512 + n_hidden neurons (as tests/test_gpu_raw.py)."""
    return K.graph(shape, seed=1, special=special)


def f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


# ---- the compiled reference kernel --------------------------------------------------------------
_ref = None


def ref_available() -> bool:
    """A reference checkout to compile, or binaries from an earlier build."""
    from abnn_amd import build as B

    return B.reference_dir() is not None or B.built_reference() is not None


def ref_lib() -> C.CDLL:
    """libref_kernel.so, (re)built where the checkout is present: a failed
    build raises (a test failure, never a skip)."""
    global _ref
    if _ref is None:
        from abnn_amd.build import build_reference

        built = build_reference()
        assert built is not None, "no reference checkout (ABNN_REFERENCE_DIR) and no oracle/_ref/"
        lib = C.CDLL(built[0])
        f, u32, vp = C.c_float, C.c_uint32, C.c_void_p
        lib.ref_pass.restype, lib.ref_pass.argtypes = None, [vp, vp, u32, vp, u32, u32, f, f, f, f]
        lib.ref_renormalise.restype, lib.ref_renormalise.argtypes = None, [vp, vp, u32]
        _ref = lib
    return _ref


class RefRunner:
    """The reference kernel's buffers on the host and Brain::encode_traversal's host side."""

    def __init__(self, syn, n_nrn, events, *, max_spikes=MAX_SPIKES, args=ARGS, clock0=0, renorm_thresh=NEVER,
                 stim=256, last_fired0=None, reward=0.0):
        from oracle import oracle as O

        self.lib = ref_lib()
        self.syn = np.ascontiguousarray(syn, dtype=O.SYN_DTYPE).copy()
        self.lastF = np.zeros(n_nrn, np.uint32) if last_fired0 is None else np.asarray(last_fired0, np.uint32).copy()
        self.scal = np.zeros(4, np.uint32)  # clock, budget, reward, rBar
        self.scal[0] = clock0 & U32
        self.scal[1] = max_spikes  # brain.cpp:66
        self.events, self.max_spikes, self.args, self.renorm_thresh, self.stim = events, max_spikes, args, renorm_thresh, stim
        self.set_reward(reward)

    def set_reward(self, r):
        self.scal[2] = f32_bits(r)

    def step(self):
        now = int(self.scal[0])
        self.lastF[:self.stim] = now  # brain.cpp:82
        self.scal[1] = self.max_spikes  # brain.cpp:90
        a = self.args
        self.lib.ref_pass(self.syn.ctypes.data, self.lastF.ctypes.data, self.lastF.shape[0], self.scal.ctypes.data,
                          self.syn.shape[0], self.events, a["a_ltp"], a["a_ltd"], a["w_min"], a["w_max"])
        if now > self.renorm_thresh:  # brain.cpp:127-128: `now` was read before the dispatch ran
            self.lib.ref_renormalise(self.lastF.ctypes.data, self.scal.ctypes.data, self.lastF.shape[0])

    def observe(self):
        return self.syn.view(np.uint32), self.lastF, int(self.scal[0]), int(self.scal[1]), int(self.scal[3])


class OracleRunner:
    """oracle_pass_serial driven as tests/test_gpu_raw.py drives it: inputs stamped `now` before each pass."""

    def __init__(self, syn, n_nrn, events, *, max_spikes=MAX_SPIKES, args=ARGS, clock0=0, renorm_thresh=NEVER,
                 stim=256, last_fired0=None, reward=0.0, dims=None):
        from oracle import oracle as O

        n_in, n_out = dims if dims is not None else (256, 256)
        self.o = o = O.OracleBrain(n_in, n_out, n_nrn - n_in - n_out, len(syn), events, max_spikes=max_spikes,
                                   renorm_thresh=renorm_thresh, **args)
        o.set_synapses(np.ascontiguousarray(syn, dtype=O.SYN_DTYPE))
        if last_fired0 is not None:
            o.last_fired[:] = np.asarray(last_fired0, np.uint32)
        o.set_scalars(clock0, reward, 0.0)
        self.max_spikes, self.stim, self.left = max_spikes, stim, max_spikes

    def set_reward(self, r):
        self.o.set_reward(r)

    def step(self):
        o = self.o
        o.set_timestamps(range(self.stim), o.clock)
        before = o.stats()["fired"]
        o.pass_serial()
        self.left = self.max_spikes - (o.stats()["fired"] - before)

    def observe(self):
        o = self.o
        return (o.syn.view(np.uint32), (o.last_fired & np.uint64(U32)).astype(np.uint32), o.clock & U32, self.left,
                f32_bits(o.s.rbar))


def case_runner(cls, name, run_index, **extra):
    """A runner of class `cls` on one run of a case, and the run's settings."""
    c = CASES[name]
    s = run_settings(c["runs"][run_index])
    n_hidden, _, events = c["shape"]
    r = cls(case_graph(c["shape"], s["special"]), 512 + n_hidden, events, max_spikes=s["max_spikes"], args=s["args"],
            clock0=s["clock0"], renorm_thresh=s["renorm_thresh"], **extra)
    return r, s


def first_difference(got, want) -> str | None:
    """None if two observations are equal on every word, else where they first differ."""
    names = ("record word", "lastF", "clock", "budget left", "rBar bits")
    for name, g, w in zip(names, got, want):
        if isinstance(w, np.ndarray):
            if g.shape != w.shape:
                return f"{name}: {g.shape} against {w.shape} words"
            d = np.flatnonzero(g != w)
            if d.size:
                i = int(d[0])
                at = f"record {i // 4} word {i % 4}" if name == "record word" else f"{name}[{i}]"
                return f"{at}: {int(g[i]):#010x} != {int(w[i]):#010x} ({d.size} words differ)"
        elif g != w:
            return f"{name}: {g:#x} != {w:#x}"
    return None


# ---- fixtures -----------------------------------------------------------------------------------
PASS_SAMPLE = 8  # weights sampled after every pass; FINAL_SAMPLE after the last
FINAL_SAMPLE = 97


def _sample_index(n_syn, k):
    return np.unique(np.linspace(0, n_syn - 1, k).astype(np.int64))


def pass_record(k, obs, before_words) -> dict:
    """One pass of a fixture (tests/golden/make_golden.py's per-pass format in
    the reference's layouts): the hashes of the records and of u32 lastF, the
    clock, the budget left, rBar's bits, a sparse sample of weight bits, and
    how many records the pass changed."""
    words, lastF, clock, left, rbar = obs
    w = words.reshape(-1, 4)
    return {"pass": k, "clock": int(clock), "budget_left": int(left), "rbar_bits": int(rbar),
            "synapses_sha256": sha(words), "last_fired_sha256": sha(lastF),
            "changed_records": int((w != before_words.reshape(-1, 4)).any(axis=1).sum()),
            "w_bits": w[_sample_index(len(w), PASS_SAMPLE), 2].tolist()}


def run_fixture(runner, settings, passes) -> dict:
    """A run's fixture: its settings and every pass's record."""
    out = {"max_spikes": settings["max_spikes"], "args": settings["args"], "reward_from": settings["reward_from"],
           "clock0": settings["clock0"], "special": settings["special"],
           "renorm_thresh": None if settings["renorm_thresh"] == NEVER else settings["renorm_thresh"], "passes": []}
    words = runner.observe()[0]
    out["initial_synapses_sha256"] = sha(words)
    for k in range(passes):
        if settings["reward_from"] is not None and k == settings["reward_from"]:
            runner.set_reward(0.5)
        before = words.copy()
        runner.step()
        obs = runner.observe()
        words = obs[0]
        out["passes"].append(pass_record(k, obs, before))
    idx = _sample_index(len(words) // 4, FINAL_SAMPLE)
    out["final_sample"] = {"index": idx.tolist(), "w_bits": words.reshape(-1, 4)[idx, 2].tolist()}
    return out


def case_fixture(cls, name, **extra) -> dict:
    c = CASES[name]
    runs = []
    for i in range(len(c["runs"])):
        r, s = case_runner(cls, name, i, **extra)
        runs.append(run_fixture(r, s, c["passes"]))
    n_hidden, n_syn, events = c["shape"]
    return {"name": name, "made_by": "ref_pass (the reference kernel's text under C1; tests/golden/make_ref_golden.py)",
            "n_input": 256, "n_output": 256, "n_hidden": n_hidden, "n_syn": n_syn, "events": events, "seed": 1,
            "stimulus": [0, 256], "runs": runs}


def fixture_text(data: dict) -> str:
    return json.dumps(data, indent=1) + "\n"


def fixture_path(name) -> str:
    return os.path.join(GOLDEN, f"ref_{name}.json")


def load_fixture(name) -> dict:
    with open(fixture_path(name)) as f:
        return json.load(f)


def fixture_settings(run: dict) -> dict:
    """A fixture run's settings as run_settings() gives them."""
    return dict(max_spikes=run["max_spikes"], args=run["args"], reward_from=run["reward_from"], clock0=run["clock0"],
                renorm_thresh=NEVER if run["renorm_thresh"] is None else run["renorm_thresh"], special=run["special"])


def check_against_fixture(runner, run: dict, what: str) -> None:
    """Drive `runner` over a fixture run's passes; every pass must reproduce its record."""
    s = fixture_settings(run)
    words = runner.observe()[0]
    assert sha(words) == run["initial_synapses_sha256"], f"{what}: initial records"
    for rec in run["passes"]:
        k = rec["pass"]
        if s["reward_from"] is not None and k == s["reward_from"]:
            runner.set_reward(0.5)
        before = words.copy()
        runner.step()
        obs = runner.observe()
        words = obs[0]
        got = pass_record(k, obs, before)
        bad = [f"{f}: {got[f]} != {rec[f]}" for f in rec if got[f] != rec[f]]
        assert not bad, f"{what} pass {k}: " + "; ".join(bad)
    idx = np.array(run["final_sample"]["index"])
    assert words.reshape(-1, 4)[idx, 2].tolist() == run["final_sample"]["w_bits"], f"{what}: final weight sample"
