"""The spike correlograms on the GPU (abnn.h abnn_corr_*, csrc/corr.hip).

Every result is compared word for word against the numpy restatement
(abnn_amd.corr.reference) and the C host rule (abnn_corr_host) over the pass
table, the raster and the records read back from the device, or over the
hand-made ones put there through abnn_spikes_load (tests/corr_helpers.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from corr_helpers import NONE, SYN, check, random_records, table
from spikes_helpers import SHAPE1, SHAPE1_LENGTHS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1 = 256 + 256 + SHAPE1[0]
INF = float("inf")


def _gpu(n_hidden, n_syn, events, seed=1, **params):
    import abnn_amd

    g = abnn_amd.Brain(256, 256, n_hidden, n_syn, events, **params)
    g.build_random_graph(seed)
    g.set_auto_stimulus(0, 256)
    return g


def _run(g, cfg):
    """abnn_corr through Brain.correlate's path, as u64 words."""
    import ctypes as C

    from abnn_amd import _lib, corr

    words = corr.n_words(cfg)
    out = np.full(words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    _lib.call("abnn_corr", g._h, C.byref(cfg), out.ctypes.data, words)
    return out


@pytest.fixture(scope="module")
def natural(gpu):
    """SHAPE1 after 16 recorded passes: the brain, its table, raster and records (read only)."""
    g = _gpu(*SHAPE1)
    g.record_spikes(raster=1 << 16, passes=32)
    g.encode_traversal(16)
    s = g.spikes()
    syn = g.download_synapses()
    assert s["passes"]["count"].tolist() == SHAPE1_LENGTHS
    for x in (s["passes"], s["raster"], syn):
        x.setflags(write=False)
    yield g, s["passes"], s["raster"], syn
    g.close()


# ---- 1. the natural raster -------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 5, 15, 16, 256])
def test_natural_raster(natural, L):
    from abnn_amd import corr

    g, passes, raster, syn = natural
    pop = check(_run(g, corr.config("pop", max_lag=L)), corr.config("pop", max_lag=L), N1, passes, raster)
    assert pop["rows"] == 16 and pop["entries"] == sum(SHAPE1_LENGTHS) == pop["in_a"] and pop["recorded"] == 16
    cfg = corr.config("pop", (512, 488), (256, 256), L, rows=(2, 12))
    check(_run(g, cfg), cfg, N1, passes, raster)
    cfg = corr.config("synapses", max_lag=L)
    d = check(_run(g, cfg), cfg, N1, passes, raster, syn)
    assert d["total"] > 0 and d["coupled"] > 0 and d["followed"] == SHAPE1[1]  # not all zero by accident
    cfg = corr.config("synapses", (0, 256), (256, 744), L, rows=(3, 10), weights=(0.25, 0.75))
    d = check(_run(g, cfg), cfg, N1, passes, raster, syn)
    assert d["coupled"] <= d["followed"] and 0 < d["followed"] < SHAPE1[1]
    cfg = corr.config("pairs", (256, 100), (500, 300), L)  # 30 000 cells: fits at L = 256
    d = check(_run(g, cfg), cfg, N1, passes, raster)
    assert d["total"] > 0


def test_natural_raster_pairs_targets_to_outputs(natural):
    """PAIRS with A = the range the inputs' targets lie in and B = the outputs, at L = 5."""
    from abnn_amd import corr

    g, passes, raster, syn = natural
    t = syn["dst"][(syn["src"] < 256) & (syn["dst"] != NONE)]
    a = (int(t.min()), int(t.max()) - int(t.min()) + 1)
    assert a[1] * 256 * 11 <= 1 << 24
    cfg = corr.config("pairs", a, (256, 256), 5)
    d = check(_run(g, cfg), cfg, N1, passes, raster)
    assert d["plane"].shape == (a[1], 256, 11) and d["total"] > 0
    assert g.correlate("pairs", a, (256, 256), 5)["plane"].tolist() == d["plane"].tolist()


# ---- 2. inside the learning loop -------------------------------------------------------------------
def test_inside_the_learning_loop(gpu):
    import torch

    from abnn_amd import corr
    from abnn_amd.learn import LearnEngine

    rng = np.random.default_rng(3)
    with _gpu(*SHAPE1) as g:
        g.record_spikes(raster=1 << 16, passes=32)
        cfgs = [corr.config("synapses", max_lag=5), corr.config("pop", (512, 488), (256, 256), 5),
                corr.config("pairs", (512, 64), (256, 256), 2)]
        outs = [torch.zeros(corr.n_words(c), dtype=torch.int64, device="cuda:0") for c in cfgs]
        g.correlate("pop")  # the handle's first call allocates the scratch
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=0)
        with LearnEngine(g) as eng:
            eng.run(rng.random((16, 256), dtype=np.float32), rng.random((16, 256), dtype=np.float32), stream=side)
            for c, o in zip(cfgs, outs):
                g.correlate_enqueue(c, o.data_ptr(), stream=side)
            side.synchronize()  # the only synchronise
            s = g.spikes()
            syn = g.download_synapses()
            assert s["info"]["passes_recorded"] == 16 and len(s["raster"]) > 0
            for c, o in zip(cfgs, outs):
                check(o.cpu().numpy().view(np.uint64), c, N1, s["passes"], s["raster"], syn)


# ---- 3. loaded rasters -----------------------------------------------------------------------------
def _loaded(g, rows, cfgs, syn=None, n_nrn=N1):
    passes, raster = table(rows)
    g.load_spikes(passes, raster)
    s = g.spikes()
    assert np.array_equal(s["passes"], passes) and np.array_equal(s["raster"], raster)
    assert s["info"]["passes_recorded"] == len(rows) and s["info"]["passes_dropped"] == 0
    return [check(_run(g, c), c, n_nrn, passes, raster, syn) for c in cfgs]


def test_loaded_rasters(gpu):
    import abnn_amd
    from abnn_amd import corr

    rng = np.random.default_rng(11)
    with _gpu(*SHAPE1) as g:
        g.record_spikes(raster=1 << 14, passes=8)
        syn = g.download_synapses()
        syn["src"][:4], syn["dst"][:4] = [0, N1 - 1, 7, 7], [N1 - 1, 0, 7, 0]
        g.upload_synapses(syn)
        modes = [corr.config("pop", max_lag=3), corr.config("synapses", max_lag=3),
                 corr.config("pairs", (0, 8), (N1 - 8, 8), 3), corr.config("pairs", (7, 1), (7, 1), 0)]
        d = _loaded(g, [], modes, syn)  # K == 0
        assert all(x["recorded"] == 0 and x["total"] == 0 for x in d)
        d = _loaded(g, [[3, 7, 7]], modes, syn)  # one row
        assert d[0]["plane"].tolist() == [0, 0, 0, 9, 0, 0, 0]
        d = _loaded(g, [[7] * 5], modes, syn)  # one id five times
        assert d[3]["plane"].tolist() == [[[25]]] and d[1]["total"] >= 25
        d = _loaded(g, [[0], [N1 - 1], [0, N1 - 1]], modes, syn)  # the first and the last id
        assert d[1]["coupled"] >= 2 and d[2]["plane"][0, 7].tolist() == [0, 0, 1, 1, 1, 1, 0]
        rows = [rng.integers(0, N1, n).astype(np.uint32) for n in (5, 0, 9, 3, 1)]
        one = [corr.config(m, a, b, 2, rows=(2, 1)) for m, a, b in (("pop", None, None), ("synapses", None, None),
                                                                     ("pairs", (0, 100), (0, 100)))]
        d = _loaded(g, rows, one, syn)  # a window of one row
        assert d[0]["rows"] == 1 and d[0]["plane"].tolist() == [0, 0, 81, 0, 0]
        past = [corr.config(m, max_lag=2, rows=(r, 3)) for m in ("pop", "synapses") for r in (5, 6, 1 << 40)]
        d = _loaded(g, rows, past, syn)  # row_first >= K
        assert all(x["rows"] == 0 and x["entries"] == 0 and x["total"] == 0 and x["recorded"] == 5 for x in d)
        # rows larger than one workgroup's chunk (and than max_spikes), with repeats
        big = [rng.integers(500, 540, 2561).astype(np.uint32), rng.integers(490, 530, 4097).astype(np.uint32),
               rng.integers(0, N1, 40).astype(np.uint32)]
        syn["src"][4:2004], syn["dst"][4:2004] = rng.integers(490, 540, 2000), rng.integers(490, 540, 2000)
        g.upload_synapses(syn)
        d = _loaded(g, big, [corr.config("pairs", (495, 40), (500, 35), 1), corr.config("synapses", max_lag=2),
                             corr.config("synapses", (500, 20), (490, 50), 1)], syn)
        assert d[0]["total"] > 1_000_000 and d[1]["coupled"] >= 2000

        # refusals leave the recorder as it was
        before = g.spikes()
        P, R = table([[1, 2], [3]])
        bad = {"too many passes": table([[1]] * 9), "too many spikes": table([[1] * ((1 << 14) + 1)]),
               "an id at N_NRN": table([[1, N1]]), "a raster longer than the counts": (P, np.arange(4, dtype=np.uint32))}
        for name, field, value in (("the first offset is not 0", "offset", [1, 3]), ("a gap", "offset", [0, 3]),
                                   ("an overlap", "offset", [0, 1]), ("counts past the raster", "count", [2, 2])):
            p = P.copy()
            p[field] = value
            bad[name] = (p, R)
        for name, (p, r) in bad.items():
            with pytest.raises(abnn_amd.AbnnError) as err:
                g.load_spikes(p, r)
            assert err.value.status == 1, name
        after = g.spikes()
        assert after["info"] == before["info"] and np.array_equal(after["passes"], before["passes"])
        assert np.array_equal(after["raster"], before["raster"])
        g.record_spikes(raster=64, passes=4, neurons=(256, 256))
        with pytest.raises(abnn_amd.AbnnError):
            g.load_spikes(*table([[255]]))  # outside the recorder's range
        g.load_spikes(*table([[256, 511]]))
        g.record_spikes(raster=0, passes=4)
        for call in (lambda: g.load_spikes(*table([[]])), lambda: g.correlate("pop")):  # no raster
            with pytest.raises(abnn_amd.AbnnError) as err:
                call()
            assert err.value.status == 1
        g.stop_spikes()
        for call in (lambda: g.load_spikes(*table([[1]])), lambda: g.correlate("pop")):  # no recorder
            with pytest.raises(abnn_amd.AbnnError) as err:
                call()
            assert err.value.status == 1
        g.record_spikes(raster=64, passes=4)
        for kw in (dict(a=(N1 - 1, 2)), dict(b=(N1, 1)), dict(max_lag=257), dict(weights=(0.5, 0.5))):
            with pytest.raises(abnn_amd.AbnnError) as err:
                g.correlate("synapses", **kw)
            assert err.value.status == 1, kw


# ---- 4. record tails -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [0, 1, 7, 8, 9, 15, 17, 4097])
def test_record_tails(gpu, n_syn):
    import abnn_amd
    from abnn_amd import corr

    rng = np.random.default_rng(n_syn)
    n_nrn = 1000
    rows = [rng.permutation(n_nrn).astype(np.uint32) for _ in range(3)]  # every neuron has entries: every record couples
    rec = random_records(rng, n_nrn, n_syn, tombstones=0.2 if n_syn > 8 else 0.0)
    if n_syn:
        rec["w"][n_syn - 1] = np.nan
        rec["src"][n_syn - 1], rec["dst"][n_syn - 1] = 1, 2  # the last record is live: the tail is read
    if n_syn > 8:
        rec["src"][3] = rec["dst"][3] = NONE
    with abnn_amd.Brain(256, 256, 488, n_syn, 100_000) as g:
        if n_syn:
            g.upload_synapses(rec)
        g.record_spikes(raster=4096, passes=4)
        cfgs = [corr.config("synapses", max_lag=2), corr.config("synapses", max_lag=1, weights=(0.25, INF)),
                corr.config("synapses", (0, 600), (300, 700), 0, weights=(-INF, 0.5))]
        d = _loaded(g, rows, cfgs, rec, n_nrn)
        live = int((rec["dst"] != NONE).sum())
        assert d[0]["followed"] == d[0]["coupled"] == live and d[0]["total"] == 9 * live
        assert d[1]["followed"] < max(live, 1)  # the NaN weight never matches


# ---- 5. a map that does not fit LDS ----------------------------------------------------------------
def test_a_map_larger_than_the_lds_fold(gpu):
    import abnn_amd
    from abnn_amd import corr

    fold = 1 << 18  # neurons n and n + 2^18 share a folded bit (csrc/corr.h kCorrFoldWords = 8192 words)
    n_hidden = fold + 700
    n_nrn = 512 + n_hidden
    x, y, z, v, w = 700, 700 + fold, 300, 300 + fold, 1234  # x and y alias; v aliases z but has no entries; w neither
    assert max(x, y, z, v, w) < n_nrn
    ids = [x, y, z, v, w, n_nrn - 1]
    rec = np.array([(s, t, 0.5, 0) for s in ids for t in ids] + [(NONE, NONE, 0.5, 0)], dtype=SYN)
    rows = [[x, z], [y], [x, y, y], [z, n_nrn - 1]]
    with abnn_amd.Brain(256, 256, n_hidden, len(rec), 1000) as g:
        g.upload_synapses(rec)
        g.record_spikes(raster=64, passes=8)
        cfgs = [corr.config("synapses", max_lag=3), corr.config("synapses", (x, fold + 1), (0, n_nrn), 1),
                corr.config("pop", (y, 1), None, 3), corr.config("pairs", (y, 1), (x, 1), 2)]
        d = _loaded(g, rows, cfgs, rec, n_nrn)
        assert d[0]["followed"] == 36 and d[0]["coupled"] == 16  # the four with entries, to and from each other
        assert d[3]["plane"].reshape(-1).tolist() == [2, 1, 2, 1, 0]  # y in rows 1, 2, 2 against x in rows 0, 2


# ---- 6. grid independence --------------------------------------------------------------------------
def test_twice_and_after_an_unrelated_call(natural):
    from abnn_amd import corr

    g, passes, raster, syn = natural
    cfg = corr.config("synapses", (512, 488), None, 7, weights=(0.1, 0.9))
    first = _run(g, cfg)
    assert np.array_equal(_run(g, cfg), first)
    _run(g, corr.config("pairs", (0, 64), (600, 64), 1))
    _run(g, corr.config("synapses", (0, 256), (256, 256), 256))
    assert np.array_equal(_run(g, cfg), first) and first[4] > 0


# ---- 7. sharded ------------------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_world2(gpu):
    """Two ranks sharing GPU 0 over gloo (tests/test_sharded_gpu.py's path): every
    rank's ShardedBrain.correlate equals the unsharded brain's."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()),
           os.path.join(ROOT, "tests", "helpers", "corr_shard_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env={**os.environ, "OMP_NUM_THREADS": "4"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CORR_SHARDED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 8. the C++ mirrors ----------------------------------------------------------------------------
def test_cpp_corr(gpu):
    from abnn_amd.build import build_corr_test

    prog = build_corr_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["followed"] == 100_000 and res["coupled"] > 1000 and res["syn_total"] > 0 and res["pop0"] > 0
