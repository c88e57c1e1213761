"""CPU checks of the spike recorder's boundary (abnn.h abnn_spikes_*): the
ctypes mirrors match the C layout, null handles without a GPU, the numpy
restatement of the per-pass rule (abnn_amd.spikes.reference) on hand-made
lists whose result is written out by hand, and the properties of the oracle's
per-pass spike lists that make them the GPU tests' reference."""
import ctypes as C
import os
import subprocess

import numpy as np

from spikes_helpers import SHAPE1, SHAPE1_LENGTHS, make_oracle, oracle_pass_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32


def test_struct_layouts_match_c(tmp_path):
    from abnn_amd import _lib, spikes

    structs = {"abnn_spikes_config": _lib.SpikesConfig, "abnn_spike_pass": _lib.SpikePass,
               "abnn_spikes_info": _lib.SpikesInfo}
    body = ""
    for name, cls in structs.items():
        body += f'printf(" %zu", sizeof({name}));\n'
        body += "".join(f'printf(" %zu", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n'
                    + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = []
    for cls in structs.values():
        want += [C.sizeof(cls), *(getattr(cls, f).offset for f, _ in cls._fields_)]
    assert got == want
    assert [C.sizeof(c) for c in structs.values()] == [32, 32, 56]
    assert spikes.SPIKE_PASS_DTYPE.itemsize == 32
    assert [spikes.SPIKE_PASS_DTYPE.fields[f][1] for f, _ in _lib.SpikePass._fields_] == \
        [getattr(_lib.SpikePass, f).offset for f, _ in _lib.SpikePass._fields_]
    assert tuple(f for f, _ in _lib.SpikesInfo._fields_) == spikes.INFO_FIELDS


def test_null_handle_is_refused():
    from abnn_amd import _lib

    lib = _lib.load()
    cfg = _lib.SpikesConfig(10, 1, 0, 0, 0)
    info = _lib.SpikesInfo()
    assert lib.abnn_spikes_start(None, C.byref(cfg)) == 1
    assert lib.abnn_spikes_stop(None) == 1
    assert lib.abnn_spikes_clear(None, 0) == 1
    assert lib.abnn_spikes_get_info(None, C.byref(info)) == 1
    assert lib.abnn_spikes_read_passes(None, 0, 0, None) == 1
    assert lib.abnn_spikes_read_raster(None, 0, 0, None) == 1
    assert lib.abnn_spikes_read_counts(None, 0, 0, None) == 1


# hand-made lists: repeats, both sides of the range [10, 15), an empty pass
LISTS = [[12, 3, 12, 14, 20, 10, 12], [], [15, 9, 14], [11, 11, 11, 11], [13]]
META = [(7, 100, 0), (8, 101, 0), (9, 102, 0), (10, 0, 1), (11, 1, 1)]


def _entries(ref):
    return [tuple(int(x) for x in p) for p in ref["passes"]]


def test_reference_keeps_order_under_a_range_and_counts_duplicates():
    from abnn_amd import spikes

    ref = spikes.reference(LISTS, META, spikes.config(100, 10, neurons=(10, 5), counts=True))
    assert ref["raster"].tolist() == [12, 12, 14, 10, 12, 14, 11, 11, 11, 11, 13]  # L's order, not sorted
    assert _entries(ref) == [(7, 100, 0, 5, 0), (8, 101, 5, 0, 0), (9, 102, 5, 1, 0), (10, 0, 6, 4, 1), (11, 1, 10, 1, 1)]
    assert ref["counts"].tolist() == [1, 4, 3, 1, 2] and ref["counts"].dtype == U32
    assert ref["info"] == dict(passes_seen=5, spikes_seen=15, selected_seen=11, passes_recorded=5, spikes_recorded=11,
                               passes_dropped=0, spikes_dropped=0)
    assert [s.tolist() for s in spikes.split(ref["passes"], ref["raster"])] == \
        [[12, 12, 14, 10, 12], [], [14], [11, 11, 11, 11], [13]]
    # no range: S is L
    ref = spikes.reference(LISTS, META, spikes.config(100, 10, counts=True), n_neuron=21)
    assert ref["raster"].tolist() == sum(LISTS, [])
    assert ref["counts"].tolist() == np.bincount(sum(LISTS, []), minlength=21).tolist()
    assert ref["info"]["selected_seen"] == ref["info"]["spikes_seen"] == 15
    # a range that selects nothing
    ref = spikes.reference(LISTS, META, spikes.config(100, 10, neurons=(0, 3)))
    assert ref["raster"].size == 0 and [e[3] for e in _entries(ref)] == [0] * 5 and ref["counts"] is None


def test_reference_sticky_drop_and_exact_fit():
    from abnn_amd import spikes

    # 7 + 0 + 3 = 10 fits exactly; the next pass (4) does not, and the last (1) is dropped although it would fit
    ref = spikes.reference(LISTS, META, spikes.config(10, 10, counts=True), n_neuron=21)
    assert [e[0] for e in _entries(ref)] == [7, 8, 9] and ref["raster"].size == 10
    assert ref["info"] == dict(passes_seen=5, spikes_seen=15, selected_seen=15, passes_recorded=3, spikes_recorded=10,
                               passes_dropped=2, spikes_dropped=5)
    assert int(ref["counts"].sum()) == 15  # the counts go on over dropped passes
    # one spike less: the third pass is dropped, and every later one
    ref = spikes.reference(LISTS, META, spikes.config(9, 10))
    assert [e[0] for e in _entries(ref)] == [7, 8] and ref["info"]["passes_dropped"] == 3
    assert ref["info"]["spikes_dropped"] == 8 and ref["raster"].tolist() == LISTS[0]
    # the pass table fills first
    ref = spikes.reference(LISTS, META, spikes.config(100, 2))
    assert [e[0] for e in _entries(ref)] == [7, 8] and ref["info"]["passes_dropped"] == 3
    # a clear re-arms: recording resumes with the next pass, at offset 0
    ref = spikes.reference(LISTS, META, spikes.config(9, 10, counts=True), n_neuron=21, clears={3: True})
    assert _entries(ref) == [(10, 0, 0, 4, 1), (11, 1, 4, 1, 1)] and ref["raster"].tolist() == [11, 11, 11, 11, 13]
    assert ref["info"] == dict(passes_seen=5, spikes_seen=15, selected_seen=15, passes_recorded=2, spikes_recorded=5,
                               passes_dropped=0, spikes_dropped=0)
    assert int(ref["counts"].sum()) == 15
    ref = spikes.reference(LISTS, META, spikes.config(9, 10, counts=True), n_neuron=21, clears={3: False})
    assert int(ref["counts"].sum()) == 5


def test_reference_without_a_raster():
    from abnn_amd import spikes

    ref = spikes.reference(LISTS, META, spikes.config(0, 4, neurons=(10, 5)))
    assert ref["raster"].size == 0
    assert _entries(ref) == [(7, 100, 0, 5, 0), (8, 101, 5, 0, 0), (9, 102, 5, 1, 0), (10, 0, 6, 4, 1)]
    assert ref["info"]["passes_dropped"] == 1 and ref["info"]["spikes_recorded"] == 10


def test_oracle_lists_are_the_spikes_of_the_pass():
    """What makes the oracle's exchange record the reference: run through the
    shard phases at world 1 the oracle ends in the same state as pass_serial,
    the list's length is the pass's increment of the fired statistic, and
    every listed neuron carries the stamp `now` after the pass."""
    o, twin = make_oracle(*SHAPE1), make_oracle(*SHAPE1)
    lengths = []
    for k in range(16):
        fired = o.stats()["fired"]
        L, (pass_index, now, epoch) = oracle_pass_list(o)
        twin.pass_serial()
        assert (pass_index, now, epoch) == (k, k, 0)
        assert len(L) == o.stats()["fired"] - fired, k
        assert np.all(o.last_fired[L] == now), k
        assert np.array_equal(o.syn.view(U32), twin.syn.view(U32)), k
        assert np.array_equal(o.last_fired, twin.last_fired) and o.scalars() == twin.scalars(), k
        assert o.stats() == twin.stats(), k
        lengths.append(len(L))
    assert lengths == SHAPE1_LENGTHS
    L3, _ = oracle_pass_list(make_oracle(*SHAPE1))  # pass 0 again, on a fresh oracle: deterministic
    assert len(L3) == 0
    # pass 3: a full budget of output spikes, most of them repeats
    o = make_oracle(*SHAPE1)
    for k in range(4):
        L, _ = oracle_pass_list(o)
    assert len(L) == 2560 and len(L) - len(np.unique(L)) == 2304 and L.min() >= 256 and L.max() < 512
