"""Test helpers of the spike recorder: the per-pass spike lists of the CPU
oracle.  One oracle pass run as shard_gate -> shard_apply -> shard_commit at
world 1 leaves the pass's list in its exchange record: 8 int32 words of summary
(the first int64 = the spike candidates), then the spikes in budget order; its
length is min(summary[0], max_spikes)."""
import numpy as np

SUMMARY_INT32 = 8


def oracle_pass_list(o, xchg=None):
    """One oracle pass through the shard phases at world 1.  Returns (list,
    (pass_index, now, epoch)): the pass's spike list (u32 copy) and the
    scalars it ran with, read before the pass."""
    if xchg is None:
        xchg = np.zeros(o.exchange_words(), dtype=np.int32)
    sc = o.scalars()
    meta = (sc["pass_index"], sc["clock"], o.renormalisations())
    o.shard_gate(xchg)
    o.shard_apply(xchg, 1, 0)
    o.shard_commit(xchg, 1)
    n = min(int(xchg[:SUMMARY_INT32].view(np.int64)[0]), int(o.p.max_spikes))
    return xchg[SUMMARY_INT32:SUMMARY_INT32 + n].astype(np.uint32), meta


def oracle_lists(o, passes):
    """`passes` oracle passes; returns (lists, meta), one entry per pass."""
    xchg = np.zeros(o.exchange_words(), dtype=np.int32)
    lists, meta = [], []
    for _ in range(passes):
        L, m = oracle_pass_list(o, xchg)
        lists.append(L)
        meta.append(m)
    return lists, meta


def make_oracle(n_hidden, n_syn, events, seed=1, **params):
    from oracle import oracle as O

    o = O.OracleBrain(256, 256, n_hidden, n_syn, events, **params)
    o.build_random_graph(seed, nthreads=16)
    o.set_auto_stimulus(0, 256)
    return o


# the first shape of the GPU tests and its per-pass list lengths
SHAPE1 = (488, 100_000, 100_000)
SHAPE1_LENGTHS = [0, 0, 0, 2560, 647, 37, 2560, 235, 82, 2560, 64, 39, 2560, 24, 16, 2560]
