"""torchrun worker for tests/test_corr_gpu.py: every rank runs ShardedBrain on
its shard (ranks share GPU 0, gloo exchange), records 16 passes, and checks
ShardedBrain.correlate in every mode against an unsharded Brain of the whole
graph, word for word."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist

    import abnn_amd
    from abnn_amd import corr
    from abnn_amd.shard import ShardedBrain, TorchComm

    shape = (488, 100_000, 100_000)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    sb = ShardedBrain(TorchComm(), 256, 256, *shape, device=0)
    sb.brain.build_random_graph(1)
    sb.brain.set_auto_stimulus(0, 256)
    sb.record_spikes(1 << 16, 32)
    sb.step(16)
    torch.cuda.synchronize()
    ref = abnn_amd.Brain(256, 256, *shape, device=0)
    ref.build_random_graph(1)
    ref.set_auto_stimulus(0, 256)
    ref.record_spikes(1 << 16, 32)
    ref.encode_traversal(16)
    why = []
    if not (np.array_equal(sb.spikes()["raster"], ref.spikes()["raster"]) and len(ref.spikes()["raster"]) > 0):
        why.append("the rasters differ")
    for args in (("synapses", None, None, 5), ("synapses", (0, 256), (256, 744), 16, (2, 12), (0.25, 0.75)),
                 ("pop", (512, 488), (256, 256), 5), ("pairs", (512, 32), (256, 256), 2)):
        got, want = sb.correlate(*args), ref.correlate(*args)
        if not np.array_equal(corr.to_words(got), corr.to_words(want)):
            why.append(f"{args}: {corr.to_words(got)[:8].tolist()} != {corr.to_words(want)[:8].tolist()}")
        if args[0] == "synapses":
            alone = sb.brain.correlate(*args)
            # a rank follows its own records only; the inputs never spike, so only the unranged plane is non-zero
            if not (0 < alone["followed"] < want["followed"] and (args[1] is not None or want["total"] > 0)):
                why.append(f"{args}: alone {alone['followed']}, whole {want['followed']}, total {want['total']}")
    if why:
        print(f"rank {rank}:", *why, sep="\n  ", flush=True)
    flag = torch.tensor([0 if why else 1], dtype=torch.int64)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("CORR_SHARDED_OK" if flag.item() == 1 else "CORR_SHARDED_MISMATCH", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
