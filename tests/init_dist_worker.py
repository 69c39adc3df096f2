"""One rank of tests/test_gpu_init_distributed.py: launched by torch.distributed.run, runs XPySom.linear_weights_init under a process
group and saves the codebooks the test compares.

    init_dist_worker.py <backend> <out_dir> <shard>     shard: contiguous | strided
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    backend, out_dir, shard = sys.argv[1], sys.argv[2], sys.argv[3]
    rank, world, local = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"))
    import torch
    import torch.distributed as dist
    from xpysom_dask_amd import XPySom
    dev = local if backend == "nccl" else 0
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group(backend)
    try:
        x, w = case()
        xd = torch.from_numpy(x).cuda(dev)
        wd = torch.from_numpy(w).cuda(dev)
        runs = {"host": (x, None), "dev": (xd, None), "hostw": (x, w), "devw": (xd, wd)}
        for name, (rows, weights) in runs.items():
            som = XPySom(9, 6, x.shape[1], random_seed=1, device=dev, shard=shard)
            som.linear_weights_init(rows, sample_weight=weights)
            np.save(os.path.join(out_dir, "%s_%s_%d.npy" % (name, shard, rank)), som._weights)
        # fewer rows than ranks: the last rank's shard is EMPTY and still takes part in both collectives
        som = XPySom(3, 2, x.shape[1], random_seed=1, device=dev, shard=shard)
        som.linear_weights_init(x[:1])
        np.save(os.path.join(out_dir, "few_%s_%d.npy" % (shard, rank)), som._weights)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def case():
    """(rows, weights) of the test: 5 001 rows (an odd count: the shards differ), 33 features, separated spectrum."""
    from tests import moments_ref as M
    x = M.spectrum_rows(5001, 33, 77)
    w = np.random.RandomState(5).uniform(0, 2, len(x)).astype(np.float32)
    w[::9] = 0
    return x, w


if __name__ == "__main__":
    main()
