"""ShardedMipsIndex.reconstruct_batch on ranks that share one GPU (gloo): global ids that span the shards, repeat, and name no row
give, on every rank, bit for bit what the unsharded index gives -- before remove_ids_global and after it, when the shards are
uneven and one of them is empty."""
import os
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import rows_cases as rc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu


def _ids(n):
    rng = np.random.default_rng(n)
    return np.concatenate([np.arange(n)[::-1], rng.integers(0, n, 300), [-1, n, n + 1, (1 << 32) + 3, rc.INT64_MIN, 0, n - 1]]).astype(np.int64)


def _rank_worker(rank, world, port, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        for storage, x in (("f32", rc.planted_f32(1001, 100)), ("bf16", rc.rows_data("bf16", 100, 1001)[0])):
            stored = rc.lc.stored_rows(x, storage)
            d = x.shape[1]
            ix = ram.ShardedMipsIndex(d, dtype=storage, device=0)
            ix.add_global(x)
            whole = ram.MipsIndex(d, dtype=storage, device=0)       # the unsharded index, on every rank
            whole.add(x)
            for step in (0, 1, 2):
                if step == 1:                                      # ids spread over the shards
                    mask = np.random.default_rng(8).random(len(stored)) < 0.3
                elif step == 2:                                    # everything shard 1 still holds: an empty shard in the middle
                    sizes = [None] * world
                    dist.all_gather_object(sizes, ix.local.ntotal)  # the shards as they are now
                    lo1, hi1, _ = ram.shard_offsets(sizes, 1)
                    mask = (np.arange(len(stored)) >= lo1) & (np.arange(len(stored)) < hi1)
                if step:
                    assert ix.remove_ids_global(mask) == whole.remove_ids(mask) == int(mask.sum())
                    stored = stored[~mask]
                counts = [None] * world
                dist.all_gather_object(counts, ix.local.ntotal)
                assert step < 2 or counts[1] == 0
                n = len(stored)
                ids = _ids(n)
                exp = rc.model_reconstruct(stored, ids)
                dev = torch.from_numpy(ids).cuda()
                got = ix.reconstruct_batch(dev)
                assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(ids), d)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), exp.view(np.uint32)), f"{storage}, step {step}"
                assert np.array_equal(got.cpu().numpy().view(np.uint32), whole.reconstruct_batch(dev).cpu().numpy().view(np.uint32))
                host = ix.reconstruct_batch(ids.reshape(-1, 1))    # NumPy ids of another shape -> NumPy
                assert isinstance(host, np.ndarray) and host.shape == (len(ids), 1, d)
                assert np.array_equal(host.view(np.uint32).reshape(len(ids), d), exp.view(np.uint32))
                every = [None] * world
                dist.all_gather_object(every, got.cpu().numpy().tobytes())
                assert all(e == every[0] for e in every)
                if storage == "f32" and step == 0:
                    assert (exp.view(np.uint32) == 0x80000000).sum() > d   # -0.0 went through the all-reduce
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_reconstruct_on_ranks_sharing_one_gpu(world):
    import torch.multiprocessing as mp

    port = 29300 + (os.getpid() % 2000) + 5 * world
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


def test_one_rank_without_a_process_group():
    x, stored = rc.rows_data("bf16", 64, 300)
    ix = ram.ShardedMipsIndex(64, device=0)
    ix.add_global(x)
    ids = _ids(300)
    got = ix.reconstruct_batch(ids)
    assert np.array_equal(got.view(np.uint32), rc.model_reconstruct(stored, ids).view(np.uint32))
