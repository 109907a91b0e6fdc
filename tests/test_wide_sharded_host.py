"""Wide top-k on the row-sharded index, the parts that need no GPU: the C ABI declares and exports the merge for sorted
lists, ShardedMipsIndex has a search_wide that route_search reaches, and the partition + pack + all-gather + merge plumbing of
that search returns the unsharded oracle's result on every rank of a gloo group (the oracle stands in for the two device
steps) -- also when every shard holds fewer rows than k, so that every part carries padding."""
import os
import re

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_sorted_merge():
    header = open(os.path.join(ROOT, "include", "mips_hip.h")).read()
    assert re.search(r"\bint\s+mips_merge_topk_sorted_packed\s*\(", header)
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", header).group(1)) == 1
    assert "mips_merge_topk_sorted_packed" in ram._lib.EXPORTS
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\s*\(", header))
    declared.discard("mips_hip")
    assert set(ram._lib.EXPORTS) == declared
    lib = ram._lib.load()
    assert hasattr(lib, "mips_merge_topk_sorted_packed")
    assert lib.mips_merge_topk_sorted_packed.argtypes == lib.mips_merge_topk_packed.argtypes
    assert callable(ram.merge_topk_sorted_packed) and "merge_topk_sorted_packed" in ram.__all__
    # the wide search no longer lists the packed payload among what it refuses
    doc = header[header.index("MIPS_E_UNSUPPORTED: k > MIPS_MAX_K_WIDE"):header.index("int mips_search_wide(")]
    assert "MIPS_OUT_PACKED" not in doc.split("How:")[0]


def test_sharded_index_has_the_wide_surface():
    assert hasattr(ram.ShardedMipsIndex, "search_wide")
    assert hasattr(ram.MipsIndex, "search_wide_packed")


def _gloo_worker(rank, world, port, n, nq, d, k, metric, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = synth.generate(9, 0, n, d, synth.KIND_LATTICE)      # lattice data: ties across the shards
        q = synth.generate(10, 0, nq, d, synth.KIND_LATTICE)
        lo, hi = ram.shard_bounds(n, world, rank)
        calls = []

        def local_search_wide(qq, kk, off, force_ip=False):   # oracle stands in for the device search of this shard
            assert off == lo
            calls.append(("wide", kk, force_ip))
            m = 0 if force_ip else metric
            if m == 0:
                return orc.search_exact_bruteforce(qq, x[lo:hi], kk, idx_offset=off)
            # L2 shards rank by the GLOBAL phi (what _sync_phi installs): distances of the whole index, this shard's rows
            s, i = orc.search_exact_bruteforce(qq, x, n, metric=1)
            keep = (i >= lo) & (i < hi)
            out_s = np.full((len(qq), kk), np.inf, np.float32)
            out_i = np.full((len(qq), kk), -1, np.int64)
            for r in range(len(qq)):
                m_ = min(kk, int(keep[r].sum()))
                out_s[r, :m_], out_i[r, :m_] = s[r][keep[r]][:m_], i[r][keep[r]][:m_]
            return out_s, out_i

        def merge(cs, ci, parts, kk, m):                        # oracle stands in for the device merge
            assert parts == world and cs.shape == (nq, world * kk)
            s, i = orc.merge_topk([cs.numpy()], [ci.numpy()], kk, m)
            return torch.from_numpy(s), torch.from_numpy(i)

        ix = ram.ShardedMipsIndex(d, metric=metric, local_search_wide=local_search_wide, merge=merge)
        assert (ix.rank, ix.world) == (rank, world)
        ix.set_global_size(n)
        es, ei = orc.search_exact_bruteforce(q, x, k, metric=metric)
        ok = True
        for got in (ix.search_wide(q, k), ram.index.route_search(ix, q, k), ix.search_async(q, k).result()):
            ok &= bool(np.array_equal(got[1], ei) and np.array_equal(got[0], es))
        ok &= calls == [("wide", k, False)] * 3
        if metric == 1:                                          # force_ip reaches the local step and the merge
            fs, fi = ix.search_wide(q, k, force_ip=True)
            es0, ei0 = orc.search_exact_bruteforce(q, x, k, metric=0)
            ok &= bool(np.array_equal(fi, ei0) and np.array_equal(fs, es0)) and calls[-1] == ("wide", k, True)
        if hi - lo < k:
            ok &= bool((ix.search_wide(q, k)[1][:, n:] == -1).all())
        try:
            ix.search_wide(q, k, idx_offset=5)
            ok = False
        except ValueError:
            pass
        try:
            ix.search_wide(q, ram.MAX_K_WIDE + 1)
            ok = False
        except NotImplementedError:
            pass
        # only local_search injected: the wide form falls back to it
        fb = ram.ShardedMipsIndex(d, local_search=lambda qq, kk, off: orc.search_exact_bruteforce(qq, x[lo:hi], kk, idx_offset=off),
                                  merge=merge)
        fb.set_global_size(n)
        if metric == 0:
            got = fb.search_wide(q, k)
            ok &= bool(np.array_equal(got[1], ei) and np.array_equal(got[0], es))
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,metric", [(2, 1003, 0), (3, 1003, 0), (3, 100, 0), (2, 1003, 1), (3, 100, 1)])
def test_sharded_search_wide_gloo(world, n, metric):
    import torch.multiprocessing as mp

    port = 27500 + (os.getpid() % 2000) + 3 * world + n % 7 + metric
    ret = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, port, n, 5, 64, 64, metric, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}
