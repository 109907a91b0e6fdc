"""Wide top-k (30 <= k <= 1024) on the row-sharded index: the merge kernel for sorted lists against NumPy and against the
counting merge, the packed output of the wide search against its plain output (re-score and settlement writers, more than
one query slice), shards merged in one process, ShardedMipsIndex.search_wide on ranks that share one GPU, and the refusals."""
import os

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu

I64_MAX = np.iinfo(np.int64).max


def _unpack(packed):
    """CUDA int64 [nq, k, 2] -> (float32 [nq, k], int64 [nq, k]) NumPy"""
    s, i = ram.unpack_gathered(packed[None], 1)
    return s.cpu().numpy(), i.cpu().numpy()


def _same(got, exp, what=""):
    s, i = got
    es, ei = exp
    if isinstance(s, torch.Tensor):
        s, i = s.cpu().numpy(), i.cpu().numpy()
    if isinstance(es, torch.Tensor):
        es, ei = es.cpu().numpy(), ei.cpu().numpy()
    bad = np.flatnonzero((i != ei).any(axis=1))
    assert np.array_equal(i, ei), f"{what}: indices differ in {len(bad)} queries, first {bad[:5]}"
    assert np.array_equal(s.view(np.int32), es.view(np.int32)), f"{what}: scores differ"


# ------------------------------------------------------------------ 1. the merge kernel alone
def _payload(nq, parts, k, metric, variant):
    """-> (gathered int64 [parts, nq, k, 2], expected scores [nq, k], expected ids [nq, k], queries with a tie across the k-th
    place).  Per query parts * k distinct ids in [2^33, 2^33 + 2^20), scores of 17 levels, dealt round-robin to the parts,
    every part in result order.  variant "truncated": part 0 keeps k / 3 entries, the rest padding; "empty": the last part
    is all padding."""
    rng = np.random.default_rng(0)
    c = parts * k
    pad_s = np.float32(np.inf if metric else -np.inf)
    S = np.full((parts, nq, k), pad_s, np.float32)
    I = np.full((parts, nq, k), -1, np.int64)
    exp_s = np.full((nq, k), pad_s, np.float32)
    exp_i = np.full((nq, k), -1, np.int64)
    straddle = 0
    for q in range(nq):
        ids = rng.choice(1 << 20, c, replace=False).astype(np.int64) + (1 << 33)
        sc = (rng.integers(0, 17, c) / 4).astype(np.float32)
        all_s, all_i = [], []
        for p in range(parts):
            ps, pi = sc[p::parts], ids[p::parts]
            order = np.lexsort((pi, ps if metric else -ps))
            ps, pi = ps[order], pi[order]
            keep = k
            if variant == "truncated" and p == 0:
                keep = k // 3
            if variant == "empty" and p == parts - 1:
                keep = 0
            S[p, q, :keep], I[p, q, :keep] = ps[:keep], pi[:keep]
            all_s.append(ps[:keep])
            all_i.append(pi[:keep])
        all_s, all_i = np.concatenate(all_s), np.concatenate(all_i)
        order = np.lexsort((all_i, all_s if metric else -all_s))[:k]
        exp_s[q, :len(order)], exp_i[q, :len(order)] = all_s[order], all_i[order]
        if len(all_s) > k:
            rest = np.lexsort((all_i, all_s if metric else -all_s))
            straddle += int(all_s[rest[k - 1]] == all_s[rest[k]])
    bits = S.view(np.uint32).astype(np.int64)              # zero-extended float32 bits, as the searches write them
    return np.ascontiguousarray(np.stack((bits, I), axis=-1)), exp_s, exp_i, straddle


MERGE_SHAPES = [(7, 2, 30), (33, 3, 100), (5, 8, 1024), (3, 16, 1024), (4, 1, 64)]


@pytest.mark.parametrize("variant", ["full", "truncated", "empty"])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("nq,parts,k", MERGE_SHAPES)
def test_sorted_merge_equals_lexsort_and_the_counting_merge(nq, parts, k, metric, variant):
    g, exp_s, exp_i, straddle = _payload(nq, parts, k, metric, variant)
    if variant == "full" and parts > 1:
        assert straddle > 0                                  # (a tie across the merged k-th place is actually exercised)
    gd = torch.from_numpy(g).cuda().view(parts * nq, k, 2)
    got = ram.merge_topk_sorted_packed(gd, nq, parts, k, metric)
    _same(got, (exp_s, exp_i), f"sorted merge {nq, parts, k, metric, variant}")
    ref = ram.merge_topk_packed(gd, nq, parts, k, metric)
    _same(got, ref, "sorted merge against the counting merge")


@pytest.mark.parametrize("nq,parts,k", [(7, 2, 30), (3, 16, 1024)])     # staged in LDS / searched in global memory
def test_sorted_merge_one_poisoned_entry_poisons_its_row_only(nq, parts, k):
    g, exp_s, exp_i, _ = _payload(nq, parts, k, 0, "full")
    g[parts - 1, 1, k - 1, 1] = ram.IDX_POISON
    gd = torch.from_numpy(g).cuda().view(parts * nq, k, 2)
    s, i = ram.merge_topk_sorted_packed(gd, nq, parts, k, 0)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert (i[1] == ram.IDX_POISON).all() and np.isnan(s[1]).all()
    clean = [r for r in range(nq) if r != 1]
    assert np.array_equal(i[clean], exp_i[clean]) and np.array_equal(s[clean], exp_s[clean])


def test_sorted_merge_limits():
    g = torch.zeros((2, 4, 2), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="MIPS_MAX_K_WIDE"):
        ram.merge_topk_sorted_packed(g, 1, 1, ram.MAX_K_WIDE + 1, 0)
    with pytest.raises(RuntimeError, match="too large"):
        ram.merge_topk_sorted_packed(g, 1, 65, 1024, 0)


# ------------------------------------------------------------------ 2. packed output of the wide search
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("metric", [0, 1])
def test_packed_equals_plain(dtype, metric):
    off = 1 << 33
    x = synth.generate(3, 0, 6000, 200, synth.KIND_GAUSS)
    q = torch.from_numpy(synth.generate(4, 0, 9, 200, synth.KIND_GAUSS)).cuda()
    ix = ram.MipsIndex(200, metric=metric, dtype=dtype)
    ix.add(x)
    plain = ix.search_wide(q, 50, idx_offset=off)
    p = ix.search_wide_packed(q, 50, idx_offset=off)
    assert p.shape == (9, 50, 2) and p.dtype == torch.int64 and p.is_cuda
    assert int(p[..., 0].min()) >= 0 and int(p[..., 0].max()) < (1 << 32)        # zero-extended score bits
    _same(_unpack(p), plain, "packed")
    assert int(plain[1].min()) >= off
    _same(plain, orc.search_exact(q.cpu().numpy(), x, 50, metric=metric, idx_offset=off), "plain")
    if metric == 1:
        _same(_unpack(ix.search_wide_packed(q, 50, idx_offset=off, force_ip=True)), ix.search_wide(q, 50, idx_offset=off, force_ip=True),
              "packed, force_ip")
    # k above ntotal: the padding of a packed row is the plain padding; an empty index is all padding
    small = ram.MipsIndex(200, metric=metric, dtype=dtype)
    ps, pi = _unpack(small.search_wide_packed(q, 40, idx_offset=off))
    assert (pi == -1).all() and (ps == (np.inf if metric else -np.inf)).all()
    small.add(x[:50])
    ps, pi = _unpack(small.search_wide_packed(q, 64, idx_offset=off))
    _same((ps, pi), small.search_wide(q, 64, idx_offset=off), "packed padding")
    assert (pi[:, 50:] == -1).all() and (pi[:, :50] >= off).all() and (ps[:, 50:] == (np.inf if metric else -np.inf)).all()


def test_packed_rows_of_settled_queries():
    """The shape of test_near_duplicates_across_the_kth_place_are_flagged_and_settled (bf16): the star queries are flagged and
    their rows rewritten by the settlement's finalize kernel -- which must write the packed form too."""
    rng = np.random.default_rng(11)
    n, d, nq, k, M = 20000, 768, 64, 100, 300
    x = synth.round_to_bf16(rng.standard_normal((n, d)).astype(np.float32))
    q = synth.round_to_bf16(rng.standard_normal((nq, d)).astype(np.float32))
    v = synth.round_to_bf16(rng.standard_normal(d).astype(np.float32))
    rows = 1003 + 16 * np.arange(M)
    x[rows] = v
    x[rows, 5] = (np.arange(M) % 16).astype(np.float32)
    x[rows, 9] = (np.arange(M) // 16).astype(np.float32)
    star = v.copy()
    star[5] = 2.0 ** -12
    star[9] = 2.0 ** -8
    q[np.arange(0, nq, 8)] = star
    ix = ram.MipsIndex(d)
    ix.add(x)
    qd = torch.from_numpy(q).cuda()
    p = ix.search_wide_packed(qd, k, idx_offset=1 << 33)
    st = ix.margin_stats()
    assert st["flagged"] > 0 and st["unresolved"] == 0 and st["rescanned"] == st["flagged"]
    exp = orc.search_exact_bruteforce(q, x, k, idx_offset=1 << 33)
    _same(_unpack(p), exp, "packed, settled")
    _same(ix.search_wide(qd, k, idx_offset=1 << 33), exp, "plain, settled")


def test_packed_more_queries_than_one_slice():
    x = synth.generate(3, 0, 3000, 64, synth.KIND_GAUSS)
    q = synth.generate(4, 0, 4100, 64, synth.KIND_GAUSS)
    ix = ram.MipsIndex(64)
    ix.add(x)
    p = ix.search_wide_packed(torch.from_numpy(q).cuda(), 40, idx_offset=7)
    assert ix.margin_stats()["unresolved"] == 0
    _same(_unpack(p), orc.search_exact(q, x, 40, idx_offset=7), "4100 queries, packed")


# ------------------------------------------------------------------ 3. shards in one process
@pytest.mark.parametrize("metric", [0, 1])
def test_three_ragged_shards_merge_to_the_unsharded_result(metric):
    n, d, nq, k = 9001, 256, 77, 64
    rng = np.random.default_rng(4)
    x = synth.round_to_bf16((synth.generate(153, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
    qn = synth.generate(154, 0, nq, d, synth.KIND_GAUSS)
    q = torch.from_numpy(qn).cuda()
    full = ram.MipsIndex(d, metric=metric)
    full.add(x)
    bounds = [(0, 2000), (2000, 2050), (2050, n)]             # the middle shard holds fewer rows than k: its part is padded
    parts = []
    for lo, hi in bounds:
        p = ram.MipsIndex(d, metric=metric)
        p.add(x[lo:hi])
        if metric == 1:
            p.set_phi(full.phi())
        parts.append(p.search_wide_packed(q, k, idx_offset=lo))
        assert p.margin_stats()["unresolved"] == 0
    assert int((parts[1][..., 1] < 0).sum()) == nq * (k - 50)
    got = ram.merge_topk_sorted_packed(torch.cat(parts, 0), nq, 3, k, metric)
    _same(got, full.search_wide(q, k), "shards against the unsharded search")
    _same(got, orc.search_exact(qn, x, k, metric=metric), "shards against the oracle")


# ------------------------------------------------------------------ 4. ranks sharing one GPU (gloo)
def _rank_worker(rank, world, port, n, nq, d, k, facade, tmp, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        rng = np.random.default_rng(3)
        x = synth.round_to_bf16((synth.generate(151, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
        qn = synth.round_to_bf16(synth.generate(152, 0, nq, d, synth.KIND_GAUSS))
        qd = torch.from_numpy(qn).cuda()
        ok = True
        for metric in (0, 1):
            ix = ram.ShardedMipsIndex(d, metric=metric, device=0)
            ix.add_global(x)
            lo, hi = ram.shard_bounds(n, world, rank)
            ok &= ix.local.ntotal == hi - lo
            exp = orc.search_exact(qn, x, k, metric=metric) if n > 4 * k else orc.search_exact_bruteforce(qn, x, k, metric=metric)
            s, i = ix.search_wide(qd, k)                          # device fast path
            ok &= s.is_cuda and bool(np.array_equal(i.cpu().numpy(), exp[1]) and np.array_equal(s.cpu().numpy(), exp[0]))
            ok &= ix.margin_stats()["unresolved"] == 0
            s, i = ix.search_wide(qn, k)                          # generic path: NumPy in, NumPy out
            ok &= isinstance(s, np.ndarray) and bool(np.array_equal(i, exp[1]) and np.array_equal(s, exp[0]))
            ok &= ix.margin_stats()["unresolved"] == 0
            s, i = ix.search_async(qd, k).result()
            ok &= bool(np.array_equal(i.cpu().numpy(), exp[1]) and np.array_equal(s.cpu().numpy(), exp[0]))
            if metric == 1:
                s, i = ix.search_wide(qd, k, force_ip=True)
                e0 = orc.search_exact(qn, x, k, metric=0) if n > 4 * k else orc.search_exact_bruteforce(qn, x, k, metric=0)
                ok &= bool(np.array_equal(i.cpu().numpy(), e0[1]) and np.array_equal(s.cpu().numpy(), e0[0]))
            if facade:
                s, i = ram.index.route_search(ix, qd, 64)
                e64 = orc.search_exact(qn, x, 64, metric=metric)
                ok &= bool(np.array_equal(i.cpu().numpy(), e64[1]) and np.array_equal(s.cpu().numpy(), e64[0]))
        if facade:
            data = {"mips_column": [f"text {t}" for t in range(n)], "aid": [f"a{t}" for t in range(n)]}
            m = ram.Mips(ram.MipsArgs(mips_metric_type=0, mips_normalize=False, mips_tmp_folder=tmp, mips_shard=True, mips_device=0),
                         data=data)
            m.build_index_sharded(x)
            index = m.embeddings.get_index(m.index_name).faiss_index
            ok &= isinstance(index, ram.ShardedMipsIndex)
            s, i = m.search(qn, k=40)
            e40 = orc.search_exact(qn, x, 40)
            ok &= bool(np.array_equal(np.asarray(i), e40[1]) and np.array_equal(np.asarray(s), e40[0]))
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,facade", [(2, 20001, 100, True), (3, 20001, 100, False), (3, 100, 64, False)])
def test_sharded_search_wide_on_ranks_sharing_one_gpu(world, n, k, facade, tmp_path):
    """Row shards on `world` processes sharing cuda:0: the wide scan per shard, the packed all-gather (gloo, host staged), the
    merge for sorted lists -- equal to the oracle on the unsharded index, CUDA and NumPy queries, both metrics; n = 100 at
    world 3 leaves every shard with fewer rows than k, so every part arrives padded.  One case also goes through route_search
    and the Mips facade with mips_shard=True."""
    import torch.multiprocessing as mp

    port = 27200 + (os.getpid() % 2000) + 5 * world + n % 7
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, n, 50, 256, k, facade, str(tmp_path), ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    q = torch.zeros((2, 64), device="cuda")
    x = synth.generate(3, 0, 300, 64, synth.KIND_GAUSS)
    ix = ram.ShardedMipsIndex(64, device=0)                      # no process group: one rank, the same checks
    ix.add_global(x)
    with pytest.raises(NotImplementedError):
        ix.search_wide(q, ram.MAX_K_WIDE + 1)
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, idx_offset=1)
    with pytest.raises(NotImplementedError):                     # search() keeps its limit
        ix.search(q, 30)
    _same(ix.search_wide(q, 40), ix.local.search_wide(q, 40), "one rank")
    f8 = ram.ShardedMipsIndex(64, dtype="fp8_e4m3", device=0)
    f8.add_global(x)
    with pytest.raises(NotImplementedError):
        f8.search_wide(q, 40)
    with pytest.raises(NotImplementedError):
        f8.local.search_wide_packed(q, 40)
    with pytest.raises(ValueError):                              # the packed payload is a device buffer
        ix.local.search_wide_packed(np.zeros((2, 64), np.float32), 40)
