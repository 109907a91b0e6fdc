"""GPU parity tests (MI355X): the HIP path, called through the C ABI, against the CPU oracle on the
same seeded inputs and against the golden vectors of the real reference.  Bar: indices AND scores
bit-exact against the oracle's canonical definition (integer/index work: exact; the scores are
float32 casts of an exactly defined fp64 sum, so they are compared bit for bit as well); against
the reference's own fp32 scores the tolerance is 1e-3 relative (BASELINE.json north star)."""
import os

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu


def _index(x, metric=0):
    ix = ram.MipsIndex(x.shape[1], metric=metric)
    ix.add(x)
    return ix


def _stored(index):
    """float32 values of the rows as the device holds them (bf16 / e4m3 storage up-cast, fp32-exact storage as it is)."""
    raw = index.rows_raw()
    if index.dtype == "bf16":
        return synth.bf16_bits_to_f32(raw)
    return raw if index.dtype == "f32" else synth.e4m3_bits_to_f32(raw)


def _as_stored(index, q):
    """what the index makes of float32 queries before it multiplies: rounded to its storage type, or left alone (fp32-exact)"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    if index.dtype in ("bf16", "fp8_e4m3_docs"):                 # (e4m3 rows, bf16 queries)
        return synth.round_to_bf16(q)
    return q if index.dtype == "f32" else synth.round_to_e4m3(q)


def _check(ix, q, x, k, metric=0, brute=False, idx_offset=0):
    s, i = ix.search(q, k, idx_offset) if idx_offset else ix.search(q, k)
    fn = orc.search_exact_bruteforce if brute else orc.search_exact
    es, ei = fn(q, x, k, metric=metric, idx_offset=idx_offset)
    assert s.dtype == np.float32 and i.dtype == np.int64 and s.shape == (len(q), k)
    assert np.array_equal(i, ei), f"indices differ in {(i != ei).any(axis=1).sum()} of {len(q)} rows"
    assert np.array_equal(s, es), f"scores differ, max abs {np.abs(s - es).max()}"
    return s, i


# ------------------------------------------------------------------ generators, conversion
@pytest.mark.parametrize("kind", [synth.KIND_LATTICE, synth.KIND_GAUSS, synth.KIND_LATTICE_FP8])
def test_device_generator_matches_host(kind):
    for d, row0, n in ((768, 0, 300), (64, 12345, 130), (1024, 1 << 33, 17)):
        ref = synth.generate(0xD0C5, row0, n, d, kind)
        got = ram.synth_fill(n, d, row0, 0xD0C5, kind, dtype="f32").cpu().numpy()
        assert np.array_equal(got, ref)
        got16 = ram.synth_fill(n, d, row0, 0xD0C5, kind, dtype="bf16").float().cpu().numpy()
        assert np.array_equal(got16, ref)
    ix = ram.MipsIndex(768)
    ix.add_synthetic(257, row0=1000, seed=77, kind=kind)
    assert ix.ntotal == 257
    assert np.array_equal(synth.bf16_bits_to_f32(ix.rows_bf16()), synth.generate(77, 1000, 257, 768, kind))


def test_add_rounds_to_bf16_and_grows():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1000, 100)).astype(np.float32)
    ix = ram.MipsIndex(100)
    ix.add(x[:10])
    ix.add(torch.from_numpy(x[10:300]))                       # host torch
    ix.add(torch.from_numpy(x[300:700]).cuda())               # device f32
    ix.add(torch.from_numpy(x[700:900]).cuda().bfloat16())    # device bf16
    ix.add(synth.bf16_bits(synth.round_to_bf16(x[900:])))     # raw bf16 bits from the host
    assert ix.ntotal == 1000 and ix.d == 100 and len(ix) == 1000
    assert np.array_equal(ix.rows_bf16(), synth.bf16_bits(synth.round_to_bf16(x)))
    assert np.array_equal(ix.rows_bf16(123, 7), synth.bf16_bits(synth.round_to_bf16(x[123:130])))
    ix.reset()
    assert ix.ntotal == 0
    ix.add(x[:5])
    assert np.array_equal(ix.rows_bf16(), synth.bf16_bits(synth.round_to_bf16(x[:5])))
    with pytest.raises(ValueError):
        ix.add(np.zeros((3, 99), np.float32))


# ------------------------------------------------------------------ search parity
def test_lattice_small_bit_exact_with_ties():
    x = synth.generate(5, 0, 1000, 64, synth.KIND_LATTICE)
    q = synth.generate(6, 0, 7, 64, synth.KIND_LATTICE)
    x[10] = x[700]
    x[333] = x[700]              # exact duplicates: ties must resolve to the lowest index
    q[0] = x[700]
    ix = _index(x)
    s, i = _check(ix, q, x, 5, brute=True)
    assert list(i[0][:3]) == [10, 333, 700] and s[0][0] == s[0][1] == s[0][2]


def test_all_equal_scores_return_lowest_indices():
    x = np.ones((500, 64), dtype=np.float32)
    q = np.ones((3, 64), dtype=np.float32)
    s, i = _index(x).search(q, 5)
    assert np.array_equal(i, np.tile(np.arange(5), (3, 1))) and (s == 64.0).all()


def test_cfg1_matches_reference_golden(golden_dir):
    """BASELINE config 1: 10 000 x 768 index, 8 queries, k = 5 -- the indices the REAL reference
    inner_product returned (tests/golden), and its fp32 scores within 1e-3 relative."""
    g = np.load(os.path.join(golden_dir, "g1_g2_inner_product.npz"))
    x = synth.generate(int(g["seed_docs"]), 0, int(g["n"]), int(g["d"]), int(g["kind"]))
    q = g["queries"]
    ix = _index(x)
    s, i = _check(ix, q, x, int(g["k"]))
    assert np.array_equal(i, g["indices_raw"])
    np.testing.assert_allclose(s, g["scores_raw"], rtol=1e-3)
    # the product's brute-force helper (mips.py:552-560 surface), un-normalised
    s2, i2 = ram.inner_product(q, x, k=5, normalize=False)
    assert np.array_equal(i2, g["indices_raw"]) and np.array_equal(s2, s)


@pytest.mark.parametrize("n,nq,d,k", [(100003, 257, 768, 5), (4099, 129, 1024, 10), (777, 5, 100, 1),
                                       (20000, 130, 769, 16), (131, 3, 64, 13), (128, 128, 64, 6),
                                       # query-stationary kernel configurations: d = 1024 (4 waves), 512, 256, padded 500
                                       (70001, 300, 1024, 5), (33, 1, 1024, 3), (50000, 513, 512, 5),
                                       (9000, 40, 256, 4), (12345, 70, 500, 5),
                                       # K' = 10 tier (k = 6, 7; k + 1 = 6 is Mips.search's fetch for top_k = 5 with ignore_indexes)
                                       (100003, 300, 768, 6), (40000, 257, 768, 7), (20011, 64, 1024, 6), (9000, 33, 512, 7),
                                       (3001, 9, 100, 6)])
def test_ragged_shapes_gauss(n, nq, d, k):
    x = synth.generate(21, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(22, 0, nq, d, synth.KIND_GAUSS)
    _check(_index(x), q, x, k)


@pytest.mark.parametrize("k", [1, 5, 6, 7, 8, 13, 14, 29])
def test_k_variants_lattice(k):
    x = synth.generate(31, 0, 5000, 128, synth.KIND_LATTICE)
    q = synth.generate(32, 0, 33, 128, synth.KIND_LATTICE)
    _check(_index(x), q, x, k, brute=True)


def test_k_limits_and_degenerate_calls():
    x = synth.generate(1, 0, 3, 64, synth.KIND_LATTICE)
    q = synth.generate(2, 0, 2, 64, synth.KIND_LATTICE)
    ix = _index(x)
    s, i = _check(ix, q, x, 5, brute=True)                    # k > ntotal: padded
    assert (i[:, 3:] == -1).all() and np.isneginf(s[:, 3:]).all()
    with pytest.raises(NotImplementedError):
        ix.search(q, ram.MAX_K + 1)
    s, i = ix.search(np.zeros((0, 64), np.float32), 4)
    assert s.shape == (0, 4) and i.shape == (0, 4)
    s, i = ix.search(q, 0)
    assert s.shape == (2, 0)
    empty = ram.MipsIndex(64)
    s, i = empty.search(q, 3)
    assert (i == -1).all() and np.isneginf(s).all()
    empty_l2 = ram.MipsIndex(64, metric=ram.METRIC_L2)
    s, i = empty_l2.search(q, 3)
    assert (i == -1).all() and np.isposinf(s).all()


def test_l2_metric_matches_oracle_and_augmented_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "g5_ip_equals_aug_l2.npz"))
    x = synth.generate(int(g["seed_b"]), 0, int(g["n"]), int(g["d"]), int(g["kind"]))
    q = synth.generate(int(g["seed_q"]), 0, int(g["nq"]), int(g["d"]), int(g["kind"]))
    ix = _index(x, metric=ram.METRIC_L2)
    s, i = _check(ix, q, x, int(g["k"]), metric=orc.METRIC_L2)
    assert np.array_equal(i, g["l2_indices"]) and np.array_equal(i, g["ip_indices"])
    np.testing.assert_allclose(s, g["l2_dist"], rtol=1e-3)     # vs brute force on the reference's augmented vectors
    assert (np.diff(s, axis=1) >= 0).all()
    assert ix.phi() == pytest.approx(float(g["phi"]), rel=1e-6)
    # padding in L2 mode
    small = _index(x[:2], metric=ram.METRIC_L2)
    s, i = small.search(q, 4)
    assert (i[:, 2:] == -1).all() and np.isposinf(s[:, 2:]).all()


def test_device_tensors_in_and_out():
    x = synth.generate(41, 0, 3000, 768, synth.KIND_GAUSS)
    q = synth.generate(42, 0, 70, 768, synth.KIND_GAUSS)
    ix = _index(torch.from_numpy(x).cuda())
    es, ei = orc.search_exact(q, x, 5)
    for qt in (torch.from_numpy(q).cuda(), torch.from_numpy(q).cuda().bfloat16()):
        s, i = ix.search(qt, 5)
        assert s.is_cuda and i.is_cuda and s.dtype == torch.float32 and i.dtype == torch.int64
        assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
    s, i = ix.search(torch.from_numpy(q), 5)                   # host torch -> numpy out
    assert np.array_equal(i, ei)


def test_non_bf16_inputs_are_rounded_like_the_oracle():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((5000, 96)).astype(np.float32)
    q = rng.standard_normal((9, 96)).astype(np.float32)
    _check(_index(x), synth.round_to_bf16(q), synth.round_to_bf16(x), 5)
    s, i = _index(x).search(q, 5)
    es, ei = orc.search_exact(synth.round_to_bf16(q), synth.round_to_bf16(x), 5)
    assert np.array_equal(i, ei) and np.array_equal(s, es)


def test_idx_offset_and_shard_merge_equal_full_index():
    n, d, k = 30011, 256, 5
    x = synth.generate(51, 0, n, d, synth.KIND_LATTICE)
    q = synth.generate(52, 0, 140, d, synth.KIND_LATTICE)
    full = _index(x)
    fs, fi = _check(full, q, x, k)
    qd = torch.from_numpy(q).cuda()
    for world in (2, 3, 8):
        ps, pi = [], []
        for r in range(world):
            lo, hi = ram.shard_bounds(n, world, r)
            s, i = _index(x[lo:hi]).search(qd, k, lo)
            ps.append(s)
            pi.append(i)
        cs, ci = torch.cat(ps, dim=1), torch.cat(pi, dim=1)
        ms, mi = ram.merge_topk(cs, ci, world, k)
        assert np.array_equal(mi.cpu().numpy(), fi) and np.array_equal(ms.cpu().numpy(), fs)
        os_, oi_ = orc.merge_topk([p.cpu().numpy() for p in ps], [p.cpu().numpy() for p in pi], k)
        assert np.array_equal(oi_, fi) and np.array_equal(os_, fs)


def test_merge_topk_kernel_padding_and_l2():
    s = torch.tensor([[5., 4., float("-inf"), 5., 1., float("-inf")]]).cuda()
    i = torch.tensor([[9, 3, -1, 2, 7, -1]]).cuda()
    ms, mi = ram.merge_topk(s, i, 2, 3)
    assert mi.cpu().tolist() == [[2, 9, 3]] and ms.cpu().tolist() == [[5., 5., 4.]]
    ms, mi = ram.merge_topk(s, i, 1, 6)
    assert mi.cpu().tolist() == [[2, 9, 3, 7, -1, -1]]
    with pytest.raises(ValueError):
        ram.merge_topk(s, i, 2, 6)
    s2 = torch.tensor([[1., 2., float("inf"), 0.5, 2., float("inf")]]).cuda()
    ms, mi = ram.merge_topk(s2, i, 2, 3, metric=ram.METRIC_L2)
    assert mi.cpu().tolist() == [[2, 9, 3]] and ms.cpu().tolist() == [[0.5, 1., 2.]]


# ------------------------------------------------------------------ facade on the device
def test_l2_normalize_kernel_and_max_norm():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((513, 768)).astype(np.float32) * 3
    x[17] = 0
    xd = torch.from_numpy(x).cuda()
    assert ram.rows_max_sumsq(xd) == pytest.approx(float((x.astype(np.float64) ** 2).sum(1).max()), rel=1e-12)
    ram.l2_normalize_(xd)
    ref = orc.l2_normalization(x.copy())
    np.testing.assert_allclose(xd.cpu().numpy(), ref, rtol=3e-6, atol=1e-8)   # fp32 sum order differs
    assert (xd[17] == 0).all()


@pytest.mark.parametrize("dtype", [None, "bf16"])          # None = the facade's default: fp32-exact storage
@pytest.mark.parametrize("metric,normalize", [(0, True), (0, False), (1, True)])
def test_mips_facade_end_to_end(tmp_path, metric, normalize, dtype):
    n, d, k = 10000, 768, 5
    rng = np.random.default_rng(11)
    emb = (synth.generate(61, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    qs = synth.generate(62, 0, 8, d, synth.KIND_GAUSS)
    data = {"mips_column": [f"text {i}" for i in range(n)], "aid": [f"a{i}" for i in range(n)]}
    args = ram.MipsArgs(mips_topk=k, mips_metric_type=metric, mips_normalize=normalize,
                        mips_tmp_folder=str(tmp_path), log_retriever_metrics=True, **({} if dtype is None else {"mips_index_dtype": dtype}))
    assert ram.MipsArgs().mips_index_dtype == "f32"             # exact on the caller's fp32 values unless asked otherwise
    m = ram.Mips(args, data=data)
    m.build_index(emb)
    assert m.max_norm == pytest.approx(float(np.linalg.norm(emb.astype(np.float64), axis=1).max()), rel=1e-6)
    index = m.embeddings.get_index(m.index_name).faiss_index
    assert index.dtype == (dtype or "f32")
    stored = _stored(index)                                      # what the device actually holds
    if normalize and metric == 0:
        np.testing.assert_allclose(np.linalg.norm(stored, axis=1), 1.0, atol=2e-2 if dtype == "bf16" else 1e-6)
    elif dtype is None:
        assert np.array_equal(stored, emb)                       # fp32-exact storage keeps the embeddings as they came
    pq = m._prepare_query(qs.copy())
    assert np.array_equal(pq, orc.prepare_query(qs.copy(), normalize, metric))
    q_for_oracle = _as_stored(index, pq[:, :d])
    es, ei = orc.search_exact(q_for_oracle, stored, k, metric=metric)
    s, i = m.search(pq, k=k)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    # ignore_indexes: mips.py:388-398
    ignore = [int(ei[j][0]) for j in range(8)]
    s2, i2 = m.search(pq, ignore_indexes=ignore, k=k)
    es2, ei2 = orc.mips_search(lambda qq, kk: orc.search_exact(q_for_oracle, stored, kk, metric=metric), pq, ignore, k)
    assert [list(map(int, r)) for r in i2] == [list(map(int, r)) for r in ei2]
    assert all(ignore[j] not in i2[j] and len(i2[j]) == k for j in range(8))
    # forward + metrics
    out = m.forward(qs.copy(), aid=[f"a{int(ei[j][1])}" for j in range(8)], aid_counts=torch.ones(8), k=k)
    assert out.examples[3][0] == f"text {int(ei[3][0])}" and len(out.flat_texts) == 8 * k
    assert out.metrics["recall"] == pytest.approx(1.0) and out.metrics["reciprocal_rank"] == pytest.approx(1.0)
    # save / load round trip (mips.py:531-549)
    m.save()
    assert m.embeddings is None
    m2 = ram.Mips(args)
    m2.load()
    assert m2.max_norm == m.max_norm
    s3, i3 = m2.search(pq, k=k)
    assert np.array_equal(i3, ei) and np.array_equal(s3, es)
    assert m2.embeddings[int(ei[0][0])]["mips_column"] == f"text {int(ei[0][0])}"
    # full-KB eval surface (retriever_lightning.py:317-321)
    sc, ex = m2.embeddings.get_nearest_examples_batch(m2.index_name, pq[:, :d], k=k)
    assert ex[0]["aid"] == [f"a{int(t)}" for t in ei[0]]


def test_index_save_load_row_range(tmp_path):
    x = synth.generate(71, 0, 5000, 128, synth.KIND_GAUSS)
    q = synth.generate(72, 0, 6, 128, synth.KIND_GAUSS)
    ix = _index(x)
    ix.save(str(tmp_path / "ix"))
    part = ram.MipsIndex.load(str(tmp_path / "ix"), row_range=(1000, 3000))
    assert part.ntotal == 2000
    s, i = part.search(q, 5, 1000)
    es, ei = orc.search_exact(q, x[1000:3000], 5, idx_offset=1000)
    assert np.array_equal(i, ei) and np.array_equal(s, es)


# ------------------------------------------------------------------ BASELINE config 2 at full size
def test_cfg2_full_size_properties_and_oracle_subset():
    """2^20 x 768 bf16 index, Q = 4096, k = 5 (the bench workload).  Oracle on a 48-query subset;
    size-independent properties on all 4096: sortedness with ties by index, returned scores equal
    the canonical re-score of (query, returned doc), a 2-shard split + merge reproduces the result,
    planted duplicates of documents are retrieved as their own nearest neighbour."""
    n, d, nq, k = 1 << 20, 768, 4096, 5
    ix = ram.MipsIndex(d)
    ix.add_synthetic(n, row0=0, seed=synth.SEED_DOCS, kind=synth.KIND_GAUSS)
    qd = ram.synth_fill(nq, d, 0, synth.SEED_QUERIES, synth.KIND_GAUSS, dtype="bf16")
    plant = np.arange(0, 4096, 64)
    rows = torch.from_numpy(synth.bf16_bits_to_f32(np.concatenate(
        [ix.rows_bf16(int(r) * 251 + 5, 1) for r in plant]))).cuda().bfloat16()
    qd[torch.from_numpy(plant).cuda()] = rows
    s, i = ix.search(qd, k)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    q = qd.float().cpu().numpy()
    assert (i >= 0).all() and (i < n).all()
    assert ((np.diff(s, axis=1) < 0) | ((np.diff(s, axis=1) == 0) & (np.diff(i, axis=1) > 0))).all()
    assert np.array_equal(i[plant, 0], plant * 251 + 5)
    # canonical re-score of every returned pair, from independently regenerated rows
    flat = np.unique(i)
    rows = {int(r): synth.generate(synth.SEED_DOCS, int(r), 1, d, synth.KIND_GAUSS)[0] for r in flat}
    docs = np.stack([rows[int(r)] for r in i.reshape(-1)]).reshape(nq, k, d)
    canon = np.stack([orc.canonical_pairs(q[j:j + 1], docs[j], np.arange(k)[None, :])[0] for j in range(nq)])
    assert np.array_equal(canon.astype(np.float32), s)
    # oracle on a subset of queries (chunked fp64 candidates + canonical re-score)
    sub = np.r_[0:32, plant[:16]]
    x = np.concatenate([b for _, b in synth.generate_blocked(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)])
    es, ei = orc.search_exact(q[sub], x, k)
    assert np.array_equal(i[sub], ei) and np.array_equal(s[sub], es)
    del x
    # shard + merge == unsharded
    ps, pi = [], []
    for r in range(2):
        lo, hi = ram.shard_bounds(n, 2, r)
        part = ram.MipsIndex(d)
        part.add_synthetic(hi - lo, row0=lo, seed=synth.SEED_DOCS, kind=synth.KIND_GAUSS)
        a, b = part.search(qd, k, lo)
        ps.append(a)
        pi.append(b)
        del part
    ms, mi = ram.merge_topk(torch.cat(ps, 1), torch.cat(pi, 1), 2, k)
    assert np.array_equal(mi.cpu().numpy(), i) and np.array_equal(ms.cpu().numpy(), s)


# ------------------------------------------------------------------ N > 1 on one GPU (gloo rehearsal)
def _rank_worker_l2(rank, world, port, n, nq, d, k, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        rng = np.random.default_rng(3)
        x = (synth.generate(151, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32)
        x = synth.round_to_bf16(x)                       # shards have very different max norms
        q = synth.generate(152, 0, nq, d, synth.KIND_GAUSS)
        ix = ram.ShardedMipsIndex(d, metric=ram.METRIC_L2, device=0)
        ix.add_global(x)
        s, i = ix.search(torch.from_numpy(q).cuda(), k)
        es, ei = orc.search_exact(q, x, k, metric=orc.METRIC_L2)
        ret[rank] = bool(np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es))
    finally:
        dist.destroy_process_group()


def test_sharded_l2_uses_global_phi():
    import torch.multiprocessing as mp

    port = 29700 + (os.getpid() % 2000)
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker_l2, args=(3, port, 20001, 50, 768, 5, ret), nprocs=3, join=True)
    assert dict(ret) == {r: True for r in range(3)}
    # single-process form of the same thing: per-shard indexes need the common phi
    n, d, k = 9000, 256, 4
    rng = np.random.default_rng(4)
    x = synth.round_to_bf16((synth.generate(153, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
    q = torch.from_numpy(synth.generate(154, 0, 20, d, synth.KIND_GAUSS)).cuda()
    full = _index(x, metric=ram.METRIC_L2)
    fs, fi = full.search(q, k)
    parts = [_index(x[lo:hi], metric=ram.METRIC_L2) for lo, hi in (ram.shard_bounds(n, 2, r) for r in range(2))]
    assert parts[0].phi() != parts[1].phi()
    for p in parts:
        p.set_phi(full.phi())
    out = [p.search(q, k, ram.shard_bounds(n, 2, r)[0]) for r, p in enumerate(parts)]
    ms, mi = ram.merge_topk(torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1), 2, k, metric=ram.METRIC_L2)
    assert torch.equal(mi, fi) and torch.equal(ms, fs)


def _rank_worker(rank, world, port, n, nq, d, k, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        ix = ram.ShardedMipsIndex(d, device=0)          # real HIP local search + device merge kernel
        ix.add_synthetic_global(n, synth.SEED_DOCS, synth.KIND_GAUSS)
        q = ram.synth_fill(nq, d, 0, synth.SEED_QUERIES, synth.KIND_GAUSS)
        s, i = ix.search(q, k)
        torch.cuda.synchronize()
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        es, ei = orc.search_exact(q.float().cpu().numpy(), x, k)
        lo, hi = ram.shard_bounds(n, world, rank)
        ok = bool(np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es) and ix.local.ntotal == hi - lo)
        # k = 10 with stream-ordered certification: every shard scans with optimistic pools, nothing synchronises before the exchange
        ix.set_param("margin_check", 3)
        s10, i10 = ix.search(q, 10)
        torch.cuda.synchronize()
        es10, ei10 = orc.search_exact(q.float().cpu().numpy(), x, 10)
        ok = ok and bool(np.array_equal(i10.cpu().numpy(), ei10) and np.array_equal(s10.cpu().numpy(), es10))
        ok = ok and ix.local.last_kernel.startswith("mips::scan_kernel_v4") and ix.margin_stats()["unresolved"] == 0
        ret[rank] = ok
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_index_multi_rank_on_one_gpu(world):
    """Row shards on `world` processes sharing cuda:0: real device scan per shard, packed all-gather
    (gloo, host staged), device merge -- must equal the oracle on the unsharded index."""
    import torch.multiprocessing as mp

    port = 29600 + (os.getpid() % 2000) + world
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, 50001, 200, 768, 5, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


def test_packed_payload_roundtrip():
    x = synth.generate(81, 0, 9001, 768, synth.KIND_LATTICE)
    q = torch.from_numpy(synth.generate(82, 0, 77, 768, synth.KIND_LATTICE)).cuda()
    k = 5
    full_s, full_i = _index(x).search(q, k)
    parts = []
    for r in range(3):
        lo, hi = ram.shard_bounds(9001, 3, r)
        p = _index(x[lo:hi]).search_packed(q, k, lo)
        assert p.shape == (77, k, 2) and p.dtype == torch.int64
        s_, i_ = _index(x[lo:hi]).search(q, k, lo)
        assert torch.equal(p[..., 1], i_) and torch.equal(p[..., 0].to(torch.int32).view(torch.float32), s_)
        parts.append(p)
    ms, mi = ram.merge_topk_packed(torch.cat(parts, dim=0), 77, 3, k)
    assert torch.equal(mi, full_i) and torch.equal(ms, full_s)
    empty = ram.MipsIndex(768).search_packed(q, k)
    assert (empty[..., 1] == -1).all()


def test_tiny_splits_cold_start_stress():
    """Few blocks per workgroup and hundreds of workgroups starting together: the first block of every
    split is consumed right after the prologue's DMA.  Repeated with cache-evicting traffic in between."""
    rng = np.random.default_rng(5)
    for n, nq, d in ((10000, 8, 768), (313 * 32, 300, 768), (7000, 3, 1024), (9000, 40, 512)):
        x = synth.generate(91, 0, n, d, synth.KIND_GAUSS)
        x /= np.linalg.norm(x, axis=1, keepdims=True)            # small scores, many negative
        q = synth.generate(92, 0, nq, d, synth.KIND_GAUSS)
        ix = _index(x)
        stored = synth.bf16_bits_to_f32(ix.rows_bf16())
        es, ei = orc.search_exact(q, stored, 5)
        junk = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
        for _ in range(12):
            junk.random_(0, 255)                                   # 256 MiB of writes: evicts L2 / Infinity Cache
            s, i = ix.search(q, 5)
            assert np.array_equal(i, ei) and np.array_equal(s, es)


def test_searches_on_two_streams_do_not_share_scratch_in_flight():
    """include/mips_hip.h conventions: calls on one index issued on different streams are ordered by the
    library (event recorded after every call), so back-to-back device-output searches on two streams with
    no synchronisation in between return what the same searches return one at a time."""
    ix = ram.MipsIndex(768)
    ix.add_synthetic(200000, 0, synth.SEED_DOCS, synth.KIND_GAUSS)
    qa = ram.synth_fill(512, 768, 0, 11, synth.KIND_GAUSS)
    qb = ram.synth_fill(512, 768, 0, 12, synth.KIND_GAUSS)
    ra, rb = ix.search(qa, 5), ix.search(qb, 5)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(10):
        with torch.cuda.stream(s1):
            a = ix.search(qa, 5)
        with torch.cuda.stream(s2):
            b = ix.search(qb, 5)
        torch.cuda.synchronize()
        assert torch.equal(a[1], ra[1]) and torch.equal(a[0], ra[0])
        assert torch.equal(b[1], rb[1]) and torch.equal(b[0], rb[0])


def _big_properties(n, d, nq, k, plant_stride, dtype="bf16"):
    """Size-independent checks for indexes too large for the oracle: sortedness (ties by index), planted
    duplicates retrieved as their own nearest neighbour, returned scores == canonical re-score of the
    returned (query, document) pairs from independently regenerated rows, and agreement with the oracle
    restricted to a window of the index that contains every planted document.  dtype "fp8_e4m3": index and
    queries are e4m3-quantised, every check is made on the quantised values."""
    f8 = dtype != "bf16"
    quant = synth.round_to_e4m3 if f8 else (lambda a: a)
    ix = ram.MipsIndex(d, dtype=dtype)
    ix.reserve(n)
    ix.add_synthetic(n, row0=0, seed=synth.SEED_DOCS, kind=synth.KIND_GAUSS)
    qd = ram.synth_fill(nq, d, 0, synth.SEED_QUERIES, synth.KIND_GAUSS, dtype="bf16")
    plant_q = np.arange(0, nq, 16)
    plant_doc = (plant_q.astype(np.int64) * plant_stride + 7) % n
    rows = np.stack([synth.generate(synth.SEED_DOCS, int(r), 1, d, synth.KIND_GAUSS)[0] for r in plant_doc])
    qd[torch.from_numpy(plant_q).cuda()] = torch.from_numpy(quant(rows)).cuda().bfloat16()
    s, i = ix.search(qd, k)
    torch.cuda.synchronize()
    ix.check()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    q = quant(qd.float().cpu().numpy())
    assert (i >= 0).all() and (i < n).all()
    ds, di = np.diff(s, axis=1), np.diff(i, axis=1)
    assert ((ds < 0) | ((ds == 0) & (di > 0))).all()
    assert np.array_equal(i[plant_q, 0], plant_doc)
    uniq = np.unique(i)
    regen = {int(r): quant(synth.generate(synth.SEED_DOCS, int(r), 1, d, synth.KIND_GAUSS))[0] for r in uniq}
    docs = np.stack([regen[int(r)] for r in i.reshape(-1)]).reshape(nq, k, d)
    canon = np.stack([orc.canonical_pairs(q[j:j + 1], docs[j], np.arange(k)[None, :])[0] for j in range(nq)])
    assert np.array_equal(canon.astype(np.float32), s)
    # no document outside the returned set beats the k-th result: check on a random sample of rows
    rng = np.random.default_rng(1)
    sample = rng.integers(0, n, 4096)
    xs = quant(np.concatenate([synth.generate(synth.SEED_DOCS, int(r), 1, d, synth.KIND_GAUSS) for r in sample]))
    sc = (q[:64].astype(np.float64) @ xs.astype(np.float64).T).astype(np.float32)
    kth = s[:64, k - 1][:, None]
    listed = (sample[None, :, None] == i[:64, None, :]).any(-1)
    assert ((sc <= kth) | listed).all()
    return ix.last_scan_ms()


def test_cfg3_size_single_gpu_properties():
    """BASELINE config 3's index (2^24 x 768 bf16, 25.8 GB) on ONE GPU, Q = 4096, k = 5."""
    _big_properties(1 << 24, 768, 4096, 5, 4099)


def test_cfg5_fp8_full_size_properties():
    """BASELINE config 5's index (2^24 x 768 e4m3, 12.9 GB) on ONE GPU, Q = 4096, k = 5 (scan_kernel_f8x)."""
    _big_properties(1 << 24, 768, 4096, 5, 4099, dtype="fp8_e4m3")


def test_cfg4_near_capacity_properties():
    """BASELINE config 4's index (2^26 x 1024 bf16 = 137 GB, near one GPU's 288 GB HBM), Q = 4096, k = 5."""
    _big_properties(1 << 26, 1024, 4096, 5, 16411)


def test_device_resident_hook_matches_host_path(tmp_path):
    """CUDA queries in, CUDA results out -- same answers as the NumPy call surface."""
    n, d, k = 6000, 768, 5
    emb = synth.generate(101, 0, n, d, synth.KIND_GAUSS) * 1.7
    qs = synth.generate(102, 0, 9, d, synth.KIND_GAUSS)
    for metric, normalize in ((0, True), (0, False), (1, True)):
        m = ram.Mips(ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=str(tmp_path)))
        m.build_index(emb)
        hs, hi = m.search(m._prepare_query(qs.copy()), k=k)
        qd = torch.from_numpy(qs).cuda()
        ds, di = m.search_device(qd, k=k)
        assert ds.is_cuda and di.is_cuda and np.array_equal(di.cpu().numpy(), hi)
        if not (normalize and metric == 0):      # device normalisation sums in another fp32 order
            assert np.array_equal(ds.cpu().numpy(), hs)
        ignore = [int(hi[j][j % k]) for j in range(9)]
        fs, fi = m.search(m._prepare_query(qs.copy()), ignore_indexes=ignore, k=k)
        gs, gi = m.search_device(qd, ignore_indexes=torch.tensor(ignore).cuda(), k=k)
        assert gi.shape == (9, k) and np.array_equal(gi.cpu().numpy(), np.array(fi))
        assert torch.equal(qd, torch.from_numpy(qs).cuda())        # caller's tensor untouched
    # filter kernel vs the oracle's list semantics, incl. a missing id and padding
    s = torch.tensor([[.9, .8, .7, .6], [.5, .4, .3, .2], [.1, float("-inf"), float("-inf"), float("-inf")]]).cuda()
    i = torch.tensor([[4, 9, 2, 7], [1, 3, 5, 8], [6, -1, -1, -1]]).cuda()
    os_, oi_ = ram.filter_ignore(s, i, [9, 77, 6], 3)
    es, ei = orc.filter_ignore(s.cpu().numpy(), i.cpu().numpy(), [9, 77, 6], 3)
    assert oi_.cpu().tolist() == [list(map(int, r)) for r in ei]
    assert torch.equal(os_.cpu(), torch.tensor(np.array(es, dtype=np.float32)))


def test_cosine_rescore_kernel():
    torch.manual_seed(0)
    q = torch.randn(7, 1, 768, device="cuda")
    c = torch.randn(7, 5, 768, device="cuda")
    ref = orc.cosine_rescore(q.cpu(), c.cpu())
    out = ram.cosine_rescore(q, c)
    assert out.shape == (7, 5) and torch.allclose(out.cpu(), ref, atol=2e-6, rtol=1e-5)
    out16 = ram.cosine_rescore(q.bfloat16(), c.bfloat16())
    ref16 = orc.cosine_rescore(q.bfloat16().float().cpu(), c.bfloat16().float().cpu())
    assert torch.allclose(out16.cpu(), ref16, atol=2e-6, rtol=1e-5)
    # memory_bias of the hook (retriever_generator.py:188-192) written by the same launch
    for mem_len, qq, cc in ((16, q, c), (131, q.bfloat16(), c.bfloat16())):
        sc, bias = ram.cosine_rescore(qq, cc, memory_seq_len=mem_len)
        assert torch.equal(sc, ram.cosine_rescore(qq, cc))
        assert bias.shape == (7, 5 * mem_len) and torch.equal(bias.cpu(), orc.memory_bias(sc.cpu(), mem_len))


# ------------------------------------------------------------------ fp8 e4m3 index (BASELINE config 5)
def _f8_index(x, metric=0):
    ix = ram.MipsIndex(x.shape[1], metric=metric, dtype="fp8_e4m3")
    ix.add(x)
    return ix


def test_fp8_quantizer_device_matches_host():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(3000).astype(np.float32) * s for s in (1e-3, 0.05, 1, 30, 300)])
    edge = np.array([0, -0.0, 448, 449, 463.9, 464, 1e9, -1e9, 2 ** -9, 2 ** -10, 2 ** -10 * 1.0001, 0.0175,
                     np.inf, -np.inf, 2 ** -6, 2 ** -6 * 0.99, 240, 232, 0.0625 * 1.0625], dtype=np.float32)
    x = np.concatenate([x, edge, np.zeros(768 * 20 - len(x) - len(edge), np.float32)]).reshape(20, 768)
    ix = _f8_index(x)
    assert np.array_equal(ix.rows_raw(), synth.e4m3_bits(x))
    ix2 = ram.MipsIndex(768, dtype="fp8_e4m3")
    ix2.add(torch.from_numpy(x).cuda().bfloat16())                 # bf16 source: quantised from the bf16 value
    assert np.array_equal(ix2.rows_raw(), synth.e4m3_bits(synth.round_to_bf16(x)))
    ix3 = ram.MipsIndex(768, dtype="fp8_e4m3")
    ix3.add(synth.e4m3_bits(x))                                    # raw codes pass through
    assert np.array_equal(ix3.rows_raw(), synth.e4m3_bits(x))
    for kind in (synth.KIND_LATTICE_FP8, synth.KIND_GAUSS):
        dev = ram.synth_fill(70, 768, 123, 9, kind, dtype="fp8_e4m3").cpu().numpy()
        assert np.array_equal(dev, synth.e4m3_bits(synth.generate(9, 123, 70, 768, kind)))


@pytest.mark.parametrize("n,nq,d,k", [(5000, 40, 768, 5), (70001, 300, 768, 5), (4099, 129, 1024, 10), (3000, 7, 256, 1),
                                       (9000, 70, 500, 13), (33, 2, 512, 5), (30001, 260, 768, 6)])
def test_fp8_index_parity(n, nq, d, k):
    """Index and queries quantised to e4m3; the oracle consumes the same quantised values."""
    for kind in (synth.KIND_LATTICE_FP8, synth.KIND_GAUSS):
        x = synth.generate(111, 0, n, d, kind)
        q = synth.generate(112, 0, nq, d, kind)
        xq, qq = synth.round_to_e4m3(x), synth.round_to_e4m3(q)
        if kind == synth.KIND_LATTICE_FP8:
            assert np.array_equal(xq, x)                            # lattice values are e4m3-exact
        ix = _f8_index(x)
        assert np.array_equal(synth.e4m3_bits_to_f32(ix.rows_raw()), xq)
        s, i = ix.search(q, k)
        fn = orc.search_exact_bruteforce if kind == synth.KIND_LATTICE_FP8 and n <= 9000 else orc.search_exact
        es, ei = fn(qq, xq, k)
        if kind == synth.KIND_LATTICE_FP8 and n > 9000:
            continue                                                # ties need the brute-force oracle: small n only
        assert np.array_equal(i, ei), f"kind {kind}: {(i != ei).any(axis=1).sum()} rows differ"
        assert np.array_equal(s, es)


@pytest.mark.parametrize("dtype", ["bf16", "fp8_e4m3"])
def test_duplicates_crowding_one_sub_list(dtype):
    """Worst case for the 16x16 kernels' sub-lists (4 per (query, split), 6 entries each): many IDENTICAL best
    documents whose rows all fall into the same sub-list (stride 16 inside one split).  Their scores tie
    exactly, the strict '>' keeps the lowest indices, and the top 5 are the 5 lowest-index copies."""
    n, d, nq = 40000, 768, 300
    kind = synth.KIND_LATTICE_FP8 if dtype != "bf16" else synth.KIND_GAUSS
    x = synth.generate(191, 0, n, d, kind)
    q = synth.generate(192, 0, nq, d, kind)
    star = np.abs(synth.generate(193, 0, 1, d, kind)[0]) + 1.0       # large positive entries: beats every random row
    if dtype != "bf16":
        star = synth.round_to_e4m3(star)
    rows = 1003 + 16 * np.arange(40)
    x[rows] = star
    q[::7] = star                                                     # these queries have 40 tied best documents
    ix = ram.MipsIndex(d, dtype=dtype)
    ix.add(x)
    stored = synth.bf16_bits_to_f32(ix.rows_bf16()) if dtype == "bf16" else synth.e4m3_bits_to_f32(ix.rows_raw())
    qq = synth.round_to_bf16(q) if dtype == "bf16" else synth.round_to_e4m3(q)   # what the device scores with
    tied = np.arange(0, nq, 7)
    free = np.setdiff1d(np.arange(nq), tied)
    es, ei = orc.search_exact(qq[free], stored, 5)                    # tie-free queries: the fast oracle
    ts, ti = orc.search_exact_bruteforce(qq[tied[:6]], stored, 5)     # tied ones: full enumeration (tie-safe), a few
    assert np.array_equal(ti, np.tile(rows[:5], (6, 1)))
    for variant in (0, 3, 4):
        ix.set_param("variant", variant)
        s, i = ix.search(q, 5)
        assert np.array_equal(i[tied], np.tile(rows[:5], (len(tied), 1))), variant
        assert np.array_equal(s[tied[:6]], ts) and (s[tied] == s[tied[0], 0]).all(), variant
        # the other queries may rank the 40 copies among their best as well: the fast oracle is not tie-safe, so
        # compare scores everywhere, indices where no copy is involved, and demand the LOWEST copies otherwise
        assert np.array_equal(s[free], es), variant
        copy_g, copy_o = np.isin(i[free], rows), np.isin(ei, rows)
        assert np.array_equal(copy_g, copy_o) and np.array_equal(i[free][~copy_g], ei[~copy_o]), variant
        for row_i, row_c in zip(i[free], copy_g):
            m = int(row_c.sum())
            assert np.array_equal(row_i[row_c], rows[:m]), variant


def _async_worker(rank, port, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        sh = ram.ShardedMipsIndex(768, device=0)
        sh.add_synthetic_global(60000, synth.SEED_DOCS, synth.KIND_GAUSS)
        qs = [ram.synth_fill(300, 768, 0, 400 + t, synth.KIND_GAUSS) for t in range(6)]
        refs = [sh.search(qq, 5) for qq in qs]                       # one rank: the plain local search
        torch.cuda.synchronize()
        # pipelined: every batch's scan is enqueued before any result is asked for; the exchange step (RCCL
        # all-gather over the single rank + merge kernel) runs on the side stream
        pend = [sh.search_async(qq, 5, _force_collective=True) for qq in qs]
        ok = True
        for p_, r_ in zip(pend, refs):
            s, i = p_.result()
            torch.cuda.synchronize()
            ok = ok and torch.equal(i, r_[1]) and torch.equal(s, r_[0])
        ret["ok"] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_search_async_pipelines_the_exchange_step():
    """ShardedMipsIndex.search_async: local scan on the caller's stream, all-gather + merge on a side stream;
    checked here through a one-rank RCCL group (the multi-rank data path is the same call sequence)."""
    import torch.multiprocessing as mp

    ret = mp.Manager().dict()
    mp.spawn(_async_worker, args=(29800 + (os.getpid() % 1500), ret), nprocs=1, join=True)
    assert ret.get("ok") is True


def test_device_search_is_graph_capturable():
    """A device-in / device-out search in steady state (scratch already sized) issues only stream operations, so
    a caller may capture it into a HIP graph (torch.cuda.graph) and replay it with new query values."""
    ix = ram.MipsIndex(768)
    ix.add_synthetic(30000, 0, synth.SEED_DOCS, synth.KIND_GAUSS)
    q = ram.synth_fill(40, 768, 0, 21, synth.KIND_GAUSS)
    q2 = ram.synth_fill(40, 768, 0, 22, synth.KIND_GAUSS)
    ref1, ref2 = ix.search(q, 5), ix.search(q2, 5)
    torch.cuda.synchronize()
    buf = q.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                    # warm-up off the default stream, as torch asks for
        ix.search(buf, 5)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s, i = ix.search(buf, 5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(i, ref1[1]) and torch.equal(s, ref1[0])
    buf.copy_(q2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(i, ref2[1]) and torch.equal(s, ref2[0])


def test_l2_results_are_ordered_by_the_float32_distance():
    """Found by tools/fuzz.py: two documents whose inner products differ can round to the SAME float32 distance
    next to |q|^2 + phi; the order is then by index, not by the hidden inner product."""
    n, nq, d, k = 47010, 526, 768, 16
    x = synth.generate(7146, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(8146, 0, nq, d, synth.KIND_GAUSS)
    ix = ram.MipsIndex(d, metric=ram.METRIC_L2)
    ix.add(x)
    s, i = ix.search(q, k)
    es, ei = orc.search_exact(q, x, k, metric=orc.METRIC_L2)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    ties = (np.diff(s, axis=1) == 0)
    assert ties.any() and (np.diff(i, axis=1)[ties] > 0).all()       # the case does contain equal distances


def test_fp8_scan_kernels_are_bit_identical():
    """The fp8 index has two scan kernels: scan_kernel_f8x (16x16x128 MFMA shape, 64-document blocks; default
    for k <= 5 and d <= 768) and scan_kernel_f8 (32x32x64; "variant" = 3 forces it).  Same bits, ragged sizes
    and single- / multi-tile query counts included."""
    for n, nq, d in ((150001, 700, 768), (64 * 37 + 5, 40, 768), (20000, 300, 512), (7001, 9, 200)):
        ix = ram.MipsIndex(d, dtype="fp8_e4m3")
        ix.add_synthetic(n, row0=0, seed=181, kind=synth.KIND_GAUSS)
        q = ram.synth_fill(nq, d, 0, 182, synth.KIND_GAUSS)
        ref_s, ref_i = ix.search(q, 5)
        ix.set_param("variant", 3)
        s, i = ix.search(q, 5)
        assert torch.equal(i, ref_i) and torch.equal(s, ref_s), (n, nq, d)
        ix.set_param("variant", 0)
        ix.set_param("nsplit", 40)
        s, i = ix.search(q, 5)
        assert torch.equal(i, ref_i) and torch.equal(s, ref_s), (n, nq, d)


def test_fp8_index_l2_padding_limits_and_persistence(tmp_path):
    x = synth.generate(121, 0, 2000, 768, synth.KIND_GAUSS)
    q = synth.generate(122, 0, 5, 768, synth.KIND_GAUSS)
    xq, qq = synth.round_to_e4m3(x), synth.round_to_e4m3(q)
    ix = _f8_index(x, metric=ram.METRIC_L2)
    s, i = ix.search(q, 4)
    es, ei = orc.search_exact(qq, xq, 4, metric=orc.METRIC_L2)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    small = _f8_index(x[:3])
    s, i = small.search(q, 5)
    assert (i[:, 3:] == -1).all() and np.isneginf(s[:, 3:]).all()
    with pytest.raises(RuntimeError, match="k <= 13"):
        small.search(q, 14)
    with pytest.raises(RuntimeError, match="d <= 1024"):
        ram.MipsIndex(2000, dtype="fp8_e4m3")
    ix.save(str(tmp_path / "f8"))
    back = ram.MipsIndex.load(str(tmp_path / "f8"))
    assert back.dtype == "fp8_e4m3" and np.array_equal(back.rows_raw(), ix.rows_raw())
    s2, i2 = back.search(torch.from_numpy(q).cuda(), 4)
    assert np.array_equal(i2.cpu().numpy(), ei)


def test_c_abi_from_plain_c(tmp_path):
    """The boundary is a C ABI: a plain-C program (no Python, no torch, host buffers) links libmips_hip.so,
    builds an index, searches, and checks the result against integer arithmetic of its own."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


def test_nan_and_inf_documents_follow_flat_index_semantics():
    """NaN scores never rank (FAISS heap comparisons are false for NaN; NumPy's argsort puts them last);
    +inf scores rank first, ties by index; -inf scores rank last among real documents."""
    x = synth.generate(131, 0, 600, 64, synth.KIND_LATTICE)
    q = np.abs(synth.generate(132, 0, 4, 64, synth.KIND_LATTICE)) + 0.25      # strictly positive queries
    x[5, 3] = np.nan
    x[77, :] = np.nan
    x[300, 0] = np.inf
    x[100, 0] = np.inf
    x[450, 1] = -np.inf
    ix = _index(x)
    s, i = ix.search(q, 5)
    es, ei = orc.search_exact_bruteforce(q, x, 5)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    assert (i[:, 0] == 100).all() and (i[:, 1] == 300).all() and np.isposinf(s[:, :2]).all()
    assert not np.isin(i, [5, 77, 450]).any()
    s, i = ix.search(q, 29)
    es, ei = orc.search_exact_bruteforce(q, x, 29)
    assert np.array_equal(i, ei) and np.array_equal(s, es)


def test_many_queries_and_non_default_stream():
    n, nq, d, k = 20000, 9001, 768, 5
    x = synth.generate(141, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(142, 0, nq, d, synth.KIND_GAUSS)
    es, ei = orc.search_exact(q, x, k)
    ix = _index(x)
    s, i = ix.search(q, k)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    side = torch.cuda.Stream()
    qd = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):                       # work is enqueued on the CURRENT torch stream
        s2, i2 = ix.search(qd, k)
        s3, i3 = ix.search(qd[:100], k)
    side.synchronize()
    assert np.array_equal(i2.cpu().numpy(), ei) and np.array_equal(s2.cpu().numpy(), es)
    assert np.array_equal(i3.cpu().numpy(), ei[:100])


# ------------------------------------------------------------------ fp32-exact index (the reference's own data type)
def test_f32_exact_index_matches_reference_on_fp32_data(golden_dir):
    """Golden G1b: the REAL reference `inner_product` on plain fp32 (not bf16-representable) inputs, raw
    and normalised.  The fp32-exact index returns the reference's indices; scores agree to fp32 rounding
    (ours are the exactly-rounded sums) and are bit-identical to the oracle's canonical definition."""
    g = np.load(os.path.join(golden_dir, "g1b_inner_product_f32.npz"))
    x, y, k = g["x"], g["y"], int(g["k"])
    assert not np.array_equal(synth.round_to_bf16(y), y)            # really needs more than bf16
    ix = ram.MipsIndex(y.shape[1], dtype="f32")
    ix.add(y)
    assert np.array_equal(ix.rows_raw(), y)
    s, i = ix.search(x, k)
    assert np.array_equal(i, g["indices_raw"])
    np.testing.assert_allclose(s, g["scores_raw"], rtol=2e-6, atol=1e-6)
    es, ei = orc.search_exact(x, y, k)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    # normalised variant (mips.py:554-556): same fp32 normalisation as the reference, then exact search
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    yn = y / np.linalg.norm(y, axis=1, keepdims=True)
    ixn = ram.MipsIndex(y.shape[1], dtype="f32")
    ixn.add(yn)
    s, i = ixn.search(xn, k)
    assert np.array_equal(i, g["indices_norm"])
    np.testing.assert_allclose(s, g["scores_norm"], rtol=2e-6, atol=1e-7)
    # a bf16 index on the same data is allowed to differ -- that is what this mode is for
    sb, ib = _index(y).search(x, k)
    assert ib.shape == i.shape


@pytest.mark.parametrize("n,nq,d,k,metric", [(10000, 8, 768, 5, 0), (30001, 130, 768, 10, 0), (5000, 33, 100, 5, 1),
                                               (4000, 5, 1024, 29, 0)])
def test_f32_exact_index_parity(tmp_path, n, nq, d, k, metric):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ix = ram.MipsIndex(d, metric=metric, dtype="f32")
    ix.add(x[: n // 2])
    ix.add(torch.from_numpy(x[n // 2:]).cuda())
    s, i = ix.search(q, k)
    es, ei = orc.search_exact(q, x, k, metric=metric)
    assert np.array_equal(i, ei), f"{(i != ei).any(axis=1).sum()} rows differ"
    assert np.array_equal(s, es)
    sd, idd = ix.search(torch.from_numpy(q).cuda(), k)
    assert np.array_equal(idd.cpu().numpy(), ei)
    if n == 10000:
        # the literal fp32 NumPy path of the reference (oracle port) picks the same neighbours
        rs, ri = orc.inner_product(q, x, k, normalize=False)
        assert np.array_equal(ri, i)
        np.testing.assert_allclose(rs, s, rtol=1e-5, atol=1e-5)
        ix.save(str(tmp_path / "f32"))
        back = ram.MipsIndex.load(str(tmp_path / "f32"))
        s2, i2 = back.search(q, k)
        assert back.dtype == "f32" and np.array_equal(i2, ei) and np.array_equal(s2, es)


@pytest.mark.parametrize("n,nq,d,k,metric", [(60000, 700, 768, 5, 0), (20000, 40, 300, 6, 1), (9000, 300, 1000, 5, 0), (30000, 100, 500, 12, 0)])
def test_f32_exact_two_stage_search(n, nq, d, k, metric):
    """fp32-exact index, k <= 7, host buffers: stage 1 scans bf16(x) with the fast bf16 kernels and re-scores on the fp32
    rows; the margin check -- widened by |x - bf16 x| |q| + |bf16 x| |q - bf16 q| -- sends what it cannot certify to the
    three-segment scan.  Same bits as the oracle and as the one-stage search ("f32_fast" = 0); device-output searches
    keep the one-stage scan unless "f32_fast" = 2."""
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    es, ei = orc.search_exact(q, x, k, metric=metric)
    ix = ram.MipsIndex(d, metric=metric, dtype="f32")
    ix.add(x[:n // 3])
    s, i = ix.search(q[:5], k)                                    # (bf16 rows are converted lazily: more rows follow)
    ix.add(x[n // 3:])
    s, i = ix.search(q, k)
    assert not ix.last_kernel.startswith("mips::scan_kernel<"), ix.last_kernel   # a query-stationary bf16 kernel, pitch 1024 included
    if d > 768:   # (round 3: pools of 32 at pitch 1024 -- scan_kernel_k3's sub-lists beyond 256 queries, true K' = 32 lists below)
        assert ix.last_kernel.startswith("mips::scan_kernel_k3<4, 32, 2, 0, 4>" if nq > 256 else "mips::scan_kernel_v3<32, 64, 1, 4"), ix.last_kernel
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    st = ix.margin_stats()
    assert st["flagged"] >= 0 and st["rescanned"] == st["flagged"] and st["unresolved"] == 0
    print("two-stage:", n, nq, d, k, metric, ix.last_kernel, st)
    assert st["flagged"] < max(2, nq // 10)                       # Gaussian rows: stage 1 certifies nearly all (K' = 32 pools)
    qd = torch.from_numpy(q).cuda()
    ix.set_param("f32_fast", 1)
    sd, idd = ix.search(qd, k)                                    # device outputs: two-stage as well, certified on the stream
    assert not ix.last_kernel.startswith("mips::scan_kernel<")   # default margin mode: nothing synchronises
    st_d = ix.margin_stats()
    assert st_d["rescanned"] == st_d["flagged"] and st_d["unresolved"] == 0
    assert np.array_equal(idd.cpu().numpy(), ei) and np.array_equal(sd.cpu().numpy(), es)
    ix.set_param("margin_check", 0)                               # no certificate, no two-stage search
    sd, idd = ix.search(qd, k)
    assert ix.last_kernel.startswith("mips::scan_kernel<")
    assert np.array_equal(idd.cpu().numpy(), ei) and np.array_equal(sd.cpu().numpy(), es)
    ix.set_param("margin_check", 1)
    ix.set_param("f32_fast", 2)                                   # forced: stage 1 even where flagged queries are only counted
    ix.set_param("margin_check", 1)
    sd, idd = ix.search(qd, k)
    assert not ix.last_kernel.startswith("mips::scan_kernel<")
    rows_ok = (idd.cpu().numpy() == ei).all(axis=1)
    assert rows_ok.sum() >= nq - max(0, ix.margin_stats()["flagged"])     # every certified query is exact
    ix.set_param("f32_fast", 0)
    s0, i0 = ix.search(q, k)
    assert ix.last_kernel.startswith("mips::scan_kernel<") and np.array_equal(i0, ei) and np.array_equal(s0, es)


@pytest.mark.parametrize("n,nq,d,k", [(50000, 600, 768, 10), (30000, 70, 500, 13), (20000, 300, 384, 8)])
def test_optimistic_pools_for_k_8_to_13(n, nq, d, k):
    """bf16 index, 8 <= k <= 13, host buffers (a call that certifies): the pool of 32 comes out of the 16x16x32 kernel's
    sub-lists of 6 and the margin check decides per query; flagged queries are re-scanned with true K' = 32 lists.  Same
    bits as the oracle and as the K' = 16 lists ("optimistic" = 0 / device outputs)."""
    x = synth.generate(401, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(402, 0, nq, d, synth.KIND_GAUSS)
    es, ei = orc.search_exact(q, x, k)
    ix = _index(x)
    s, i = ix.search(q, k)
    assert ix.last_kernel.startswith("mips::scan_kernel_v4"), ix.last_kernel
    st = ix.margin_stats()
    print("optimistic:", n, nq, d, k, ix.last_kernel, st)
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    assert st["unresolved"] == 0 and st["rescanned"] == st["flagged"]
    sd, idd = ix.search(torch.from_numpy(q).cuda(), k)           # device outputs: the same, certified on the stream
    assert ix.last_kernel.startswith("mips::scan_kernel_v4")
    assert np.array_equal(idd.cpu().numpy(), ei) and np.array_equal(sd.cpu().numpy(), es)
    ix.set_param("margin_check", 0)                               # no certificate: true K' = 16 lists
    sd, idd = ix.search(torch.from_numpy(q).cuda(), k)
    assert not ix.last_kernel.startswith("mips::scan_kernel_v4")
    assert np.array_equal(idd.cpu().numpy(), ei) and np.array_equal(sd.cpu().numpy(), es)
    ix.set_param("margin_check", 1)
    ix.set_param("optimistic", 0)
    s0, i0 = ix.search(q, k)
    assert not ix.last_kernel.startswith("mips::scan_kernel_v4") and np.array_equal(i0, ei) and np.array_equal(s0, es)
    # crowd one sub-list: rows congruent mod 16 inside one split, all near the top of query 0 -> that query must be flagged or exact
    y = x.copy()
    for j in range(12):
        y[160 + 16 * j] = q[0] * np.float32(1.0 + 0.01 * j)
    y = synth.round_to_bf16(y)
    ix2 = _index(y)
    es2, ei2 = orc.search_exact(q, y, k)
    s2, i2 = ix2.search(q, k)
    assert np.array_equal(i2, ei2) and np.array_equal(s2, es2)


def test_optimistic_pools_agree_with_true_lists_at_full_size():
    """BASELINE config 2's index (2^20 x 768), k = 10: optimistic pools of 32 out of the 16x16x32 kernel's sub-lists (each
    sub-list vouching for its 4th best: 8 classes x 4 = 32 documents above the shared insert bound) against true K' = 16 and
    K' = 32 lists.  With the 8-document bound of the k <= 5 instances two of these 4096 queries lost their 10th neighbour
    uncertified -- this size is what showed it."""
    ix = ram.MipsIndex(768)
    ix.add_synthetic(1 << 20, 0, synth.SEED_DOCS, synth.KIND_GAUSS)
    q = ram.synth_fill(4096, 768, 0, synth.SEED_QUERIES, synth.KIND_GAUSS)
    ix.set_param("margin_check", 2)
    ix.set_param("optimistic", 0)
    s0, i0 = ix.search(q, 10)
    assert ix.last_kernel.startswith("mips::scan_kernel_v3<16")
    ix.set_param("optimistic", 1)
    s1, i1 = ix.search(q, 10)
    assert ix.last_kernel.startswith("mips::scan_kernel_v4") and ix.last_kernel.endswith(", 4>")
    assert ix.margin_stats()["unresolved"] == 0
    s2, i2 = ix.search(q, 14)                                     # (round 3: k = 14 .. 29 take the pools of 32 as well)
    assert ix.last_kernel.startswith("mips::scan_kernel_v4") and ix.last_kernel.endswith(", 4>") and ix.margin_stats()["unresolved"] == 0
    ix.set_param("optimistic", 0)
    s3, i3 = ix.search(q, 14)
    assert ix.last_kernel.startswith("mips::scan_kernel_v3<32")
    assert torch.equal(i0, i1) and torch.equal(s0, s1)
    assert torch.equal(i0, i2[:, :10]) and torch.equal(s0, s2[:, :10])
    assert torch.equal(i2, i3) and torch.equal(s2, s3)


def test_f32_exact_two_stage_near_duplicates():
    """Near-duplicate clusters: bf16(x) cannot separate the members, nearly every query goes to the second stage -- the
    results must not care (and stage 1 is skipped for the next calls)."""
    rng = np.random.default_rng(5)
    c = rng.standard_normal((300, 768)).astype(np.float32)
    x = (np.repeat(c, 40, axis=0) * (1.0 + 1e-4 * rng.standard_normal((12000, 1)))).astype(np.float32)
    x += (1e-4 * rng.standard_normal(x.shape)).astype(np.float32)
    q = (c[rng.integers(0, 300, 64)] + 0.01 * rng.standard_normal((64, 768))).astype(np.float32)
    es, ei = orc.search_exact(q, x, 5)
    ix = ram.MipsIndex(768, dtype="f32")
    ix.add(x)
    for rep in range(3):
        s, i = ix.search(q, 5)
        assert np.array_equal(i, ei) and np.array_equal(s, es), rep
        if rep == 0:
            assert ix.margin_stats()["flagged"] > 16 and not ix.last_kernel.startswith("mips::scan_kernel<")
        else:
            assert ix.last_kernel.startswith("mips::scan_kernel<")   # stage 1 skipped after the call that did not pay


def test_f32_exact_synthetic_and_ties():
    ix = ram.MipsIndex(768, dtype="f32")
    ix.add_synthetic(3000, row0=10, seed=5, kind=synth.KIND_LATTICE)
    x = synth.generate(5, 10, 3000, 768, synth.KIND_LATTICE)
    assert np.array_equal(ix.rows_raw(), x)
    q = synth.generate(6, 0, 9, 768, synth.KIND_LATTICE)
    s, i = ix.search(q, 5)
    es, ei = orc.search_exact_bruteforce(q, x, 5)
    assert np.array_equal(i, ei) and np.array_equal(s, es)


def test_np_search_is_inner_product_even_on_an_l2_index(tmp_path):
    """Mips.np_search (mips.py:527-529) is the reference's exhaustive inner-product cross-check whatever the
    index metric; on the L2 index it must not return distances."""
    n, d, k = 4000, 768, 4
    emb = synth.generate(161, 0, n, d, synth.KIND_GAUSS) * 1.3
    qs = synth.generate(162, 0, 6, d, synth.KIND_GAUSS)
    m = ram.Mips(ram.MipsArgs(mips_metric_type=1, mips_normalize=False, mips_tmp_folder=str(tmp_path)))
    m.build_index(emb)
    s, i = m.np_search(qs, k)
    stored = _stored(m.embeddings.get_index(m.index_name).faiss_index)
    es, ei = orc.search_exact(_as_stored(m.embeddings.get_index(m.index_name).faiss_index, qs), stored, k, metric=orc.METRIC_INNER_PRODUCT)
    assert np.array_equal(i, ei) and np.array_equal(s, es) and (np.diff(s, axis=1) <= 0).all()
    s2, i2 = m.search(m._prepare_query(qs.copy()), k=k)          # the index itself still answers in L2
    assert (np.diff(s2, axis=1) >= 0).all() and np.array_equal(i2, ei)   # same neighbours (IP == augmented L2)


def test_experimental_scan_variants_are_bit_identical():
    """Launch-tuning knobs never change results: the 16x16x32 kernel (variant 4), the 6-entry-list forms
    (sub 10 / 11), the s_barrier form (sub 3), the other insert-bound schemes (sub 4 none, sub 6 shared K'-th
    bests, sub 15 class maxima re-read every block), the generic kernel (variant 1) and other split counts
    all return the shipped configuration's bits."""
    n, nq, d, k = 150001, 700, 768, 5
    ix = ram.MipsIndex(d)
    ix.add_synthetic(n, row0=0, seed=171, kind=synth.KIND_GAUSS)
    q = ram.synth_fill(nq, d, 0, 172, synth.KIND_GAUSS)
    ref_s, ref_i = ix.search(q, k)
    x = synth.generate(171, 0, n, d, synth.KIND_GAUSS)
    es, ei = orc.search_exact(q.float().cpu().numpy()[:64], x, k)
    assert np.array_equal(ref_i[:64].cpu().numpy(), ei) and np.array_equal(ref_s[:64].cpu().numpy(), es)
    for params in ({"variant": 4}, {"variant": 3}, {"variant": 1}, {"variant": 3, "nsplit": 40}, {"variant": 3, "qgroups": 2},
                   {"variant": 4, "nsplit": 8}, {"variant": 4, "qgroups": 4},
                   {"variant": 5}, {"variant": 5, "nsplit": 40}):   # 5 / 6 select kernels of the A/B library; the shipped one ignores them
        for name in ("variant", "nsplit", "qgroups"):
            ix.set_param(name, params.get(name, 0))
        s, i = ix.search(q, k)
        assert torch.equal(i, ref_i) and torch.equal(s, ref_s), params
    # the experimental `sub` instances (several of them wrong by design) went with the retired A/B library
    with pytest.raises(RuntimeError, match="experimental"):
        ix.set_param("sub", 8)
    ix.set_param("sub", 0)


# ------------------------------------------------------------------ scan-error word on every path
def test_scan_timeout_poisons_and_raises_on_every_path():
    """A scan kernel whose block barrier gives up must never return plausible garbage.  "spin_limit" = -1 makes
    every launch raise its error word (test-only knob): the exact re-score then writes idx = IDX_POISON / NaN
    into every slot, raises the sticky host flag, and the failure surfaces as RuntimeError -- on the host path at
    once, on the device-output / packed / sharded paths through check() or the next call; the cross-shard merge
    propagates poison so a timed-out shard cannot drop out of a global top-k silently."""
    n, d, nq, k = 60000, 768, 700, 5
    for dtype in ("bf16", "fp8_e4m3"):
        ix = ram.MipsIndex(d, dtype=dtype)
        ix.add_synthetic(n, 0, synth.SEED_DOCS, synth.KIND_GAUSS)
        q = ram.synth_fill(nq, d, 0, synth.SEED_QUERIES, synth.KIND_GAUSS)
        ref_s, ref_i = ix.search(q, k)
        ix.check()                                                    # healthy index: nothing raised
        for variant, nqq in ((0, nq), (3, nq), (0, 100)):             # v4 / f8x, v3 / f8, single-tile nt kernel
            ix.set_param("variant", variant)
            ix.set_param("spin_limit", -1)
            s, i = ix.search(q[:nqq], k)                              # device output: no exception here
            torch.cuda.synchronize()
            assert (i == ram.IDX_POISON).all() and torch.isnan(s).all(), (dtype, variant)
            with pytest.raises(RuntimeError, match="gave up"):
                ix.check()
            ix.check()                                                # reported once, then cleared
            p = ix.search_packed(q[:nqq], k, 1000)                    # the all-gather payload is poisoned as well
            torch.cuda.synchronize()
            assert (p[..., 1] == ram.IDX_POISON).all()
            with pytest.raises(RuntimeError, match="gave up"):        # ... and the NEXT call on the index reports it
                ix.search(q[:nqq], k)
            with pytest.raises(RuntimeError, match="gave up"):        # host buffers: raised by the call itself
                ix.search(q[:nqq].float().cpu().numpy(), k)
            ix.set_param("spin_limit", 0)
            s, i = ix.search(q[:nqq], k)
            ix.check()
            assert torch.equal(i, ref_i[:nqq]) and torch.equal(s, ref_s[:nqq]), (dtype, variant)
        ix.set_param("variant", 0)
    # a tiny REAL spin bound: either nothing timed out (results exact) or the call is poisoned and reported
    ix = ram.MipsIndex(d)
    ix.add_synthetic(n, 0, synth.SEED_DOCS, synth.KIND_GAUSS)
    ref_s, ref_i = ix.search(q, k)
    ix.set_param("spin_limit", 1)
    s, i = ix.search(q, k)
    torch.cuda.synchronize()
    if (i == ram.IDX_POISON).any():
        assert (i == ram.IDX_POISON).all() and torch.isnan(s).all()
        with pytest.raises(RuntimeError, match="gave up"):
            ix.check()
    else:
        ix.check()
        assert torch.equal(i, ref_i) and torch.equal(s, ref_s)
    ix.set_param("spin_limit", 0)
    # stream-ordered certification ("margin_check" = 3) enqueues a re-scan behind every search: it must not touch the poison
    ix.set_param("margin_check", 3)
    ix.search(q, k)
    ix.set_param("spin_limit", -1)
    s, i = ix.search(q, k)
    torch.cuda.synchronize()
    assert (i == ram.IDX_POISON).all() and torch.isnan(s).all()
    with pytest.raises(RuntimeError, match="gave up"):
        ix.check()
    ix.set_param("spin_limit", 0)
    s, i = ix.search(q, k)
    ix.check()
    assert torch.equal(i, ref_i) and torch.equal(s, ref_s)
    ix.set_param("margin_check", 1)
    # merge kernels: one poisoned shard poisons the merged rows
    good = ix.search_packed(q, k, 0)
    bad = good.clone()
    bad[5] = torch.tensor([0x7fc00000, ram.IDX_POISON], device="cuda")
    ms, mi = ram.merge_topk_packed(torch.cat([good, bad], 0), nq, 2, k)
    assert (mi[5] == ram.IDX_POISON).all() and torch.isnan(ms[5]).all() and (mi[:5] >= 0).all() and (mi[6:] >= 0).all()
    cs = torch.cat([ref_s, ref_s], 1)
    ci = torch.cat([ref_i, ref_i + n], 1)
    ci[7, 3] = ram.IDX_POISON
    ms, mi = ram.merge_topk(cs, ci, 2, k)
    assert (mi[7] == ram.IDX_POISON).all() and torch.isnan(ms[7]).all() and (mi[8] >= 0).all()


def _timeout_worker(rank, world, port, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        sh = ram.ShardedMipsIndex(768, device=0)
        sh.add_synthetic_global(40000, synth.SEED_DOCS, synth.KIND_GAUSS)
        q = ram.synth_fill(300, 768, 0, synth.SEED_QUERIES, synth.KIND_GAUSS)
        ref = sh.search(q, 5)
        if rank == 1:
            sh.local.set_param("spin_limit", -1)                      # only rank 1's shard times out
        s, i = sh.search(q, 5)
        torch.cuda.synchronize()
        poisoned = bool((i == ram.IDX_POISON).all() and torch.isnan(s).all())   # EVERY rank sees it in the results
        raised = False
        try:
            sh.check()
        except RuntimeError:
            raised = True
        sh.local.set_param("spin_limit", 0)
        s2, i2 = sh.search(q, 5)
        ret[rank] = (poisoned, raised, bool(torch.equal(i2, ref[1]) and torch.equal(s2, ref[0])))
    finally:
        dist.destroy_process_group()


def test_scan_timeout_on_one_shard_reaches_every_rank():
    import torch.multiprocessing as mp

    ret = mp.Manager().dict()
    mp.spawn(_timeout_worker, args=(2, 29900 + (os.getpid() % 1500), ret), nprocs=2, join=True)
    assert dict(ret) == {0: (True, False, True), 1: (True, True, True)}


# ------------------------------------------------------------------ a9 / f4: the full-KB eval consumer, a10: in-batch scoring
@pytest.mark.parametrize("dtype", [None, "bf16"])          # None = add_faiss_index's default: fp32-exact storage
@pytest.mark.parametrize("d", [768, 1024])
@pytest.mark.parametrize("inner_product", [False, True])
def test_full_kb_eval_call_text(d, inner_product, dtype):
    """retriever_lightning.py:372-404 + 313-321 replayed against KnowledgeBase: phi-augment the `cls` column
    (default, L2) or keep it (inner_product=True), `add_faiss_index(column="cls", index_name="mips_cls",
    metric_type=metric)`, then `get_nearest_examples_batch("mips_cls", queries=augment_xq(q) | q, k=top_k)`."""
    n, nq, top_k = 6000, 16, 5
    rng = np.random.default_rng(d)
    cls = (synth.generate(201, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.4, 1.6, (n, 1))).astype(np.float32)
    query_cls = synth.generate(202, 0, nq, d, synth.KIND_GAUSS)
    kb_cols = {"mips_column": [f"abstract {t}" for t in range(n)], "aid": [[f"a{t}", f"b{t % 7}"] for t in range(n)]}
    column, metric = orc.full_kb_eval_index(cls, inner_product)                 # what the reference puts into "cls"
    kb = ram.KnowledgeBase(dict(kb_cols, cls=column))
    kb.add_faiss_index(column="cls", index_name="mips_cls", metric_type=metric, **({} if dtype is None else {"dtype": dtype}))
    q = query_cls if inner_product else ram.augment_xq(query_cls)               # :313-315
    scores, examples = kb.get_nearest_examples_batch("mips_cls", queries=q, k=top_k)
    index = kb.get_index("mips_cls").faiss_index
    assert index.d == d and index.metric_type == metric and index.ntotal == n and index.dtype == (dtype or "f32")
    stored = _stored(index)
    np.testing.assert_array_equal(stored, _as_stored(index, cls))               # the augmentation column is not stored
    es, ex = orc.nearest_examples_batch(lambda qq, kk: orc.search_exact(_as_stored(index, qq[:, :d]), stored, kk, metric=metric),
                                        kb_cols, q, top_k)
    assert len(scores) == nq and all(np.array_equal(a, b) for a, b in zip(scores, es))
    assert [e["aid"] for e in examples] == [e["aid"] for e in ex]
    assert [e["mips_column"] for e in examples] == [e["mips_column"] for e in ex]
    if not inner_product:
        # the distances are those of brute force on the reference's augmented fp32 vectors (1e-3: bf16 storage)
        d2 = ((orc.augment_xq(query_cls).astype(np.float64)[:, None, :] - column.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        np.testing.assert_allclose(np.stack(scores), np.sort(d2, axis=1)[:, :top_k], rtol=2e-2 if dtype == "bf16" else 1e-4)
        with pytest.raises(ValueError, match="not zero"):
            bad = q.copy()
            bad[0, -1] = 1.0
            kb.get_nearest_examples_batch("mips_cls", queries=bad, k=top_k)
        with pytest.raises(NotImplementedError, match="phi-augmented"):
            ram.KnowledgeBase(dict(cls=cls)).add_faiss_index(column="cls", metric_type=ram.METRIC_L2)   # not augmented
    # metrics of :327-335 on CUDA tensors == the oracle's (golden G4 pins the oracle)
    pred = torch.tensor([[f"a{int(ex[j]['aid'][0][0][1:])}" in a for a in e["aid"]] for j, e in enumerate(examples)]).float()
    counts = torch.ones(nq)
    assert ram.retriever_metrics(pred.cuda(), counts.cuda()) == pytest.approx(orc.retriever_metrics(pred, counts))


def test_fp32_exact_eval_index_returns_the_reference_neighbours():
    """The same call text on plain fp32 embeddings with dtype="f32": the neighbours of an fp64 brute force on the
    reference's augmented vectors, distances to fp32 rounding."""
    n, d, nq, top_k = 5000, 768, 16, 5
    rng = np.random.default_rng(5)
    cls = (rng.standard_normal((n, d)) * rng.uniform(0.4, 1.6, (n, 1))).astype(np.float32)
    query_cls = rng.standard_normal((nq, d)).astype(np.float32)
    column, metric = orc.full_kb_eval_index(cls, False)
    kb = ram.KnowledgeBase(dict(cls=column, mips_column=list(range(n))))
    kb.add_faiss_index(column="cls", index_name="mips_cls", metric_type=metric, dtype="f32")
    scores, examples = kb.get_nearest_examples_batch("mips_cls", queries=ram.augment_xq(query_cls), k=top_k)
    d2 = ((orc.augment_xq(query_cls).astype(np.float64)[:, None, :] - column.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    assert [e["mips_column"] for e in examples] == np.argsort(d2, axis=1)[:, :top_k].tolist()
    np.testing.assert_allclose(np.stack(scores), np.sort(d2, axis=1)[:, :top_k], rtol=1e-4)


@pytest.mark.parametrize("normalize", [True, False])
def test_in_batch_scoring(normalize):
    """a10 -- retriever_lightning.py:304-305 (and the normalised form of :273-277), B = 16, topk(1)."""
    torch.manual_seed(3)
    b, d = 16, 768
    query_cls = torch.randn(b, d)
    mips_cls = query_cls[torch.randperm(b)] * 0.8 + 0.6 * torch.randn(b, d)      # a noisy permutation: top-1 is non-trivial
    es, ei = orc.in_batch_scores(query_cls, mips_cls, normalize)
    s, i = ram.in_batch_scores(query_cls.cuda(), mips_cls.cuda(), normalize=normalize)
    assert s.shape == (b, b) and torch.equal(i.cpu(), ei)
    torch.testing.assert_close(s.cpu(), es, rtol=1e-3, atol=1e-5)                # north-star tolerance on scores
    acc = (i.cpu() == torch.arange(b)).float().mean()                             # :306-308 consume it like this
    assert acc == (ei == torch.arange(b)).float().mean()
    s16, i16 = ram.in_batch_scores(query_cls.cuda().bfloat16(), mips_cls.cuda().bfloat16(), normalize=normalize)
    assert i16.shape == (b,)


def test_inner_product_normalized_matches_reference_golden(golden_dir):
    """Golden G2: the REAL reference inner_product(..., normalize=True) on the config-1 shape."""
    g = np.load(os.path.join(golden_dir, "g1_g2_inner_product.npz"))
    x = synth.generate(int(g["seed_docs"]), 0, int(g["n"]), int(g["d"]), int(g["kind"]))
    # the default (fp32-exact index): the reference's neighbours and scores (the normalised rows are NOT bf16 values)
    s32, i32 = ram.inner_product(g["queries"], x, k=int(g["k"]), normalize=True)
    assert np.array_equal(i32, g["indices_norm"])
    np.testing.assert_allclose(s32, g["scores_norm"], rtol=2e-6, atol=1e-7)
    # bf16 storage, an explicit opt-in: exact on the bf16-ROUNDED normalised rows, so against the fp32
    # reference a near-tie may legitimately swap; the neighbour SETS and the scores still agree closely
    s, i = ram.inner_product(g["queries"], x, k=int(g["k"]), normalize=True, dtype="bf16")
    assert np.array_equal(i[:, 0], g["indices_norm"][:, 0])
    same = [len(set(a) & set(b)) for a, b in zip(i.tolist(), g["indices_norm"].tolist())]
    assert min(same) >= int(g["k"]) - 1 and sum(same) >= 8 * int(g["k"]) - 2
    np.testing.assert_allclose(s, g["scores_norm"], rtol=5e-3)


# ------------------------------------------------------------------ the hook's re-score is differentiable like the reference's
def test_cosine_rescore_gradients_match_the_reference_expression():
    """retriever_generator.py:158-172: only the norms are under no_grad; memory_bias carries the retrieval
    gradient to the query / memory encoders.  Gradient parity with the torch expression, fp32 and bf16."""
    torch.manual_seed(1)
    b, k, d, mem_len = 6, 5, 768, 37
    for dt, tol in ((torch.float32, 2e-5), (torch.bfloat16, 2e-2)):
        q0 = torch.randn(b, 1, d, device="cuda").to(dt)
        c0 = torch.randn(b, k, d, device="cuda").to(dt)
        w_s = torch.randn(b, k, device="cuda")
        w_b = torch.randn(b, k * mem_len, device="cuda")
        # reference expression (oracle restatement with the norms under no_grad, as in the reference)
        q, c = q0.clone().float().requires_grad_(True), c0.clone().float().requires_grad_(True)
        sc = (q @ c.transpose(1, 2)).squeeze(1)
        with torch.no_grad():
            nrm = (torch.norm(q, dim=2, keepdim=True) * torch.norm(c, dim=2, keepdim=True)).squeeze(2)
        sc = sc / nrm
        bias = orc.memory_bias(sc, mem_len)
        ((sc * w_s).sum() + (bias * w_b).sum()).backward()
        # product
        q2, c2 = q0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        sc2, bias2 = ram.cosine_rescore(q2, c2, memory_seq_len=mem_len)
        assert sc2.requires_grad and bias2.requires_grad
        ((sc2 * w_s).sum() + (bias2 * w_b).sum()).backward()
        assert q2.grad.shape == q0.shape and c2.grad.shape == c0.shape and q2.grad.dtype == dt
        torch.testing.assert_close(sc2, sc.detach(), rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(q2.grad.float(), q.grad, rtol=tol, atol=tol * q.grad.abs().max().item())
        torch.testing.assert_close(c2.grad.float(), c.grad, rtol=tol, atol=tol * c.grad.abs().max().item())
        # scores only (no bias), and no graph when nothing requires grad
        q3 = q0.clone().requires_grad_(True)
        sc3 = ram.cosine_rescore(q3, c0)
        sc3.sum().backward()
        assert q3.grad is not None and not ram.cosine_rescore(q0, c0).requires_grad


# ------------------------------------------------------------------ the facade row-shards under a process group
def _facade_shard_worker(rank, world, port, tmp, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        n, d, k = 9001, 768, 5
        rng = np.random.default_rng(17)
        emb = (synth.generate(211, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.2, (n, 1))).astype(np.float32)
        qs = synth.generate(212, 0, 8, d, synth.KIND_GAUSS)
        data = {"mips_column": [f"text {t}" for t in range(n)], "aid": [f"a{t}" for t in range(n)]}
        ok = True
        for metric, normalize in ((0, True), (1, True)):
            folder = os.path.join(tmp, f"m{metric}")
            args = ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=folder, mips_shard=True,
                                mips_device=0, mips_batch_size=1000)
            m = ram.Mips(args, data=data)
            m.encoder = lambda texts: emb[[int(t.split()[1]) for t in texts]]   # stands in for the SPECTER2 encoder
            # ---- the call text of lightning_model.py:168-180, unchanged
            m.init_embeddings_folder()
            dist.barrier()
            m.encode_text2(rank=rank, num_rank=world)
            dist.barrier()
            m.build_index()
            m.save()
            dist.barrier()
            m.rebuilt_steps.append(1)
            m.load()
            # ----
            index = m.embeddings.get_index(m.index_name).faiss_index
            lo, hi = ram.shard_bounds(n, world, rank)
            ok &= isinstance(index, ram.ShardedMipsIndex) and index.local.ntotal == hi - lo and index.ntotal == n
            whole = ram.Mips(ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=folder, mips_device=0))
            whole.load()                                                         # the reference's replicated form
            ok &= isinstance(whole.embeddings.get_index(m.index_name).faiss_index, ram.MipsIndex)
            pq = m._prepare_query(qs.copy())
            s1, i1 = whole.search(pq, k=k)
            s2, i2 = m.search(pq, k=k)
            ok &= np.array_equal(i1, i2) and np.array_equal(s1, s2)
            ignore = [int(i1[j][j % k]) for j in range(8)]
            a, b = whole.search(pq, ignore_indexes=ignore, k=k), m.search(pq, ignore_indexes=ignore, k=k)
            ok &= [list(map(int, r)) for r in a[1]] == [list(map(int, r)) for r in b[1]] and \
                [list(map(float, r)) for r in a[0]] == [list(map(float, r)) for r in b[0]]
            qd = torch.from_numpy(qs).cuda()
            ds1, di1 = whole.search_device(qd, ignore_indexes=torch.tensor(ignore).cuda(), k=k)
            ds2, di2 = m.search_device(qd, ignore_indexes=torch.tensor(ignore).cuda(), k=k)
            ok &= torch.equal(di1, di2) and torch.equal(ds1, ds2)
            n1, n2 = whole.np_search(qs, k), m.np_search(qs, k)
            ok &= np.array_equal(n1[1], n2[1]) and np.array_equal(n1[0], n2[0])
            out1, out2 = whole.forward(qs.copy(), k=k), m.forward(qs.copy(), k=k)
            ok &= out1.examples == out2.examples and m.max_norm == whole.max_norm and m.phi == whole.phi
            # vs the oracle on the stored rows
            stored = _stored(whole.embeddings.get_index(m.index_name).faiss_index)
            es, ei = orc.search_exact(_as_stored(whole.embeddings.get_index(m.index_name).faiss_index, pq[:, :d]), stored, k, metric=metric)
            ok &= np.array_equal(i2, ei) and np.array_equal(s2, es)
            # ---- collective build without the disk round trip, then a collective save read back by one process
            c = ram.Mips(ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=folder + "c",
                                      mips_shard=True, mips_device=0), data=data)
            c.build_index_sharded(emb)
            s3, i3 = c.search(pq, k=k)
            ok &= np.array_equal(i3, i1) and np.array_equal(s3, s1) and c.max_norm == pytest.approx(whole.max_norm, rel=1e-12)
            ok &= (c.phi == whole.phi)
            c.save()
            dist.barrier()
            back = ram.Mips(ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=folder + "c", mips_device=0))
            back.load()
            s4, i4 = back.search(pq, k=k)
            ok &= np.array_equal(i4, i1) and np.array_equal(s4, s1)
            dist.barrier()
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_facade_row_shards_under_a_process_group(tmp_path):
    """MipsArgs.mips_shard: the reference's own rebuild call text (lightning_model.py:168-180) leaves every rank
    with ITS row range of the index; Mips.search / search_device / np_search / forward return what the replicated
    index returns, bit for bit, inner product and L2 (2 gloo ranks sharing cuda:0)."""
    import torch.multiprocessing as mp

    ret = mp.Manager().dict()
    mp.spawn(_facade_shard_worker, args=(2, 29300 + (os.getpid() % 1500), str(tmp_path), ret), nprocs=2, join=True)
    assert dict(ret) == {0: True, 1: True}


def test_sharded_l2_save_load_and_incremental_add(tmp_path):
    """(1) MipsIndex.save persists phi and load(row_range) restores the FILE's phi, so a shard loaded
    alone measures the same distances as the whole index; (2) after set_phi an incremental add followed by
    _sync_phi sees the new, larger norms."""
    n, d, k = 8000, 256, 4
    rng = np.random.default_rng(9)
    x = synth.round_to_bf16((synth.generate(221, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
    x[n - 1] *= 4.0                                                   # the global maximum norm sits in the LAST shard
    x = synth.round_to_bf16(x)
    q = synth.generate(222, 0, 12, d, synth.KIND_GAUSS)
    full = _index(x, metric=ram.METRIC_L2)
    fs, fi = full.search(q, k)
    full.save(str(tmp_path / "l2"))
    parts = [ram.MipsIndex.load(str(tmp_path / "l2"), row_range=ram.shard_bounds(n, 2, r)) for r in range(2)]
    assert parts[0].phi() == parts[1].phi() == full.phi()
    out = [p.search(torch.from_numpy(q).cuda(), k, ram.shard_bounds(n, 2, r)[0]) for r, p in enumerate(parts)]
    ms, mi = ram.merge_topk(torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1), 2, k, metric=ram.METRIC_L2)
    assert np.array_equal(mi.cpu().numpy(), fi) and np.array_equal(ms.cpu().numpy(), fs)
    es, ei = orc.search_exact(q, x, k, metric=orc.METRIC_L2)
    assert np.array_equal(fi, ei) and np.array_equal(fs, es)
    # (2) override, add bigger rows, drop the override: phi follows
    p0 = parts[0]
    old = p0.phi()
    big = synth.round_to_bf16(x[:3] * 50.0)
    p0.add(big)
    assert p0.phi() == old                                            # still the override
    p0.clear_phi()
    assert p0.phi() > old and p0.phi() == pytest.approx(float((big.astype(np.float64) ** 2).sum(1).max()), rel=1e-12)


# ------------------------------------------------------------------ margin check: thin margins are detected, not assumed away
def _near_duplicate_case(n=40000, d=768, nq=300, ncopy=10):
    """Adversarial for the 16x16 kernels' sub-lists AND for fp32 accumulation.  Every document carries +1 on the first
    256 coordinates and -1 on the last 256; the "star" queries carry 16 there, so for them every MFMA chain climbs to
    4096, adds the informative middle part (|score| <= 256) at a granularity of 2^-11, and comes back -- the fp64
    canonical score keeps 2^-15.  `ncopy` near-duplicates of the star document differ by ONE bf16 ulp steps in a
    coordinate the star query weighs 2^-7: exact scores rise by 2^-14 per copy (distinct float32 values), MFMA scores
    are (nearly) tied.  The copies sit 16 rows apart inside one split: one sub-list of 6 for all of them, which keeps the
    LOWEST indices on ties -- while the exact top 5 are the HIGHEST-index copies."""
    rng = np.random.default_rng(77)
    x = synth.generate(231, 0, n, d, synth.KIND_GAUSS)
    x[:, :256] = 1.0
    x[:, 512:] = -1.0
    q = synth.generate(232, 0, nq, d, synth.KIND_GAUSS)
    sign = np.where(rng.random(256) < 0.5, -1.0, 1.0).astype(np.float32)
    star_x = np.ones(d, np.float32)
    star_x[512:] = -1.0
    star_x[256:512] = sign
    star_q = np.full(d, 16.0, np.float32)
    star_q[256:512] = sign
    j = 300
    star_q[j] = 2.0 ** -7
    rows = 1003 + 16 * np.arange(ncopy)
    for t, r in enumerate(rows):
        x[r] = star_x
        x[r, j] = 1.0 + t * 2.0 ** -7                       # t bf16 ulps above 1.0
    stars = np.arange(0, nq, 7)
    q[stars] = star_q
    assert np.array_equal(synth.round_to_bf16(x), x) and np.array_equal(synth.round_to_bf16(q), q)
    return x, q, rows, stars


@pytest.mark.parametrize("nq", [300, 100])                  # > 256: scan_kernel_v4 (4 sub-lists of 6); <= 256: scan_kernel_v3
def test_near_duplicates_crowding_one_sub_list_are_certified(nq):
    x, q, rows, stars = _near_duplicate_case(nq=nq)
    k = 5
    ix = _index(x)
    es, ei = orc.search_exact_bruteforce(q[stars], x, k)     # tie-safe full enumeration for the star queries
    assert np.array_equal(ei, np.tile(rows[::-1][:k], (len(stars), 1)))          # the k HIGHEST-index copies, best first
    assert len(np.unique(es[0])) == k                                            # distinct canonical float32 scores
    free = np.setdiff1d(np.arange(nq), stars)
    fs, fi = orc.search_exact(q[free], x, k)
    # NumPy in / out: the search synchronises anyway, so flagged queries are re-scanned with the widest lists
    s, i = ix.search(q, k)
    st = ix.margin_stats()
    assert np.array_equal(i[stars], ei) and np.array_equal(s[stars], es)
    assert np.array_equal(i[free], fi) and np.array_equal(s[free], fs)
    assert st["flagged"] >= len(stars) and st["rescanned"] == st["flagged"] and st["unresolved"] == 0, st
    # the older way to settle flagged queries -- re-scan with the widest lists instead of the exact brute-force pass -- still
    # serves rows of more than 1024 columns and searches that flag more than 1024 queries; same answer here
    ix.set_param("resolve", 0)
    s0, i0 = ix.search(q, k)
    assert np.array_equal(i0, i) and np.array_equal(s0, s) and ix.margin_stats()["rescanned"] == st["flagged"]
    ix.set_param("resolve", 1)
    # device tensors: certified by default as well -- WITHOUT a synchronisation (the exact pass is enqueued behind the scan) ...
    qd = torch.from_numpy(q).cuda()
    ds, di = ix.search(qd, k)
    assert ix.margin_stats() == st
    assert np.array_equal(di.cpu().numpy()[stars], ei) and np.array_equal(ds.cpu().numpy()[stars], es)
    assert np.array_equal(di.cpu().numpy()[free], fi) and np.array_equal(ds.cpu().numpy()[free], fs)
    # ... "margin_check" = 4 only COUNTS the flagged queries (the first results stand) ...
    ix.set_param("margin_check", 4)
    ds, di = ix.search(qd, k)
    st1 = ix.margin_stats()
    assert st1["flagged"] == st["flagged"] and st1["rescanned"] == 0 and st1["unresolved"] == st["flagged"]
    # ... 2 certifies and synchronises to read the counts
    ix.set_param("margin_check", 2)
    ds, di = ix.search(qd, k)
    assert ix.margin_stats() == st
    assert np.array_equal(di.cpu().numpy()[stars], ei) and np.array_equal(ds.cpu().numpy()[stars], es)
    assert np.array_equal(di.cpu().numpy()[free], fi)
    pk = ix.search_packed(qd, k, 500)                         # the packed payload is patched the same way
    assert np.array_equal(pk[..., 1].cpu().numpy()[stars], ei + 500)
    # ... or certified WITHOUT a synchronisation: the re-scan is enqueued behind the first scan, sized for all queries,
    # and reads the flagged count on the device (mode 3); a graph replay does the same
    ix.set_param("margin_check", 3)
    for rep in range(3):
        ds, di = ix.search(qd, k)
    st3 = ix.margin_stats()
    assert st3 == st, (st3, st)
    assert np.array_equal(di.cpu().numpy()[stars], ei) and np.array_equal(ds.cpu().numpy()[stars], es)
    assert np.array_equal(di.cpu().numpy()[free], fi) and np.array_equal(ds.cpu().numpy()[free], fs)
    pk = ix.search_packed(qd, k, 500)
    assert np.array_equal(pk[..., 1].cpu().numpy()[stars], ei + 500) and np.array_equal(pk[..., 1].cpu().numpy()[free], fi + 500)
    # split-tail searches (scan on the current stream, select + re-score + the certificate on another): three in flight
    tail = torch.cuda.Stream()
    outs = [ix.search(qd, k, tail_stream=tail) for _ in range(3)]
    torch.cuda.synchronize()
    for ts, ti in outs:
        assert np.array_equal(ti.cpu().numpy()[stars], ei) and np.array_equal(ts.cpu().numpy()[stars], es)
        assert np.array_equal(ti.cpu().numpy()[free], fi) and np.array_equal(ts.cpu().numpy()[free], fs)
    assert ix.margin_stats() == st
    g = torch.cuda.CUDAGraph()
    buf = qd.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ix.search(buf, k)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        gs, gi = ix.search(buf, k)
    buf.copy_(qd.flip(0))                                     # other queries through the captured launches
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(gi.flip(0).cpu().numpy()[stars], ei) and np.array_equal(gi.flip(0).cpu().numpy()[free], fi)
    # off: no flags, no statistics
    ix.set_param("margin_check", 0)
    ix.search(q, k)
    assert ix.margin_stats()["flagged"] in (-1, 0)


def test_stream_ordered_certification_opens_the_fast_paths_to_device_outputs():
    """ "margin_check" = 3: device-output searches certify without synchronising, so they may take the paths that depend on
    the certificate -- optimistic pools for 8 <= k <= 13 and the two-stage search of the fp32-exact index -- and stay exact
    where those paths flag nearly everything (near-duplicate clusters)."""
    x = synth.generate(411, 0, 40000, 768, synth.KIND_GAUSS)
    q = synth.generate(412, 0, 500, 768, synth.KIND_GAUSS)
    qd = torch.from_numpy(q).cuda()
    es, ei = orc.search_exact(q, x, 10)
    ix = _index(x)
    ix.set_param("margin_check", 3)
    s, i = ix.search(qd, 10)
    assert ix.last_kernel.startswith("mips::scan_kernel_v4") and ix.last_kernel.endswith(", 4>")
    assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
    assert ix.margin_stats()["unresolved"] == 0
    # fp32-exact index, clustered rows
    rng = np.random.default_rng(5)
    c = rng.standard_normal((300, 768)).astype(np.float32)
    y = (np.repeat(c, 40, axis=0) * (1.0 + 1e-4 * rng.standard_normal((12000, 1)))).astype(np.float32)
    y += (1e-4 * rng.standard_normal(y.shape)).astype(np.float32)
    qq = (c[rng.integers(0, 300, 200)] + 0.01 * rng.standard_normal((200, 768))).astype(np.float32)
    es, ei = orc.search_exact(qq, y, 5)
    f = ram.MipsIndex(768, dtype="f32")
    f.add(y)
    f.set_param("margin_check", 3)
    s, i = f.search(torch.from_numpy(qq).cuda(), 5)
    assert not f.last_kernel.startswith("mips::scan_kernel<")        # stage 1 on the bf16 rows
    st = f.margin_stats()
    assert st["flagged"] > 50 and st["rescanned"] == st["flagged"], st   # (40 members within 1e-4 of each other: the widest
    assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)   # lists cannot CERTIFY these either)
    g = rng.standard_normal((30000, 768)).astype(np.float32)            # well-separated rows: nothing to re-scan
    qg = rng.standard_normal((300, 768)).astype(np.float32)
    f2 = ram.MipsIndex(768, dtype="f32")
    f2.add(g)
    f2.set_param("margin_check", 3)
    s, i = f2.search(torch.from_numpy(qg).cuda(), 5)
    es, ei = orc.search_exact(qg, g, 5)
    assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es) and f2.margin_stats()["flagged"] == 0


def test_margin_check_on_ordinary_data_flags_few_and_changes_nothing():
    """Gaussian data: the rigorous error bound (d 2^-23 |q| |x|, ~0.07 at score scale 130) flags a few per cent of the
    queries; re-scanning them returns the same rows (the first pass was right), every mode returns the oracle's bits."""
    n, d, nq, k = 100003, 768, 600, 5
    x = synth.generate(241, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(242, 0, nq, d, synth.KIND_GAUSS)
    es, ei = orc.search_exact(q, x, k)
    for dtype in ("bf16", "fp8_e4m3"):
        xx, qq = (x, q) if dtype == "bf16" else (synth.round_to_e4m3(x), synth.round_to_e4m3(q))
        es, ei = orc.search_exact(qq, xx, k)
        ix = ram.MipsIndex(d, dtype=dtype)
        ix.add(x)
        s, i = ix.search(q, k)                                 # certified (host buffers)
        st = ix.margin_stats()
        assert np.array_equal(i, ei) and np.array_equal(s, es)
        assert 0 <= st["flagged"] <= nq // 4 and st["rescanned"] == st["flagged"] and st["unresolved"] <= st["flagged"], (dtype, st)
        ds, di = ix.search(torch.from_numpy(q).cuda(), k)      # device outputs: certified on the stream
        assert np.array_equal(di.cpu().numpy(), ei) and ix.margin_stats() == st
    l2 = _index(x, metric=ram.METRIC_L2)
    s, i = l2.search(q, 10)                                    # K' = 16 first pass, L2 distances, rescan with K' = 32
    es, ei = orc.search_exact(q, x, 10, metric=orc.METRIC_L2)
    assert np.array_equal(i, ei) and np.array_equal(s, es) and l2.margin_stats()["unresolved"] <= l2.margin_stats()["flagged"]


# ------------------------------------------------------------------ the reference's own call shape in one launch
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("n,nq,d,k,metric", [(10000, 8, 768, 5, 0), (33, 16, 768, 5, 0), (65536, 3, 1024, 6, 0), (4099, 16, 100, 1, 0),
                                               (10000, 8, 768, 5, 1), (3, 2, 64, 5, 0), (20011, 11, 512, 4, 1)])
def test_tiny_search_is_the_general_path_in_one_launch(n, nq, d, k, metric, dtype):
    """<= 16 queries on a small bf16 or fp32-exact index take tiny_search_kernel (staging + MFMA scan + select + exact
    re-score in ONE launch): bit-identical to the general path ("tiny" = 0) and to the oracle, NumPy and CUDA call shapes,
    packed payload and row offsets included; the ticket of its last-workgroup hand-off survives repeated calls.  The
    fp32-exact index scans bf16(x) . bf16(q) and re-scores on the fp32 rows (sequential fp64, the canonical sum)."""
    x = synth.generate(251, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(252, 0, nq, d, synth.KIND_GAUSS)
    if dtype == "f32":   # rows that are NOT bf16 values (the queries stay bf16 values: the bfloat16 call below is lossless)
        x = (x * np.random.default_rng(n).uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    es, ei = orc.search_exact(q, x, k, metric=metric, idx_offset=700)
    ix = ram.MipsIndex(d, metric=metric, dtype=dtype)
    ix.add(x)
    qd = torch.from_numpy(q).cuda()
    for rep in range(3):
        s, i = ix.search(q, k, 700)
        assert ix.last_kernel.startswith("mips::tiny_search_kernel")
        assert np.array_equal(i, ei) and np.array_equal(s, es), rep
        ds, di = ix.search(qd, k, 700)
        assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(ds.cpu().numpy(), es)
        ds, di = ix.search(qd.bfloat16(), k, 700)
        assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(ds.cpu().numpy(), es)
    pk = ix.search_packed(qd, k, 700)
    assert np.array_equal(pk[..., 1].cpu().numpy(), ei)
    assert np.array_equal(pk[..., 0].to(torch.int32).view(torch.float32).cpu().numpy(), es)
    st = ix.margin_stats()
    ix.set_param("tiny", 0)
    gs, gi = ix.search(qd, k, 700)
    assert not ix.last_kernel.startswith("mips::tiny") and torch.equal(gi, di) and torch.equal(gs, ds)
    if dtype == "bf16":
        assert ix.margin_stats()["flagged"] == st["flagged"]      # the same queries are flagged by either path
    else:                                                         # (fp32-exact: pools of 32 there, 8 + refined scores here)
        assert ix.margin_stats()["unresolved"] == 0 and st["unresolved"] == 0
    if dtype == "f32":   # queries that are not bf16 values either
        q2 = (q * np.random.default_rng(nq).uniform(0.5, 2.0, (nq, 1))).astype(np.float32)
        es2, ei2 = orc.search_exact(q2, x, k, metric=metric)
        ix.set_param("tiny", 1)
        s2, i2 = ix.search(torch.from_numpy(q2).cuda(), k)
        assert ix.last_kernel.startswith("mips::tiny_search_kernel") and ix.last_kernel.endswith("true>")
        assert np.array_equal(i2.cpu().numpy(), ei2) and np.array_equal(s2.cpu().numpy(), es2)
        assert ix.margin_stats()["unresolved"] == 0


def test_tiny_search_ties_and_stream_of_calls():
    x = synth.generate(5, 0, 3000, 768, synth.KIND_LATTICE)
    q = synth.generate(6, 0, 16, 768, synth.KIND_LATTICE)
    x[10] = x[700]
    x[333] = x[700]
    q[0] = x[700]
    ix = _index(x)
    es, ei = orc.search_exact_bruteforce(q, x, 5)
    qd = torch.from_numpy(q).cuda()
    outs = [ix.search(qd, 5) for _ in range(20)]                   # back to back, no synchronisation in between
    torch.cuda.synchronize()
    for s, i in outs:
        assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
    assert ix.last_kernel.startswith("mips::tiny_search_kernel") and list(ei[0][:3]) == [10, 333, 700]
    g = torch.cuda.CUDAGraph()                                     # one kernel node: capturable
    buf = qd.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ix.search(buf, 5)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        s, i = ix.search(buf, 5)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(i.cpu().numpy(), ei)


@pytest.mark.parametrize("metric", [0, 1])
def test_tiny_search_fallback_paths(metric):
    """tiny_search_kernel's fast selection (threshold + rank by counting) hands over to the pop selection when more than
    64 candidates tie at the threshold, and its parallel exact re-score to the sequential sum when the products' exponent
    range is too wide for the exactness certificate: both must return the oracle's bits; "tiny" = 2 forces the
    fall-backs everywhere and must agree too."""
    rng = np.random.default_rng(77)
    # (1) thousands of identical rows: every list head ties, > 64 survivors at both selection levels
    x = synth.generate(301, 0, 6000, 768, synth.KIND_GAUSS)
    x[100:5100] = x[100]
    q = synth.generate(302, 0, 8, 768, synth.KIND_GAUSS)
    q[0] = x[100]
    # (2) rows and queries with elements down to 2^-60 next to O(1) ones: exponent range of the products > 27
    y = synth.generate(303, 0, 4000, 768, synth.KIND_GAUSS)
    scale = np.where(rng.random((4000, 768)) < 0.05, np.float32(2.0 ** -60), np.float32(1.0)).astype(np.float32)
    y = (y * scale).astype(np.float32)
    qy = synth.generate(304, 0, 12, 768, synth.KIND_GAUSS)
    qy[:, ::7] *= np.float32(2.0 ** -40)
    for data, qq in ((x, q), (y, qy)):
        ix = _index(data, metric=metric)
        stored = synth.bf16_bits_to_f32(ix.rows_bf16())
        qb = synth.round_to_bf16(qq)                                # the queries are rounded to the index's bf16 (RNE)
        es, ei = orc.search_exact_bruteforce(qb, stored, 5, metric=metric)   # (thousands of exact ties: the plain definition)
        qd = torch.from_numpy(qq).cuda()                           # device outputs: flagged queries are counted, not re-scanned
        for mode in (1, 2):
            ix.set_param("tiny", mode)
            s, i = ix.search(qd, 5)
            assert ix.last_kernel.startswith("mips::tiny_search_kernel")
            assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es), (mode, metric)
        ix.set_param("tiny", 0)
        s, i = ix.search(qq, 5)
        assert np.array_equal(i, ei) and np.array_equal(s, es)


@pytest.mark.parametrize("dtype", [None, "bf16"])          # None = the facade's default: fp32-exact storage
@pytest.mark.parametrize("metric,normalize", [(0, True), (0, False), (1, True)])
def test_fused_hook_search_prepare_search_ignore_in_one_call(tmp_path, metric, normalize, dtype):
    """Mips.search_device -> mips_search_fused: `_prepare_query` + `search` + the ignore filter of mips.py:388-398 as
    one library call (one launch at B = 8, N = 10^4): equal to the separate device steps and to the oracle."""
    n, d, k, b = 10000, 768, 5, 8
    rng = np.random.default_rng(3)
    emb = (synth.generate(261, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    qs = (synth.generate(262, 0, b, d, synth.KIND_GAUSS) * rng.uniform(0.5, 2.0, (b, 1))).astype(np.float32)
    m = ram.Mips(ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=str(tmp_path),
                              **({} if dtype is None else {"mips_index_dtype": dtype})))
    m.build_index(emb)
    index = m.embeddings.get_index(m.index_name).faiss_index
    stored = _stored(index)
    qd = torch.from_numpy(qs).cuda()
    keep = qd.clone()
    # separate device steps (the round-1 form)
    qn = ram.l2_normalize_(qd.clone()) if (normalize and metric == 0) else qd
    rs, ri = index.search(qn, k + 1)
    ignore = ri[:, 1].clone()                                      # ban the second hit of every query
    fs, fi = ram.filter_ignore(rs, ri, ignore, k)
    s, i = m.search_device(qd, ignore_indexes=ignore, k=k)
    assert index.last_kernel.startswith("mips::tiny_search_kernel")
    assert torch.equal(i, fi) and torch.equal(s, fs) and torch.equal(qd, keep)
    s0, i0 = m.search_device(qd, k=k)
    assert torch.equal(i0, ri[:, :k]) and torch.equal(s0, rs[:, :k])
    # the oracle on what the device searched with
    q_used = _as_stored(index, qn.cpu().numpy())
    es, ei = orc.mips_search(lambda qq, kk: orc.search_exact(q_used, stored, kk, metric=metric), q_used, ignore.cpu().tolist(), k)
    assert [list(map(int, r)) for r in ei] == i.cpu().tolist()
    assert np.array_equal(np.array(es, dtype=np.float32), s.cpu().numpy())
    assert index.margin_stats()["unresolved"] == 0             # the hook's path is certified on the stream
    # larger batches take the same call through separate launches: same answers
    big = torch.cat([qd] * 5)[:33]
    s2, i2 = m.search_device(big, ignore_indexes=torch.cat([ignore] * 5)[:33], k=k)
    assert not index.last_kernel.startswith("mips::tiny") and torch.equal(i2[:b], i) and torch.equal(s2[:b], s)


def test_pitch_1024_k_split_kernel_is_bit_identical():
    """Row pitch 1024: scan_kernel_v3's one-wave-per-SIMD configuration ("variant" = 3; the default up to 256 queries) and
    scan_kernel_k3 ("variant" = 7, the default beyond 256 queries: wave pairs split K, partial sums meet in LDS, 48 queries per
    pair, 192-query tiles, sub-lists of 4) return the same bits -- and the oracle's -- on ragged sizes, single- and multi-tile
    query counts, forced split counts, ties.  (scan_kernel_ks, "variant" = 6, the first K-split kernel, went with the retired A/B
    library; the shipped library ignores the value and the default kernels answer.)"""
    for n, nq, d, k in ((70001, 300, 1024, 5), (150001, 700, 1000, 5), (64 * 37 + 5, 129, 800, 4), (5000, 40, 1024, 1), (40000, 193, 1024, 5)):
        ix = ram.MipsIndex(d)
        ix.add_synthetic(n, row0=0, seed=171, kind=synth.KIND_GAUSS)
        q = ram.synth_fill(nq, d, 0, 172, synth.KIND_GAUSS)
        ref_s, ref_i = ix.search(q, k)
        assert ("scan_kernel_k3" if nq > 256 else "scan_kernel_v3") in ix.last_kernel, ix.last_kernel
        x = synth.generate(171, 0, n, d, synth.KIND_GAUSS)
        es, ei = orc.search_exact(q.float().cpu().numpy(), x, k)
        assert np.array_equal(ref_i.cpu().numpy(), ei) and np.array_equal(ref_s.cpu().numpy(), es)
        for variant, name in ((6, "scan_kernel_k"), (7, "scan_kernel_k3<"), (3, "scan_kernel_v3")):
            if variant == 6 and nq <= 256:
                continue                                            # (ignored by the shipped library: the default kernel, scan_kernel_v3 here)
            ix.set_param("variant", variant)
            for ns in (0, 8, 40):
                ix.set_param("nsplit", ns)
                s, i = ix.search(q, k)
                assert name in ix.last_kernel and torch.equal(i, ref_i) and torch.equal(s, ref_s), (n, nq, d, ns, variant)
            ix.set_param("nsplit", 0)
            hs, hi = ix.search(q.float().cpu().numpy(), k)        # host buffers: certified with a synchronisation
            assert np.array_equal(hi, ei) and np.array_equal(hs, es) and ix.margin_stats()["unresolved"] == 0
        ix.check()
    x = synth.generate(5, 0, 3000, 1024, synth.KIND_LATTICE)
    ql = synth.generate(6, 0, 300, 1024, synth.KIND_LATTICE)
    x[10] = x[700]
    x[333] = x[700]
    ql[0] = x[700]
    es, ei = orc.search_exact_bruteforce(ql, x, 5)
    for variant, name in ((6, "scan_kernel_k"), (7, "scan_kernel_k3<"), (0, "scan_kernel_k3")):
        ix = _index(x)
        ix.set_param("variant", variant)
        s, i = ix.search(ql, 5)
        assert np.array_equal(i, ei) and np.array_equal(s, es) and name in ix.last_kernel


def test_split_tail_searches_overlap_without_sharing_scratch():
    """mips_search_split: scan on the current stream, select + exact re-score on a side stream, two alternating scratch
    sets.  A train of back-to-back searches with DIFFERENT queries and shapes (no synchronisation in between, plain
    searches interleaved) returns exactly what the same searches return one at a time."""
    ix = ram.MipsIndex(768)
    ix.add_synthetic(150001, 0, synth.SEED_DOCS, synth.KIND_GAUSS)
    side = torch.cuda.Stream()
    qs = [ram.synth_fill(n, 768, 0, 500 + t, synth.KIND_GAUSS) for t, n in enumerate((700, 300, 4096, 8, 513, 700, 100, 1024))]
    refs = [ix.search(q, 5, 1000) for q in qs]
    torch.cuda.synchronize()
    outs = []
    for t, q in enumerate(qs):
        if t == 4:
            outs.append(ix.search(q, 5, 1000))                       # a plain search in the middle of the train
        else:
            outs.append(ix.search(q, 5, 1000, tail_stream=side))
    packed = ix.search_packed(qs[0], 5, 1000, tail_stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    ix.check()
    for (s, i), (rs, ri) in zip(outs, refs):
        assert torch.equal(i, ri) and torch.equal(s, rs)
    assert torch.equal(packed[..., 1], refs[0][1])
    # ShardedMipsIndex.search_async without a process group: the same overlap for consecutive batches on one GPU
    sh = ram.ShardedMipsIndex(768)
    sh.add_synthetic_global(150001, synth.SEED_DOCS, synth.KIND_GAUSS)
    pend = [sh.search_async(q, 5) for q in qs]
    for p_, (rs, ri) in zip(pend, refs):
        s, i = p_.result()
        torch.cuda.synchronize()
        assert torch.equal(i, ri - 1000) and torch.equal(s, rs)


@pytest.mark.parametrize("metric,normalize", [(0, True), (1, True), (0, False)])
def test_streaming_index_build_equals_one_shot_build(tmp_path, metric, normalize):
    """begin_index_build / add_embeddings (encoder batches, CUDA or NumPy, with their text columns) /
    end_index_build give the index, max_norm and phi of build_index on the whole matrix, bit for bit."""
    n, d, k = 7003, 768, 5
    rng = np.random.default_rng(21)
    emb = (synth.generate(271, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.4, 2.5, (n, 1))).astype(np.float32)
    qs = synth.generate(272, 0, 9, d, synth.KIND_GAUSS)
    data = {"mips_column": [f"text {t}" for t in range(n)], "aid": [f"a{t}" for t in range(n)]}
    args = ram.MipsArgs(mips_metric_type=metric, mips_normalize=normalize, mips_tmp_folder=str(tmp_path), mips_db_max_size=6500)
    one = ram.Mips(args, data=data)
    one.build_index(emb)
    st = ram.Mips(args)
    st.begin_index_build(d)
    cuts = [0, 1000, 1001, 2500, 6400, 6900, n]                   # the last batches cross mips_db_max_size
    for a, b in zip(cuts[:-1], cuts[1:]):
        batch = torch.from_numpy(emb[a:b]).cuda() if (a // 1000) % 2 == 0 else emb[a:b]
        keep = batch.clone() if isinstance(batch, torch.Tensor) else None
        st.add_embeddings(batch, {c: v[a:b] for c, v in data.items()})
        assert keep is None or torch.equal(batch, keep)            # the encoder's tensor is left alone
    st.end_index_build()
    i1, i2 = one._index(), st._index()
    assert i2.ntotal == i1.ntotal == 6500 and i1.dtype == "f32" and np.array_equal(i1.rows_raw(), i2.rows_raw())
    assert st.max_norm == one.max_norm and st.phi == one.phi
    assert st.embeddings.columns["aid"] == data["aid"][:6500]
    pq = one._prepare_query(qs.copy())
    s1, j1 = one.search(pq, k=k)
    s2, j2 = st.search(pq, k=k)
    assert np.array_equal(j1, j2) and np.array_equal(s1, s2)
    assert st.forward(qs.copy(), k=k).examples == one.forward(qs.copy(), k=k).examples


# ------------------------------------------------------------------ round 3: exact by default on the drop-in surface
@pytest.mark.parametrize("case", ["g2_cfg1", "g1b_fp32"])
def test_default_facade_returns_the_reference_neighbours(tmp_path, golden_dir, case):
    """At DEFAULT MipsArgs (fp32-exact storage) the facade returns the REAL reference's neighbours index for index: golden G2
    (BASELINE config 1: 10 000 x 768, 8 queries, inner_product(normalize=True)) and golden G1b (plain fp32 data that is not
    bf16-representable), inner product on normalised rows and L2, host (NumPy) and device-resident (search_device: one
    launch) call shapes, with and without `ignore_indexes` (sotasum/mips.py:368-400, 552-560)."""
    if case == "g2_cfg1":
        g = np.load(os.path.join(golden_dir, "g1_g2_inner_product.npz"))
        docs = synth.generate(int(g["seed_docs"]), 0, int(g["n"]), int(g["d"]), int(g["kind"]))
        qs, k = g["queries"], int(g["k"])
    else:
        g = np.load(os.path.join(golden_dir, "g1b_inner_product_f32.npz"))
        docs, qs, k = g["y"], g["x"], 5                              # (the golden holds the top 10: its first 5 are the top 5)
    nq = len(qs)
    gold = {0: g["indices_norm"][:, :k], 1: g["indices_raw"][:, :k]}  # L2 on the phi-augmented rows ranks like the raw inner product
    gold_s = {0: g["scores_norm"][:, :k], 1: g["scores_raw"][:, :k]}
    for metric in (0, 1):
        args = ram.MipsArgs(mips_metric_type=metric, mips_tmp_folder=str(tmp_path / f"m{metric}"))   # every other knob at its default
        assert args.mips_index_dtype == "f32" and args.mips_normalize
        m = ram.Mips(args)
        m.build_index(docs)
        index = m._index()
        pq = m._prepare_query(qs.copy())
        s, i = m.search(pq, k=k)
        assert np.array_equal(i, gold[metric]), (case, metric)
        if metric == 0:
            np.testing.assert_allclose(s, gold_s[0], rtol=2e-6, atol=1e-7)
        else:   # squared distances on the augmented vectors: |q|^2 + phi - 2 q.x
            want = (qs.astype(np.float64) ** 2).sum(1)[:, None] + m.phi - 2.0 * gold_s[1].astype(np.float64)
            np.testing.assert_allclose(s, want, rtol=1e-5)
            assert (np.diff(s, axis=1) >= 0).all()
        # ignore_indexes: the reference fetches k + 1, drops the banned id, keeps k
        ban = [int(gold[metric][j][j % 2]) for j in range(nq)]
        s2, i2 = m.search(pq, ignore_indexes=ban, k=k)
        stored, q_used = _stored(index), _as_stored(index, pq[:, :docs.shape[1]])
        es2, ei2 = orc.mips_search(lambda qq, kk: orc.search_exact(q_used, stored, kk, metric=metric), pq, ban, k)
        assert [list(map(int, r)) for r in i2] == [list(map(int, r)) for r in ei2]
        for j in range(nq):
            assert [int(t) for t in i2[j][:k - 1]] == [int(t) for t in gold[metric][j] if int(t) != ban[j]][:k - 1]
        # the device-resident hook (retriever_generator.py:143-153 without the .cpu() hop): same neighbours, certified, no sync
        qd = torch.from_numpy(qs).cuda()
        ds, di = m.search_device(qd, k=k)
        assert index.last_kernel.startswith("mips::tiny_search_kernel") and index.last_kernel.endswith("true>")
        st = index.margin_stats()
        assert st["unresolved"] == 0 and st["rescanned"] == st["flagged"], st
        assert np.array_equal(di.cpu().numpy(), gold[metric])
        gs, gi = m.search_device(qd, ignore_indexes=torch.tensor(ban).cuda(), k=k)
        assert gi.cpu().tolist() == [list(map(int, r)) for r in ei2] and index.margin_stats()["unresolved"] == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_hook_near_duplicates_are_certified_on_the_stream(tmp_path, dtype):
    """The scoring hook's own call shape (B <= 16, Mips.search_device -> mips_search_fused -> ONE launch) on the adversarial
    near-duplicate case: MFMA scores tie, the sub-lists keep the wrong copies, the margin check flags the query -- and the exact
    pass enqueued behind the one-launch kernel (no synchronisation) returns the oracle's rows, with and without the ignore
    filter.  `unresolved` stays 0."""
    x, q, rows, stars = _near_duplicate_case(nq=16)
    k = 5
    m = ram.Mips(ram.MipsArgs(mips_normalize=False, mips_index_dtype=dtype, mips_tmp_folder=str(tmp_path)))
    m.build_index(x)
    index = m._index()
    es, ei = orc.search_exact_bruteforce(q[stars], x, k + 1)
    free = np.setdiff1d(np.arange(16), stars)
    fs, fi = orc.search_exact(q[free], x, k + 1)
    qd = torch.from_numpy(q).cuda()
    for rep in range(3):
        s, i = m.search_device(qd, k=k)
    assert index.last_kernel.startswith("mips::tiny_search_kernel")
    st = index.margin_stats()
    assert st["flagged"] >= len(stars) and st["rescanned"] == st["flagged"] and st["unresolved"] == 0, st
    i, s = i.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(i[stars], ei[:, :k]) and np.array_equal(s[stars], es[:, :k])
    assert np.array_equal(i[free], fi[:, :k]) and np.array_equal(s[free], fs[:, :k])
    assert np.array_equal(i[stars], np.tile(rows[::-1][:k], (len(stars), 1)))    # the k HIGHEST-index copies, best first
    # ban the best copy (star queries) / the second hit (the others): k + 1 fetched, filtered, cut to k -- by the exact pass too
    ban = np.zeros(16, np.int64)
    ban[stars] = ei[:, 0]
    ban[free] = fi[:, 1]
    s2, i2 = m.search_device(qd, ignore_indexes=torch.from_numpy(ban).cuda(), k=k)
    st2 = index.margin_stats()
    assert st2["flagged"] >= len(stars) and st2["unresolved"] == 0, st2
    i2, s2 = i2.cpu().numpy(), s2.cpu().numpy()
    assert np.array_equal(i2[stars], ei[:, 1:]) and np.array_equal(s2[stars], es[:, 1:])
    assert np.array_equal(i2[free], np.delete(fi, 1, axis=1)) and np.array_equal(s2[free], np.delete(fs, 1, axis=1))
    # "margin_check" = 4: count only, the first results stand
    index.set_param("margin_check", 4)
    s4, i4 = m.search_device(qd, k=k)
    st4 = index.margin_stats()
    assert st4["flagged"] >= len(stars) and st4["rescanned"] == 0 and st4["unresolved"] == st4["flagged"]
    if dtype == "bf16":   # (an fp32-exact index that may not certify scans hi.qhi + hi.qlo + lo.qhi with true lists instead)
        assert st4["flagged"] == st["flagged"]
    index.set_param("margin_check", 1)
    # the host (NumPy) call of the same shape certifies as well
    hs, hi = m.search(q, k=k)
    assert np.array_equal(hi[stars], ei[:, :k]) and np.array_equal(hi[free], fi[:, :k])


def test_hook_on_clustered_fp32_rows_returns_the_brute_force_neighbours(tmp_path):
    """fp32 rows that bf16 cannot tell apart (clusters of 40 members within 1e-4 of each other), the hook's call shape on the
    default fp32-exact index: the one-launch kernel scans bf16(x) . bf16(q), its widened margin flags what that cannot decide and
    the stream-ordered exact pass settles it on the fp32 rows -- the result is the fp32 brute force's, bit for bit."""
    rng = np.random.default_rng(5)
    c = rng.standard_normal((300, 768)).astype(np.float32)
    x = (np.repeat(c, 40, axis=0) * (1.0 + 1e-4 * rng.standard_normal((12000, 1)))).astype(np.float32)
    x += (1e-4 * rng.standard_normal(x.shape)).astype(np.float32)
    q = (c[rng.integers(0, 300, 16)] + 0.01 * rng.standard_normal((16, 768))).astype(np.float32)
    for metric in (0, 1):
        m = ram.Mips(ram.MipsArgs(mips_metric_type=metric, mips_normalize=False, mips_tmp_folder=str(tmp_path / str(metric))))
        m.build_index(x)
        es, ei = orc.search_exact(q, x, 5, metric=metric)
        s, i = m.search_device(torch.from_numpy(q).cuda(), k=5)
        index = m._index()
        assert index.last_kernel.startswith("mips::tiny_search_kernel") and index.dtype == "f32"
        st = index.margin_stats()
        assert st["flagged"] > 0 and st["rescanned"] == st["flagged"] and st["unresolved"] == 0, st
        assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
        ban = torch.from_numpy(ei[:, 2].copy()).cuda()
        s2, i2 = m.search_device(torch.from_numpy(q).cuda(), ignore_indexes=ban, k=4)
        es5, ei5 = orc.search_exact(q, x, 5, metric=metric)
        assert np.array_equal(i2.cpu().numpy(), np.delete(ei5, 2, axis=1)) and np.array_equal(s2.cpu().numpy(), np.delete(es5, 2, axis=1))


@pytest.mark.parametrize("dtype,d,metric", [("bf16", 768, 0), ("bf16", 1000, 1), ("bf16", 320, 0), ("f32", 768, 0), ("f32", 1000, 0), ("f32", 300, 1)])
def test_exact_pass_mfma_prefilter_equals_the_plain_pass(dtype, d, metric):
    """The exact pass of flagged queries behind its MFMA pre-filter ("resolve" = 1, the default: 16 flagged queries per pass, only
    rows whose approximate score comes within the error bound of the k-th key are evaluated canonically) against the plain pass
    ("resolve" = 2: the canonical fp64 score of EVERY row for 8 queries per pass): the same results, the same statistics, and the
    brute-force oracle's rows -- on clusters of near-identical rows (dozens of flagged queries, exact ties among the hits),
    with 40 flagged queries (three passes of the filtered form) and with one."""
    rng = np.random.default_rng(d + metric)
    nc, per = 160, 45
    c = rng.standard_normal((nc, d)).astype(np.float32)
    x = (np.repeat(c, per, axis=0) * (1.0 + 1e-4 * rng.standard_normal((nc * per, 1)))).astype(np.float32)
    x += (1e-4 * rng.standard_normal(x.shape)).astype(np.float32)
    x[7 * per + 3] = x[7 * per + 1]                                  # two exact duplicates inside a cluster: a tie among the hits
    x = np.concatenate([x, rng.standard_normal((20011, d)).astype(np.float32)])     # a ragged tail of ordinary rows
    if dtype == "bf16":
        x = synth.round_to_bf16(x)
    k = 5
    for nq in (40, 1):
        q = (c[rng.integers(0, nc, nq)] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
        if nq == 40:
            q[0] = c[7]
        if dtype == "bf16":
            q = synth.round_to_bf16(q)
        es, ei = orc.search_exact_bruteforce(q, x, k, metric=metric)          # (tie-safe enumeration)
        ix = ram.MipsIndex(d, metric=metric, dtype=dtype)
        ix.add(x)
        out = {}
        for mode in (2, 1):
            ix.set_param("resolve", mode)
            s, i = ix.search(torch.from_numpy(q).cuda(), k)
            out[mode] = (s.cpu().numpy(), i.cpu().numpy(), ix.margin_stats())
            hs, hi = ix.search(q, k)                                 # host buffers: the synchronising form of the same pass
            assert np.array_equal(hi, out[mode][1]) and np.array_equal(hs, out[mode][0]), (mode, nq)
        assert out[1][2] == out[2][2] and out[1][2]["unresolved"] == 0, (out[1][2], out[2][2])
        assert nq == 1 or out[1][2]["flagged"] > 0, (nq, out[1][2])   # (the single query runs the one-launch kernel: flagged or not, same rows)
        assert np.array_equal(out[1][1], out[2][1]) and np.array_equal(out[1][0], out[2][0])
        assert np.array_equal(out[1][0], es) and np.array_equal(out[1][1], ei)   # (equal scores in the oracle's order: idx asc)
        ix.check()


# ------------------------------------------------------------------ round 3: the certification budget and what lies beyond it
def test_resolve_budget_exactly_met_and_exceeded():
    """"resolve_budget": flagged queries ONE search settles at most (default 1024).  A device-output search that flags exactly
    the budget is settled and equals the oracle; one that flags budget + 1 keeps its first results -- every one of them a real
    row, nothing poisoned -- and says so: {flagged n, rescanned 0, unresolved n}.  Host-buffer searches over the budget go
    through the tile re-scan instead (they synchronise anyway).  The statistics of two identical calls are identical: nothing
    a search does depends on when an earlier one's counters arrive."""
    nq, k = 300, 5
    x, q, rows, stars = _near_duplicate_case(nq=nq)
    ix = _index(x)
    qd = torch.from_numpy(q).cuda()
    es, ei = orc.search_exact(q, x, k)
    es[stars], ei[stars] = orc.search_exact_bruteforce(q[stars], x, k)       # (tie-safe enumeration for the star queries)
    s, i = ix.search(qd, k)                                                   # default: certified on the stream, no budget in the way
    st = ix.margin_stats()
    n = st["flagged"]
    assert n >= len(stars) and st["rescanned"] == n and st["unresolved"] == 0, st
    assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
    ix.set_param("margin_check", 4)                                           # the uncertified first results, for comparison
    s_first, i_first = ix.search(qd, k)
    ix.set_param("margin_check", 1)
    ix.set_param("resolve_budget", n)                                         # exactly met
    for rep in range(2):
        s, i = ix.search(qd, k)
        assert ix.margin_stats() == {"flagged": n, "rescanned": n, "unresolved": 0}
        assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
    ix.set_param("resolve_budget", n - 1)                                     # exceeded by one
    for rep in range(2):
        s, i = ix.search(qd, k)
        assert ix.margin_stats() == {"flagged": n, "rescanned": 0, "unresolved": n}
        assert torch.equal(i, i_first) and torch.equal(s, s_first)            # first results kept ...
        assert int(i.min()) >= 0 and bool(torch.isfinite(s).all())            # ... no poison, no padding
    pk = ix.search_packed(qd, k)
    assert torch.equal(pk[..., 1], i_first)
    hs, hi = ix.search(q, k)                                                  # host buffers: the tile re-scan settles them
    sth = ix.margin_stats()
    assert sth["flagged"] == n and sth["rescanned"] == n, sth
    assert np.array_equal(hi, ei) and np.array_equal(hs, es)
    ix.set_param("resolve_budget", 0)                                         # back to the default: exact again
    s, i = ix.search(qd, k)
    assert np.array_equal(i.cpu().numpy(), ei) and ix.margin_stats() == {"flagged": n, "rescanned": n, "unresolved": 0}


def test_optimistic_first_scan_over_the_budget_is_rescanned_not_kept():
    """a device-output search on the fp32-exact index scans bf16(x) . bf16(q) first (two-stage search) -- when
    it flags more queries than the exact pass settles (> 1024 here: clustered rows that bf16 cannot separate, 4096 queries),
    its first results were selected by bf16 scores and must not stand.  The stream-ordered fall-back (three-segment scan, true
    K' = 32 lists, sized on the device) runs exactly then: the results are the fp32 brute force's.  Same for pools of 32 out
    of sub-lists (bf16 index, k = 10) with a small budget."""
    rng = np.random.default_rng(9)
    c = rng.standard_normal((500, 768)).astype(np.float32)               # clusters of 40 > the pool of 32: stage 1 cannot certify
    x = (np.repeat(c, 40, axis=0) * (1.0 + 1e-4 * rng.standard_normal((20000, 1)))).astype(np.float32)
    x += (1e-4 * rng.standard_normal(x.shape)).astype(np.float32)
    nq = 4096
    q = (c[rng.integers(0, 500, nq)] + 0.01 * rng.standard_normal((nq, 768))).astype(np.float32)
    es, ei = orc.search_exact(q, x, 5)
    f = ram.MipsIndex(768, dtype="f32")
    f.add(x)
    qd = torch.from_numpy(q).cuda()
    for rep in range(2):
        s, i = f.search(qd, 5)
        assert not f.last_kernel.startswith("mips::scan_kernel<")            # stage 1 on the bf16 rows, every time
        st = f.margin_stats()
        assert st["flagged"] > 1024 and st["rescanned"] == st["flagged"], st
        ok = (i.cpu().numpy() == ei).all(axis=1) & (s.cpu().numpy() == es).all(axis=1)
        assert ok.sum() >= nq - st["unresolved"], (int(ok.sum()), st)        # what the K' = 32 three-segment re-scan certified is exact
        assert ok.sum() >= nq - 8, (int(ok.sum()), st)                       # ... and in practice that is (nearly) everything
    f.set_param("margin_check", 4)                                            # for contrast: the uncertified three-segment scan
    f.set_param("margin_check", 1)
    # within the budget the exact pass settles them and the fall-back's launches leave at once
    s, i = f.search(qd[:512], 5)
    st = f.margin_stats()
    assert 0 < st["flagged"] <= 512 and st["unresolved"] == 0 and np.array_equal(i.cpu().numpy(), ei[:512]) and np.array_equal(s.cpu().numpy(), es[:512])
    # bf16 index, k = 10: pools of 32 out of the 16x16x32 kernel's sub-lists, budget 4, near-duplicate data that flags more
    xb, qb, rows, stars = _near_duplicate_case(nq=300)
    ib = _index(xb)
    e10s, e10i = orc.search_exact(qb, xb, 10)
    e10s[stars], e10i[stars] = orc.search_exact_bruteforce(qb[stars], xb, 10)
    ib.set_param("resolve_budget", 4)
    s, i = ib.search(torch.from_numpy(qb).cuda(), 10)
    assert ib.last_kernel.startswith("mips::scan_kernel_v4") and ib.last_kernel.endswith(", 4>")
    st = ib.margin_stats()
    assert st["flagged"] > 4 and st["rescanned"] == st["flagged"], st
    ok = (i.cpu().numpy() == e10i).all(axis=1)
    assert ok.sum() >= 300 - st["unresolved"]                                 # whatever the K' = 32 re-scan certified is exact
    assert ok[np.setdiff1d(np.arange(300), stars)].all()


def test_pitch_1024_pools_over_the_budget_fall_back_to_true_lists():
    """Row pitch 1024, bf16, k = 10, more than 256 queries: pools of 32 out of scan_kernel_k3's sub-lists (an optimistic first
    scan).  With clusters of 45 near-identical rows and a budget of 4 the search flags more than it may settle exactly: the
    stream-ordered fall-back (true K' = 32 lists on the 4-wave kernel) runs, and every query it certifies -- all the ordinary
    ones -- carries the oracle's rows; within the budget the exact pass settles all of them."""
    rng = np.random.default_rng(1024)
    d, nc, per, k = 1024, 30, 45, 10
    c = rng.standard_normal((nc, d)).astype(np.float32)
    x = (np.repeat(c, per, axis=0) * (1.0 + 1e-4 * rng.standard_normal((nc * per, 1)))).astype(np.float32)   # (mostly equal after bf16 rounding)
    x = synth.round_to_bf16(np.concatenate([x, rng.standard_normal((30011, d)).astype(np.float32)]))
    nq = 300
    q = rng.standard_normal((nq, d)).astype(np.float32)
    hard = np.arange(0, nq, 11)
    q[hard] = c[rng.integers(0, nc, len(hard))] + 0.01 * rng.standard_normal((len(hard), d)).astype(np.float32)
    q = synth.round_to_bf16(q)
    es, ei = orc.search_exact(q, x, k)
    es[hard], ei[hard] = orc.search_exact_bruteforce(q[hard], x, k)       # (tie-safe enumeration where ties can be)
    ix = _index(x)
    qd = torch.from_numpy(q).cuda()
    s, i = ix.search(qd, k)                                               # default budget: everything flagged is settled exactly
    assert ix.last_kernel.startswith("mips::scan_kernel_k3<4, 32, 2, 0, 4>"), ix.last_kernel
    st = ix.margin_stats()
    assert st["flagged"] > 4 and st["unresolved"] == 0, st
    assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)
    ix.set_param("resolve_budget", 4)
    s, i = ix.search(qd, k)
    st4 = ix.margin_stats()
    assert st4["flagged"] == st["flagged"] and st4["rescanned"] == st4["flagged"], (st, st4)
    ok = (i.cpu().numpy() == ei).all(axis=1) & (s.cpu().numpy() == es).all(axis=1)
    assert ok.sum() >= nq - st4["unresolved"], (int(ok.sum()), st4)
    assert ok[np.setdiff1d(np.arange(nq), hard)].all()
    assert not (i.cpu().numpy() == ram.IDX_POISON).any()
    ix.check()


def test_bench_two_rank_line_carries_the_sharded_regimes():
    """`python bench.py --gpus 2 --backend gloo --rows 65536 --full` (both ranks on this one GPU, host-staged collective): the N > 1
    line keeps the headline contract AND carries `regimes` -- the row-sharded BASELINE config 3 / 5 forms (here at reduced size)
    measured in the same run, with per-GPU shard sizes, scan-kernel times and roofline fractions, the system rate and what
    process group was formed.  This is the line the driver's 1/2/4/8-GPU curve is read from."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--rows", "65536", "--queries", "512",
                          "--steps", "3", "--warmup", "1", "--full"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0 and line["config"]["rows_per_gpu"] == [32768, 32768]
    assert line["distributed"]["world_size"] == 2 and line["distributed"]["self_launched"] is True
    assert line["margin_check"]["unresolved"] == 0
    regs = line["regimes"]
    assert [r["workload"].split(" index")[0] for r in regs] == ["262144x768 bf16", "262144x768 fp8_e4m3"]
    for r in regs:
        assert r["queries_per_s"] > 0 and r["ranks_agree"] is True and r["scaling"] == "strong" and r["margin"]["unresolved"] == 0
        assert r["distributed"]["world_size"] == 2 and [g["rows"] for g in r["per_gpu"]] == [131072, 131072]
        for g in r["per_gpu"]:
            assert g["scan_kernel_ms"] > 0 and 0 < g["mfma_frac"] < 1 and 0 < g["hbm_frac"] < 1


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """`python bench.py ... --dump-outputs DIR` without --full: the line carries the headline and nothing that takes a run
    of its own, and DIR holds the last timed step's top-k -- the oracle's answer on the same seeded workload."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, d, nq, k = 65536, 768, 64, 5
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--rows", str(n), "--queries", str(nq), "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["full"] is False and line["margin_check"]["unresolved"] == 0
    assert line["value"] == pytest.approx(nq * 1e3 / line["ms_per_step"])
    assert line["step_ms"] is None and line["cpu_baseline"] is None and line["regimes"] is None
    s, i = np.load(tmp_path / "out" / "scores.npy"), np.load(tmp_path / "out" / "indices.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == i.shape == (nq, k)
    x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
    es, ei = orc.search_exact(q, x, k)
    assert np.array_equal(i, ei) and np.array_equal(s, es)


# ------------------------------------------------------------------ round 3: a real datasets.Dataset in the loop
def test_real_hf_dataset_reaches_the_index_the_way_the_reference_does(tmp_path, monkeypatch):
    """The reference never calls FAISS directly: it reaches the index as `Dataset.add_faiss_index(...)`,
    `Dataset.get_index(name).faiss_index.search(q, k)`, `Dataset[i]["mips_column"]` (sotasum/mips.py:333-345, 383-386, 428) and
    `Dataset.get_nearest_examples_batch("mips_cls", q, k)` (retriever_lightning.py:317-321).  Here a REAL HF `datasets.Dataset`
    does exactly that on the MI355X backend, two ways:
      (1) the reference's call text unchanged -- string_factory="Flat", metric_type, train_size, faiss_verbose -- with
          `faiss_shim.install()` answering `import faiss` (faiss itself is not installed in this image);
      (2) HF's own hook `add_faiss_index(custom_index=MipsIndex(...))`.
    Inner product on plain fp32 rows and L2 on the phi-augmented rows the reference builds; results == the oracle's."""
    datasets = pytest.importorskip("datasets")
    import sys

    monkeypatch.delitem(sys.modules, "faiss", raising=False)
    fs = ram.faiss_shim.install()
    import faiss
    assert faiss is fs and faiss.METRIC_INNER_PRODUCT == 0 and faiss.METRIC_L2 == 1
    try:
        n, d, nq, k = 3000, 768, 8, 5
        rng = np.random.default_rng(31)
        emb = (rng.standard_normal((n, d)) * rng.uniform(0.5, 1.5, (n, 1))).astype(np.float32)       # plain fp32: not bf16 values
        q = rng.standard_normal((nq, d)).astype(np.float32)
        texts = [f"abstract {t}" for t in range(n)]
        # ---- (1) mips.py:333-345 + 383-386 + 428, inner product, the reference's keyword arguments
        ds = datasets.Dataset.from_dict({"embeddings": emb, "mips_column": texts, "aid": [f"a{t}" for t in range(n)]})
        ds.add_faiss_index(column="embeddings", index_name="mips_embeddings", string_factory="Flat", train_size=-1,
                           metric_type=faiss.METRIC_INNER_PRODUCT, faiss_verbose=True)
        fi = ds.get_index("mips_embeddings").faiss_index
        fi.nprobe = 16                                                                               # mips.py:343-345
        assert isinstance(fi.mips_index, ram.MipsIndex) and fi.ntotal == n and fi.mips_index.dtype == "f32"
        qn = q.copy()
        faiss.normalize_L2(qn)                                                                       # mips.py:524
        np.testing.assert_allclose(np.linalg.norm(qn, axis=1), 1.0, rtol=1e-6)
        scores, indices = fi.search(qn, k)                                                           # mips.py:383-386
        es, ei = orc.search_exact(qn, emb, k)
        assert scores.dtype == np.float32 and indices.dtype == np.int64
        assert np.array_equal(indices, ei) and np.array_equal(scores, es)
        examples = [ds[int(t)]["mips_column"] for t in indices[0]]                                   # mips.py:428
        assert examples == [texts[int(t)] for t in ei[0]]
        # save_faiss_index / load_faiss_index (mips.py:536, 547) through HF's callback writers
        ds.save_faiss_index("mips_embeddings", str(tmp_path / "index.faiss"))
        ds2 = datasets.Dataset.from_dict({"mips_column": texts})
        ds2.load_faiss_index("mips_embeddings", str(tmp_path / "index.faiss"))
        s2, i2 = ds2.get_index("mips_embeddings").faiss_index.search(qn, k)
        assert np.array_equal(i2, ei) and np.array_equal(s2, es)
        # ---- retriever_lightning.py:372-404 + 313-321: phi-augmented "cls", default metric (L2), get_nearest_examples_batch
        column, metric = orc.full_kb_eval_index(emb, False)
        kb = datasets.Dataset.from_dict({"cls": column, "mips_column": texts})
        kb.add_faiss_index(column="cls", index_name="mips_cls", metric_type=metric)
        got_s, got_e = kb.get_nearest_examples_batch("mips_cls", queries=ram.augment_xq(q), k=k)
        e2s, e2i = orc.search_exact(q, emb, k, metric=orc.METRIC_L2)
        assert [e["mips_column"] for e in got_e] == [[texts[int(t)] for t in row] for row in e2i]
        np.testing.assert_allclose(np.stack(got_s), e2s, rtol=1e-5)                                  # (phi: fp32 in the reference's column, fp64 here)
        with pytest.raises(NotImplementedError, match="Flat"):
            datasets.Dataset.from_dict({"embeddings": emb[:64]}).add_faiss_index(column="embeddings", string_factory="IVF16,Flat")
        # ---- (2) HF's custom_index hook with the backend's own object
        ds3 = datasets.Dataset.from_dict({"cls": emb, "mips_column": texts})
        ds3.add_faiss_index(column="cls", index_name="mips_cls", custom_index=ram.MipsIndex(d, metric=ram.METRIC_IP, dtype="f32"))
        s3, e3 = ds3.get_nearest_examples_batch("mips_cls", queries=qn, k=k)
        assert [e["mips_column"] for e in e3] == [[texts[int(t)] for t in row] for row in ei]
        s4, i4 = ds3.get_index("mips_cls").faiss_index.search(qn, k)
        assert np.array_equal(i4, ei) and np.array_equal(s4, es)
    finally:
        sys.modules.pop("faiss", None)


@pytest.mark.parametrize("n,nq,d,k", [(60000, 300, 768, 20), (40000, 130, 640, 29), (50000, 300, 1024, 10), (30000, 70, 1000, 25),
                                       (30000, 40, 1024, 14), (20000, 300, 900, 5), (45000, 513, 1000, 25), (64 * 43 + 9, 257, 1024, 13)])
def test_wide_k_pools_and_pitch_1024_lists(n, nq, d, k):
    """Round 3: (1) k = 14 .. 29 at row pitch 384 .. 768 take the optimistic pools of 32 (16x16x32 kernel, every sub-list vouching
    for its 4th best) like k = 8 .. 13 did; (2) row pitch 1024 has true K' = 16 / 32 lists on the query-stationary 4-wave kernel:
    k = 8 .. 29 there, and stage 1 of the two-stage search of an fp32-exact index of Longformer-large width, leave the generic
    kernel.  Bit-identical to the oracle, host and device call shapes, certified."""
    x = synth.generate(501, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(502, 0, nq, d, synth.KIND_GAUSS)
    es, ei = orc.search_exact(q, x, k)
    ix = _index(x)
    s, i = ix.search(q, k)
    name = ix.last_kernel
    if k >= 8 and d <= 768:
        assert name.startswith("mips::scan_kernel_v4") and name.endswith(", 4>"), name
    elif k >= 8 and nq > 256:   # pools of 32 out of scan_kernel_k3's sub-lists (every sub-list vouches for its 4th best)
        assert name.startswith("mips::scan_kernel_k3<4, 32, 2, 0, 4>"), name
    elif k >= 8:
        assert name.startswith(f"mips::scan_kernel_v3<{16 if k <= 13 else 32}, 64, 1, 4"), name
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    assert ix.margin_stats()["unresolved"] == 0
    ds, di = ix.search(torch.from_numpy(q).cuda(), k)
    assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(ds.cpu().numpy(), es) and ix.margin_stats()["unresolved"] == 0
    # the fp32-exact index of the same width: two-stage search with pools of 32 at every pitch
    rng = np.random.default_rng(n)
    nf = min(n, 20000)
    xf = (x[:nf] * rng.uniform(0.5, 2.0, (nf, 1))).astype(np.float32)
    qf = (q * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float32)
    fs, fi = orc.search_exact(qf, xf, k)
    f = ram.MipsIndex(d, dtype="f32")
    f.add(xf)
    s2, i2 = f.search(torch.from_numpy(qf).cuda(), k)
    # (k <= 13: two-stage search; beyond that the widened margin no longer fits between the k-th and the pool's 33rd score
    # and the three-segment scan with true K' = 32 lists is the cheaper way to be exact)
    assert f.last_kernel.startswith("mips::scan_kernel<32>") == (k > 13), f.last_kernel
    st = f.margin_stats()
    assert st["unresolved"] == 0 and st["flagged"] <= max(2, nq // 8), st
    assert np.array_equal(i2.cpu().numpy(), fi) and np.array_equal(s2.cpu().numpy(), fs)


def test_pitch_1024_deep_pool_on_large_indexes():
    """bf16 rows at pitch 1024, k <= 5, 2^21 rows or more, more than 256 queries: the candidate pool is 16 deep (scan_kernel_k3
    with every sub-list vouching for its 2nd best) so that the MFMA error bound at K = 1024 no longer reaches from the k-th exact
    score to the pool's edge (with the pool of 8 one Gaussian query in a few thousand is flagged there, and each costs a pass over
    the index).  Same bits as the pool-of-8 search ("optimistic" = 0) and as the brute-force oracle on a sample of the queries'
    neighbourhoods; nothing flagged on Gaussian data."""
    n, d, nq, k = (1 << 21) + 77, 1024, 1200, 5
    ix = ram.MipsIndex(d)
    ix.add_synthetic(n, row0=0, seed=synth.SEED_DOCS, kind=synth.KIND_GAUSS)
    q = ram.synth_fill(nq, d, 0, synth.SEED_QUERIES, synth.KIND_GAUSS)
    s, i = ix.search(q, k)
    assert ix.last_kernel.startswith("mips::scan_kernel_k3<4, 32, 2, 0, 2>"), ix.last_kernel
    st = ix.margin_stats(synchronize=True)
    assert st["flagged"] <= 1 and st["unresolved"] == 0, st
    ix.set_param("optimistic", 0)
    s8, i8 = ix.search(q, k)
    assert ix.last_kernel.startswith("mips::scan_kernel_k3<4, 32, 2, 0, 1>"), ix.last_kernel
    assert ix.margin_stats(synchronize=True)["unresolved"] == 0
    assert torch.equal(i, i8) and torch.equal(s, s8)
    ix.set_param("optimistic", 1)
    hs, hi = ix.search(q.float().cpu().numpy()[:300], k)              # 300 queries, host buffers: same rows
    assert np.array_equal(hi, i[:300].cpu().numpy()) and np.array_equal(hs, s[:300].cpu().numpy())
    # the returned scores are the canonical scores of the returned rows, and no row of a 200 000-row window beats the k-th
    ii = i[:8].cpu().numpy()
    rows = np.unique(ii.ravel())
    xr = np.stack([synth.generate(synth.SEED_DOCS, int(r), 1, d, synth.KIND_GAUSS)[0] for r in rows])
    q8 = q[:8].float().cpu().numpy()
    es, ei = orc.search_exact(q8, xr, k)
    assert np.array_equal(rows[ei], ii) and np.array_equal(es, s[:8].cpu().numpy())
    w0 = 700001
    xw = synth.generate(synth.SEED_DOCS, w0, 200000, d, synth.KIND_GAUSS)
    ws, wi = orc.search_exact(q8, xw, 1)
    for t in range(8):
        assert ws[t, 0] <= s[t, k - 1].item() or (w0 + wi[t, 0]) in ii[t]
    ix.check()


# ------------------------------------------------------------------ round 3: BASELINE config 5 as worded -- e4m3 documents, bf16 queries
@pytest.mark.parametrize("n,nq,d,k,metric", [(5000, 8, 768, 5, 0), (70001, 64, 768, 5, 0), (30000, 40, 1024, 5, 0), (20000, 300, 768, 5, 0),
                                               (9000, 33, 512, 6, 1), (3000, 7, 256, 1, 0), (25000, 16, 1000, 10, 0), (40000, 20, 640, 20, 0),
                                               (64 * 31 + 3, 65, 768, 5, 1), (33, 3, 100, 5, 0)])
def test_e4m3_documents_bf16_queries_parity(tmp_path, n, nq, d, k, metric):
    """dtype "fp8_e4m3_docs": rows stored as OCP e4m3 (half the bytes of a bf16 index), queries kept in bf16, products on the bf16
    MFMA after an exact e4m3 -> bf16 up-conversion (scan_kernel_e8: the 8 waves split K, partial sums meet in LDS).  Canonical
    score = exact products of (e4m3 row element, bf16 query element), sequential fp64 sum: bit-identical to the oracle on those
    operands -- host and device call shapes, single- and multi-tile query counts, ragged sizes, pools of 8 / 10 / 16 / 32, L2."""
    rng = np.random.default_rng(n + nq)
    x = (synth.generate(601, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    q = (synth.generate(602, 0, nq, d, synth.KIND_GAUSS) * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float32)
    x8, qb = synth.round_to_e4m3(x), synth.round_to_bf16(q)
    es, ei = orc.search_exact(qb, x8, k, metric=metric)
    ix = ram.MipsIndex(d, metric=metric, dtype="fp8_e4m3_docs")
    ix.add(x[:n // 2])
    ix.add(torch.from_numpy(x[n // 2:]).cuda())
    assert np.array_equal(synth.e4m3_bits_to_f32(ix.rows_raw()), x8)
    s, i = ix.search(q, k)
    assert ix.last_kernel.startswith("mips::scan_kernel_e8"), ix.last_kernel
    assert np.array_equal(i, ei) and np.array_equal(s, es)
    st = ix.margin_stats()
    assert st["unresolved"] == 0 and st["rescanned"] == st["flagged"], st
    ds, di = ix.search(torch.from_numpy(q).cuda(), k)
    assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(ds.cpu().numpy(), es) and ix.margin_stats()["unresolved"] == 0
    ds, di = ix.search(torch.from_numpy(qb).cuda().bfloat16(), k, 1000)       # bf16 queries as they come, row offset
    assert np.array_equal(di.cpu().numpy(), ei + 1000) and np.array_equal(ds.cpu().numpy(), es)
    for ns in (8, 24):                                                        # forced split counts
        ix.set_param("nsplit", ns)
        s2, i2 = ix.search(q, k)
        assert np.array_equal(i2, ei) and np.array_equal(s2, es), ns
    ix.set_param("nsplit", 0)
    ix.save(str(tmp_path / "ix"))
    back = ram.MipsIndex.load(str(tmp_path / "ix"))
    assert back.dtype == "fp8_e4m3_docs" and np.array_equal(back.rows_raw(), ix.rows_raw())
    s3, i3 = back.search(q, k)
    assert np.array_equal(i3, ei) and np.array_equal(s3, es)
    # the all-e4m3 index of the same rows answers with e4m3-rounded queries: a different (coarser) question
    both = ram.MipsIndex(d, metric=metric, dtype="fp8_e4m3")
    both.add(x)
    assert np.array_equal(both.rows_raw(), ix.rows_raw())
