"""Two-stage search on PQ codes on the GPU (include/mips_hip_refine.h): search_candidates of PqIndex and IvfPqIndex for
k <= 1024, MipsIndex.rerank and RefinedIndex, everything bit for bit (the bits of D, and I) against the NumPy restatement of
tests/refine_cases.py -- no tolerance anywhere.  Indexes are planted (set_centroids / set_codebook / add_codes): nothing trains.  The CPU
side (that the cases bite, the header, the kernels' registers) is tests/test_refine_host.py; graph capture is
tests/test_gpu_refine_graph.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivfpq_cases as vc  # noqa: E402
import lifecycle_cases as lc  # noqa: E402
import pq_cases as pc  # noqa: E402
import refine_cases as rc  # noqa: E402
import rows_cases as rwc  # noqa: E402
import sq8_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.uint32
NQ = max(rc.NQS)


def planted_pq(case):
    ix = ram.PqIndex(case["d"], case["M"])
    ix.set_codebook(case["codebook"])
    if len(case["codes"]):
        ix.add_codes(case["codes"])
    return ix


def planted_ivfpq(case, by_residual=True):
    ix = ram.IvfPqIndex(case["d"], case["nlist"], case["M"], by_residual=by_residual)
    ix.set_centroids(case["centroids"])
    ix.set_codebook(case["codebook"])
    if len(case["codes"]):
        ix.add_codes(case["codes"], case["assign"])
    return ix


def same(got, want, what=""):
    D, I = got
    D = D.cpu().numpy() if isinstance(D, torch.Tensor) else np.asarray(D)
    I = I.cpu().numpy() if isinstance(I, torch.Tensor) else np.asarray(I)
    assert I.shape == want[1].shape and D.shape == want[0].shape, what
    assert np.array_equal(I, want[1]), what
    assert np.array_equal(D.view(U), want[0].view(U)), what


def ranked(full, k, rows_of=None, idx_offset=0):
    """the best k by (score descending, row ascending) of all rows, or of rows_of(j), from the scores `full` [nq, n]"""
    out_d = np.full((len(full), k), -np.inf, np.float32)
    out_i = np.full((len(full), k), -1, np.int64)
    for j in range(len(full)):
        rows = np.arange(full.shape[1]) if rows_of is None else rows_of(j)
        order = np.lexsort((rows, -full[j, rows].astype(np.float64)))[:k]
        out_d[j, :len(order)] = full[j, rows[order]]
        out_i[j, :len(order)] = rows[order] + idx_offset
    return out_d, out_i


@functools.lru_cache(maxsize=None)
def pq_case(d, M, n):
    c = pc.case_planted(d, M, n, NQ)
    c["full"] = pc.scores(pc.lut(c["q"], c["codebook"]), c["codes"]) if n else np.zeros((NQ, 0), np.float32)
    return c


@functools.lru_cache(maxsize=None)
def ivfpq_case(d, M, nlist, n, nq=NQ, one_list=None):
    c = vc.case_planted(d, M, nlist, n, nq, one_list=one_list)
    c["full"] = vc.all_scores(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"])
    return c


def probed_rows(case, nprobe):
    lists, _ = vc.probe(case["q"], case["centroids"], nprobe)
    return lambda j: np.flatnonzero(np.isin(case["assign"], lists[j]))


# ------------------------------------------------------------------ search_candidates: the shape matrix
@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("d,M", rc.GEOMETRY)
def test_pq_candidates_shapes(d, M, k):
    for n in rc.ntotals(k):
        case = pq_case(d, M, n)
        ix = planted_pq(case)
        for nq in rc.NQS:
            same(ix.search_candidates(case["q"][:nq], k), ranked(case["full"][:nq], k), (d, M, k, n, nq))


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("d,M", rc.GEOMETRY)
def test_ivfpq_candidates_shapes(d, M, k):
    for n in rc.ntotals(k):
        case = ivfpq_case(d, M, 8, n)
        ix = planted_ivfpq(case)
        for nprobe, nq in ((3, 17), (8, 3), (1, 1), (8, 1)):
            want = ranked(case["full"][:nq], k, probed_rows(case, nprobe))
            same(ix.search_candidates(case["q"][:nq], k, nprobe=nprobe), want, (d, M, k, n, nprobe, nq))


@pytest.mark.parametrize("k", rc.KS)
def test_ivfpq_candidates_worst_lds_case(k):
    """M = 128, 1024 probed lists: the largest table beside the longest prefix -- two pools at k > 256"""
    w = rc.WORST
    case = ivfpq_case(w["d"], w["M"], w["nlist"], w["n"], 3)
    ix = planted_ivfpq(case)
    same(ix.search_candidates(case["q"], k, nprobe=1024), ranked(case["full"], k, probed_rows(case, 1024)), k)
    if k in (64, 1024):
        same(ix.search_candidates(case["q"][:1], k, nprobe=200), ranked(case["full"][:1], k, probed_rows(case, 200)), k)


def test_pq_candidates_largest_table():
    case = pq_case(256, 128, 4097)
    ix = planted_pq(case)
    for k in (30, 256, 1024):
        same(ix.search_candidates(case["q"][:3], k), ranked(case["full"][:3], k), k)


# ------------------------------------------------------------------ search_candidates: properties
def test_prefix_property_and_narrow_k_is_search():
    cp, cv = pq_case(80, 40, 4097), ivfpq_case(80, 40, 8, 4097)
    fp, fv = planted_pq(cp), planted_ivfpq(cv)
    fv.nprobe = 5
    Dp, Ip = fp.search_candidates(cp["q"][:3], 300)
    Dv, Iv = fv.search_candidates(cv["q"][:3], 300)
    for k in range(1, 300):
        if k > 66 and k % 37:
            continue
        same(fp.search_candidates(cp["q"][:3], k), (Dp[:, :k], Ip[:, :k]), k)
        same(fv.search_candidates(cv["q"][:3], k), (Dv[:, :k], Iv[:, :k]), k)
    for k in (1, 5, 29):                                                        # k <= MAX_K: search itself
        same(fp.search_candidates(cp["q"], k), fp.search(cp["q"], k), k)
        same(fv.search_candidates(cv["q"], k, nprobe=3), fv.search(cv["q"], k, nprobe=3), k)


def test_every_k_prefix_on_one_small_case():
    case = ivfpq_case(32, 4, 8, 1000)
    ix = planted_ivfpq(case)
    D, I = ix.search_candidates(case["q"][:1], 1024, nprobe=8)
    same((D, I), ranked(case["full"][:1], 1024))
    for k in range(1, 1024):
        same(ix.search_candidates(case["q"][:1], k, nprobe=8), (D[:, :k], I[:, :k]), k)


def test_list_sizes_and_all_rows_in_one_list():
    for d, M in rc.GEOMETRY:
        case = ivfpq_case(d, M, 33, 4097)
        sizes = set(np.bincount(case["assign"], minlength=33).tolist())
        assert {0, 1, 63, 64, 65} <= sizes
        ix = planted_ivfpq(case)
        for k, nprobe in ((64, 33), (257, 7), (1024, 33)):
            same(ix.search_candidates(case["q"][:3], k, nprobe=nprobe), ranked(case["full"][:3], k, probed_rows(case, nprobe)), (d, M, k, nprobe))
        one = ivfpq_case(d, M, 8, 1000, 3, one_list=5)
        ix = planted_ivfpq(one)
        for nprobe in (1, 8):
            same(ix.search_candidates(one["q"], 256, nprobe=nprobe), ranked(one["full"], 256, probed_rows(one, nprobe)), (d, M, nprobe))


@pytest.mark.parametrize("d,M", rc.GEOMETRY)
def test_scan_segments_and_query_slice_give_identical_bits(d, M):
    case = ivfpq_case(d, M, 33, 4097)
    ix = planted_ivfpq(case)
    ix.nprobe = 7
    q = case["q"][:5]
    want = {k: ranked(case["full"][:5], k, probed_rows(case, 7)) for k in (64, 1024)}
    for S in (1, 2, 7, 64):
        ix.scan_segments = S
        for k in want:
            same(ix.search_candidates(q, k), want[k], (S, k))
    ix.scan_segments = 0
    ix.query_slice = 2                                                          # 5 queries: slices of 2, 2 and 1
    same(ix.search_candidates(q, 64), want[64])
    same(ix.search_candidates(torch.from_numpy(q).cuda(), 1024), want[1024])
    flat = planted_pq(pq_case(d, M, 4097))
    flat.query_slice = 2
    same(flat.search_candidates(pq_case(d, M, 4097)["q"][:5], 65), ranked(pq_case(d, M, 4097)["full"][:5], 65))


def test_flood_of_identical_rows_is_cut_by_row_number():
    f = rc.case_flood()
    ix = planted_ivfpq(f)
    want = rc.candidates_ivfpq(f["q"], f["centroids"], f["codebook"], f["codes"], f["assign"], 256, 8)
    in_flood = np.isin(want[1][0], f["flood"])
    assert 0 < in_flood.sum() < len(f["flood"])
    same(ix.search_candidates(f["q"], 256, nprobe=8), want)
    t = pc.case_ties(n=300)                                                     # 300 identical rows in a PqIndex
    same(planted_pq(t).search_candidates(t["q"], 256), rc.candidates_pq(t["q"], t["codebook"], t["codes"], 256))


@pytest.mark.parametrize("ascending", [True, False])
def test_rows_in_score_order(ascending):
    """ascending: every row is an insertion at the front; descending: behind the fill nothing is"""
    for n, k in ((700, 64), (4097, 256), (4097, 1024)):
        c = rc.case_ordered(n, ascending=ascending)
        same(planted_pq(c).search_candidates(c["q"], k), rc.candidates_pq(c["q"], c["codebook"], c["codes"], k), (n, k))
        a = (np.arange(n) % 3).astype(np.int32)                                 # the same rows over three lists, one centroid for all
        v = dict(c, nlist=3, centroids=np.tile(np.ones((1, 32), np.float32), (3, 1)), assign=a)
        same(planted_ivfpq(v).search_candidates(c["q"], k, nprobe=3),
             rc.candidates_ivfpq(c["q"], v["centroids"], c["codebook"], c["codes"], a, k, 3), (n, k))


@pytest.mark.parametrize("d,M", [(32, 16), (80, 40)])
def test_by_residual_false_with_every_list_probed_is_the_pq_index(d, M):
    case = ivfpq_case(d, M, 8, 1000)
    ix = planted_ivfpq(case, by_residual=False)
    flat = ram.PqIndex(d, M)
    flat.set_codebook(case["codebook"])
    flat.add_codes(case["codes"])
    for k in (30, 256, 1000, 1024):
        got = flat.search_candidates(case["q"][:3], k)
        same(ix.search_candidates(case["q"][:3], k, nprobe=8), got, k)
        same(got, rc.candidates_pq(case["q"][:3], case["codebook"], case["codes"], k), k)


def test_scores_by_id_forms_dtypes_and_offset():
    cv, cp = ivfpq_case(80, 40, 8, 4097), pq_case(80, 40, 4097)
    fv, fp = planted_ivfpq(cv), planted_pq(cp)
    q = cv["q"][:3]
    D, I = fv.search_candidates(q, 300, nprobe=3, idx_offset=1000)
    same((D, I), ranked(cv["full"][:3], 300, probed_rows(cv, 3), idx_offset=1000))
    assert np.array_equal(fv.compute_distance_subset(q, I, idx_offset=1000).view(U), D.view(U))
    Dd, Id = fv.search_candidates(torch.from_numpy(q).cuda(), 300, nprobe=3, idx_offset=1000)
    assert Dd.is_cuda and Id.is_cuda and Id.dtype == torch.int64
    same((Dd, Id), (D, I))
    D, I = fp.search_candidates(cp["q"][:3], 300, idx_offset=7)
    same((D, I), ranked(cp["full"][:3], 300, idx_offset=7))
    assert np.array_equal(fp.compute_distance_subset(cp["q"][:3], I, idx_offset=7).view(U), D.view(U))
    same(fp.search_candidates(torch.from_numpy(cp["q"][:3]).cuda(), 300, idx_offset=7), (D, I))
    qb = torch.from_numpy(cp["q"][:3]).bfloat16()                               # bf16 queries: widened exactly
    want = rc.candidates_pq(qb.float().numpy(), cp["codebook"], cp["codes"], 100)
    same(fp.search_candidates(qb, 100), want)
    same(fp.search_candidates(qb.cuda(), 100), want)
    wv = rc.candidates_ivfpq(qb.float().numpy(), cv["centroids"], cv["codebook"], cv["codes"], cv["assign"], 100, 3)
    same(fv.search_candidates(qb.cuda(), 100, nprobe=3), wv)


def test_refusals_and_what_stays_refused():
    cp, cv = pq_case(32, 4, 1000), ivfpq_case(32, 4, 8, 1000)
    fp, fv = planted_pq(cp), planted_ivfpq(cv)
    for ix in (fp, fv):
        with pytest.raises(RuntimeError):
            ix.search_candidates(cp["q"], 0)
        with pytest.raises(NotImplementedError):
            ix.search_candidates(cp["q"], 1025)
        with pytest.raises(NotImplementedError):
            ix.search(cp["q"], 30)
        with pytest.raises(NotImplementedError):
            ix.search_wide(cp["q"], 30)
    with pytest.raises(RuntimeError):
        ram.PqIndex(32, 4).search_candidates(cp["q"], 64)                        # untrained
    with pytest.raises(RuntimeError):
        ram.IvfPqIndex(32, 8, 4).search_candidates(cp["q"], 64)
    D, I = fp.search_candidates(np.zeros((0, 32), np.float32), 64)
    assert D.shape == (0, 64) and I.shape == (0, 64)


# ------------------------------------------------------------------ rerank
def store_scores(q, x, storage):
    stored, qs = lc.stored_rows(x, storage), lc.stored_queries(q, storage)
    return lambda local: rwc.model_scores(qs, stored, local)


def flat_case(n, d, nq, seed=3):
    rng = np.random.default_rng([seed, n, d])
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_rerank_of_a_permutation_of_all_rows_is_the_search(storage):
    for n, d in ((1, 32), (64, 32), (65, 100), (1000, 32), (1024, 32)):
        x, q = flat_case(n, d, 5)
        x[n // 2] = x[0]                                                        # two equal rows: a tie the row number settles
        ix = ram.MipsIndex(d, dtype=storage)
        ix.add(x)
        rng = np.random.default_rng(n)
        ids = np.stack([rng.permutation(n) for _ in range(5)]).astype(np.int64)
        for k in sorted({1, min(5, n), min(29, n), min(30, n), min(64, n), min(257, n), n}):
            want = ix.search(q, k) if k <= ram.MAX_K else ix.search_wide(q, k)
            got = ix.rerank(q, ids, k)
            same(got, (np.asarray(want[0]), np.asarray(want[1])), (storage, n, k))
            same(got, rc.rerank(store_scores(q, x, storage), ids, k, n), (storage, n, k))
            assert np.array_equal(ix.compute_distance_subset(q, got[1]).view(U), got[0].view(U))


@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("kc", [1, 64, 65, 1024])
def test_rerank_ids_with_padding_out_of_range_and_repeats(storage, kc):
    n, d, nq = 500, 48, 4
    x, q = flat_case(n, d, nq)
    ix = ram.MipsIndex(d, dtype=storage)
    ix.add(x)
    for off in (0, 1000):
        ids = rc.rerank_ids(n, nq, kc, idx_offset=off)
        ids[0, :] = -1                                                          # a query without a valid id: padding only
        if kc >= 64:
            ids[1, 3:] = ids[1, 0]                                              # fewer valid ids than k
        for k in sorted({1, min(5, kc), min(64, kc), kc}):
            want = rc.rerank(store_scores(q, x, storage), ids, k, n, idx_offset=off)
            got = ix.rerank(q, ids, k, idx_offset=off)                          # host ids: nothing raises
            same(got, want, (storage, kc, k, off))
            assert (got[1][0] == -1).all() and np.isneginf(got[0][0]).all()
            dev = ix.rerank(torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda(), k, idx_offset=off)
            assert dev[0].is_cuda and dev[1].is_cuda
            same(dev, want, (storage, kc, k, off))
            same(ix.rerank(torch.from_numpy(q).cuda(), ids, k, idx_offset=off), want)
            back = ix.compute_distance_subset(q, np.where(got[1] >= 0, got[1], off - 1), idx_offset=off)
            assert np.array_equal(back.view(U), got[0].view(U))
    if kc > 1:
        assert (want[1][1] == -1).any() or kc < 64


def test_rerank_on_an_sq8_store():
    case = sc.case_gauss(700, 64, 4)
    vmin, vdiff, codes = sc.prepared(case)
    ix = ram.MipsIndex(64, dtype="sq8")
    ix.train(case["train"])
    ix.add(case["rows"])
    score_of = lambda local: sc.subset_scores(case["q"], codes, vmin, vdiff, local)  # noqa: E731
    for kc, k in ((64, 5), (300, 29), (1024, 100)):
        ids = rc.rerank_ids(700, 4, kc)
        want = rc.rerank(score_of, ids, k, 700)
        got = ix.rerank(case["q"], ids, k)
        same(got, want, (kc, k))
        same(ix.rerank(torch.from_numpy(case["q"]).cuda(), torch.from_numpy(ids).cuda(), k), want, (kc, k))
        safe = np.where(got[1] >= 0, got[1], -1)
        assert np.array_equal(ix.compute_distance_subset(case["q"], safe).view(U), got[0].view(U))


def test_rerank_refusals():
    x, q = flat_case(100, 32, 2)
    ix = ram.MipsIndex(32)
    ix.add(x)
    ids = np.zeros((2, 8), np.int64)
    for k in (0, 9):
        with pytest.raises(ValueError):
            ix.rerank(q, ids, k)
    with pytest.raises(NotImplementedError):
        ix.rerank(q, np.zeros((2, 1025), np.int64), 5)
    with pytest.raises(ValueError):
        ix.rerank(q, np.zeros((3, 8), np.int64), 5)
    with pytest.raises(NotImplementedError):
        ram.MipsIndex(32, metric=ram.METRIC_L2).rerank(q, ids, 5)
    with pytest.raises(RuntimeError):
        ram.MipsIndex(32, dtype="sq8").rerank(q, ids, 5)


# ------------------------------------------------------------------ RefinedIndex
def refined_case(d, M, nlist, n, nq=5, seed=1):
    """an IVFPQ case and float32 rows a little off their decoding: the two stages rank differently"""
    c = vc.case_planted(d, M, nlist, n, nq, seed)
    rng = np.random.default_rng(seed + n)
    c["x"] = (vc.reconstruct(c["codes"], c["assign"], c["centroids"], c["codebook"]) + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    return c


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_refined_index_is_the_composition_of_the_two_restatements(storage):
    c = refined_case(80, 40, 8, 2000)
    store = ram.MipsIndex(80, dtype=storage)
    store.add(c["x"])
    score_of = store_scores(c["q"], c["x"], storage)
    for base, cand in ((planted_ivfpq(c), lambda kc, off: rc.candidates_ivfpq(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"], kc, 3, off)),
                       (planted_pq(c), lambda kc, off: rc.candidates_pq(c["q"], c["codebook"], c["codes"], kc, off))):
        ivf = isinstance(base, ram.IvfPqIndex)
        if ivf:
            base.nprobe = 3
        rx = ram.RefinedIndex(base, store, k_factor=4)
        assert rx.ntotal == 2000 and rx.d == 80 and rx.is_trained
        for k, kf, off in ((5, None, 0), (29, 10, 0), (64, 16, 500), (300, None, 0)):
            kc = min(k * (kf or 4), 1024)
            want = rc.refined(cand(kc, off)[1], score_of, k, 2000, off)
            same(rx.search(c["q"], k, k_factor=kf, idx_offset=off), want, (k, kf, off))
            dev = rx.search(torch.from_numpy(c["q"]).cuda(), k, k_factor=kf, idx_offset=off)
            assert dev[0].is_cuda and dev[1].is_cuda
            same(dev, want, (k, kf, off))
        if ivf:
            want = rc.refined(rc.candidates_ivfpq(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"], 20, 8)[1], score_of, 5, 2000)
            same(rx.search(c["q"], 5, nprobe=8), want)
        else:
            with pytest.raises(ValueError):
                rx.search(c["q"], 5, nprobe=8)
        with pytest.raises(NotImplementedError):
            rx.search(c["q"], 1025)
    exact = store.search(c["q"], 5)                                             # the point of it all: the exact best 5 come back
    got = ram.RefinedIndex(planted_pq(c), store).search(c["q"], 5, k_factor=200)
    assert (np.asarray(got[1]) == np.asarray(exact[1])).mean() > 0.9


def test_refined_index_with_every_row_a_candidate_is_the_store_search(tmp_path):
    c = refined_case(32, 4, 8, 100)
    store = ram.MipsIndex(32)
    store.add(c["x"])
    base = planted_ivfpq(c)
    rx = ram.RefinedIndex(base, store, k_factor=4)
    for k, kf in ((5, 20), (29, None)):                                         # k * k_factor >= ntotal, every list probed
        want = store.search(c["q"], k)
        same(rx.search(c["q"], k, k_factor=kf, nprobe=8), (np.asarray(want[0]), np.asarray(want[1])), k)
    # add goes to both parts; a part that was filled alone is caught
    more = (c["x"][:10] * np.float32(1.5)).astype(np.float32)
    rx.add(more)
    assert rx.ntotal == 110 and base.ntotal == 110 and store.ntotal == 110
    want = store.search(c["q"], 29)
    same(rx.search(c["q"], 29, nprobe=8), (np.asarray(want[0]), np.asarray(want[1])))
    path = str(tmp_path / "refined")
    rx.save(path)
    assert sorted(os.listdir(path)) == ["base", "meta.json", "store"]
    back = ram.RefinedIndex.load(path)
    assert isinstance(back.base, ram.IvfPqIndex) and back.ntotal == 110 and back.k_factor == 4
    same(back.search(c["q"], 29, nprobe=8), (np.asarray(want[0]), np.asarray(want[1])))
    same(back.search(c["q"], 5, nprobe=2), rx.search(c["q"], 5, nprobe=2))
    store.add(more)
    for call in (lambda: rx.ntotal, lambda: rx.search(c["q"], 5), lambda: rx.add(more), lambda: rx.save(path)):
        with pytest.raises(RuntimeError):
            call()
    rx.reset()
    assert rx.ntotal == 0
    D, I = rx.search(c["q"], 5)
    assert (I == -1).all() and np.isneginf(D).all()
    with pytest.raises(ValueError):
        ram.RefinedIndex(planted_pq(pq_case(32, 4, 0)), ram.MipsIndex(48))
    with pytest.raises(TypeError):
        ram.RefinedIndex(store, store)


def test_c_abi_refine_from_plain_c(tmp_path):
    import subprocess

    lib_dir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_refine_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_refine_smoke.c"), "-I", os.path.join(ROOT, "include"), "-L", lib_dir,
                           "-lmips_hip", f"-Wl,-rpath,{lib_dir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "c_abi_refine_smoke ok" in out.stdout, out.stdout + out.stderr
