"""Rows by id on the GPU (include/mips_hip_rows.h): reconstruct_batch against the model of tests/rows_cases.py bit for bit -- every
storage, every row pitch, every id pattern, float32 and raw, NumPy and CUDA ids, strided outputs --, on indexes that were
reserved, grown, reset and compacted; compute_distance_subset reproduces the D of every search from its I; the layers above
(search_and_reconstruct, the faiss shim, Mips) and the C ABI from plain C."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import rows_cases as rc
finally:
    sys.path.pop(0)

lc = rc.lc
pytestmark = pytest.mark.gpu


def _bits(a):
    """Any result as a NumPy array of integers: float32 -> its bits, bfloat16 -> uint16."""
    if isinstance(a, torch.Tensor):
        a = a.view(torch.int16).cpu().numpy().view(np.uint16) if a.dtype == torch.bfloat16 else a.cpu().numpy()
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, exp, what):
    g, e = _bits(got), _bits(exp)
    assert g.shape == e.shape and g.dtype == e.dtype and np.array_equal(g, e), what


def _index(storage, d, x, metric=0):
    ix = ram.MipsIndex(d, metric=metric, dtype=storage, device=0)
    ix.add(x)
    return ix


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. reconstruct against the model
@pytest.mark.parametrize("storage,d", [(s, d) for s in rc.STORAGES for d in rc.dims_of(s)])
def test_reconstruct_every_pattern(storage, d):
    big_x, big_stored = rc.rows_data(storage, d, max(rc.NTOTALS))
    for n in rc.NTOTALS:
        x, stored = big_x[:n], big_stored[:n]
        ix = _index(storage, d, x)
        _same(ix.rows_raw(), rc.raw_bits(stored, storage), "the model of the storage is what the index holds")
        for name, ids in rc.id_patterns(n).items():
            what = f"{storage} d={d} n={n} {name}"
            exp, exp_raw = rc.model_reconstruct(stored, ids), rc.model_reconstruct_raw(stored, storage, ids)
            _same(ix.reconstruct_batch(_cuda(ids)), exp, what + " (CUDA ids)")
            _same(ix.reconstruct_batch(_cuda(ids), raw=True), exp_raw, what + " (CUDA ids, raw)")
            if name.startswith("bad_"):                            # host ids are checked before anything is launched
                with pytest.raises(RuntimeError, match="mips_index_reconstruct"):
                    ix.reconstruct_batch(ids)
            else:
                _same(ix.reconstruct_batch(ids), exp, what + " (NumPy ids)")
                _same(ix.reconstruct_batch(ids, raw=True), exp_raw, what + " (NumPy ids, raw)")
    # (n = 5000, the last index) reconstruct / reconstruct_n, an offset, a shard's view, ids of another shape
    _same(ix.reconstruct(n - 1), stored[n - 1], "reconstruct")
    _same(ix.reconstruct_n(127, 130), stored[127:257], "reconstruct_n")
    _same(ix.reconstruct_n(), stored, "reconstruct_n()")
    with pytest.raises(IndexError):
        ix.reconstruct(n)
    with pytest.raises(IndexError):
        ix.reconstruct_n(n - 1, 2)
    ids = rc.id_patterns(n)["minus_one"].reshape(17, 241)
    shifted = np.where(ids >= 0, ids + 1000, ids)
    _same(ix.reconstruct_batch(shifted, idx_offset=1000), rc.model_reconstruct(stored, shifted, 1000), "idx_offset")
    glob = np.concatenate([np.arange(0, 2 * n, 37), [-1, (1 << 32) + 3, rc.INT64_MIN]]).astype(np.int64)   # a shard that holds rows [n/2, n/2 + n)
    _same(ix.reconstruct_batch(_cuda(glob), idx_offset=n // 2, zero_missing=True), rc.model_reconstruct(stored, glob, n // 2, True), "zero_missing")
    _same(ix.reconstruct_batch(_cuda(ids)), rc.model_reconstruct(stored, ids), "ids [17, 241]")


@pytest.mark.parametrize("storage", rc.STORAGES)
@pytest.mark.parametrize("d", [7, 100, 768])
def test_reconstruct_into_a_strided_view_leaves_the_gaps(storage, d):
    n = 129
    x, stored = rc.rows_data(storage, d, n)
    ix = _index(storage, d, x)
    ids = np.concatenate([rc.id_patterns(n)["reversed"], [-1, n]]).astype(np.int64)
    for raw in (False, True):
        exp = rc.model_reconstruct_raw(stored, storage, ids) if raw else rc.model_reconstruct(stored, ids)
        tdt = torch.float32 if (not raw or storage == "f32") else torch.bfloat16 if storage == "bf16" else torch.uint8
        for pad, col0 in ((5, 0), (5, 1), (8, 4), (1, 0)):         # pitch d + pad, the view starts at column col0: (mis)aligned rows
            wide = torch.zeros((len(ids), d + pad), dtype=tdt, device="cuda")
            wide.view(torch.uint8).fill_(0xA5)
            before = wide.clone()
            out = wide[:, col0:col0 + d]
            assert ix.reconstruct_batch(_cuda(ids), raw=raw, out=out) is out
            _same(out.contiguous(), exp, f"{storage} d={d} raw={raw} pad={pad} col0={col0}")
            keep = torch.ones(d + pad, dtype=torch.bool)
            keep[col0:col0 + d] = False
            assert torch.equal(wide[:, keep.cuda()].contiguous().view(torch.uint8), before[:, keep.cuda()].contiguous().view(torch.uint8)), "a gap was written"
    with pytest.raises(ValueError):
        ix.reconstruct_batch(_cuda(ids), out=torch.zeros((len(ids), d), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ix.reconstruct_batch(_cuda(ids), out=torch.zeros((len(ids), 2 * d), device="cuda")[:, ::2])
    # ids [2, 3]: a slice of wider rows collapses to one pitch, a slice along the middle dimension does not
    ids23 = _cuda(np.array([[0, 5, -1], [n - 1, 5, 1]], np.int64))
    ok = torch.zeros((2, 3, d + 4), device="cuda")[:, :, :d]
    _same(ix.reconstruct_batch(ids23, out=ok).contiguous(), rc.model_reconstruct(stored, ids23.cpu().numpy()), "out [2, 3, d] at pitch d + 4")
    with pytest.raises(ValueError, match="one row pitch"):
        ix.reconstruct_batch(ids23, out=torch.zeros((2, 4, d), device="cuda")[:, :3, :])
    with pytest.raises(ValueError, match="int64"):
        ix.reconstruct_batch(np.array([0, 1 << 63], np.uint64))
    _same(ix.reconstruct_batch(np.array([0, n - 1], np.uint64)), stored[[0, n - 1]], "unsigned ids that fit")


def test_f32_index_returns_the_bits_it_was_given():
    x = rc.planted_f32()
    n, d = x.shape
    ix = _index("f32", d, x)
    ids = rc.id_patterns(n)["reversed"]
    for got in (ix.reconstruct_batch(ids), ix.reconstruct_batch(_cuda(ids)), ix.reconstruct_batch(ids, raw=True)):
        _same(got, x[ids], "-0.0, denormals and NaN payloads")
    got = _bits(ix.reconstruct_batch(ids))
    assert (got == 0x80000000).sum() == d + 2 and (got == 0x7FC12345).sum() == 1 and (got == 0xFFC54321).sum() == 1 and (got == 1).sum() == 1


def test_host_ids_past_the_index_write_nothing():
    n, d = 127, 100
    x, stored = rc.rows_data("bf16", d, n)
    ix = _index("bf16", d, x)
    lib, h = ix._lib, ix._h
    out = np.full((3, d), 7.0, np.float32)
    ids = np.array([0, n, 1], np.int64)
    rc_ = lib.mips_index_reconstruct(h, ids.ctypes.data, 3, 0, out.ctypes.data, ram._lib.DTYPE_F32, d, 0, None)
    assert rc_ != 0 and b"ids[1]" in lib.mips_last_error() and np.all(out == 7.0)
    dev = torch.full((3, d), 7.0, device="cuda")
    rc_ = lib.mips_index_reconstruct(h, ids.ctypes.data, 3, 0, dev.data_ptr(), ram._lib.DTYPE_F32, d, ram._lib.OUT_DEVICE, None)
    torch.cuda.synchronize()
    assert rc_ != 0 and bool((dev == 7.0).all())
    for bad in (dict(out_ld=d - 1), dict(dtype=ram._lib.DTYPE_FP8_E4M3), dict(n=-1)):   # refused arguments
        assert lib.mips_index_reconstruct(h, ids.ctypes.data, bad.get("n", 1), 0, out.ctypes.data, bad.get("dtype", ram._lib.DTYPE_F32),
                                          bad.get("out_ld", d), 0, None) != 0
    lab = np.full(3, 5, np.int32)
    assert lib.mips_index_gather_labels(h, ids.ctypes.data, 3, 0, lab.ctypes.data, 0, None) != 0 and np.all(lab == 5)
    sc = np.full((1, 3), 5.0, np.float32)
    assert lib.mips_score_subset(h, x.ctypes.data, ram._lib.DTYPE_F32, 1, ids.ctypes.data, 3, sc.ctypes.data, 0, 0, None) != 0 and np.all(sc == 5.0)
    with pytest.raises(RuntimeError):
        ix.compute_distance_subset(x[:1], ids[None, :])
    _same(ix.reconstruct_batch(np.array([0, -1, 1])), rc.model_reconstruct(stored, np.array([0, -1, 1])), "the index still answers")


# ------------------------------------------------------------------ 2. indexes that changed
@pytest.mark.parametrize("storage", rc.STORAGES)
def test_reconstruct_follows_reserve_growth_reset_and_removal(storage):
    d = 100
    x, stored = rc.rows_data(storage, d, 3000)
    ix = ram.MipsIndex(d, dtype=storage, device=0)
    assert ix.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, d)
    _same(ix.reconstruct_batch(_cuda(np.array([0, -1]))), rc.model_reconstruct(stored[:0], np.array([0, -1])), "an empty index: no row")
    ix.reserve(10)
    ix.add(x[:100])
    ids = _cuda(np.arange(100)[::-1].copy())
    _same(ix.reconstruct_batch(ids), stored[:100][::-1], "after reserve + add")
    ix.add(x[100:2000])                                             # growth: the storage moves
    _same(ix.reconstruct_batch(ids), stored[:100][::-1], "after growth")
    _same(ix.reconstruct_n(), stored[:2000], "all rows after growth")
    ix.reserve(6000)                                               # an exact reservation moves it again
    _same(ix.reconstruct_n(1990, 10), stored[1990:2000], "after reserve")
    ix.reset()
    ix.add(x[2000:])
    _same(ix.reconstruct_n(), stored[2000:], "after reset + add")
    with pytest.raises(RuntimeError):
        ix.reconstruct_batch(np.array([1000]))                     # the index has 1000 rows now
    labels = (np.arange(1000) * 7 % 13).astype(np.int32)
    ix.set_labels(labels[:800])                                    # a labelled prefix
    probe = np.array([0, 799, 800, 999, -1], np.int64)
    exp = np.array([labels[0], labels[799], ram.LABEL_NONE, ram.LABEL_NONE, ram.LABEL_NONE], np.int32)
    _same(ix.labels_of(probe), exp, "labels_of (NumPy)")
    _same(ix.labels_of(_cuda(np.append(probe, 1000)).reshape(2, 3)), np.append(exp, ram.LABEL_NONE).astype(np.int32).reshape(2, 3), "labels_of (CUDA)")
    mask = np.random.default_rng(5).random(1000) < 0.4
    mask[[0, 999]] = True
    assert ix.remove_ids(mask) == int(mask.sum())
    left = stored[2000:][~mask]
    _same(ix.reconstruct_n(), left, "after remove_ids")
    _same(ix.reconstruct_batch(_cuda(np.array([len(left) - 1, len(left), 0]))), rc.model_reconstruct(left, np.array([len(left) - 1, len(left), 0])), "the new end")
    nlab = int((~mask[:800]).sum())
    exp_lab = np.full(len(left), ram.LABEL_NONE, np.int32)
    exp_lab[:nlab] = labels[:800][~mask[:800]]
    _same(ix.labels_of(np.arange(len(left))), exp_lab, "labels travel with their rows")


# ------------------------------------------------------------------ 3. scores reproduce search
def _pad_csr(lims, D, I, metric):
    lims, D, I = (np.asarray(t.cpu()) if isinstance(t, torch.Tensor) else np.asarray(t) for t in (lims, D, I))
    nq, width = len(lims) - 1, int(np.diff(lims).max(initial=0)) + 1   # at least one -1 slot per query
    Dp = np.full((nq, width), np.inf if metric == 1 else -np.inf, np.float32)
    Ip = np.full((nq, width), -1, np.int64)
    for j in range(nq):
        m = int(lims[j + 1] - lims[j])
        Dp[j, :m], Ip[j, :m] = D[lims[j]:lims[j + 1]], I[lims[j]:lims[j + 1]]
    return Dp, Ip


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("storage", rc.STORAGES)
def test_scoring_the_ids_of_a_search_gives_its_distances(storage, metric):
    n, d, nq = 3000, 100, 40
    x, stored = rc.rows_data(storage, d, n)
    q = rc.rows_data("f32", d, nq, seed=2)[0]
    qs = lc.stored_queries(q, storage)
    ix = _index(storage, d, x, metric)
    qd = _cuda(q)
    wide = not storage.startswith("fp8")
    for force_ip in (False, True):
        m = 0 if force_ip else metric
        kw = {"force_ip": True} if force_ip else {}
        kmax = 13 if storage == "fp8_e4m3" else 29                  # the largest k search() serves: MAX_K, on the all-e4m3 index 13
        results = {"search k=5": ix.search(q, 5, **kw), f"search k={kmax}": ix.search(q, kmax, **kw), "search k=5 (CUDA)": ix.search(qd, 5, **kw),
                   "search, 8 queries": ix.search(q[:8], 5, **kw)}
        if wide:
            results["search_wide k=100"] = ix.search_wide(q, 100, **kw)
            radius = results["search_wide k=100"][0][:, 30].copy()   # the 31st score: 30 hits and whatever ties with it
            results["range_search"] = _pad_csr(*ix.range_search(q, radius, **kw), m)
        if not force_ip:
            results["search_fused"] = ix.search_fused(qd, 5)
        for name, (D, I) in results.items():
            rows = slice(0, 8) if "8 queries" in name else slice(None)
            host_I = I.cpu().numpy() if isinstance(I, torch.Tensor) else I
            assert (host_I >= 0).any()
            _same(ix.compute_distance_subset(q[rows], host_I, **kw), D, f"{storage} metric {metric} force_ip {force_ip}: {name} (NumPy)")
            _same(ix.compute_distance_subset(qd[rows], _cuda(host_I), **kw), D, f"{storage} metric {metric} force_ip {force_ip}: {name} (CUDA)")
        # ids no search returned: duplicates, no order, -1 slots, any k
        phi = ix.phi() if m == 1 else 0.0
        assert m == 0 or phi == float(orc.sumsq_canonical(stored).max())
        for k in (1, 37, 1500):
            ids = rc.score_ids(n, nq, k)
            exp = rc.model_scores(qs, stored, ids, m, phi)
            _same(ix.compute_distance_subset(q, ids, **kw), exp, f"model, k={k}")
            _same(ix.compute_distance_subset(qd, _cuda(ids), **kw), exp, f"model, k={k} (CUDA)")
        shifted = np.where(ids >= 0, ids + 500, ids)
        _same(ix.compute_distance_subset(q, shifted, idx_offset=500, **kw), exp, "idx_offset")
        dev_only = ids.copy()
        dev_only[:, 0] = n                                          # a device id past the index: no row
        exp2 = exp.copy()
        exp2[:, 0] = np.inf if m == 1 else -np.inf
        _same(ix.compute_distance_subset(qd, _cuda(dev_only), **kw), exp2, "device ids past the index")
    assert ix.compute_distance_subset(q, np.zeros((nq, 0), np.int64)).shape == (nq, 0)


def test_scores_follow_the_order_of_the_sum():
    x, q = rc.spread_data()
    ix = _index("f32", x.shape[1], x)
    ids = rc.score_ids(len(x), len(q), 9)
    exp = rc.model_scores(q, x, ids)
    assert not np.array_equal(_bits(rc.kernel_scores(q, x, ids, mutant="pairwise")), _bits(exp))
    _same(ix.compute_distance_subset(q, ids), exp, "sequential fp64 sum")
    D, I = ix.search(q, 5)
    _same(ix.compute_distance_subset(q, I), D, "and it is the sum search uses")


@pytest.mark.parametrize("storage,d", [("bf16", 1536), ("f32", 1536), ("bf16", 7), ("fp8_e4m3", 1024), ("fp8_e4m3_docs", 800)])
def test_scores_at_other_row_pitches(storage, d):
    n, nq = 300, 9
    x, stored = rc.rows_data(storage, d, n)
    q = rc.rows_data("f32", d, nq, seed=2)[0]
    ix = _index(storage, d, x, 1)
    ids = rc.score_ids(n, nq, 21)
    _same(ix.compute_distance_subset(q, ids), rc.model_scores(lc.stored_queries(q, storage), stored, ids, 1, ix.phi()), f"{storage} d={d}")
    D, I = ix.search(q, 5)
    _same(ix.compute_distance_subset(q, I), D, "search")


# ------------------------------------------------------------------ 4. the layers above
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_search_and_reconstruct(storage):
    n, d, nq = 2000, 100, 12
    x, stored = rc.rows_data(storage, d, n)
    q = rc.rows_data("f32", d, nq, seed=2)[0]
    ix = _index(storage, d, x)
    for k in (5, 40):                                              # 40 > MAX_K: the wide search
        for qq in (q, _cuda(q)):
            D, I, R = ix.search_and_reconstruct(qq, k)
            _same((D if k == 5 else D), (ix.search(qq, k) if k == 5 else ix.search_wide(qq, k))[0], "D")
            _same(I, (ix.search(qq, k) if k == 5 else ix.search_wide(qq, k))[1], "I")
            _same(R, rc.model_reconstruct(stored, _bits(I)), f"R, k={k}")
            assert type(R) is type(D) and tuple(R.shape) == (nq, k, d)
    mask = np.arange(n) % 2 == 0
    D, I, R = ix.search_and_reconstruct(q, 5, selector=mask)
    assert (I % 2 == 0).all()
    _same(R, stored[I], "selector")
    small = _index(storage, d, x[:3])
    D, I, R = small.search_and_reconstruct(q, 5)
    assert (I[:, 3:] == -1).all() and np.isnan(R[:, 3:]).all() and not np.isnan(R[:, :3]).any()
    _same(R, rc.model_reconstruct(stored[:3], I), "k > ntotal")


def test_faiss_shim_round_trip():
    fs = ram.faiss_shim
    n, d, nq = 500, 33, 6
    x = rc.rows_data("f32", d, n)[0]
    q = rc.rows_data("f32", d, nq, seed=2)[0]
    ip = fs.IndexFlat(d, fs.METRIC_INNER_PRODUCT)
    ip.add(x)
    _same(ip.reconstruct(17), x[17], "reconstruct")
    _same(ip.reconstruct_n(10, 5), x[10:15], "reconstruct_n")
    _same(ip.reconstruct_n(), x, "reconstruct_n()")
    _same(ip.reconstruct_batch(np.array([[3, 3], [499, 0]])), x[[[3, 3], [499, 0]]], "reconstruct_batch")
    D, I, R = ip.search_and_reconstruct(q, 4)
    _same((D, I), ip.search(q, 4), "search_and_reconstruct")
    _same(R, x[I], "R")
    _same(ip.compute_distance_subset(q, I), D, "compute_distance_subset")
    for call in (lambda: ip.reconstruct(n), lambda: ip.reconstruct(-1), lambda: ip.reconstruct_batch(np.array([n])), lambda: ip.reconstruct_n(n - 1, 2)):
        with pytest.raises(IndexError):
            call()
    ip.reset()
    with pytest.raises(IndexError):
        ip.reconstruct(0)
    assert ip.reconstruct_n().shape == (0, d) and ip.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, d)
    # L2: phi-augmented rows in, the augmentation column re-attached on the way out (recomputed, not stored)
    aug, qa = orc.augment_xb(x), orc.augment_xq(q)
    l2 = fs.IndexFlat(d + 1, fs.METRIC_L2)
    l2.add(aug)
    phi = l2.mips_index.phi()
    back = l2.reconstruct_n()
    assert back.shape == (n, d + 1) and back.dtype == np.float32
    _same(back[:, :d], x, "the stored columns")
    _same(back[:, d], rc.l2_column(x, phi), "the recomputed column")
    assert np.allclose(back[:, d], aug[:, d], rtol=1e-4, atol=1e-3 * np.sqrt(phi))
    _same(l2.reconstruct(7), back[7], "reconstruct (L2)")
    D, I, R = l2.search_and_reconstruct(qa, 50)                    # the wide search; 50 <= n
    _same(R, back[I], "R (L2)")
    _same(l2.compute_distance_subset(qa, I), D, "compute_distance_subset (L2)")
    pad = np.concatenate([I[:, :3], np.full((nq, 1), -1)], axis=1)
    got = l2.compute_distance_subset(qa, pad)
    assert np.all(got[:, 3] == np.inf) and np.isnan(l2.reconstruct_batch(pad)[:, 3]).all()


def test_mips_rows_feed_the_rescore_and_group_hits_are_the_list_comprehension():
    n, d, B, k = 400, 64, 6, 5
    x = rc.rows_data("f32", d, n)[0]
    q = rc.rows_data("f32", d, B, seed=2)[0]
    aid = [f"a{r % 23}" for r in range(n)]
    args = ram.MipsArgs(mips_topk=k, mips_metric_type=0, mips_normalize=False)
    m = ram.Mips(args, data={"mips_column": [f"text {r}" for r in range(n)], "aid": aid})
    m.build_index(x)
    qd = _cuda(q)
    s, i = m.search_device(qd, k=k)
    s2, i2, rows = m.search_device(qd, k=k, return_rows=True)
    _same((s2, i2)[0], s, "scores")
    _same(i2, i, "indices")
    assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == (B, k, d)
    host_rows = _cuda(x[i.cpu().numpy()])                           # the caller's own copy of the index: what the rows replace
    _same(rows, host_rows, "rows")
    _same(ram.cosine_rescore(qd, rows), ram.cosine_rescore(qd, host_rows), "cosine_rescore")
    q_aid = [aid[int(i[j, 1])] if j % 2 else "nobody" for j in range(B)]
    ind = i.cpu().numpy()
    full = [m.embeddings[[t for t in row if t >= 0]] for row in ind]
    pred = torch.tensor([[b == v for v in e[m.index_column]] for e, b in zip(full, q_aid)]).float()   # Mips.forward's expression
    for got in (m.retrieved_group_hits(i, q_aid), m.retrieved_group_hits(ind, q_aid)):
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), pred)
    assert pred.sum() >= B // 2 and m.retrieved_group_hits(i, q_aid).is_cuda
    metrics = ram.retriever_metrics(m.retrieved_group_hits(ind, q_aid), torch.ones(B))
    assert metrics == ram.retriever_metrics(pred, torch.ones(B))


# ------------------------------------------------------------------ 5. the C ABI from plain C
def test_c_abi_rows_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_rows_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_rows_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
