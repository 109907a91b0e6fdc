"""IVF index over PQ codes on the GPU (include/mips_hip_ivfpq.h): everything bit for bit against the NumPy restatement
of tests/ivfpq_cases.py, no tolerance anywhere.  The scan is tested on planted centroids, codebooks, codes and assignments
(set_centroids / set_codebook / add_codes), so list sizes are chosen and nothing depends on training; training, add, the calls by id,
save / load and the refusals have their own tests.  The CPU side (that the cases bite, the header, the kernels' registers) is
tests/test_ivfpq_host.py; graph capture is tests/test_gpu_ivfpq_graph.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivfpq_cases as vc  # noqa: E402
import pq_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.uint32


def planted(case, by_residual=True):
    ix = ram.IvfPqIndex(case["d"], case["nlist"], case["M"], by_residual=by_residual)
    ix.set_centroids(case["centroids"])
    ix.set_codebook(case["codebook"])
    if len(case["codes"]):
        ix.add_codes(case["codes"], case["assign"])
    return ix


def same(got, want, what=""):
    D, I = got
    assert np.array_equal(np.asarray(I), want[1]), what
    assert np.array_equal(np.asarray(D).view(U), want[0].view(U)), what


def ref(case, k, nprobe, **kw):
    return vc.search(case["q"], case["centroids"], case["codebook"], case["codes"], case["assign"], k, nprobe, **kw)


def ranked(full, lists, assign, k, idx_offset=0):
    """the best k of the rows whose list is in lists[j], from the scores `full` [nq, n] of all rows"""
    out_d = np.full((len(full), k), -np.inf, np.float32)
    out_i = np.full((len(full), k), -1, np.int64)
    for j in range(len(full)):
        rows = np.flatnonzero(np.isin(assign, lists[j]))
        order = np.lexsort((rows, -full[j, rows].astype(np.float64)))[:k]
        out_d[j, :len(order)] = full[j, rows[order]]
        out_i[j, :len(order)] = rows[order] + idx_offset
    return out_d, out_i


@pytest.mark.parametrize("nlist", vc.NLISTS)
@pytest.mark.parametrize("d,M", vc.GEOMETRY)
def test_scan_geometry(d, M, nlist):
    """ntotal, list sizes (0, 1, 63, 64, 65, 64 WAVES +- 1, everything in the last list), nq, k and nprobe across their ranges;
    fewer probed rows than k (padding)"""
    padded = 0
    for n in vc.NTOTALS:
        case = vc.case_planted(d, M, nlist, n, max(vc.NQS))
        ix = planted(case)
        assert ix.ntotal == n and ix.is_trained and ix.bytes_per_row == M + 4
        assert np.array_equal(ix.list_sizes(), np.bincount(case["assign"], minlength=nlist))
        assert np.array_equal(ix.codes(), case["codes"]) and np.array_equal(ix.assignments(), case["assign"])
        full = vc.all_scores(case["q"], case["centroids"], case["codebook"], case["codes"], case["assign"])
        for nprobe in sorted({1, 3, nlist, nlist + 5}):
            lists, _ = vc.probe(case["q"], case["centroids"], nprobe)
            for nq, k in ((1, 1), (3, 5), (17, 29), (1, 29), (17, 1)):
                want = ranked(full[:nq], lists[:nq], case["assign"], k)
                same(ix.search(case["q"][:nq], k, nprobe=nprobe), want, (d, M, nlist, n, nprobe, nq, k))
                padded += int((want[1] == -1).any())
    assert padded > 0


def test_all_rows_in_one_list():
    for d, M in ((32, 4), (80, 40)):
        case = vc.case_planted(d, M, 8, 1000, 3, one_list=5)
        ix = planted(case)
        assert list(ix.list_sizes()) == [0, 0, 0, 0, 0, 1000, 0, 0]
        for nprobe in (1, 3, 8):
            same(ix.search(case["q"], 29, nprobe=nprobe), ref(case, 29, nprobe), (d, M, nprobe))


@pytest.mark.parametrize("d,M", [(32, 4), (80, 40)])
def test_scan_segments_and_query_slice_give_identical_bits(d, M):
    case = vc.case_planted(d, M, 33, 4097, 5)
    ix = planted(case)
    ix.nprobe = 7
    want = ref(case, 29, 7)
    same(ix.search(case["q"], 29), want)
    assert ix.scan_segments == 0
    for S in (1, 2, 3, 7, 64, 65536):                              # (65536: clipped to what the merge takes)
        ix.scan_segments = S
        same(ix.search(case["q"], 29), want, S)
        same(ix.search(case["q"], 5, nprobe=33), ref(case, 5, 33), S)
    ix.scan_segments = 0
    ix.query_slice = 2                                             # 5 queries: slices of 2, 2 and 1
    same(ix.search(case["q"], 29), want)
    D, I = ix.search(torch.from_numpy(case["q"]).cuda(), 29)
    same((D.cpu().numpy(), I.cpu().numpy()), want)
    assert np.array_equal(ix.compute_distance_subset(case["q"], want[1]).view(U), want[0].view(U))


@pytest.mark.parametrize("d,M", [(32, 16), (80, 40)])
def test_by_residual_false_is_the_pq_index_when_every_list_is_probed(d, M):
    case = vc.case_planted(d, M, 8, 1000, 3)
    ix = planted(case, by_residual=False)
    flat = ram.PqIndex(d, M)
    flat.set_codebook(case["codebook"])
    flat.add_codes(case["codes"])
    for nprobe in (8, 13):
        same(ix.search(case["q"], 29, nprobe=nprobe), flat.search(case["q"], 29), nprobe)
    same(ix.search(case["q"], 5, nprobe=3), ref(case, 5, 3, by_residual=False))
    rows = pc.reconstruct(case["codes"], case["codebook"])         # a plain decode
    assert np.array_equal(ix.reconstruct_n().view(U), rows.view(U))
    D, I = ix.search(case["q"], 5, nprobe=3)
    assert np.array_equal(ix.compute_distance_subset(case["q"], I).view(U), D.view(U))


def test_training_equals_its_two_halves_and_the_restatement():
    case = vc.case_train()
    x = case["x"]
    ix = ram.IvfPqIndex(case["d"], case["nlist"], case["M"])
    assert not ix.is_trained and ix.niter == 10 and ix.pq_niter == 10
    ix.niter = 3
    ix.pq_niter = 3
    ix.train(x)
    assert ix.is_trained
    ix.add(x)
    ivf = ram.IvfIndex(case["d"], case["nlist"], "bf16")          # the coarse half: the IVF index's own trainer and assignment
    ivf.niter = 3
    ivf.train(x)
    ivf.add(x)
    assert np.array_equal(ix.centroids().view(U), ivf.centroids().view(U)) and np.array_equal(ix.assignments(), ivf.assignments())
    cen, cb = vc.train(x, case["nlist"], case["M"], 3, 3)          # the restatement
    assert np.array_equal(ix.centroids().view(U), cen.view(U)) and np.array_equal(ix.codebook().view(U), cb.view(U))
    half = ram.PqIndex(case["d"], case["M"])                       # the PQ half: the PQ index's own trainer on the residuals
    half.niter = 3
    half.train(vc.training_residuals(x, cen))
    assert np.array_equal(ix.codebook().view(U), half.codebook().view(U))
    codes, a = vc.encode(x, cen, cb)
    assert np.array_equal(ix.codes(), codes) and np.array_equal(ix.assignments(), a)
    c = dict(case, centroids=cen, codebook=cb, codes=codes, assign=a)
    same(ix.search(case["q"], 5, nprobe=3), ref(c, 5, 3))
    dev = ram.IvfPqIndex(case["d"], case["nlist"], case["M"])      # device rows, then bf16 rows: the same rule on the widened values
    dev.niter = dev.pq_niter = 3
    dev.train(torch.from_numpy(x).cuda())
    assert np.array_equal(dev.codebook().view(U), cb.view(U)) and np.array_equal(dev.centroids().view(U), cen.view(U))
    xb = torch.from_numpy(x).to(torch.bfloat16)
    dev.train(xb)                                                  # training again while empty is allowed
    cen_b, cb_b = vc.train(xb.float().numpy(), case["nlist"], case["M"], 3, 3)
    assert np.array_equal(dev.centroids().view(U), cen_b.view(U)) and np.array_equal(dev.codebook().view(U), cb_b.view(U))
    dev.add(xb.cuda())
    codes_b, a_b = vc.encode(xb.float().numpy(), cen_b, cb_b)
    assert np.array_equal(dev.codes(), codes_b) and np.array_equal(dev.assignments(), a_b)
    raw = ram.IvfPqIndex(case["d"], case["nlist"], case["M"], by_residual=False)
    raw.niter = raw.pq_niter = 3
    raw.train(x)
    assert np.array_equal(raw.codebook().view(U), vc.train(x, case["nlist"], case["M"], 3, 3, by_residual=False)[1].view(U))


def test_training_refusals():
    case = vc.case_train()
    ix = ram.IvfPqIndex(case["d"], case["nlist"], case["M"])
    ix.niter = ix.pq_niter = 1
    with pytest.raises(RuntimeError):
        ix.train(case["x"][:255])                                  # n < 256
    many = ram.IvfPqIndex(case["d"], 300, case["M"])
    with pytest.raises(RuntimeError):
        many.train(case["x"][:290])                                # n < nlist
    x = case["x"].copy()
    x[300, 7] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        ix.train(x)
    with pytest.raises(RuntimeError, match="NaN"):
        ix.train(torch.from_numpy(x).cuda())
    with pytest.raises(RuntimeError):
        ix.add(case["x"][:3])                                      # not trained
    with pytest.raises(RuntimeError):
        ix.centroids()
    ix.train(case["x"])
    ix.add(case["x"][:10])
    for call in (lambda: ix.train(case["x"]), lambda: ix.set_codebook(ix.codebook()), lambda: ix.set_centroids(ix.centroids())):
        with pytest.raises(RuntimeError, match="holds"):
            call()
    ix.reset()
    ix.train(case["x"])                                            # empty again: allowed
    half = ram.IvfPqIndex(case["d"], case["nlist"], case["M"])     # trained once BOTH halves are set
    half.set_centroids(ix.centroids())
    assert not half.is_trained
    half.set_codebook(ix.codebook())
    assert half.is_trained


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_probe_reports_the_canonical_score_of_query_and_centroid(dtype):
    case = vc.case_planted(80, 40, 33, 1000, 17)
    ix = planted(case)
    q = torch.from_numpy(case["q"])
    if dtype == "bf16":
        q = q.to(torch.bfloat16)
    cen = ram.MipsIndex(80, dtype="f32")                           # the centroids as rows of a flat fp32-exact index
    cen.add(case["centroids"])
    for nprobe in (1, 3, 29, 33):                                  # (through mips_search up to 29 lists, mips_search_wide beyond)
        L, T = ix.probe(q, nprobe, return_scores=True)
        wl, wt = vc.probe(q.float().numpy(), case["centroids"], nprobe)
        assert np.array_equal(L, wl) and np.array_equal(T.view(U), wt.view(U)), nprobe
        by_id = cen.compute_distance_subset(q if dtype == "bf16" else case["q"], L.astype(np.int64))
        assert np.array_equal(np.asarray(by_id).view(U), T.view(U)), nprobe            # mips_score_subset on the centroids
        Ld, Td = ix.probe(q.cuda(), nprobe, return_scores=True)
        assert np.array_equal(Ld.cpu().numpy(), L) and np.array_equal(Td.cpu().numpy().view(U), T.view(U))
    assert np.array_equal(ix.probe(q, 3), L[:, :3])


def test_by_id():
    case = vc.case_planted(48, 24, 8, 1000, 3)
    ix = planted(case)
    D, I = ix.search(case["q"], 5, nprobe=2, idx_offset=100)
    rows = vc.reconstruct(case["codes"], case["assign"], case["centroids"], case["codebook"])
    got = ix.reconstruct_batch(I, idx_offset=100)
    assert got.shape == (3, 5, 48) and np.array_equal(got.view(U), rows[I - 100].view(U))
    assert np.array_equal(ix.reconstruct(17).view(U), rows[17].view(U)) and np.array_equal(ix.reconstruct_n(998).view(U), rows[998:].view(U))
    assert not np.array_equal(rows, vc.reconstruct(case["codes"], case["assign"], case["centroids"], case["codebook"], wrong="no_centroid"))
    assert np.array_equal(ix.compute_distance_subset(case["q"], I, idx_offset=100).view(U), D.view(U))   # scoring I reproduces D
    full = vc.all_scores(case["q"], case["centroids"], case["codebook"], case["codes"], case["assign"])
    every = np.tile(np.arange(1000), (3, 1))                       # rows of lists that were not probed too: their own coarse term
    assert np.array_equal(ix.compute_distance_subset(case["q"], every).view(U), full.view(U))
    ids = torch.tensor([[3, -1, 1000], [999, 1 << 33, 0], [5, 5, -7]], device="cuda")
    got = ix.reconstruct_batch(ids).cpu().numpy()
    sc = ix.compute_distance_subset(torch.from_numpy(case["q"]).cuda(), ids).cpu().numpy()
    for j in range(3):
        for t in range(3):
            r = int(ids[j, t])
            if 0 <= r < 1000:
                assert np.array_equal(got[j, t].view(U), rows[r].view(U)) and sc[j, t].view(U) == full[j, r].view(U)
            else:
                assert (got[j, t].view(U) == 0x7FC00000).all() and sc[j, t] == -np.inf                # "no row"
    with pytest.raises(RuntimeError):
        ix.reconstruct_batch(np.array([1000]))                     # a host id past the index
    assert np.isnan(ix.reconstruct_batch(np.array([-1]))).all()
    with pytest.raises(IndexError):
        ix.reconstruct(1000)
    qb = torch.from_numpy(case["q"]).to(torch.bfloat16)            # bf16 queries: the coarse term of their widened values
    Db, Ib = ix.search(qb, 5, nprobe=2)
    assert np.array_equal(ix.compute_distance_subset(qb, Ib).view(U), Db.view(U))


def test_ties_and_the_zero_query():
    case = vc.case_ties()
    ix = planted(case)
    D, I = ix.search(case["q"], 29, nprobe=3)
    lowest = np.flatnonzero(np.isin(case["assign"], [0, 1, 2]))[:29]
    assert (I == lowest).all()                                     # duplicated codes in different lists: the lowest rows
    same((D, I), ref(case, 29, 3))
    case = vc.case_planted(32, 4, 8, 1000, 3)
    ix = planted(case)
    z = np.zeros((2, 32), np.float32)
    D, I = ix.search(z, 5, nprobe=3)                               # the zero query: lists 0, 1, 2 and every score +0
    assert (D.view(U) == 0).all() and (I == np.flatnonzero(np.isin(case["assign"], [0, 1, 2]))[:5]).all()


def test_order_of_the_sum_and_magnitudes():
    case = vc.case_sum_order()
    want = ref(case, 29, 3)
    same(planted(case).search(case["q"], 29, nprobe=3), want)
    for wrong in ("coarse_last", "no_coarse", "fp64"):             # (what the case is for: these sums give other bits)
        assert not np.array_equal(ref(case, 29, 3, wrong=wrong)[0].view(U), want[0].view(U)), wrong
    case = vc.case_planted(48, 24, 8, 1000, 3)
    base = ref(case, 5, 3)
    for e in (30, -30):                                            # rows x 2^e: centroids and codebook scaled, scores scaled exactly
        s = np.float32(2.0 ** e)
        scaled = dict(case, centroids=case["centroids"] * s, codebook=case["codebook"] * s)
        D, I = planted(scaled).search(case["q"], 5, nprobe=3)
        assert np.array_equal(I, base[1]) and np.array_equal(D, base[0] * s)
        same((D, I), ref(scaled, 5, 3))


def test_forms_prefix_and_bf16():
    case = vc.case_planted(80, 40, 33, 4097, 17)
    ix = planted(case)
    D, I = ix.search(case["q"], 29, nprobe=5)
    same((D, I), ref(case, 29, 5))
    for k in (1, 5, 28):                                           # the prefix property
        same(ix.search(case["q"], k, nprobe=5), (D[:, :k], I[:, :k]), k)
    Dd, Id = ix.search(torch.from_numpy(case["q"]).cuda(), 29, nprobe=5)      # a CUDA tensor in gives CUDA tensors out
    assert isinstance(Dd, torch.Tensor) and Dd.is_cuda and Id.is_cuda and Id.dtype == torch.int64
    same((Dd.cpu().numpy(), Id.cpu().numpy()), (D, I))
    Dh, Ih = ix.search(torch.from_numpy(case["q"]), 29, nprobe=5)             # a host tensor is host memory: NumPy out
    assert isinstance(Dh, np.ndarray)
    same((Dh, Ih), (D, I))
    qb = torch.from_numpy(case["q"]).to(torch.bfloat16)            # bf16 queries: their widened values
    Db, Ib = ix.search(qb.cuda(), 5, nprobe=5)
    same((Db.cpu().numpy(), Ib.cpu().numpy()), ref(dict(case, q=qb.float().numpy()), 5, 5))
    same(ix.search(case["q"], 5, nprobe=5, idx_offset=1 << 40), ref(case, 5, 5, idx_offset=1 << 40))
    dev = ram.IvfPqIndex(80, 33, 40)                               # device codes and assignments
    dev.set_centroids(case["centroids"])
    dev.set_codebook(case["codebook"])
    dev.add_codes(torch.from_numpy(case["codes"]).cuda(), torch.from_numpy(case["assign"]).cuda())
    same(dev.search(case["q"], 29, nprobe=5), (D, I))


def test_add_after_add_save_load_and_reset(tmp_path):
    case = vc.case_train()
    x = case["x"]
    ix = ram.IvfPqIndex(case["d"], case["nlist"], case["M"])
    ix.niter = ix.pq_niter = 2
    ix.train(x)
    cen, cb = ix.centroids(), ix.codebook()
    ix.add(x[:123])
    ix.add(torch.from_numpy(x[123:]).cuda())                       # add after add (growth in between): the table is rebuilt
    codes, a = vc.encode(x, cen, cb)
    assert ix.ntotal == 1000 and np.array_equal(ix.codes(), codes) and np.array_equal(ix.assignments(), a)
    assert np.array_equal(ix.list_sizes(), np.bincount(a, minlength=case["nlist"]))
    c = dict(case, centroids=cen, codebook=cb, codes=codes, assign=a)
    ix.nprobe = 3
    D, I = ix.search(case["q"], 5)
    same((D, I), ref(c, 5, 3))
    path = str(tmp_path / "ivfpq")
    ix.save(path)
    assert sorted(os.listdir(path)) == ["assign.i32", "centroids.f32", "codebook.f32", "codes.u8", "meta.json"]
    assert os.path.getsize(os.path.join(path, "codes.u8")) == 1000 * 4 and os.path.getsize(os.path.join(path, "assign.i32")) == 4000
    back = ram.IvfPqIndex.load(path)
    assert back.ntotal == 1000 and back.is_trained and (back.niter, back.pq_niter, back.nprobe) == (2, 2, 3)
    assert (back.d, back.nlist, back.M, back.by_residual) == (ix.d, ix.nlist, ix.M, True)
    assert np.array_equal(back.codebook().view(U), cb.view(U)) and np.array_equal(back.centroids().view(U), cen.view(U))
    assert np.array_equal(back.codes(), codes) and np.array_equal(back.assignments(), a)
    same(back.search(case["q"], 5), (D, I))
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and (ix.list_sizes() == 0).all()
    assert np.array_equal(ix.codebook().view(U), cb.view(U)) and np.array_equal(ix.centroids().view(U), cen.view(U))   # rows go, the training stays
    D0, I0 = ix.search(case["q"], 3)
    assert (I0 == -1).all() and np.isneginf(D0).all()
    ix.add(x[:50])
    same(ix.search(case["q"], 5), ref(dict(c, codes=codes[:50], assign=a[:50]), 5, 3))
    with pytest.raises(RuntimeError):
        ram.IvfPqIndex(case["d"], case["nlist"], case["M"]).save(str(tmp_path / "untrained"))


def test_refusals():
    for kw in (dict(metric=ram.METRIC_L2), dict(nbits=4)):
        with pytest.raises(NotImplementedError):
            ram.IvfPqIndex(64, 16, 8, **kw)
    for args in ((2048, 16, 8), (516, 16, 129), (64, 0, 8), (64, 65537, 8)):
        with pytest.raises(NotImplementedError):
            ram.IvfPqIndex(*args)
    with pytest.raises(ValueError):
        ram.IvfPqIndex(30, 16, 8)
    lib = ram._lib.load()
    import ctypes
    h = ctypes.c_void_p()
    assert lib.mips_ivfpq_create(ctypes.byref(h), 0, 64, 16, 8, 8, 1, ram.METRIC_L2) == -3 and b"inner product" in lib.mips_last_error()   # MIPS_E_UNSUPPORTED
    assert lib.mips_ivfpq_create(ctypes.byref(h), 0, 64, 16, 8, 6, 1, ram.METRIC_IP) == -3
    assert lib.mips_ivfpq_create(ctypes.byref(h), 0, 516, 16, 129, 8, 1, 0) == -3 and lib.mips_ivfpq_create(ctypes.byref(h), 0, 64, 65537, 8, 8, 1, 0) == -3
    case = vc.case_planted(32, 4, 8, 100, 2)
    ix = planted(case)
    with pytest.raises(NotImplementedError):
        ix.search(case["q"], 30)
    with pytest.raises(RuntimeError):
        ix.search(case["q"], 0)
    with pytest.raises(RuntimeError):
        ix.search(case["q"], 5, nprobe=0)
    with pytest.raises(ValueError):
        ix.search(case["q"][:, :31], 5)
    with pytest.raises(NotImplementedError):
        ix.add(np.zeros((3, 32), np.uint8))                        # integers are not rows: codes go through add_codes
    with pytest.raises(ValueError):
        ix.add_codes(case["codes"][:, :3], case["assign"])
    with pytest.raises(ValueError):
        ix.add_codes(case["codes"], case["assign"] + 8)            # a list outside [0, nlist)
    with pytest.raises(RuntimeError):
        ix.add_codes(torch.from_numpy(case["codes"]).cuda(), torch.from_numpy(case["assign"] + 8).cuda())
    assert ix.ntotal == 100
    for name in ("search_wide", "range_search", "remove_ids", "update_rows"):
        with pytest.raises(NotImplementedError):
            getattr(ix, name)(case["q"], 5)
    wide = ram.IvfPqIndex(32, 2000, 4)                             # p > 1024
    with pytest.raises(NotImplementedError):
        wide.search(case["q"], 5, nprobe=1025)
    fresh = ram.IvfPqIndex(32, 8, 4)
    with pytest.raises(RuntimeError):
        fresh.search(case["q"], 5)                                 # not trained
    with pytest.raises(RuntimeError):
        fresh.add_codes(case["codes"], case["assign"])
    D, I = ix.search(np.zeros((0, 32), np.float32), 5)
    assert D.shape == (0, 5) and I.shape == (0, 5)


def test_c_abi_ivfpq_from_plain_c(tmp_path):
    lib_dir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_ivfpq_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_ivfpq_smoke.c"), "-I", os.path.join(ROOT, "include"), "-L", lib_dir,
                           "-lmips_hip", f"-Wl,-rpath,{lib_dir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches: 0" in out.stdout, out.stdout + out.stderr
