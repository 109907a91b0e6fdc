"""The 8-bit scalar-quantised index (dtype "sq8", include/mips_hip_sq8.h) on the GPU, against the NumPy restatement of
tests/sq8_cases.py bit for bit: training, stored codes, decoded rows, search results (I and D) on every case, every shipped
sq8_scan_kernel instance by name, subset scores, removal, save / load, the refusals, the faiss shim, the Mips facade and the C ABI
from plain C."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from retrieval_augmented_mds_amd import faiss_shim

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import sq8_cases as sq
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

NS, DS, NQS, KS = (1, 31, 33, 4099), (100, 256, 768, 1000), (1, 17, 33, 130), (1, 5, 7, 13, 29)
_REF = {}


def _ref(kind, n, d):
    """One reference per (case, n, d): 130 queries, top-29 -- the first nq queries and the first k columns are the reference of
    every smaller search (a top-k list is a prefix of the top-29 list).  Computed once, never modified."""
    key = (kind, n, d)
    if key not in _REF:
        case = {"gauss": sq.case_gauss, "outside": sq.case_outside, "duplicates": sq.case_duplicates}[kind](n, d, max(NQS))
        vmin, vdiff, codes = sq.prepared(case)
        D, I = sq.search(case["q"], codes, vmin, vdiff, max(KS))
        for a in (vmin, vdiff, codes, D, I):
            a.setflags(write=False)
        _REF[key] = (case, vmin, vdiff, codes, D, I)
    return _REF[key]


def _index(case, device_rows=False):
    ix = ram.MipsIndex(case["rows"].shape[1], dtype="sq8", device=0)
    ix.train(torch.from_numpy(case["train"]).cuda() if device_rows else case["train"])
    h = len(case["rows"]) // 2
    ix.add(case["rows"][:h])                                   # host rows, then device rows: two adds, growth in between
    ix.add(torch.from_numpy(case["rows"][h:]).cuda())
    return ix


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bits = (lambda a: a.view(np.uint32)) if want.dtype == np.float32 else (lambda a: a)
    assert np.array_equal(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(want))), what


def _certified(ix):
    st = ix.margin_stats()
    assert st["unresolved"] == 0 and st["rescanned"] == st["flagged"], st


# ------------------------------------------------------------------ training, codes, decoded rows
@pytest.mark.parametrize("d", DS)
def test_training_codes_and_decoded_rows(d):
    case, vmin, vdiff, codes, _, _ = _ref("gauss", 4099, d)
    for device_rows in (False, True):
        ix = ram.MipsIndex(d, dtype="sq8", device=0)
        assert not ix.is_trained
        with pytest.raises(RuntimeError):
            ix.add(case["rows"][:2])
        with pytest.raises(RuntimeError):
            ix.sq8_params()
        ix = _index(case, device_rows)
        assert ix.is_trained and ix.ntotal == 4099
        gmin, gdiff = ix.sq8_params()
        _same(gmin, vmin, "vmin"), _same(gdiff, vdiff, "vdiff")
        _same(ix.reconstruct_batch(np.arange(4099), raw=True), codes, "codes")
        _same(ix.rows_raw(), codes, "rows_raw")
        _same(ix.reconstruct_n(0, 4099), sq.decode(codes, vmin, vdiff), "decoded rows")
    ids = torch.tensor([[4098, -1], [0, 7]], device="cuda")
    dec = ix.reconstruct_batch(ids).cpu().numpy()
    assert np.isnan(dec[0, 1]).all()
    _same(dec[1], sq.decode(codes[[0, 7]], vmin, vdiff), "decoded rows, CUDA ids")
    assert (ix.reconstruct_batch(ids, raw=True)[0, 1] == 0).all() and (ix.reconstruct_batch(ids, zero_missing=True)[0, 1] == 0).all()
    # bf16 rows and bf16 training data are widened first
    xb = torch.from_numpy(case["rows"][:500]).cuda().bfloat16()
    ib = ram.MipsIndex(d, dtype="sq8", device=0)
    ib.train(xb)
    ib.add(xb)
    wide = xb.float().cpu().numpy()
    bmin, bdiff = sq.train(wide)
    _same(ib.sq8_params()[0], bmin, "vmin of bf16 rows"), _same(ib.rows_raw(), sq.encode(wide, bmin, bdiff), "codes of bf16 rows")


def test_training_rules():
    case, vmin, vdiff, codes, _, _ = _ref("gauss", 33, 100)
    ix = ram.MipsIndex(100, dtype="sq8", device=0)
    # before training: a search answers as an empty index does, scoring its I is refused (by the library itself, with the error
    # code, for host and device ids alike), reconstruct finds no row
    q3 = case["q"][:3]
    d0, i0 = ix.search(q3, 5)
    assert (i0 == -1).all() and np.isneginf(d0).all()
    with pytest.raises(RuntimeError, match="not trained"):
        ix.compute_distance_subset(q3, i0)
    out = np.full((3, 5), 7.0, np.float32)
    assert ix._lib.mips_score_subset(ix._h, q3.ctypes.data, ram._lib.DTYPE_F32, 3, i0.ctypes.data, 5, out.ctypes.data, 0, 0, None) == -1
    assert b"not trained" in ix._lib.mips_last_error() and (out == 7.0).all()
    qd, idd, od = torch.from_numpy(q3).cuda(), torch.from_numpy(i0).cuda(), torch.full((3, 5), 7.0, device="cuda")
    flags = ram._lib.Q_DEVICE | ram._lib.OUT_DEVICE | ram._lib.IDS_DEVICE
    assert ix._lib.mips_score_subset(ix._h, qd.data_ptr(), ram._lib.DTYPE_F32, 3, idd.data_ptr(), 5, od.data_ptr(), 0, flags, None) == -1
    assert (od == 7.0).all().item()
    assert torch.isnan(ix.reconstruct_batch(torch.tensor([-1, 0], device="cuda"))).all().item()
    for badv in (np.nan, np.inf, -np.inf):
        x = case["rows"].copy()
        x[17, 60] = badv
        with pytest.raises(RuntimeError, match="NaN or an infinity"):
            ix.train(x)
        with pytest.raises(RuntimeError, match="NaN or an infinity"):
            ix.train(torch.from_numpy(x).cuda())
        assert not ix.is_trained
    with pytest.raises(RuntimeError, match="no training rows"):
        ix.train(np.zeros((0, 100), np.float32))
    ix.train(case["rows"] * 2)
    ix.train(case["rows"])                                     # an empty index may be trained again
    _same(ix.sq8_params()[1], vdiff, "vdiff after the second training")
    ix.add(case["rows"])
    with pytest.raises(RuntimeError, match="holds 33 rows"):
        ix.train(case["rows"])
    with pytest.raises(RuntimeError, match="holds 33 rows"):
        ix.set_sq8_params(vmin, vdiff)
    ix.reset()                                                 # the parameters stay; training is possible again
    assert ix.is_trained and ix.ntotal == 0
    ix.add(codes)                                              # raw codes as rows
    _same(ix.rows_raw(), codes, "raw codes")
    # rows added after training may hold anything: NaN -> 0, +inf -> 255, -inf -> 0, values outside the range clamp (host and
    # device rows; column 3 is the constant column: code 0 whatever comes)
    odd = case["rows"][:4].copy()
    odd[0, ::3], odd[1, ::2], odd[2, 1::2], odd[3] = np.nan, np.inf, -np.inf, np.float32(1e30)
    odd[0, 1], odd[1, 1] = np.float32(-1e30), np.float32(-0.0)
    want = sq.encode(odd, vmin, vdiff)
    assert (want[0, 0] == 0) and (want[1, 0] == 255) and (want[2, 1] == 0) and (want[3, 0] == 255) and (want[:, 3] == 0).all()
    ix.add(odd)
    ix.add(torch.from_numpy(odd).cuda())
    ix.add(torch.from_numpy(odd).cuda().bfloat16())
    _same(ix.rows_raw(33, 4), want, "codes of non-finite host rows"), _same(ix.rows_raw(37, 4), want, "codes of non-finite device rows")
    _same(ix.rows_raw(41, 4), sq.encode(torch.from_numpy(odd).bfloat16().float().numpy(), vmin, vdiff), "codes of non-finite bf16 rows")
    with pytest.raises(ValueError, match="rows only"):
        ix.search(codes[:2], 1)                                # uint8 arrays are never queries
    with pytest.raises(ValueError, match="rows only"):
        ix.compute_distance_subset(torch.from_numpy(codes[:2].copy()).cuda(), np.zeros((2, 1), np.int64))
    iy = ram.MipsIndex(100, dtype="sq8", device=0)
    bad = vdiff.copy()
    bad[5] = -1
    with pytest.raises(RuntimeError, match="vdiff >= 0"):
        iy.set_sq8_params(vmin, bad)
    iy.set_sq8_params(vmin, vdiff)
    assert iy.is_trained


# ------------------------------------------------------------------ search results against the reference
def _check_search(ix, case, D, I, nq, k, what):
    q = case["q"][:nq]
    d, i = ix.search(q, k)
    _same(i, I[:nq, :k], f"{what}: I, host"), _same(d, D[:nq, :k], f"{what}: D, host")
    _certified(ix)
    d, i = ix.search(torch.from_numpy(q).cuda(), k)
    _same(i, I[:nq, :k], f"{what}: I, device"), _same(d, D[:nq, :k], f"{what}: D, device")
    _certified(ix)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_search_matches_the_reference(n, d):
    """(a), (c), (f), (g): every n x d with every nq and k -- the 16 / 32 / 64-query tiles, a second query tile, the four pools;
    n = 1 / 31 / 33 with k up to 29 is k > ntotal"""
    case, vmin, vdiff, codes, D, I = _ref("gauss", n, d)
    ix = _index(case)
    for nq in NQS:
        for k in KS:
            _check_search(ix, case, D, I, nq, k, f"n={n} d={d} nq={nq} k={k}")
            assert ix.last_kernel.startswith("mips::sq8_scan_kernel<6, "), ix.last_kernel
    if n < 29:
        assert (I[:, n:] == -1).all() and np.isneginf(D[:, n:]).all()


@pytest.mark.parametrize("kind,n,d", [("outside", 4099, 100), ("outside", 33, 768), ("duplicates", 4099, 1000), ("duplicates", 900, 256)])
def test_clamped_rows_and_planted_duplicates(kind, n, d):
    """(d) rows outside the trained range, (e) 3 and 70 copies of a best row: ties to the lowest row, > 64 rows at the k-th score"""
    case, vmin, vdiff, codes, D, I = _ref(kind, n, d)
    ix = _index(case)
    _same(ix.rows_raw(), codes, "codes")
    if kind == "duplicates":
        assert (D[1, :29] == D[1, 0]).all() and (np.diff(I[1]) > 0).all()          # query 1: 29 of the 70 copies, ascending rows
    for nq, k in ((130, 29), (33, 5), (17, 13), (2, 7), (130, 1)):
        _check_search(ix, case, D, I, nq, k, f"{kind} n={n} d={d} nq={nq} k={k}")
    for ns in (8, 24):                                                             # both split geometries
        ix.set_param("nsplit", ns)
        _check_search(ix, case, D, I, 130, 5, f"{kind} nsplit={ns}")
        _check_search(ix, case, D, I, 17, 29, f"{kind} nsplit={ns}")
    ix.set_param("nsplit", 0)


def test_all_codes_in_every_column():
    """(b): all 256 codes in every column, whole rows of 255 and of 0"""
    for d in (100, 256):
        case = sq.case_all_codes(d, 33)
        vmin, vdiff, codes = sq.prepared(case)
        assert all(set(codes[:, j]) == set(range(256)) for j in range(d))
        ix = _index(case)
        _same(ix.rows_raw(), codes, "codes")
        _same(ix.reconstruct_n(0, len(codes)), sq.decode(codes, vmin, vdiff), "decoded")
        D, I = sq.search(case["q"], codes, vmin, vdiff, 29)
        for nq, k in ((33, 29), (17, 5), (1, 13)):
            _check_search(ix, case, D, I, nq, k, f"all codes d={d} nq={nq} k={k}")


def test_packed_bf16_queries_offset_and_split_tail():
    case, vmin, vdiff, codes, D, I = _ref("gauss", 4099, 768)
    ix = _index(case)
    q = torch.from_numpy(case["q"][:33]).cuda()
    p = ix.search_packed(q, 7, idx_offset=1000)
    _same(p[:, :, 1], I[:33, :7] + 1000, "packed: ids")
    _same(p[:, :, 0].to(torch.int32).cpu().numpy().view(np.float32), D[:33, :7], "packed: D")
    # bf16 queries are widened first: the reference of the widened values
    qb = q.bfloat16()
    Db, Ib = sq.search(qb.float().cpu().numpy(), codes, vmin, vdiff, 5)
    d, i = ix.search(qb, 5)
    _same(i, Ib, "bf16 queries: I"), _same(d, Db, "bf16 queries: D")
    tail = torch.cuda.Stream()
    d, i = ix.search(q, 5, tail_stream=tail)
    tail.synchronize()
    _same(i, I[:33, :5], "split tail: I"), _same(d, D[:33, :5], "split tail: D")
    d, i = ix.search_fused(q[:9], 5)                                               # the ungrouped hook call goes through mips_search
    _same(i, I[:9, :5], "fused: I"), _same(d, D[:9, :5], "fused: D")
    ix.check()


# ------------------------------------------------------------------ every shipped instance, by name
PITCH = {100: 256, 500: 512, 768: 768, 1000: 1024}
TILES = {1: (1, "true"), 17: (2, "true"), 33: (4, "true"), 130: (4, "false")}      # nq -> (ncb, non-temporal documents)
POOLS = {5: 1, 13: 2, 29: 4}                                                       # k -> PUB


def _instance(ldb, ncb, nt, pub):
    stages = 3 if (ldb == 1024 or ncb == 4) else 4
    pipe = "false" if (ldb == 1024 and ncb == 4) else "true"
    return f"mips::sq8_scan_kernel<6, {ldb}, {ncb}, {stages}, {nt}, {pub}, {pipe}, {8 if ncb == 1 else 4}>"


@pytest.mark.parametrize("d", sorted(PITCH))
def test_every_shipped_instance_runs_and_is_exact(d):
    case = sq.case_gauss(1500, d, 130, seed=9)
    vmin, vdiff, codes = sq.prepared(case)
    D, I = sq.search(case["q"], codes, vmin, vdiff, 29)
    ix = _index(case)
    seen = set()
    for nq, (ncb, nt) in TILES.items():
        for k, pub in POOLS.items():
            d_, i_ = ix.search(torch.from_numpy(case["q"][:nq]).cuda(), k)
            assert ix.last_kernel == _instance(PITCH[d], ncb, nt, pub), (ix.last_kernel, nq, k)
            seen.add(ix.last_kernel)
            _same(i_, I[:nq, :k], f"{ix.last_kernel}: I"), _same(d_, D[:nq, :k], f"{ix.last_kernel}: D")
            _certified(ix)
    assert len(seen) == 12                                                         # 4 pitches x 12 = the 48 shipped instances


# ------------------------------------------------------------------ rows by id, removal, persistence
def test_subset_scores_reproduce_D():
    case, vmin, vdiff, codes, D, I = _ref("duplicates", 4099, 1000)
    ix = _index(case)
    for nq, k in ((130, 29), (17, 5)):
        d, i = ix.search(case["q"][:nq], k)
        _same(ix.compute_distance_subset(case["q"][:nq], i), d, "subset scores of I, host")
        dd, ii = ix.search(torch.from_numpy(case["q"][:nq]).cuda(), k)
        _same(ix.compute_distance_subset(torch.from_numpy(case["q"][:nq]).cuda(), ii), d, "subset scores of I, device")
    ids = np.array([[0, 4098, -1, 77], [5, 5, 4100 - 2, -7]], dtype=np.int64)
    _same(ix.compute_distance_subset(case["q"][:2], ids), sq.subset_scores(case["q"][:2], codes, vmin, vdiff, ids), "any pairs")
    case1, vmin1, vdiff1, codes1, D1, I1 = _ref("gauss", 31, 100)                  # k > ntotal: the -1 slots score -inf
    i1 = _index(case1)
    d, i = i1.search(case1["q"][:17], 29)
    _same(i1.compute_distance_subset(case1["q"][:17], i), d, "subset scores with padding")


def test_remove_ids_then_search():
    case, vmin, vdiff, codes, _, _ = _ref("gauss", 4099, 256)
    ix = _index(case)
    gone = np.unique(np.concatenate([np.arange(0, 4099, 3), np.arange(1024, 1536), [4098]]))
    assert ix.remove_ids(gone) == len(gone)
    keep = np.setdiff1d(np.arange(4099), gone)
    _same(ix.rows_raw(), codes[keep], "surviving codes")
    _same(ix.sq8_params()[0], vmin, "the parameters stay")
    D, I = sq.search(case["q"], codes[keep], vmin, vdiff, 13)
    _check_search(ix, case, D, I, 130, 13, "after remove_ids")
    _check_search(ix, case, D, I, 17, 5, "after remove_ids")
    ix.add(case["rows"][:5])                                                       # an add appends behind the survivors
    _same(ix.rows_raw()[-5:], codes[:5], "rows added after the removal")


def test_save_load_and_row_range(tmp_path):
    case, vmin, vdiff, codes, D, I = _ref("gauss", 4099, 100)
    ix = _index(case)
    ix.save(str(tmp_path / "ix"))
    assert os.path.exists(tmp_path / "ix" / "rows.sq8")
    back = ram.MipsIndex.load(str(tmp_path / "ix"), device=0)
    assert back.dtype == "sq8" and back.is_trained and back.ntotal == 4099
    _same(back.sq8_params()[0], vmin, "vmin"), _same(back.sq8_params()[1], vdiff, "vdiff"), _same(back.rows_raw(), codes, "codes")
    _check_search(back, case, D, I, 130, 5, "loaded index")
    part = ram.MipsIndex.load(str(tmp_path / "ix"), device=0, row_range=(1000, 3000))
    _same(part.sq8_params()[1], vdiff, "the row range keeps the file's parameters"), _same(part.rows_raw(), codes[1000:3000], "row range")
    Dp, Ip = sq.search(case["q"], codes[1000:3000], vmin, vdiff, 5)
    _check_search(part, case, Dp, Ip, 33, 5, "row range")
    empty = ram.MipsIndex(100, dtype="sq8", device=0)
    empty.train(case["train"])
    empty.save(str(tmp_path / "empty"))
    e2 = ram.MipsIndex.load(str(tmp_path / "empty"), device=0)
    assert e2.is_trained and e2.ntotal == 0
    d, i = e2.search(case["q"][:3], 5)
    assert (i == -1).all() and np.isneginf(d).all()


# ------------------------------------------------------------------ what is not served
def test_refusals():
    case, vmin, vdiff, codes, D, I = _ref("gauss", 33, 100)
    ix = _index(case)
    q = case["q"][:3]
    lib, h, st = ix._lib, ix._h, 0
    qp, out_s, out_i = q.ctypes.data, np.empty((3, 40), np.float32), np.empty((3, 40), np.int64)
    UNSUPPORTED, INVALID = -3, -1
    assert lib.mips_search_wide(h, qp, ram._lib.DTYPE_F32, 3, 40, out_s.ctypes.data, out_i.ctypes.data, 0, 0, None) == UNSUPPORTED
    assert b"SQ8" in lib.mips_last_error()
    lims, radii = np.empty(4, np.int64), np.zeros(3, np.float32)
    assert lib.mips_range_search(h, qp, ram._lib.DTYPE_F32, 3, radii.ctypes.data, lims.ctypes.data, out_s.ctypes.data, out_i.ctypes.data, 100, 0, 0,
                                 None) == UNSUPPORTED
    bits = np.full(8, 255, np.uint8)
    assert lib.mips_search_wide_sel(h, qp, ram._lib.DTYPE_F32, 3, 5, out_s.ctypes.data, out_i.ctypes.data, 0, 0, bits.ctypes.data, 64, 0, None) == UNSUPPORTED
    ix.set_labels(np.zeros(33, np.int32))
    qd, lab = torch.from_numpy(q).cuda(), torch.zeros(3, dtype=torch.int32, device="cuda")
    od, oi = torch.empty((3, 5), device="cuda"), torch.empty((3, 5), dtype=torch.int64, device="cuda")
    assert lib.mips_search_fused_grp(h, qd.data_ptr(), ram._lib.DTYPE_F32, 3, 5, 0, None, od.data_ptr(), oi.data_ptr(), 0, lab.data_ptr(), 0,
                                     ram._lib.GRP_DEVICE, None) == UNSUPPORTED
    assert lib.mips_search_wide_grp(h, qp, ram._lib.DTYPE_F32, 3, 5, out_s.ctypes.data, out_i.ctypes.data, 0, 0, None, 0, 0,
                                    np.zeros(3, np.int32).ctypes.data, 0, None) == UNSUPPORTED
    assert lib.mips_index_add_synthetic(h, 10, 0, 1, 1, None) == UNSUPPORTED
    assert lib.mips_search(h, codes.ctypes.data, ram._lib.DTYPE_SQ8, 3, 5, out_s.ctypes.data, out_i.ctypes.data, 0, 0, None) == INVALID
    assert lib.mips_index_add(h, codes.ctypes.data, 3, ram._lib.DTYPE_FP8_E4M3, 0, None) == INVALID
    import ctypes
    h2 = ctypes.c_void_p()
    assert lib.mips_index_create(ctypes.byref(h2), 0, 100, ram._lib.DTYPE_SQ8, ram._lib.METRIC_L2) == UNSUPPORTED
    assert b"inner product" in lib.mips_last_error() and not h2.value
    assert lib.mips_index_create(ctypes.byref(h2), 0, 1025, ram._lib.DTYPE_SQ8, ram._lib.METRIC_IP) == UNSUPPORTED
    bf = ram.MipsIndex(100, device=0)
    assert lib.mips_index_sq8_train(bf._h, qp, 3, ram._lib.DTYPE_F32, 0, None) == INVALID and lib.mips_index_sq8_is_trained(bf._h) == -1
    assert bf.is_trained and bf.train(q) is None                                   # other storages have nothing to train
    # the Python layer says the same before it calls
    with pytest.raises(NotImplementedError, match="sq8"):
        ix.search_wide(q, 40)
    with pytest.raises(NotImplementedError, match="sq8"):
        ix.range_search(q, 0.0)
    with pytest.raises(NotImplementedError, match="sq8"):
        ix.search_fused(qd, 5, groups=lab)
    with pytest.raises(NotImplementedError, match="inner product"):
        ram.MipsIndex(100, metric=ram._lib.METRIC_L2, dtype="sq8", device=0)
    with pytest.raises(NotImplementedError, match="sq8"):
        ram.ShardedMipsIndex(100, dtype="sq8")
    _check_search(ix, case, D, I, 3, 5, "after the refusals")                      # the index is as it was


# ------------------------------------------------------------------ the layers above
def test_faiss_shim_route(tmp_path):
    case, vmin, vdiff, codes, D, I = _ref("gauss", 4099, 100)
    direct = _index(case)
    fx = faiss_shim.index_factory(100, "SQ8", faiss_shim.METRIC_INNER_PRODUCT)
    assert not fx.is_trained
    with pytest.raises(RuntimeError):
        fx.add(case["rows"])
    fx.train(case["train"])
    assert fx.is_trained
    fx.add(case["rows"])
    for nq, k in ((130, 5), (17, 29)):
        d0, i0 = direct.search(case["q"][:nq], k)
        d1, i1 = fx.search(case["q"][:nq], k)
        _same(i1, i0, "shim: I"), _same(d1, d0, "shim: D"), _same(i1, I[:nq, :k], "shim: I against the reference")
    _same(fx.reconstruct(7), sq.decode(codes[7], vmin, vdiff), "shim: reconstruct")
    path = str(tmp_path / "ix.faiss")
    faiss_shim.write_index(fx, path)
    back = faiss_shim.read_index(path)
    assert isinstance(back, faiss_shim.IndexScalarQuantizer) and back.is_trained and back.ntotal == 4099
    d2, i2 = back.search(case["q"][:33], 5)
    _same(i2, I[:33, :5], "read_index: I"), _same(d2, D[:33, :5], "read_index: D")


def test_knowledge_base_and_mips_facade():
    case, vmin, vdiff, codes, D, I = _ref("gauss", 4099, 100)
    kb = ram.KnowledgeBase({"cls": case["rows"], "id": np.arange(4099)})
    kb.add_faiss_index("cls", index_name="sq", string_factory="SQ8", metric_type=ram._lib.METRIC_IP, train_size=1000)
    ix = kb.get_index("sq").faiss_index
    tmin, tdiff = sq.train(case["rows"][:1000])                                    # trained on the first train_size rows
    assert ix.dtype == "sq8"
    _same(ix.sq8_params()[0], tmin, "train_size: vmin"), _same(ix.rows_raw(), sq.encode(case["rows"], tmin, tdiff), "train_size: codes")
    kb.add_faiss_index("cls", index_name="sq_all", string_factory="SQ8", metric_type=ram._lib.METRIC_IP)
    _same(kb.get_index("sq_all").faiss_index.rows_raw(), codes, "train_size=None: all rows")
    with pytest.raises(NotImplementedError, match="inner product"):
        kb.add_faiss_index("cls", index_name="l2", string_factory="SQ8", metric_type=ram._lib.METRIC_L2)
    with pytest.raises(NotImplementedError):
        kb.add_faiss_index("cls", index_name="ivf", string_factory="IVF256,SQ8", metric_type=ram._lib.METRIC_IP)
    m = ram.Mips(ram.MipsArgs(mips_string_factory="SQ8", mips_metric_type=ram._lib.METRIC_IP, mips_normalize=False))
    m.build_index(case["rows"])
    mi = m.embeddings.get_index(m.index_name).faiss_index
    assert mi.dtype == "sq8"
    _same(mi.rows_raw(), codes, "Mips: codes")
    d, i = mi.search(case["q"][:17], 5)
    _same(i, I[:17, :5], "Mips: I"), _same(d, D[:17, :5], "Mips: D")
    with pytest.raises(NotImplementedError, match="inner product"):
        ram.Mips(ram.MipsArgs(mips_string_factory="SQ8", mips_metric_type=ram._lib.METRIC_L2)).build_index(case["rows"])


def test_c_abi_sq8_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_sq8_smoke")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", os.path.join(root, "tests", "c_abi_sq8_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
