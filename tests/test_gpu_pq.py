"""Product-quantised index on the GPU (include/mips_hip_pq.h): everything bit for bit against the NumPy restatement of
tests/pq_cases.py, no tolerance anywhere.  The scan is tested on planted codebooks and codes (set_codebook / add_codes), so it does
not depend on training; training, encoding, the calls by id, save / load and the refusals have their own tests.  The CPU side
(that the cases bite, the header, the kernels' registers) is tests/test_pq_host.py; graph capture is tests/test_gpu_pq_graph.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pq_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.uint32


def planted(case, n=None):
    ix = ram.PqIndex(case["d"], case["M"])
    ix.set_codebook(case["codebook"])
    codes = case["codes"] if n is None else case["codes"][:n]
    if len(codes):
        ix.add_codes(codes)
    return ix


def same(got, want, what=""):
    D, I = got
    assert np.array_equal(I, want[1]), what
    assert np.array_equal(np.asarray(D).view(U), want[0].view(U)), what


@pytest.mark.parametrize("d,M", pc.GEOMETRY)
def test_scan_geometry(d, M):
    """ntotal across the wave, workgroup and uneven-segment boundaries, nq and k across their ranges, k > ntotal (padding)"""
    case = pc.case_planted(d, M, max(pc.NTOTALS), max(pc.NQS))
    table = pc.lut(case["q"], case["codebook"])
    full = pc.scores(table, case["codes"])                       # the score of a row does not depend on the other rows
    ix = ram.PqIndex(d, M)
    ix.set_codebook(case["codebook"])
    assert ix.bytes_per_row == M and ix.M == M and ix.dsub == d // M
    for n in pc.NTOTALS:
        ix.reset()
        assert ix.is_trained and ix.ntotal == 0
        if n:
            ix.add_codes(case["codes"][:n])
        assert len(ix) == n
        for nq in pc.NQS:
            for k in pc.KS:
                same(ix.search(case["q"][:nq], k), pc.top_k(full[:nq, :n], k), (d, M, n, nq, k))
    assert np.array_equal(ix.codes(), case["codes"]) and np.array_equal(ix.codes(63, 3), case["codes"][63:66])


def test_query_slice_boundary():
    case = pc.case_planted(32, 4, 1000, 9)
    ix = planted(case)
    want = pc.search(case["q"], case["codebook"], case["codes"], 5)
    same(ix.search(case["q"], 5), want)
    ix.query_slice = 4                                            # 9 queries: slices of 4, 4 and 1
    same(ix.search(case["q"], 5), want)
    D, I = ix.search(torch.from_numpy(case["q"]).cuda(), 5)
    same((D.cpu().numpy(), I.cpu().numpy()), want)
    assert np.array_equal(ix.compute_distance_subset(case["q"], want[1]).view(U), want[0].view(U))


def test_ties_go_to_the_lowest_row():
    case = pc.case_ties()
    D, I = planted(case).search(case["q"], 29)
    assert (I == np.arange(29)).all()
    same((D, I), pc.search(case["q"], case["codebook"], case["codes"], 29))
    case = pc.case_duplicates()                                   # copies across wave, workgroup and segment boundaries
    ix = planted(case)
    for k in (5, 29):
        for off in (0, 7, 1 << 40):
            same(ix.search(case["q"], k, idx_offset=off), pc.search(case["q"], case["codebook"], case["codes"], k, idx_offset=off), (k, off))
    D, I = ix.search(case["q"], 29, idx_offset=7)
    assert list(I[0, :len(case["planted"])]) == [r + 7 for r in case["planted"]]
    case = pc.case_duplicates(d=768, M=96)                        # the 16-wave workgroup
    same(planted(case).search(case["q"], 29), pc.search(case["q"], case["codebook"], case["codes"], 29))


def test_order_of_the_sum():
    for d, M in ((32, 8), (768, 96)):
        case = pc.case_sum_order(d, M)
        want = pc.search(case["q"], case["codebook"], case["codes"], 29)
        same(planted(case).search(case["q"], 29), want, (d, M))
        for wrong in ("fp64", "pairwise"):                        # (what the case is for: these orders give other bits)
            assert not np.array_equal(pc.search(case["q"], case["codebook"], case["codes"], 29, wrong=wrong)[0].view(U), want[0].view(U))


def test_magnitudes_and_the_zero_query():
    case = pc.case_planted(24, 8, 1000, 3)
    base = pc.search(case["q"], case["codebook"], case["codes"], 5)
    for e in (30, -30):
        scaled = dict(case, codebook=(case["codebook"] * np.float32(2.0 ** e)).astype(np.float32))
        D, I = planted(scaled).search(case["q"], 5)
        assert np.array_equal(I, base[1]) and np.array_equal(D, base[0] * np.float32(2.0 ** e))   # scaled exactly
        same((D, I), pc.search(case["q"], scaled["codebook"], case["codes"], 5))
    D, I = planted(case).search(np.zeros((2, 24), np.float32), 5)
    assert (D.view(U) == 0).all() and (I == np.arange(5)).all()  # every score +0: rows 0 .. k - 1


@pytest.mark.parametrize("name,niter", [("gauss", 4), ("distinct", 3), ("cancel", 1), ("subsample", 1), ("gauss", 0)])
def test_training_matches_the_restatement(name, niter):
    case = {"gauss": pc.case_train_gauss, "distinct": pc.case_train_distinct, "cancel": pc.case_train_cancel, "subsample": pc.case_train_subsample}[name]()
    ix = ram.PqIndex(case["d"], case["M"])
    assert not ix.is_trained and ix.niter == 10
    ix.niter = niter
    ix.train(case["x"])
    assert ix.is_trained
    want = pc.train(case["x"], case["M"], niter)
    assert np.array_equal(ix.codebook().view(U), want.view(U))
    if name == "cancel":
        assert want[0, 0, 0] == 0.0                               # 0, 2^70, 1, -2^70 in ascending row order: the 1 is absorbed
    if name == "gauss" and niter:
        dev = ram.PqIndex(case["d"], case["M"])                   # device rows, and bf16 rows: the same rule on the widened values
        dev.niter = niter
        dev.train(torch.from_numpy(case["x"]).cuda())
        assert np.array_equal(dev.codebook().view(U), want.view(U))
        xb = torch.from_numpy(case["x"]).to(torch.bfloat16)
        dev.train(xb)                                             # training again while empty is allowed
        assert np.array_equal(dev.codebook().view(U), pc.train(xb.float().numpy(), case["M"], niter).view(U))


def test_training_refusals():
    case = pc.case_train_gauss()
    ix = ram.PqIndex(case["d"], case["M"])
    with pytest.raises(RuntimeError):
        ix.train(case["x"][:255])
    x = case["x"].copy()
    x[300, 7] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        ix.train(x)
    with pytest.raises(RuntimeError, match="NaN"):
        ix.train(torch.from_numpy(x).cuda())
    with pytest.raises(RuntimeError):
        ix.add(case["x"][:3])                                     # not trained
    with pytest.raises(RuntimeError):
        ix.codebook()
    ix.niter = 1
    ix.train(case["x"])
    ix.add(case["x"][:10])
    with pytest.raises(RuntimeError, match="holds"):
        ix.train(case["x"])
    with pytest.raises(RuntimeError, match="holds"):
        ix.set_codebook(ix.codebook())
    bad = ix.codebook()
    bad[1, 2, 3] = np.inf
    ix.reset()
    with pytest.raises(RuntimeError):
        ix.set_codebook(bad)
    ix.train(case["x"])                                           # empty again: allowed


def test_encode():
    case = pc.case_encode()
    want = pc.encode(case["x"], case["codebook"])
    assert want[3, 1] == 0 and want[5, 3] == 0 and (want[7] == 0).all() and (want[9] == 0).all()
    ix = ram.PqIndex(case["d"], case["M"])
    ix.set_codebook(case["codebook"])
    ix.add(case["x"])
    assert np.array_equal(ix.codes(), want)
    two = ram.PqIndex(case["d"], case["M"])                       # two adds equal one add (growth in between), device rows too
    two.set_codebook(case["codebook"])
    two.add(case["x"][:123])
    two.add(torch.from_numpy(case["x"][123:]).cuda())
    assert two.ntotal == len(want) and np.array_equal(two.codes(), want)
    xb = torch.from_numpy(case["x"]).to(torch.bfloat16)           # bf16 input equals its widened float32
    wide = pc.encode(xb.float().numpy(), case["codebook"])
    for rows in (xb, xb.cuda(), xb.view(torch.int16).numpy().view(np.uint16)):
        b = ram.PqIndex(case["d"], case["M"])
        b.set_codebook(case["codebook"])
        b.add(rows)
        assert np.array_equal(b.codes(), wide)
    big = pc.case_planted(768, 96, 0, 1)                          # the large shape: 300 rows x 96 sub-quantisers
    x = np.random.default_rng(3).standard_normal((300, 768)).astype(np.float32)
    ix = planted(big)
    ix.add(x)
    assert np.array_equal(ix.codes(), pc.encode(x, big["codebook"]))


def test_by_id():
    case = pc.case_planted(24, 8, 1000, 3)
    ix = planted(case)
    D, I = ix.search(case["q"], 5, idx_offset=100)
    rows = pc.reconstruct(case["codes"], case["codebook"])
    got = ix.reconstruct_batch(I, idx_offset=100)
    assert got.shape == (3, 5, 24) and np.array_equal(got.view(U), rows[I - 100].view(U))
    assert np.array_equal(ix.reconstruct(17).view(U), rows[17].view(U)) and np.array_equal(ix.reconstruct_n(998).view(U), rows[998:].view(U))
    assert np.array_equal(ix.compute_distance_subset(case["q"], I, idx_offset=100).view(U), D.view(U))   # scoring I reproduces D
    ids = torch.tensor([[3, -1, 1000], [999, 1 << 33, 0], [5, 5, -7]], device="cuda")
    got = ix.reconstruct_batch(ids).cpu().numpy()
    sc = ix.compute_distance_subset(torch.from_numpy(case["q"]).cuda(), ids).cpu().numpy()
    full = pc.scores(pc.lut(case["q"], case["codebook"]), case["codes"])
    for j in range(3):
        for t in range(3):
            r = int(ids[j, t])
            if 0 <= r < 1000:
                assert np.array_equal(got[j, t].view(U), rows[r].view(U)) and sc[j, t].view(U) == full[j, r].view(U)
            else:
                assert (got[j, t].view(U) == 0x7FC00000).all() and sc[j, t] == -np.inf                # "no row"
    with pytest.raises(RuntimeError):
        ix.reconstruct_batch(np.array([1000]))                    # a host id past the index
    assert np.isnan(ix.reconstruct_batch(np.array([-1]))).all()
    with pytest.raises(IndexError):
        ix.reconstruct(1000)


def test_host_and_device_forms_give_the_same_bits():
    case = pc.case_planted(768, 96, 4097, 17)
    ix = planted(case)
    D, I = ix.search(case["q"], 5)
    same((D, I), pc.search(case["q"], case["codebook"], case["codes"], 5))
    Dd, Id = ix.search(torch.from_numpy(case["q"]).cuda(), 5)     # a CUDA tensor in gives CUDA tensors out
    assert isinstance(Dd, torch.Tensor) and Dd.is_cuda and Id.is_cuda and Id.dtype == torch.int64
    same((Dd.cpu().numpy(), Id.cpu().numpy()), (D, I))
    Dh, Ih = ix.search(torch.from_numpy(case["q"]), 5)            # a host tensor is host memory: NumPy out
    assert isinstance(Dh, np.ndarray)
    same((Dh, Ih), (D, I))
    qb = torch.from_numpy(case["q"]).to(torch.bfloat16)           # bf16 queries: their widened values
    Db, Ib = ix.search(qb.cuda(), 5)
    same((Db.cpu().numpy(), Ib.cpu().numpy()), pc.search(qb.float().numpy(), case["codebook"], case["codes"], 5))
    dev = ram.PqIndex(768, 96)                                     # device codes
    dev.set_codebook(case["codebook"])
    dev.add_codes(torch.from_numpy(case["codes"]).cuda())
    same(dev.search(case["q"], 5), (D, I))


def test_save_load_and_reset(tmp_path):
    case = pc.case_train_gauss()
    ix = ram.PqIndex(case["d"], case["M"])
    ix.niter = 2
    ix.train(case["x"])
    ix.add(case["x"])
    q = case["x"][:4] * np.float32(0.5)
    D, I = ix.search(q, 5)
    same((D, I), pc.search(q, ix.codebook(), ix.codes(), 5))
    path = str(tmp_path / "pq")
    ix.save(path)
    assert sorted(os.listdir(path)) == ["codebook.f32", "codes.u8", "meta.json"] and os.path.getsize(os.path.join(path, "codes.u8")) == 700 * 4
    back = ram.PqIndex.load(path)
    assert back.ntotal == 700 and back.is_trained and back.niter == 2 and (back.d, back.M) == (ix.d, ix.M)
    assert np.array_equal(back.codebook().view(U), ix.codebook().view(U)) and np.array_equal(back.codes(), ix.codes())
    same(back.search(q, 5), (D, I))
    cb = ix.codebook()
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and np.array_equal(ix.codebook().view(U), cb.view(U))       # rows go, the codebook stays
    D0, I0 = ix.search(q, 3)
    assert (I0 == -1).all() and np.isneginf(D0).all()
    ix.add(case["x"][:50])
    same(ix.search(q, 5), pc.search(q, cb, back.codes()[:50], 5))
    empty = ram.PqIndex(case["d"], case["M"])
    with pytest.raises(RuntimeError):
        empty.save(str(tmp_path / "untrained"))


def test_refusals():
    with pytest.raises(NotImplementedError):
        ram.PqIndex(64, 8, metric=ram.METRIC_L2)
    with pytest.raises(NotImplementedError):
        ram.PqIndex(64, 8, nbits=4)
    with pytest.raises(NotImplementedError):
        ram.PqIndex(516, 129)
    with pytest.raises(NotImplementedError):
        ram.PqIndex(2048, 8)
    with pytest.raises(ValueError):
        ram.PqIndex(30, 8)
    lib = ram._lib.load()
    import ctypes
    h = ctypes.c_void_p()
    assert lib.mips_pq_create(ctypes.byref(h), 0, 64, 8, 8, ram.METRIC_L2) == -3 and b"inner product" in lib.mips_last_error()   # MIPS_E_UNSUPPORTED
    assert lib.mips_pq_create(ctypes.byref(h), 0, 64, 8, 6, ram.METRIC_IP) == -3 and lib.mips_pq_create(ctypes.byref(h), 0, 516, 129, 8, 0) == -3
    case = pc.case_planted(32, 4, 100, 2)
    ix = planted(case)
    with pytest.raises(NotImplementedError):
        ix.search(case["q"], 30)
    with pytest.raises(RuntimeError):
        ix.search(case["q"], 0)
    with pytest.raises(ValueError):
        ix.search(case["q"][:, :31], 5)
    with pytest.raises(NotImplementedError):
        ix.add(np.zeros((3, 32), np.uint8))                       # integers are not rows: codes go through add_codes
    with pytest.raises(ValueError):
        ix.add_codes(case["codes"][:, :3])
    for name in ("search_wide", "range_search", "remove_ids", "update_rows"):
        with pytest.raises(NotImplementedError):
            getattr(ix, name)(case["q"], 5)
    fresh = ram.PqIndex(32, 4)
    with pytest.raises(RuntimeError):
        fresh.search(case["q"], 5)                                # not trained
    with pytest.raises(RuntimeError):
        fresh.add_codes(case["codes"])
    D, I = ix.search(np.zeros((0, 32), np.float32), 5)
    assert D.shape == (0, 5) and I.shape == (0, 5)


def test_c_abi_pq_from_plain_c(tmp_path):
    lib_dir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_pq_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_pq_smoke.c"), "-I", os.path.join(ROOT, "include"), "-L", lib_dir,
                           "-lmips_hip", f"-Wl,-rpath,{lib_dir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches: 0" in out.stdout, out.stdout + out.stderr
