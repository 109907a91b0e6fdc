"""IVF search on the GPU (mips_ivf_search, IvfIndex.search_probed): everything bit for bit against the NumPy restatement of
tests/ivf_search_cases.py, no tolerance anywhere -- planted lists of 0, 1, 63, 64, 65, 100, 200 and 2500 rows (an empty probed list,
fewer admitted rows than k, lists shorter than the number of segments, segment boundaries, the first and the last row of a list and
of the index), Gaussian rows at d = 1, 64, 768, 1024 with host, device and bf16 queries and nprobe beyond nlist, ties spread over
lists and segments, the three identities that need no restatement, the index as it changes, save / load, a probe of 40 lists
through the wide search, the refusals and the C ABI.

Segments: with 256 compute units a call of nq queries and p probed lists uses S = the smallest power of two with nq p S >= 512, at
most 32.  The planted case (24 queries) runs at S = 32, 16, 8 and 4 for nprobe = 1, 2, 3 and 8; the merge's limit p S k <= 65536
cannot bind below 2 p S < 1024 workgroups' worth of lists, so it is exercised by tests/ivf_search_math_check.cpp, not here."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_cases as iv  # noqa: E402
import ivf_search_cases as sc  # noqa: E402

STORAGES = sc.STORAGES


def _ram():
    import retrieval_augmented_mds_amd as ram

    return ram


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _same(got, want):
    gd, gi = _np(got[0]), _np(got[1])
    assert np.array_equal(gi, want[1]), (gi, want[1])
    assert np.array_equal(gd.view(np.uint32), want[0].view(np.uint32))


_built = {}


def _build(case, dtype, niter=2):
    """-> (index, centroids, assignments by the restatement, sq8 parameters or None)"""
    ram = _ram()
    rows = case["rows"]
    ix = ram.IvfIndex(rows.shape[1], case["nlist"], dtype=dtype)
    ix.niter = niter
    if "centroids" in case:
        ix.set_centroids(case["centroids"])
        if dtype == "sq8":
            vmin = rows.min(axis=0)
            ix.set_sq8_params(vmin, rows.max(axis=0) - vmin)
    else:
        ix.train(rows)
    ix.add(rows)
    c = ix.centroids()
    return ix, c, iv.nearest(rows, c)[:, 0], (ix.flat.sq8_params() if dtype == "sq8" else None)


def built(name, make, dtype):
    if (name, dtype) not in _built:
        case = make()
        _built[(name, dtype)] = (case,) + _build(case, dtype)
    return _built[(name, dtype)]


# ------------------------------------------------------------------ planted lists
@pytest.mark.parametrize("dtype", STORAGES)
@pytest.mark.parametrize("d", [40, 100])
def test_planted_lists(d, dtype):
    case, ix, c, assign, par = built(f"planted{d}", lambda: iv.case_planted(d), dtype)
    assert np.array_equal(assign, case["labels"]) and tuple(ix.list_sizes()) == iv.PLANTED_SIZES
    q = case["q"]
    for nprobe in (1, 2, 3, 8):
        for k in (1, 2, 5, 29):
            want = sc.search(case["rows"], q, assign, c, k, nprobe, dtype, par)
            _same(ix.search_probed(q, k, nprobe), want)
        _same(ix.search_probed(_dev(q), 29, nprobe), want)                               # device in, device out
    d1, i1 = ix.search_probed(q, 29, 1)
    assert (i1[case["qlabels"] == 0] == -1).all() and np.isneginf(d1[case["qlabels"] == 0]).all()     # the empty list: padding only
    assert ((i1[case["qlabels"] == 2] >= 0).sum(axis=1) == 1).all()                                   # a list of one row
    n = len(case["rows"])
    big = np.flatnonzero(assign == 1)
    _, i5 = ix.search_probed(q, 5, 1)                                                    # (a planted row 2 q_j scores ~8, its list's other rows ~6)
    assert {0, n - 1, int(big[0]), int(big[-1])} <= set(i5.ravel().tolist())             # first / last row of the index and of the large list
    ix.nprobe = 3                                                                        # the attribute is the default
    _same(ix.search_probed(q, 5), sc.search(case["rows"], q, assign, c, 5, 3, dtype, par))
    ix.nprobe = 1
    _same(ix.search_probed(q, 5, 2, idx_offset=1 << 40), sc.search(case["rows"], q, assign, c, 5, 2, dtype, par, idx_offset=1 << 40))


# ------------------------------------------------------------------ Gaussian rows, every query form
@pytest.mark.parametrize("dtype", STORAGES)
@pytest.mark.parametrize("d", [1, 64, 768, 1024])
def test_gauss(d, dtype):
    import torch

    case, ix, c, assign, par = built(f"gauss{d}", lambda: iv.case_gauss(3000, d, 9, 16), dtype)
    q = case["q"]
    qb = iv.synth.round_to_bf16(q)
    for nprobe in (1, 4, 16, 100):
        want = sc.search(case["rows"], q, assign, c, 5, nprobe, dtype, par)
        _same(ix.search_probed(q, 5, nprobe), want)                                      # NumPy float32
        got = ix.search_probed(_dev(q), 5, nprobe)                                       # CUDA float32
        assert got[0].is_cuda and got[1].is_cuda and got[1].dtype == torch.int64
        _same(got, want)
        _same(ix.search_probed(_dev(q).to(torch.bfloat16), 5, nprobe), sc.search(case["rows"], qb, assign, c, 5, nprobe, dtype, par))   # CUDA bf16


# ------------------------------------------------------------------ ties across lists and segments
@pytest.mark.parametrize("dtype", STORAGES)
def test_ties_across_lists_and_segments(dtype):
    ram = _ram()
    from retrieval_augmented_mds_amd.index import _stream_handle

    case = sc.case_ties()
    rows = case["rows"]
    ix = ram.IvfIndex(rows.shape[1], 4, dtype=dtype)
    ix.set_centroids(case["centroids"])
    par = None
    if dtype == "sq8":
        par = sc.sq.train(rows)
        ix.set_sq8_params(*par)
    ix.add(rows)
    a = np.ascontiguousarray(case["assign"], dtype=np.int32)
    ram._lib.check(ix._lib.mips_ivf_set_assign(ix._h, a.ctypes.data, len(a), _stream_handle(ix.device)), "mips_ivf_set_assign")
    assert np.array_equal(ix.assignments(), a) and np.array_equal(ix.probe(case["q"], 3)[0], [0, 1, 2])
    d, i = ix.search_probed(case["q"], 29, 3)
    assert np.array_equal(i[0], case["copies"][:29]) and (d[0] == d[0, 0]).all()         # the lowest 29 copies, ascending
    _same((d, i), sc.search(rows, case["q"], a, case["centroids"], 29, 3, dtype, par))
    d, i = ix.search_probed(case["q"], 29, 1)                                            # one list: its 14 copies, then the rest of it
    _same((d, i), sc.search(rows, case["q"], a, case["centroids"], 29, 1, dtype, par))
    assert np.array_equal(i[0, :14], case["copies"][0::3])


# ------------------------------------------------------------------ identities that need no restatement
@pytest.mark.parametrize("dtype", STORAGES)
def test_identities(dtype):
    case, ix, c, assign, par = built("gauss64", lambda: iv.case_gauss(3000, 64, 9, 16), dtype)
    q = case["q"]
    for nprobe in (1, 4):
        d, i = ix.search_probed(q, 5, nprobe)
        again = ix.flat.compute_distance_subset(q, i)                                    # scoring I reproduces D
        assert np.array_equal(again.view(np.uint32), d.view(np.uint32))
    for nprobe in (16, 17):
        _same(ix.search_probed(q, 5, nprobe), ix.flat.search(q, 5))                      # every list probed: the flat result
    _same(ix.search_probed(_dev(q), 29, 16), ix.flat.search(q, 29))
    if dtype == "sq8":
        return                                                                           # (no wide search on SQ8 rows)
    ram = _ram()
    iy = ram.IvfIndex(64, 16, dtype=dtype)                                               # an index of its own: it gets labels
    iy.set_centroids(c)
    iy.add(case["rows"])
    iy.flat.set_labels(iy.assignments())
    P = iy.probe(q, 1)
    wd, wi = iy.flat.search_wide(q, 30, groups=P[:, 0], group_mode="only")
    d, i = iy.search_probed(q, 29, 1)
    assert np.array_equal(wi[:, :29], i) and np.array_equal(wd[:, :29].view(np.uint32), d.view(np.uint32))


# ------------------------------------------------------------------ the index as it changes
@pytest.mark.parametrize("dtype", STORAGES)
def test_after_mutation(dtype):
    ram = _ram()
    case = iv.case_gauss(3000, 100, 9, 8, seed=9)
    x, q = case["rows"], case["q"]
    ix = ram.IvfIndex(100, 8, dtype=dtype)
    ix.niter = 2
    ix.train(x)
    c = ix.centroids()
    par = ix.flat.sq8_params() if dtype == "sq8" else None
    assign = iv.nearest(x, c)[:, 0]
    _same(ix.search_probed(q, 5, 3), (np.full((9, 5), -np.inf, np.float32), np.full((9, 5), -1, np.int64)))   # empty: padding
    ix.add(x[:700])
    _same(ix.search_probed(q, 5, 3), sc.search(x[:700], q, assign[:700], c, 5, 3, dtype, par))
    ix.add(_dev(x[700:]))                                                                # storage and list table grow
    _same(ix.search_probed(q, 5, 3), sc.search(x, q, assign, c, 5, 3, dtype, par))
    keep = np.arange(3000) % 3 != 0
    assert ix.remove_ids(~keep) == 1000
    _same(ix.search_probed(_dev(q), 5, 3), sc.search(x[keep], q, assign[keep], c, 5, 3, dtype, par))
    ix.reset()
    ix.add(x[1000:1500])
    _same(ix.search_probed(q, 29, 2), sc.search(x[1000:1500], q, assign[1000:1500], c, 29, 2, dtype, par))


@pytest.mark.parametrize("dtype", STORAGES)
def test_save_load(tmp_path, dtype):
    ram = _ram()
    case, ix, c, assign, par = built("gauss64", lambda: iv.case_gauss(3000, 64, 9, 16), dtype)
    ix.save(str(tmp_path / "ivf"))
    iy = ram.IvfIndex.load(str(tmp_path / "ivf"))
    for nprobe, k in ((1, 5), (4, 29)):
        _same(iy.search_probed(case["q"], k, nprobe), ix.search_probed(case["q"], k, nprobe))
    _same(iy.search_probed(case["q"], 5, 4), sc.search(case["rows"], case["q"], assign, c, 5, 4, dtype, par))


@pytest.mark.parametrize("dtype", STORAGES)
def test_wide_probe(dtype):
    """40 of 64 lists: the probe goes through mips_search_wide; 9 x 40 probed lists in 2 segments each, 80 partial lists per query"""
    case, ix, c, assign, par = built("wide", lambda: iv.case_gauss(3000, 64, 9, 64, seed=4), dtype)
    assert np.array_equal(ix.probe(case["q"], 40), iv.nearest(case["q"], c, 40))
    _same(ix.search_probed(case["q"], 29, 40), sc.search(case["rows"], case["q"], assign, c, 29, 40, dtype, par))
    _same(ix.search_probed(_dev(case["q"][:1]), 29, 40), sc.search(case["rows"], case["q"][:1], assign, c, 29, 40, dtype, par))   # one query: S = 16


def test_refusals():
    import ctypes

    ram = _ram()
    x = iv.case_gauss(300, 64, 3, 4)
    ix = ram.IvfIndex(64, 4, dtype="sq8")
    with pytest.raises(RuntimeError, match="not trained"):
        ix.search_probed(x["q"], 5, 1)                                                   # untrained
    ix.train(x["rows"])
    ix.add(x["rows"])
    for k in (0, 30):
        with pytest.raises(RuntimeError, match="k must be"):
            ix.search_probed(x["q"], k, 1)
    with pytest.raises(RuntimeError, match="nprobe"):
        ix.search_probed(x["q"], 5, 0)
    lib = ix._lib
    q = np.ascontiguousarray(x["q"])
    out_s = np.empty((3, 5), np.float32)
    args = (ix._h, q.ctypes.data, ram.DTYPE_F32, 3, 5, 2)
    assert lib.mips_ivf_search(*args, out_s.ctypes.data, None, 0, 0, None) == -1         # MIPS_E_INVALID: NULL output with nq > 0
    assert b"NULL" in lib.mips_last_error()
    assert lib.mips_ivf_search(ix._h, None, ram.DTYPE_F32, 0, 5, 2, None, None, 0, 0, None) == 0      # nq = 0
    assert lib.mips_ivf_search(ix._h, q.ctypes.data, ram.DTYPE_SQ8, 3, 5, 2, out_s.ctypes.data, out_s.ctypes.data, 0, 0, None) == -1
    big = ram.IvfIndex(64, 2000, dtype="f32")
    big.set_centroids(np.random.default_rng(0).standard_normal((2000, 64)).astype(np.float32))
    h = ctypes.c_void_p(big._h.value)
    oi = np.empty((3, 5), np.int64)
    assert lib.mips_ivf_search(h, q.ctypes.data, ram.DTYPE_F32, 3, 5, 1025, out_s.ctypes.data, oi.ctypes.data, 0, 0, None) == -3   # p > 1024
    assert lib.mips_ivf_search(h, q.ctypes.data, ram.DTYPE_F32, 3, 5, 1024, out_s.ctypes.data, oi.ctypes.data, 0, 0, None) == 0
    assert (oi == -1).all()                                                              # (an empty index)
    for name in ("search", "search_packed", "search_wide", "range_search", "search_fused"):
        with pytest.raises(NotImplementedError, match="search_probed"):
            getattr(ix, name)(x["q"], 5)                                                 # the faiss-shaped forms still raise


def test_c_abi_ivf_search_from_plain_c(tmp_path):
    ram = _ram()
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_ivf_search_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_ivf_search_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
