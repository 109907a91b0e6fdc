"""IVF index on the GPU: everything bit for bit against the NumPy restatement of tests/ivf_cases.py, no tolerance anywhere --
training (centroids after 0, 1 and 10 iterations, host and device rows, above and below 256 nlist rows, an empty cluster, a
mean whose sum depends on its order), assignments, list table and probe on every case and storage (host and device inputs, up to
29 probes and beyond), the inner flat index against a MipsIndex over the same rows, two adds, remove, reset, save / load, the
refusals, the C ABI and the create / destroy memory drift."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_cases as iv  # noqa: E402

STORAGES = ("bf16", "f32", "sq8")


def _ram():
    import retrieval_augmented_mds_amd as ram

    return ram


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ training
def _planted_dups(n, d, nlist):
    """the duplicates case: the evenly spaced initial rows are copies of one vector, so the first iteration sends every row to
    list 0 and the other lists are empty in it (they keep their centroid)"""
    base = iv.case_gauss(n // nlist, d, 4, nlist, seed=7)["rows"]
    return np.ascontiguousarray(np.tile(base, (nlist, 1)))


TRAIN = {  # name: (rows, nlist, what)
    "below": (lambda: iv.case_gauss(4099, 100, 4, 40)["rows"], 40),            # n < 256 nlist: every row trains
    "above": (lambda: iv.case_gauss(4099, 100, 4, 4)["rows"], 4),              # n > 256 nlist: 1024 evenly spaced rows
    "wide_d": (lambda: iv.case_gauss(1500, 768, 4, 16)["rows"], 16),
    "empty": (lambda: _planted_dups(900, 64, 3), 3),
    "cancel": (lambda: iv.case_cancel(300, 40)["rows"], 1),                     # the order of the mean's sum shows
}


@pytest.mark.parametrize("name,niter,where", [("below", 0, "host"), ("below", 1, "host"), ("below", 10, "host"), ("below", 10, "device"),
                                              ("above", 0, "device"), ("above", 1, "host"), ("above", 10, "device"), ("above", 10, "bf16"),
                                              ("wide_d", 10, "host"), ("empty", 10, "host"), ("empty", 1, "device"), ("cancel", 1, "host"),
                                              ("cancel", 1, "device")])
def test_training_matches_the_restatement(name, niter, where):
    import torch

    ram = _ram()
    make, nlist = TRAIN[name]
    x = make()
    if where == "bf16":
        x = iv.synth.round_to_bf16(x)
    want = iv.train(x, nlist, niter)
    ix = ram.IvfIndex(x.shape[1], nlist, dtype="f32")
    ix.niter = niter
    assert not ix.is_trained
    ix.train(x if where == "host" else _dev(x) if where == "device" else _dev(x).to(torch.bfloat16))
    assert ix.is_trained
    got = ix.centroids()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if name == "empty":                                                         # the first iteration sends every row to list 0:
        a = iv.nearest(iv.training_set(x, nlist), iv.train(x, nlist, 0))[:, 0]  # lists 1 .. are empty then and keep their centroid
        assert (a == 0).all()
    ix.train(x)                                                                 # training again on an empty index is allowed


# ------------------------------------------------------------------ assignments, list table, probe
CONFIGS = {  # name: (case, niter, nprobes)
    "tiny1": (lambda: iv.case_gauss(31, 100, 1, 1), 2, (1,)),
    "tiny4": (lambda: iv.case_gauss(31, 100, 9, 4), 2, (1, 3, 4, 9)),
    "clustered": (lambda: iv.case_clustered(4099, 256, 17, 16), 10, (1, 3)),
    "many_q": (lambda: iv.case_gauss(4099, 768, 130, 4), 2, (4,)),
    "wide_p": (lambda: iv.case_gauss(20011, 1000, 9, 40), 1, (40,)),        # 40 probes: the coarse step is the wide search
    "large": (lambda: iv.case_gauss(20011, 768, 17, 16), 2, (3,)),
    "dups": (lambda: iv.case_duplicates(4099, 100, 9, 4), 2, (3, 4)),
    "planted": (lambda: iv.case_planted(256), 0, (1, 3)),
}
_built = {}


def built(name, dtype):
    """-> (index, case, centroids) -- the index trained (or planted) and filled on the GPU, once per (config, storage)"""
    key = (name, dtype)
    if key not in _built:
        ram = _ram()
        make, niter, _ = CONFIGS[name]
        case = make()
        ix = ram.IvfIndex(case["rows"].shape[1], case["nlist"], dtype=dtype)
        ix.niter = niter
        if "centroids" in case:
            ix.set_centroids(case["centroids"])
            if dtype == "sq8":
                vmin = case["rows"].min(axis=0)
                ix.set_sq8_params(vmin, case["rows"].max(axis=0) - vmin)
        else:
            ix.train(case["rows"])
        ix.add(case["rows"])
        _built[key] = (ix, case, ix.centroids())
    return _built[key]


@pytest.mark.parametrize("name", ["tiny1", "tiny4", "clustered", "dups", "planted"])
def test_centroids_of_the_cases(name):
    """what `built` trains is what the restatement trains (the large configurations' training is covered by
    test_training_matches_the_restatement at sizes whose restatement is quick)"""
    make, niter, _ = CONFIGS[name]
    ix, case, c = built(name, "f32")
    assert np.array_equal(c, iv.centroids_of(case, niter))


@pytest.mark.parametrize("dtype", STORAGES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_assignments_list_table_and_probe_match_the_restatement(name, dtype):
    ram = _ram()
    ix, case, c = built(name, dtype)
    assign = iv.nearest(case["rows"], c)[:, 0]                                           # of the float32 input, whatever the storage
    assert ix.ntotal == len(assign) and np.array_equal(ix.assignments(), assign)
    assert np.array_equal(ix.list_sizes(), np.bincount(assign, minlength=case["nlist"]))
    for nprobe in CONFIGS[name][2]:
        P = iv.nearest(case["q"], c, min(nprobe, case["nlist"]))
        assert np.array_equal(ix.probe(case["q"], nprobe), P)                            # host queries
        assert np.array_equal(ix.probe(_dev(case["q"]), nprobe), P)                      # device queries
    ix.nprobe = CONFIGS[name][2][0]
    assert np.array_equal(ix.probe(case["q"]), iv.nearest(case["q"], c, min(ix.nprobe, case["nlist"])))   # the attribute
    ix.nprobe = 1
    # the inner index holds the rows in arrival order: it IS the flat index over them
    flat = ram.MipsIndex(case["rows"].shape[1], dtype=dtype)
    if dtype == "sq8":
        flat.set_sq8_params(*ix.flat.sq8_params())
    flat.add(case["rows"])
    k = min(5, len(assign))
    fd, fi = flat.search(case["q"][:9], k)
    vd, vi = ix.flat.search(case["q"][:9], k)
    assert np.array_equal(vi, fi) and np.array_equal(vd.view(np.uint32), fd.view(np.uint32))
    assert np.array_equal(ix.flat.rows_raw(0, 5), flat.rows_raw(0, 5))
    assert np.array_equal(ix.reconstruct_batch(np.array([0, 3])), flat.reconstruct_batch(np.array([0, 3])))


def test_planted_lists():
    ix, case, c = built("planted", "bf16")
    assert tuple(ix.list_sizes()) == iv.PLANTED_SIZES and np.array_equal(ix.assignments(), case["labels"])
    assert np.array_equal(ix.probe(case["q"], 1)[:, 0], case["qlabels"])


# ------------------------------------------------------------------ the index as it changes
@pytest.mark.parametrize("dtype", STORAGES)
def test_two_adds_remove_reset(dtype):
    ram = _ram()
    case = iv.case_gauss(3000, 100, 9, 8, seed=9)
    x, q = case["rows"], case["q"]
    ix = ram.IvfIndex(100, 8, dtype=dtype)
    ix.niter = 2
    ix.train(x)
    c = ix.centroids()
    ix.add(x[:200])                                                                      # host rows ...
    ix.add(_dev(x[200:]))                                                                # ... then device rows: storage grows in between
    assign = iv.nearest(x, c)[:, 0]
    assert ix.ntotal == 3000 and np.array_equal(ix.assignments(), assign)
    assert np.array_equal(ix.list_sizes(), np.bincount(assign, minlength=8))
    rows = ix.flat.rows_raw(0, 3000)
    # remove every third row: the survivors keep their order, their assignments and their stored form
    gone = np.arange(3000) % 3 == 0
    assert ix.remove_ids(gone) == 1000 and ix.ntotal == 2000
    keep = ~gone
    assert np.array_equal(ix.assignments(), assign[keep]) and np.array_equal(ix.flat.rows_raw(0, 2000), rows[keep])
    assert np.array_equal(ix.list_sizes(), np.bincount(assign[keep], minlength=8))
    assert ix.remove_ids(np.array([0, 5, 5])) == 2 and ix.ntotal == 1998
    assert np.array_equal(ix.assignments(), np.delete(assign[keep], [0, 5]))
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and np.array_equal(ix.centroids(), c) and (ix.list_sizes() == 0).all()
    ix.add(x[:500])
    assert np.array_equal(ix.assignments(), assign[:500]) and np.array_equal(ix.probe(q, 2), iv.nearest(q, c, 2))


@pytest.mark.parametrize("dtype", STORAGES)
def test_save_load(tmp_path, dtype):
    ram = _ram()
    ix, case, c = built("dups", dtype)
    ix.save(str(tmp_path / "ivf"))
    for f in ("meta.json", "centroids.f32", "assign.i32"):
        assert (tmp_path / "ivf" / f).exists()
    iy = ram.IvfIndex.load(str(tmp_path / "ivf"))
    assert (iy.ntotal, iy.nlist, iy.d, iy.dtype, iy.niter) == (ix.ntotal, ix.nlist, ix.d, dtype, ix.niter) and iy.is_trained
    assert np.array_equal(iy.centroids(), c) and np.array_equal(iy.assignments(), ix.assignments())
    assert np.array_equal(iy.list_sizes(), ix.list_sizes()) and np.array_equal(iy.probe(case["q"], 3), ix.probe(case["q"], 3))
    assert np.array_equal(iy.flat.rows_raw(0, iy.ntotal), ix.flat.rows_raw(0, ix.ntotal))
    a, b = ix.flat.search(case["q"], 5), iy.flat.search(case["q"], 5)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_refusals():
    ram = _ram()
    with pytest.raises(NotImplementedError, match="inner product"):
        ram.IvfIndex(64, 4, metric=ram.METRIC_L2)
    lib = ram._lib.load()
    import ctypes

    h = ctypes.c_void_p()
    assert lib.mips_ivf_create(ctypes.byref(h), 0, 64, ram.DTYPE_F32, ram.METRIC_L2, 4) == -3
    assert b"inner product" in lib.mips_last_error()
    for kw in ({"d": 1025}, {"dtype": "fp8_e4m3"}, {"dtype": "fp8_e4m3_docs"}, {"nlist": 0}, {"nlist": 65537}):
        args = {"d": 64, "nlist": 4, "dtype": "bf16", **kw}
        with pytest.raises(NotImplementedError):
            ram.IvfIndex(args["d"], args["nlist"], dtype=args["dtype"])
    x = iv.case_gauss(200, 64, 3, 4)["rows"]
    ix = ram.IvfIndex(64, 4, dtype="sq8")
    with pytest.raises(RuntimeError):
        ix.add(x)                                                                        # not trained
    with pytest.raises(RuntimeError, match="training rows"):
        ix.train(x[:3])                                                                  # n < nlist
    bad = x.copy()
    bad[7, 7] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        ix.train(bad)
    bad[7, 7] = np.inf
    with pytest.raises(RuntimeError, match="infinity"):
        ix.train(_dev(bad))
    assert not ix.is_trained
    ix.train(x)
    ix.add(x)
    with pytest.raises(RuntimeError, match="holds"):
        ix.train(x)
    with pytest.raises(RuntimeError, match="holds"):
        ix.set_centroids(np.zeros((4, 64), np.float32))
    with pytest.raises(NotImplementedError):
        ix.add(np.zeros((2, 64), np.uint8))                                              # raw SQ8 codes
    with pytest.raises(NotImplementedError):
        ix.add(np.zeros((2, 64), np.uint16))                                             # raw bf16 bits
    rc = lib.mips_ivf_add(ix._h, _dev(np.zeros((2, 64), np.uint8)).data_ptr(), 2, ram.DTYPE_SQ8, 1, None)
    assert rc == -3                                                                      # MIPS_E_UNSUPPORTED at the C boundary
    with pytest.raises(ValueError):
        ix.probe(x[:2], 0)
    for name in ("search", "search_packed", "search_wide", "range_search", "search_fused"):
        with pytest.raises(NotImplementedError):
            getattr(ix, name)(x[:2], 5)                                                  # (the search over the probed lists: not in this build)
    with pytest.raises(RuntimeError):
        ix.flat.add(x)                                                                   # the inner index changes through the IvfIndex only
    e = ram.IvfIndex(64, 4)
    with pytest.raises(RuntimeError, match="a NaN"):
        e.set_centroids(np.full((4, 64), np.nan, np.float32))


def test_c_abi_ivf_from_plain_c(tmp_path):
    ram = _ram()
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_ivf_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_ivf_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


def _cycle(kind):
    import torch

    ram = _ram()
    x = iv.case_gauss(1 << 14, 64, 9, 16, seed=15)
    if kind == "ivf":
        ix = ram.IvfIndex(64, 16, dtype="f32")
        ix.niter = 1
        ix.train(x["rows"][:4096])
    else:
        ix = ram.MipsIndex(64, dtype="f32")
    ix.add(x["rows"][:5000])
    ix.add(_dev(x["rows"][5000:]))
    flat = ix.flat if kind == "ivf" else ix
    out = [flat.search(x["q"], 5), flat.search(_dev(x["q"]), 5)]
    if kind == "ivf":
        out.append(ix.probe(x["q"], 3))
    out.append(ix.remove_ids(np.arange(1 << 14) % 5 == 0))
    out.append(flat.search(x["q"], 5))
    torch.cuda.synchronize()
    del ix
    gc.collect()
    torch.cuda.synchronize()
    return out


def test_nothing_is_lost_on_destroy():
    """16 create / destroy cycles: free memory after the 16th may lie below that after the 2nd by no more than the drift of the same
    loop over a flat index in this process plus 8 MiB, the allowance of tests/test_gpu_index_ownership.py: the rows of the two
    inner indexes lost once per cycle would cost 14 x 4 MiB."""
    import torch

    drift = {}
    for kind in ("flat", "ivf"):
        free = {}
        for cyc in range(1, 17):
            _cycle(kind)
            if cyc in (2, 16):
                free[cyc] = torch.cuda.mem_get_info()[0]
        drift[kind] = free[2] - free[16]
    print(f"drift over 14 cycles: flat {drift['flat']} bytes, ivf {drift['ivf']} bytes")
    assert drift["ivf"] <= max(drift["flat"], 0) + 8 * (1 << 20), drift
