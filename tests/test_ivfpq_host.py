"""IVF index over PQ codes, CPU side: every deliberate mistake of tests/ivfpq_cases.py (`wrong=`) changes the bits of a D, an I, a
code or a row on a named case -- so the cases bite --; csrc/ivfpq_math.hpp -- the text the kernels compile -- holds its properties
under AddressSanitizer and UBSan in a stand-alone program and agrees with the restatement bit for bit; the new header is additive; a
plain-C consumer compiles against it; every ivfadc_ kernel allocates without a spill or scratch and the scan's LDS and registers
fit; the older census counts stand; and the factory strings still refuse.  The GPU tests are tests/test_gpu_ivfpq.py and
tests/test_gpu_ivfpq_graph.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram
from retrieval_augmented_mds_amd import faiss_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivfpq_cases as vc  # noqa: E402
import pq_cases as pc  # noqa: E402

U = np.uint32


def run(c, k, nprobe, wrong=None, **kw):
    return vc.search(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"], k, nprobe, wrong=wrong, **kw)


@pytest.fixture(scope="module")
def order_case():
    c = vc.case_sum_order()
    c["want"] = run(c, 29, 3)
    return c


@pytest.mark.parametrize("wrong", ["coarse_last", "no_coarse", "fp64"])
def test_sum_order_case_rejects_other_sums(order_case, wrong):
    D, _ = order_case["want"]
    W, _ = run(order_case, 29, 3, wrong=wrong)
    assert (W.view(U) != D.view(U)).mean() > 0.3, wrong                 # the bits of D differ
    c = order_case                                                        # ... and for one row T + (a + b) != (T + a) + b outright
    full = vc.all_scores(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"])
    last = vc.all_scores(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"], wrong="coarse_last")
    assert (full.view(U) != last.view(U)).any()


def test_ties_go_to_the_lowest_probed_row():
    c = vc.case_ties()
    D, I = run(c, 29, 3)
    L, _ = vc.probe(c["q"], c["centroids"], 3)
    assert (L == np.arange(3)).all()                                     # equal centroids: ties to the lowest list
    lowest = np.flatnonzero(np.isin(c["assign"], [0, 1, 2]))[:29]
    assert (I == lowest).all() and (D == D[:, :1]).all()
    assert not np.array_equal(run(c, 29, 3, wrong="tie_high")[1], I)


def test_one_probed_list_less_changes_the_rows():
    c = vc.case_planted(32, 4, 8, 1000, 3)
    c["q"][0] = 3 * c["centroids"][0]                                     # the nearest list of query 0 is list 0: empty
    good, bad = run(c, 5, 2), run(c, 5, 2, wrong="one_list_less")
    assert (good[1][0] >= 0).all() and (bad[1][0] == -1).all()
    few = dict(c, codes=c["codes"][:25], assign=(np.arange(25) % 8).astype(np.int32))   # 25 rows over 8 lists, k = 29: every list counts
    for nprobe in (3, 8, 13):
        good, bad = run(few, 29, nprobe), run(few, 29, nprobe, wrong="one_list_less")
        assert ((good[1] >= 0).sum(axis=1) > (bad[1] >= 0).sum(axis=1)).all(), nprobe
    D, I = run(c, 29, 1)                                                  # fewer probed rows than k: padding
    sizes = np.bincount(c["assign"], minlength=8)
    L, _ = vc.probe(c["q"], c["centroids"], 1)
    for j in range(3):
        have = min(29, sizes[L[j, 0]])
        assert (I[j, have:] == -1).all() and np.isneginf(D[j, have:]).all() and (I[j, :have] >= 0).all()
    assert (sizes[L[:, 0]] < 29).any()


def test_residual_coding_and_reconstruct_cases_bite():
    c = vc.case_train()
    cen, cb = vc.train(c["x"], c["nlist"], c["M"], 3, 3)
    codes, a = vc.encode(c["x"], cen, cb)
    raw, _ = vc.encode(c["x"], cen, cb, wrong="raw_codes")
    assert (codes != raw).mean() > 0.5                                   # codes of the row instead of the residual
    rows = vc.reconstruct(codes, a, cen, cb)
    bare = vc.reconstruct(codes, a, cen, cb, wrong="no_centroid")
    assert (rows.view(U) != bare.view(U)).mean() > 0.9
    err = lambda r: float(np.linalg.norm(r - c["x"]) / np.linalg.norm(c["x"]))  # noqa: E731
    assert err(rows) < 0.5 * err(bare)                                   # (the centroid belongs to the row)
    flat_cb = pc.train(pc.training_set(c["x"]), c["M"], 3)
    assert not np.array_equal(flat_cb, cb)                               # the codebook is trained on residuals
    cen0, cb0 = vc.train(c["x"], c["nlist"], c["M"], 3, 3, by_residual=False)
    assert np.array_equal(cen0, cen) and np.array_equal(cb0, flat_cb)


def test_by_residual_false_is_the_pq_search_when_every_list_is_probed():
    c = vc.case_planted(32, 16, 8, 1000, 3)
    got = run(c, 29, 8, by_residual=False)
    want = pc.search(c["q"], c["codebook"], c["codes"], 29)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(U), want[0].view(U))


def test_scoring_the_rows_of_a_search_reproduces_its_scores():
    c = vc.case_planted(48, 24, 33, 1000, 3)
    D, I = run(c, 5, 3, idx_offset=7)
    full = vc.all_scores(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"])
    assert np.array_equal(np.take_along_axis(full, I - 7, axis=1).view(U), D.view(U))
    for n, sizes in ((1000, vc.list_sizes(33, 1000, 24)), (4097, vc.list_sizes(33, 4097, 128))):
        assert sizes.sum() == n and {0, 1, 63, 64, 65} <= set(sizes.tolist())
    assert {255, 257} <= set(vc.list_sizes(33, 1000, 24).tolist()) and {1023, 1025} <= set(vc.list_sizes(33, 4097, 128).tolist())


def test_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "ivfpq_math_check"), str(tmp_path / "vectors.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivfpq_math_check.cpp"), "-o", exe])
    rng = np.random.default_rng(21)
    M, dsub, nlist, n, nq = 5, 3, 6, 70, 4
    d = M * dsub
    cen = (rng.standard_normal((nlist, d)) * 8).astype(np.float32)
    cb = (rng.standard_normal((M, 256, dsub)) * np.exp(rng.uniform(-6, 2, (M, 1, 1)))).astype(np.float32)
    x = (cen[rng.integers(0, nlist, n)] + rng.standard_normal((n, d))).astype(np.float32)
    a = vc.assign(x, cen)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[3] = 0
    with open(inp, "w") as f:
        f.write(f"{M} {dsub} {nlist} {n} {nq}\n")
        for arr in (cen, cb, x, q):
            f.write(" ".join(f"{v:08x}" for v in arr.view(np.uint32).reshape(-1)) + "\n")
        f.write(" ".join(str(int(v)) for v in a) + "\n")
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0].split()[0] == "ok" and int(lines[0].split()[1]) >= 500
    codes = np.array(lines[1].split(), dtype=np.int64).reshape(n, M)
    want, a2 = vc.encode(x, cen, cb)
    assert np.array_equal(codes, want) and np.array_equal(a2, a)
    bits = lambda line: np.array([int(v, 16) for v in line.split()], dtype=np.uint32)  # noqa: E731
    full = vc.all_scores(q, cen, cb, want, a)
    assert np.array_equal(np.stack([bits(line) for line in lines[2:2 + nq]]), full.view(np.uint32))
    assert np.array_equal(np.stack([bits(line) for line in lines[2 + nq:2 + nq + n]]), vc.reconstruct(want, a, cen, cb).view(np.uint32))


def test_header_is_additive():
    lib_ = ram._lib
    with open(lib_.HEADER_IVFPQ) as f:
        text = f.read()
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(lib_.EXPORTS_IVFPQ) and len(lib_.EXPORTS_IVFPQ) == len(declared) == 22
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text and "MIPS_DTYPE_PQ" not in text
    assert len(lib_.EXPORTS) == 41 and len(lib_.EXPORTS_IVF) == 21 and len(lib_.EXPORTS_PQ) == 16
    assert not (set(lib_.EXPORTS) | set(lib_.EXPORTS_IVF) | set(lib_.EXPORTS_PQ)) & declared
    assert lib_.HEADER_IVFPQ in lib_._sources()                                               # a change of the header rebuilds the library
    lib = lib_.load()
    for name in lib_.EXPORTS_IVFPQ:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name                                                  # bound with its argument types
    hip = open(os.path.join(lib_.CSRC, "mips_hip.hip")).read()
    assert '#include "ivfpq_kernels.hpp"' in hip
    assert hip.index('#include "host_ivfpq.hpp"') > max(hip.index('#include "host_pq.hpp"'), hip.index('#include "host_ivf.hpp"'))   # one translation unit
    math = open(os.path.join(lib_.CSRC, "ivfpq_math.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', math) == ["pq_math.hpp"]                # no HIP in the arithmetic


def test_c_consumer_compiles_against_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_ivfpq_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "c_abi_ivfpq_smoke.o")])


def test_ivfadc_kernels_allocate_without_spill_and_the_scan_fits():
    ram.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("llvm tools of the ROCm image not found")
    all_ks = kernel_regs.kernels()
    ks = {k["demangled"]: k for k in all_ks if "ivfadc_" in k["demangled"]}
    assert {"mips::ivfadc_scan_kernel<4>", "mips::ivfadc_scan_kernel<16>", "mips::ivfadc_residual_kernel<float>", "mips::ivfadc_residual_kernel<unsigned short>",
            "mips::ivfadc_score_subset_kernel<float>", "mips::ivfadc_score_subset_kernel<unsigned short>", "mips::ivfadc_rows_kernel",
            "mips::ivfadc_finish_kernel", "mips::ivfadc_lists_kernel"} == set(ks)
    for name, k in ks.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
    # the scan: static + dynamic LDS at M = 128 and p = 1024 (the table, 16 waves' lists and counts, the prefix, starts and coarse
    # terms of 1024 lists) within the compute unit's 160 KiB; a 1024-thread workgroup gets at most 128 registers per lane
    for w in (4, 16):
        k = ks[f"mips::ivfadc_scan_kernel<{w}>"]
        assert k["lds"] + 128 * 1024 + 16 * 32 * 8 + 16 * 4 + (3 * 1024 + 1) * 4 <= 160 * 1024 and k["vgpr"] <= 128 and k["agpr"] == 0
    src = open(os.path.join(ram._lib.CSRC, "ivfpq_math.hpp")).read()
    assert "return pq::scan_lds_bytes(M) + ((int64_t)3 * p + 1) * 4;" in src
    # the names the older tests filter by: no new kernel falls into their sets, and their counts are what they were
    names = [k["demangled"] for k in all_ks]
    assert sum("ivf_list_scan" in n for n in names) == 24 and sum("pq_" in n for n in names) == 14
    assert not [n for n in ks if "pq_" in n or n.startswith(("mips::scan_kernel", "mips::tiny_search_kernel", "mips::wide_scan_kernel")) or "ivf_list_scan" in n
                or "ivf_range" in n]


def test_factory_strings_still_refuse_and_the_class_is_reached_by_name():
    for bad in ("IVF4096,PQ32", "IVF256,PQ16", "PQ16", "OPQ16,IVF256,PQ16"):
        with pytest.raises(NotImplementedError):
            faiss_shim.index_factory(64, bad, faiss_shim.METRIC_INNER_PRODUCT)
        with pytest.raises(NotImplementedError):
            ram.mips.factory_dtype(bad, "f32")
    assert isinstance(ram.IvfPqIndex, type) and "IvfPqIndex" in ram.__all__
    for kw in (dict(metric=ram.METRIC_L2), dict(nbits=4)):
        with pytest.raises(NotImplementedError):
            ram.IvfPqIndex(64, 16, 8, **kw)
    for args in ((2048, 16, 8), (516, 16, 129), (64, 0, 8), (64, 65537, 8)):
        with pytest.raises(NotImplementedError):
            ram.IvfPqIndex(*args)
    with pytest.raises(ValueError):
        ram.IvfPqIndex(30, 16, 8)
