"""Product-quantised index, CPU side: every deliberate mistake of tests/pq_cases.py (`wrong=`) changes the bits of a score, a code or
the codebook on a named case -- so the cases bite --; the restatement has the properties the definition claims; csrc/pq_math.hpp --
the text the kernels compile -- holds its properties under AddressSanitizer and UBSan in a stand-alone program and agrees with the
restatement bit for bit; the new header is additive; a plain-C consumer compiles against it; every pq_ kernel allocates without a
spill or scratch and the scan's LDS fits; the older census counts stand; and the factory strings still refuse PQ.  The GPU tests
are tests/test_gpu_pq.py and tests/test_gpu_pq_graph.py."""
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
import pq_cases as pc  # noqa: E402

U = np.uint32


@pytest.fixture(scope="module")
def big():
    """8 queries x 5000 rows, M = 96, dsub = 8: the shape the index is for"""
    c = pc.case_planted(768, 96, 5000, 8)
    c["lut"] = pc.lut(c["q"], c["codebook"])
    c["D"] = pc.scores(c["lut"], c["codes"])
    return c


def test_wrong_sums_change_most_scores_but_not_the_ranking(big):
    D = big["D"]
    _, top = pc.top_k(D, 5)
    for wrong in ("fp64", "pairwise"):
        W = pc.scores(big["lut"], big["codes"], wrong=wrong)
        frac = (W.view(U) != D.view(U)).mean()
        assert 0.7 < frac < 0.95, (wrong, frac)                      # most scores differ in their last bits ...
        assert np.array_equal(pc.top_k(W, 5)[1], top)                # ... and the best rows do not: the tests compare the bits of D


def test_signed_codes_change_every_score(big):
    W = pc.scores(big["lut"], big["codes"], wrong="signed")
    assert (W.view(U) != big["D"].view(U)).all()
    assert (pc.top_k(W, 5)[1] != pc.top_k(big["D"], 5)[1]).any(axis=1).all()


def test_bf16_table_changes_scores(big):
    W = pc.scores(pc.lut(big["q"], big["codebook"], wrong="bf16_table"), big["codes"])
    assert (W.view(U) != big["D"].view(U)).mean() > 0.9


def test_scaling_by_a_power_of_two_scales_every_score_exactly(big):
    for e in (20, 30, -30):
        cb = (big["codebook"] * np.float32(2.0 ** e)).astype(np.float32)
        assert np.array_equal(pc.scores(pc.lut(big["q"], cb), big["codes"]), big["D"] * np.float32(2.0 ** e))


def test_sum_order_case_rejects_other_orders():
    c = pc.case_sum_order()
    table = pc.lut(c["q"], c["codebook"])
    D = pc.scores(table, c["codes"])
    for wrong in ("fp64", "pairwise"):
        assert (pc.scores(table, c["codes"], wrong=wrong).view(U) != D.view(U)).mean() > 0.3, wrong


def test_ties_go_to_the_lowest_row():
    c = pc.case_ties()
    D, I = pc.search(c["q"], c["codebook"], c["codes"], 29)
    assert (I == np.arange(29)).all() and (D == D[:, :1]).all()
    assert not np.array_equal(pc.search(c["q"], c["codebook"], c["codes"], 29, wrong="tie_high")[1], I)
    c = pc.case_duplicates()
    D, I = pc.search(c["q"], c["codebook"], c["codes"], 29, idx_offset=7)
    assert list(I[0, :len(c["planted"])]) == [r + 7 for r in c["planted"]]     # the planted copies, in ascending row order
    z = pc.search(np.zeros_like(c["q"]), c["codebook"], c["codes"], 5)
    assert (z[0].view(U) == 0).all() and (z[1] == np.arange(5)).all()          # a zero query: every score +0, rows 0 .. k - 1
    D, I = pc.search(c["q"], c["codebook"], c["codes"][:3], 5)
    assert (I[:, 3:] == -1).all() and np.isneginf(D[:, 3:]).all() and (I[:, :3] >= 0).all()


def test_training_cases_exercise_the_rules():
    c = pc.case_train_distinct()
    stats = {}
    good = pc.train(c["x"], c["M"], 3, stats=stats)
    assert stats["empty_updates"] > 4000                                        # of 8 * 256 * 3: "keeps its value" is exercised
    codes = pc.encode(c["x"], good)
    assert not np.array_equal(codes, pc.encode(c["x"], good, wrong="le"))       # equal centroids: <= sends a row to the highest of them
    assert len(np.unique(codes[:, 0])) <= 40 and np.array_equal(pc.reconstruct(codes, good), c["x"])   # (every row is a centroid)
    c = pc.case_train_cancel()
    good, bad = pc.train(c["x"], 2, 1), pc.train(c["x"], 2, 1, wrong="sum_order")
    assert good[0, 0, 0] == 0.0 and bad[0, 0, 0] == 0.25                        # members 0, 2^70, 1, -2^70 of centroid 0
    a = pc.nearest(c["x"][:, :1], np.ascontiguousarray(c["x"][0::2, :1]))
    assert list(np.flatnonzero(a == 0)) == [0, 1, 3, 5]
    c = pc.case_train_gauss()
    good = pc.train(c["x"], c["M"], 4)
    assert not np.array_equal(good, pc.train(c["x"], c["M"], 3)) and np.isfinite(good).all()                # (the iterations move the centroids)
    assert np.array_equal(pc.train(c["x"], c["M"], 0)[2, 5], c["x"][5 * 700 // 256, 16:24])    # niter = 0: the initial rows


def test_subsample_rule():
    x = pc.case_train_subsample()["x"]
    T = pc.training_set(x)
    assert len(T) == 65536 and all(np.array_equal(T[i], x[i * len(x) // 65536]) for i in (0, 1, 1771, 1772, 40000, 65535))
    assert not np.array_equal(T[40000], x[40000]) and pc.training_set(x[:65536]) is not None and len(pc.training_set(x[:65536])) == 65536


def test_encode_gives_every_input_a_code():
    c = pc.case_encode()
    codes = pc.encode(c["x"], c["codebook"])
    assert codes[3, 1] == 0 and codes[5, 3] == 0 and (codes[7] == 0).all() and (codes[9] == 0).all()   # NaN / inf sub-vectors: code 0
    assert codes[3, 0] == pc.nearest(c["x"][3:4, 0:3], c["codebook"][0])[0]                          # the other sub-vectors as usual
    assert np.array_equal(pc.reconstruct(codes, c["codebook"])[:, 3:6], c["codebook"][1][codes[:, 1]])


def test_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "pq_math_check"), str(tmp_path / "vectors.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pq_math_check.cpp"), "-o", exe])
    rng = np.random.default_rng(12)
    M, dsub, n, nq = 5, 3, 70, 4
    cb = (rng.standard_normal((M, 256, dsub)) * np.exp(rng.uniform(-8, 8, (M, 1, 1)))).astype(np.float32)
    cb[1, 17] = cb[1, 3]                                             # equal centroids: a tie
    x = rng.standard_normal((n, M * dsub)).astype(np.float32)
    x[4, 3:6] = cb[1, 3]
    x[6, 0] = np.nan
    x[8, 7] = np.inf
    q = rng.standard_normal((nq, M * dsub)).astype(np.float32)
    q[3] = 0
    with open(inp, "w") as f:
        f.write(f"{M} {dsub} {n} {nq}\n")
        for a in (cb, x, q):
            f.write(" ".join(f"{v:08x}" for v in a.view(np.uint32).reshape(-1)) + "\n")
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0].split()[0] == "ok" and int(lines[0].split()[1]) >= 500
    codes = np.array(lines[1].split(), dtype=np.int64).reshape(n, M)
    want = pc.encode(x, cb)
    assert np.array_equal(codes, want) and codes[4, 1] == 3 and codes[6, 0] == 0 and codes[8, 2] == 0
    bits = lambda line: np.array([int(v, 16) for v in line.split()], dtype=np.uint32)  # noqa: E731
    table = pc.lut(q, cb)
    assert np.array_equal(np.stack([bits(line) for line in lines[2:2 + nq]]), table.view(np.uint32).reshape(nq, -1))
    assert np.array_equal(np.stack([bits(line) for line in lines[2 + nq:2 + 2 * nq]]), pc.scores(table, want).view(np.uint32))


def test_header_is_additive():
    lib_ = ram._lib
    with open(lib_.HEADER_PQ) as f:
        text = f.read()
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(lib_.EXPORTS_PQ) and len(lib_.EXPORTS_PQ) == len(declared) == 16
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text and "MIPS_DTYPE_PQ" not in text
    assert len(lib_.EXPORTS) == 41 and len(lib_.EXPORTS_IVF) == 21 and not (set(lib_.EXPORTS) | set(lib_.EXPORTS_IVF)) & declared
    assert lib_.HEADER_PQ in lib_._sources()                                                  # a change of the header rebuilds the library
    assert (lib_.DTYPE_F32, lib_.DTYPE_BF16, lib_.DTYPE_FP8_E4M3, lib_.DTYPE_FP8_E4M3_DOCS, lib_.DTYPE_SQ8) == (0, 1, 2, 3, 4)
    lib = lib_.load()
    for name in lib_.EXPORTS_PQ:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name                                                  # bound with its argument types
    hip = open(os.path.join(lib_.CSRC, "mips_hip.hip")).read()
    assert '#include "pq_kernels.hpp"' in hip and '#include "host_pq.hpp"' in hip            # one translation unit


def test_c_consumer_compiles_against_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_pq_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "c_abi_pq_smoke.o")])


def test_pq_kernels_allocate_without_spill_and_the_table_fits():
    ram.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("llvm tools of the ROCm image not found")
    all_ks = kernel_regs.kernels()
    ks = {k["demangled"]: k for k in all_ks if "pq_" in k["demangled"]}
    assert {"mips::pq_adc_scan_kernel<4>", "mips::pq_adc_scan_kernel<16>", "mips::pq_lut_kernel<float>", "mips::pq_lut_kernel<unsigned short>",
            "mips::pq_assign_kernel<float>", "mips::pq_assign_kernel<unsigned short>", "mips::pq_rows_kernel", "mips::pq_score_subset_kernel",
            "mips::pq_finish_kernel", "mips::pq_init_codebook_kernel", "mips::pq_hist_kernel", "mips::pq_offsets_kernel", "mips::pq_list_fill_kernel",
            "mips::pq_centroid_mean_kernel"} == set(ks)
    for name, k in ks.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
    # the scan: static + dynamic LDS at M = 128 (the table, 16 waves' lists and counts) within the compute unit's 160 KiB; a
    # 1024-thread workgroup gets at most 128 registers per lane
    for w in (4, 16):
        k = ks[f"mips::pq_adc_scan_kernel<{w}>"]
        assert k["lds"] + 128 * 1024 + 16 * 32 * 8 + 16 * 4 <= 160 * 1024 and k["vgpr"] <= 128 and k["agpr"] == 0
    src = open(os.path.join(ram._lib.CSRC, "pq_math.hpp")).read()
    assert "return (int64_t)M * kSub * 4 + (int64_t)w * kListSlots * 8 + (int64_t)w * 4;" in src and "constexpr int kListSlots = 32;" in src
    # the census of the older tests: the names they count are what they were
    names = [k["demangled"] for k in all_ks]
    assert sum("ivf_list_scan" in n for n in names) == 24
    assert not [n for n in ks if n.startswith(("mips::scan_kernel", "mips::tiny_search_kernel", "mips::wide_scan_kernel")) or "ivf_list_scan" in n or "ivf_range" in n]


def test_factory_strings_still_refuse_and_the_class_is_reached_by_name():
    for bad in ("PQ16", "IVF4096,PQ32", "OPQ16,PQ16"):
        with pytest.raises(NotImplementedError):
            faiss_shim.index_factory(64, bad, faiss_shim.METRIC_INNER_PRODUCT)
        with pytest.raises(NotImplementedError):
            ram.mips.factory_dtype(bad, "f32")
    assert isinstance(ram.PqIndex, type) and "PqIndex" in ram.__all__
    for kw in (dict(metric=ram.METRIC_L2), dict(nbits=4)):
        with pytest.raises(NotImplementedError):
            ram.PqIndex(64, 8, **kw)
    with pytest.raises(NotImplementedError):
        ram.PqIndex(2048, 8)
    with pytest.raises(NotImplementedError):
        ram.PqIndex(516, 129)
    with pytest.raises(ValueError):
        ram.PqIndex(30, 8)
