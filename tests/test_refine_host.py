"""Two-stage search on PQ codes, CPU side: the pool restatement of tests/refine_cases.py without a mistake IS the definition, and every
deliberate mistake (`wrong=`) changes an I or a D on a named case -- so the cases bite --; csrc/adc_wide_math.hpp -- the text the
kernels compile -- holds its properties under AddressSanitizer and UBSan in a stand-alone program; the new header is additive; a
plain-C consumer compiles against it; the cand_ / rerank_ kernels are exactly the documented ones, allocate without a spill or
scratch and fit their LDS and register bounds; the older census counts stand.  The GPU tests are tests/test_gpu_refine.py and
tests/test_gpu_refine_graph.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivfpq_cases as vc  # noqa: E402
import pq_cases as pc  # noqa: E402
import refine_cases as rc  # noqa: E402

U = np.uint32


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(U), b[0].view(U))


# ------------------------------------------------------------------ the pools restate the definition
@pytest.mark.parametrize("M,d,n,k", [(4, 32, 1000, 30), (4, 32, 1000, 64), (4, 32, 700, 257), (40, 80, 1500, 65), (4, 32, 50, 64), (4, 32, 0, 30)])
def test_pools_without_a_mistake_are_the_definition_pq(M, d, n, k):
    c = pc.case_planted(d, M, n, 2)
    assert same(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], k), rc.candidates_pq(c["q"], c["codebook"], c["codes"], k))


@pytest.mark.parametrize("M,d,nlist,n,k,nprobe", [(4, 32, 8, 1000, 64, 3), (40, 80, 33, 1500, 65, 20), (4, 32, 8, 1000, 300, 8)])
def test_pools_without_a_mistake_are_the_definition_ivfpq(M, d, nlist, n, k, nprobe):
    c = vc.case_planted(d, M, nlist, n, 2)
    args = (c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"], k, nprobe)
    assert same(rc.pool_candidates_ivfpq(*args), rc.candidates_ivfpq(*args))


def test_pool_count_rule_matches_the_issue_table():
    assert rc.pools_of(128, 1024, 1024) == 2 and rc.pools_of(128, 64, 1024) == 16 and rc.pools_of(4, 1024) == 4 and rc.pools_of(96, 1024) == 7
    assert rc.pools_of(40, 65) == 16 and rc.pools_of(40, 64) == 16


# ------------------------------------------------------------------ the mistakes
def test_threshold_at_slot_k_drops_later_rows():
    c = pc.case_planted(32, 4, 1000, 2)
    want = rc.candidates_pq(c["q"], c["codebook"], c["codes"], 64)
    assert not same(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], 64, wrong="threshold_at_k"), want)


def test_ties_go_to_the_lowest_row():
    c = pc.case_ties(n=300)
    D, I = rc.candidates_pq(c["q"], c["codebook"], c["codes"], 64)
    assert (I == np.arange(64)).all() and (D == D[:, :1]).all()
    assert not np.array_equal(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], 64, wrong="tie_high")[1], I)
    f = rc.case_flood()
    args = (f["q"], f["centroids"], f["codebook"], f["codes"], f["assign"], 256, 8)
    D, I = rc.candidates_ivfpq(*args)
    in_flood = np.isin(I[0], f["flood"])
    assert 0 < in_flood.sum() < len(f["flood"])                              # k = 256 cuts inside the flood
    assert np.array_equal(I[0][in_flood], f["flood"][:in_flood.sum()])          # ... and keeps its lowest rows
    assert not np.array_equal(rc.pool_candidates_ivfpq(*args, wrong="tie_high")[1], I)


def test_a_pool_that_ends_below_k_must_be_sorted():
    c = pc.case_planted(32, 4, 100, 2)                                          # 100 rows over 4 pools: none reaches k = 64
    want = rc.candidates_pq(c["q"], c["codebook"], c["codes"], 64)
    assert same(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], 64), want)
    assert not same(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], 64, wrong="unsorted_short"), want)


def test_the_final_rank_counts_every_pool():
    c = pc.case_planted(80, 40, 1500, 2)                                        # M = 40: 16 pools
    want = rc.candidates_pq(c["q"], c["codebook"], c["codes"], 65)
    assert not same(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], 65, wrong="four_pools"), want)
    c4 = pc.case_planted(32, 4, 1500, 2)                                        # (four pools: the mistake cannot show)
    assert same(rc.pool_candidates_pq(c4["q"], c4["codebook"], c4["codes"], 65, wrong="four_pools"), rc.candidates_pq(c4["q"], c4["codebook"], c4["codes"], 65))


def test_ordered_rows_make_every_candidate_an_insertion_or_none():
    for asc in (True, False):
        c = rc.case_ordered(700, ascending=asc)
        D = pc.scores(pc.lut(c["q"], c["codebook"]), c["codes"])
        step = np.diff(D, axis=1)
        assert (step >= 0).all() if asc else (step <= 0).all()
        assert (step != 0).sum() >= 2 * 255
        assert same(rc.pool_candidates_pq(c["q"], c["codebook"], c["codes"], 64), rc.candidates_pq(c["q"], c["codebook"], c["codes"], 64))


def _flat_scores(q, x):
    def score_of(local):
        out = np.full(local.shape, -np.inf, np.float32)
        for j in range(len(q)):
            ok = local[j] >= 0
            out[j, ok] = (x[local[j, ok]].astype(np.float64) @ q[j].astype(np.float64)).astype(np.float32)
        return out
    return score_of


def test_rerank_cases_reject_a_kept_duplicate_and_a_ranked_padding():
    rng = np.random.default_rng(5)
    n, d, nq, kc, k = 200, 16, 3, 64, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    x[n - 1] = 100 * q[0]                                                       # the last row is query 0's best: row -1 of an unchecked read
    ids = rc.rerank_ids(n, nq, kc)
    ids[ids == n - 1] = 0                                                       # (nobody names the last row)
    ids[:, 0] = ids[:, kc - 1] = np.argmax(x[:n - 1] @ q.T, axis=0)             # the repeat (columns 0 and kc - 1) is every query's best row
    assert (ids == -1).any(axis=1).all() and (ids >= n).any()
    D, I = rc.rerank(_flat_scores(q, x), ids, k, n)
    for j in range(nq):
        got = I[j][I[j] >= 0]
        assert len(set(got.tolist())) == len(got) and ((got >= 0) & (got < n)).all()
        assert (np.diff(D[j][: len(got)]) <= 0).all()
    Dd, Id = rc.rerank(_flat_scores(q, x), ids, k, n, wrong="keep_duplicate")
    assert (Id[:, 0] == Id[:, 1]).all() and not np.array_equal(Id, I)
    Dp, Ip = rc.rerank(_flat_scores(q, x), ids, k, n, wrong="pad_as_row")
    assert Ip[0, 0] == -1 and Dp[0, 0] > D[0, 0] and not np.array_equal(Ip, I)
    # fewer valid ids than k: padding; idx_offset shifts validity, not the ids that come back
    few = np.array([[5, -1, 5, n, 7]] * nq, np.int64)
    D2, I2 = rc.rerank(_flat_scores(q, x), few, 4, n)
    assert (np.sort(I2[:, :2], axis=1) == [5, 7]).all() and (I2[:, 2:] == -1).all() and np.isneginf(D2[:, 2:]).all()
    D3, I3 = rc.rerank(_flat_scores(q, x), few + 1000, 4, n, idx_offset=1000)
    assert np.array_equal(I3[:, :2], I2[:, :2] + 1000) and np.array_equal(D3.view(U), D2.view(U))


# ------------------------------------------------------------------ the arithmetic header, the ABI, the kernels
def test_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "adc_wide_math_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "adc_wide_math_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0].split()[0] == "ok" and int(lines[0].split()[1]) >= 100000
    table = {tuple(int(v) for v in line.split()[1:6:2]): int(line.split()[7]) for line in lines[1:]}
    for (M, KP, p), pools in table.items():                                     # the restatement's rule is the header's
        assert pools == rc.pools_of(M, KP, p), (M, KP, p)
    math = open(os.path.join(ram._lib.CSRC, "adc_wide_math.hpp")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', math)) == ["ivf_wide_math.hpp", "ivfpq_math.hpp"]   # no HIP in the arithmetic


def test_header_is_additive():
    lib_ = ram._lib
    with open(lib_.HEADER_REFINE) as f:
        text = f.read()
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(lib_.EXPORTS_REFINE) == {"mips_pq_search_candidates", "mips_ivfpq_search_candidates", "mips_index_rerank"}
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text
    assert len(lib_.EXPORTS) == 41 and len(lib_.EXPORTS_IVF) == 21 and len(lib_.EXPORTS_PQ) == 16 and len(lib_.EXPORTS_IVFPQ) == 22
    assert not (set(lib_.EXPORTS) | set(lib_.EXPORTS_IVF) | set(lib_.EXPORTS_PQ) | set(lib_.EXPORTS_IVFPQ) | set(lib_.EXPORTS_ROWS)) & declared
    assert lib_.HEADER_REFINE in lib_._sources()                                              # a change of the header rebuilds the library
    lib = lib_.load()
    for name in lib_.EXPORTS_REFINE:
        assert getattr(lib, name).argtypes is not None, name                                  # bound with its argument types
    hip = open(os.path.join(lib_.CSRC, "mips_hip.hip")).read()
    assert '#include "refine_kernels.hpp"' in hip and hip.index('#include "host_refine.hpp"') > hip.index('#include "host_ivfpq.hpp"')
    kern = open(os.path.join(lib_.CSRC, "refine_kernels.hpp")).read()
    for inc in ("adc_wide_math.hpp", "ivf_wide_kernels.hpp", "ivfpq_kernels.hpp"):           # included, not restated
        assert f'#include "{inc}"' in kern
    for restated in ("bitonic_low(int", "count_before(const", "fill_slot(int", "shift_dst(int", "pool_class(int"):
        assert restated not in kern and restated not in open(os.path.join(lib_.CSRC, "adc_wide_math.hpp")).read()
    assert isinstance(ram.RefinedIndex, type) and "RefinedIndex" in ram.__all__


def test_c_consumer_compiles_against_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_refine_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "c_abi_refine_smoke.o")])


def test_candidate_and_rerank_kernels_allocate_without_spill_and_fit():
    ram.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("llvm tools of the ROCm image not found")
    all_ks = kernel_regs.kernels()
    ks = {k["demangled"]: k for k in all_ks if "cand_" in k["demangled"] or "rerank_" in k["demangled"]}
    assert {f"mips::cand_{which}_scan_kernel<{kp}>" for which in ("flat", "list") for kp in (64, 256, 1024)} | {"mips::rerank_select_kernel"} == set(ks)
    for name, k in ks.items():
        assert k["spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, (name, k)
    # the scans: no static LDS, so static + dynamic is adcw::lds_bytes <= 160 KiB (the stand-alone check walks every shape); a
    # workgroup of 1024 threads gets at most 128 registers per lane
    for name, k in ks.items():
        if "cand_" in name:
            assert k["lds"] == 0 and k["vgpr"] <= 128, (name, k)
    assert ks["mips::rerank_select_kernel"]["lds"] <= 16 * 1024                  # 1024 (float32, int64) pairs and four wave totals
    # the names the older tests filter by: no new kernel falls into their sets, and their counts are what they were
    names = [k["demangled"] for k in all_ks]
    assert sum("ivf_list_scan" in n for n in names) == 24 and sum("pq_" in n for n in names) == 14
    assert not [n for n in ks if "pq_" in n or "ivfadc_" in n or "ivf_list_scan" in n or "ivf_range" in n
                or n.startswith(("mips::scan_kernel", "mips::tiny_search_kernel", "mips::wide_scan_kernel"))]
