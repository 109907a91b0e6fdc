"""Wide IVF search, CPU side: csrc/ivf_wide_math.hpp (every index that addresses a pool of the wide list scan) holds its properties
under AddressSanitizer and UBSan in a stand-alone program; the restatement agrees with the oracle's brute force over the admitted
rows at k = 30, 100 and 1024; every deliberate mistake of tests/ivf_wide_cases.py (`wrong=`) changes the result of at least one case
-- so the cases bite --; mips_ivf_search_wide / _grp are declared, listed, exported and bound, and a plain-C consumer compiles.  The
GPU tests are tests/test_gpu_ivf_wide.py and tests/test_gpu_ivf_wide_graph.py."""
import inspect
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
import ivf_cases as iv  # noqa: E402
import ivf_filter_cases as fc  # noqa: E402
import ivf_search_cases as sc  # noqa: E402
import ivf_wide_cases as wc  # noqa: E402


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_wide_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "ivf_wide_math_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivf_wide_math_check.cpp"), "-o", exe])
    for seed in ("1", "20261020"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 1000000


def test_pool_class_of_the_cases_is_the_headers():
    with open(os.path.join(ram._lib.CSRC, "ivf_wide_math.hpp")) as f:
        text = f.read()
    assert "return k <= 64 ? 64 : k <= 256 ? 256 : 1024;" in text
    assert [wc.pool_class(k) for k in (1, 64, 65, 256, 257, 1024)] == [64, 64, 256, 256, 1024, 1024]
    assert wc.MAX_K_WIDE == ram._lib.MAX_K_WIDE == 1024 and ram._lib.MAX_K == 29


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_restatement_equals_bruteforce_on_the_admitted_rows(dtype):
    c = wc.case_gauss()
    cen = iv.train(c["rows"], 16, 2)
    assign = iv.nearest(c["rows"], cen)[:, 0]
    base = (c["rows"], c["q"], assign, cen)
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 40, 3000).astype(np.int32)
    ql = rng.integers(0, 40, 12).astype(np.int32)
    ql[5] = fc.LABEL_NONE
    mask = rng.random(3000) < 0.5
    for k, nprobe in ((30, 1), (100, 4), (1024, 4), (1024, 16)):
        for kw in ({}, {"sel": mask}, {"labels": labels, "q_labels": ql, "mode": "exclude"}, {"sel": mask, "labels": labels, "q_labels": ql, "mode": "only"}):
            got = wc.search(*base, k, nprobe, dtype, **kw)
            assert _same(got, fc.bruteforce_on_admitted(*base, k, nprobe, dtype, **kw)), (k, nprobe, kw.keys())
            assert _same(wc.prefix(got, 29), fc.search(*base, 29, nprobe, dtype, **kw))                   # the prefix identity of the definition
    d, i = wc.search(*base, 1024, 1, dtype, sel=mask)
    assert (i[:, -1] == -1).all() and np.isneginf(d[:, -1]).all() and (i[:, 0] >= 0).all()                 # fewer than k admitted: padding last


def test_flood_gives_the_lowest_copies_ascending():
    c = wc.case_flood()
    d, i = wc.search(c["rows"], c["q"], c["assign"], c["centroids"], 1024, 3, "f32")
    assert np.array_equal(i[0], c["copies"][:1024]) and (d[0] == d[0, 0]).all() and len(c["copies"]) == wc.FLOOD_COPIES
    assert sorted(np.bincount(c["assign"][c["copies"]], minlength=4).tolist()) == [0, 366, 367, 367]        # spread over three lists


def test_ordered_case_is_exact_on_every_storage():
    c = wc.case_ordered(8)
    asc, desc = np.flatnonzero(c["assign"] == 0), np.flatnonzero(c["assign"] == 1)
    assert (np.diff(c["score"][asc]) == 1).all() and (np.diff(c["score"][desc]) == -1).all() and len(asc) == wc.ORDERED_L
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    want = None
    for dtype in sc.STORAGES:
        d, i = wc.search(*base, 64, 2, dtype, c["sq8_params"] if dtype == "sq8" else None)
        scale = (2.0 ** (np.arange(8) % 4))[:, None]
        half = 64.5 if dtype == "sq8" else 0.0                                                            # B_q: a code c decodes to c + 1/2
        assert np.array_equal(d, ((c["score"][i] + half) * scale).astype(np.float32))                     # the score IS 2^e s (+ B_q)
        assert want is None or np.array_equal(i, want[1])
        want = (d, i)
    assert (c["score"][want[1][0, 0::2]] == c["score"][want[1][0, 1::2]]).all() and (want[1][0, 0::2] < want[1][0, 1::2]).all()   # ties across the lists


def test_fill_case_sizes():
    c = wc.case_fill(4)
    assert tuple(np.bincount(c["assign"])) == wc.FILL_SIZES
    assert wc.queries_for_one_segment(4, 256) == 128 and fc.segments(128, 4, 1024) == 1 and fc.segments(127, 4, 1024) == 2
    windows = lambda L: [len([p for p in range(L) if (p % 256) // 64 == w]) for w in range(4)]            # positions a wave sees at S = 1
    assert windows(4095) == [1024, 1024, 1024, 1023] and windows(4096) == [1024] * 4 and windows(4097) == [1025, 1024, 1024, 1024]


def test_every_deliberate_mistake_is_rejected_by_a_case():
    f = wc.case_flood()
    g = wc.case_gauss()
    cen = iv.train(g["rows"], 16, 2)
    cases = [("flood 1024", (f["rows"], f["q"], f["assign"], f["centroids"], 1024, 3, "f32")),
             ("gauss 30", (g["rows"], g["q"][:3], iv.nearest(g["rows"], cen)[:, 0], cen, 30, 4, "f32"))]
    right = [wc.search(*a) for _, a in cases]
    hits = {}
    for wrong in wc.WRONG:
        hits[wrong] = [name for (name, a), want in zip(cases, right) if not _same(wc.search(*a, wrong=wrong), want)]
        assert hits[wrong], wrong
    assert "flood 1024" in hits["arrival_ties"] and "flood 1024" in hits["key_only_threshold"]            # both lose the tie flood
    assert hits["capacity_for_k"] == ["gauss 30"]                                                          # k = 30 in a pool of 64


def test_wide_search_is_declared_listed_exported_and_bound():
    lib_ = ram._lib
    with open(lib_.HEADER_IVF) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", code))
    assert {"mips_ivf_search_wide", "mips_ivf_search_wide_grp"} <= declared and declared == set(lib_.EXPORTS_IVF)
    assert len(lib_.EXPORTS_IVF) == len(set(lib_.EXPORTS_IVF)) == 21 and len(lib_.EXPORTS) == 41
    head = ("mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx, "
            "int64_t idx_offset, int flags, ")
    tail = "const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels, int grp_mode, void* hip_stream"
    for name, rest in (("mips_ivf_search_wide", "void* hip_stream"), ("mips_ivf_search_wide_grp", tail)):
        m = re.search(rf"int {name}\(([^;]*)\);", code)
        assert m and re.sub(r"\s+", " ", m.group(1)) == head + rest, name
    assert "mips_ivf_search_wide_sel" not in text                                                         # bitmap only is q_labels == NULL
    lib = lib_.load()
    for name in ("mips_ivf_search_wide", "mips_ivf_search_wide_grp"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", lib_.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mips_ivf_search_wide$", out, flags=re.M) and re.search(r" T mips_ivf_search_wide_grp$", out, flags=re.M)
    par = inspect.signature(ram.IvfIndex.search_probed_wide).parameters
    assert list(par) == list(inspect.signature(ram.IvfIndex.search_probed).parameters)
    assert ram.IvfIndex.search_wide is ram.IvfIndex.search                                                 # the faiss-shaped forms stay refused


def test_list_scan_instances_registers_and_lds():
    """tools/kernel_regs.py (the code object's notes, no GPU): the six narrow instances as they were -- 113 / 114 / 114 VGPRs, 46 096
    bytes of LDS, filtered 114 and 48 144 --, eighteen wide ones (3 storages x filtered or not x 3 pool classes), none with a spill or
    scratch, each with the narrow instance's LDS less its two 32-slot lists (1024 bytes) plus four pools of KP entries of 8 bytes."""
    ram.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("llvm tools of the ROCm image not found")
    ks = {k["demangled"]: k for k in kernel_regs.kernels() if "ivf_list_scan" in k["demangled"]}
    assert all(k["spill"] == 0 and k["scratch"] == 0 for k in ks.values())
    pairs = {"f32": "mips::ElemF32, mips::ElemF32", "sq8": "mips::ElemU8, mips::ElemBF16", "bf16": "mips::ElemBF16, mips::ElemBF16"}
    narrow = {(dt, filt): ks[f"mips::ivf_list_scan_kernel<{p}, {'true' if filt else 'false'}>"] for dt, p in pairs.items() for filt in (False, True)}
    assert [narrow[(dt, False)]["vgpr"] for dt in ("f32", "sq8", "bf16")] == [113, 114, 114]
    assert all(narrow[(dt, True)]["vgpr"] == 114 for dt in pairs)
    assert all(narrow[(dt, False)]["lds"] == 46096 and narrow[(dt, True)]["lds"] == 48144 for dt in pairs)
    wide = [n for n in ks if n.startswith("mips::ivf_list_scan_wide_kernel<")]
    assert len(wide) == 18 and len(ks) == 24
    for dt, p in pairs.items():
        for filt in (False, True):
            for kp in (64, 256, 1024):
                k = ks[f"mips::ivf_list_scan_wide_kernel<{p}, {'true' if filt else 'false'}, {kp}>"]
                assert k["lds"] == narrow[(dt, filt)]["lds"] - 1024 + 4 * kp * 8 and k["lds"] <= 160 * 1024, (dt, filt, kp, k)


def test_c_consumer_of_the_wide_search_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_ivf_wide_smoke.c"), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "c_abi_ivf_wide_smoke.o")])
