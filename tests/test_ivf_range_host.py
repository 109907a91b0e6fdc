"""Range search over the probed lists, CPU side: every deliberate mistake of tests/ivf_range_cases.py (`wrong=`) is rejected by a named
case -- so the cases bite --; the restatement equals a brute force over the probed and admitted rows; csrc/ivf_range_math.hpp (every
index that addresses the staging buffer, the caller's arrays or a sort partner) holds its properties under AddressSanitizer and UBSan
in a stand-alone program; mips_ivf_range_search / _grp are declared in a header of their own, listed, exported and bound, and the
lists the older tests pin keep their lengths; a plain-C consumer compiles; the new kernels use no scratch and spill nothing, and the
list-scan kernels are the 24 they were.  The GPU tests are tests/test_gpu_ivf_range.py and tests/test_gpu_ivf_range_graph.py."""
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
import ivf_filter_cases as fc  # noqa: E402
import ivf_range_cases as rc  # noqa: E402
import ivf_search_cases as sc  # noqa: E402


def _base(c):
    return c["rows"], c["q"], c["assign"], c["centroids"]


def _mid_radii(c, nprobe, dtype, frac=0.5, **kw):
    """per query the reported score at `frac` of its probed rows, descending: a radius that splits them"""
    per = rc.probed_scores(*_base(c), nprobe, dtype, **kw)
    return np.array([np.sort(rep)[::-1][int(len(rep) * frac)] for _, _, rep, _ in per], np.float32)


# ------------------------------------------------------------------ the named cases: (arguments, keywords) of rc.range_search
def _named_cases():
    eq = rc.case_equal()
    g =rc.case_round_robin(900, 32, 5, 6)
    mask = np.arange(900) % 3 != 1
    labels = (np.arange(900) // 7).astype(np.int32)
    ql = np.array([3, fc.LABEL_NONE, 40, 41, 100], np.int32)
    cases = {}
    # the radius of query 0 IS the score of the three copies (all four lists probed, so they are probed whatever their list)
    per4 = rc.probed_scores(*_base(eq), 4, "f32")
    r_eq = np.array([per4[0][2][list(per4[0][0]).index(7)]] + [0.0] * 3, np.float32)
    cases["equal scores f32"] = ((*_base(eq), r_eq, 4, "f32"), {})
    cases["sq8 bias"] = ((*_base(g), _mid_radii(g, 3, "sq8"), 3, "sq8"), {})
    cases["interleaved lists"] = ((*_base(g), _mid_radii(g, 3, "f32"), 3, "f32"), {})
    r = _mid_radii(g, 2, "bf16")
    r[0], r[1] = np.float32(np.inf), np.float32(-np.inf)                                     # query 0 hits nothing, query 1 everything probed
    cases["per-query radii"] = ((*_base(g), r, 2, "bf16"), {})
    cases["two of six lists"] = ((*_base(g), np.full(5, -np.inf, np.float32), 2, "f32"), {})
    cases["filtered"] = ((*_base(g), _mid_radii(g, 3, "f32", frac=0.8), 3, "f32"),
                         {"sel": np.concatenate([np.ones(5, bool), mask]), "sel_bit0": 5, "labels": labels, "q_labels": ql, "mode": "exclude"})
    return cases


def test_every_deliberate_mistake_is_rejected_by_a_named_case():
    cases = _named_cases()
    right = {name: rc.range_search(*a, **kw) for name, (a, kw) in cases.items()}
    hits = {w: [name for name, (a, kw) in cases.items() if not rc.same(rc.range_search(*a, **kw, wrong=w), right[name])] for w in rc.WRONG}
    assert all(hits[w] for w in rc.WRONG), hits
    assert "equal scores f32" in hits["non_strict"]
    assert "sq8 bias" in hits["rule_on_S"] and hits["rule_on_S"] == ["sq8 bias"]                # S == D on the other storages
    assert "interleaved lists" in hits["list_order"]
    assert "per-query radii" in hits["first_radius"]
    assert "two of six lists" in hits["all_rows"]
    assert hits["post_count"] == ["filtered"]
    # what the strict rule does in the planted case: the three copies score the radius exactly and stay out
    lims, _, I = right["equal scores f32"]
    eq = rc.case_equal()
    assert not np.isin(eq["copies"], I[lims[0]:lims[1]]).any()
    _, _, I2 = rc.range_search(*cases["equal scores f32"][0], wrong="non_strict")
    assert np.isin(eq["copies"], I2).all()
    # ascending rows inside every stretch, and the lists really interleave
    lims, _, I = right["interleaved lists"]
    assert all((np.diff(I[lims[j]:lims[j + 1]]) > 0).all() for j in range(5)) and lims[-1] > 100


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_restatement_equals_bruteforce_on_the_probed_and_admitted_rows(dtype):
    g = rc.case_round_robin(900, 32, 5, 6)
    mask = np.arange(900) % 3 != 1
    labels = (np.arange(900) // 7).astype(np.int32)
    ql = np.array([3, fc.LABEL_NONE, 40, 41, 100], np.int32)
    for nprobe in (1, 3, 6):
        r = _mid_radii(g, nprobe, dtype, frac=0.3)
        r[3], r[4] = np.float32(np.inf), np.float32(-np.inf)
        for kw in ({}, {"sel": mask}, {"labels": labels, "q_labels": ql, "mode": "exclude"}, {"sel": mask, "labels": labels, "q_labels": ql, "mode": "only"}):
            got = rc.range_search(*_base(g), r, nprobe, dtype, **kw)
            assert rc.same(got, rc.bruteforce(*_base(g), r, nprobe, dtype, **kw)), (nprobe, kw.keys())
            assert got[0][0] == 0 and got[0][4] == got[0][3] and len(got[1]) == got[0][-1]
    lims, D, I = rc.range_search(*_base(g), np.float32(0.5), 6, dtype, idx_offset=1000)         # a scalar radius, an offset
    assert rc.same((lims, D, I - 1000), rc.bruteforce(*_base(g), 0.5, 6, dtype))


def test_radius_for_count_and_the_size_classes():
    s = np.array([5, 3, 3, 1], np.float32)
    assert rc.radius_for_count(s, 0) == 5 and rc.radius_for_count(s, 1) == 3 and rc.radius_for_count(s, 2) is None
    assert rc.radius_for_count(s, 3) == 1 and np.isneginf(rc.radius_for_count(s, 4)) and rc.radius_for_count(s, 5) is None
    with open(os.path.join(ram._lib.CSRC, "ivf_range_math.hpp")) as f:
        text = f.read()
    assert "constexpr int kRangeSortLds = 4096;" in text and "constexpr int64_t kRangeSlice = 4096;" in text
    assert rc.SORT_LDS == 4096 and rc.SLICE == 4096 and [rc.sort_class(n) for n in (1, 2, 3, 4, 5, 4096, 4097)] == [1, 2, 4, 4, 8, 4096, 8192]


def test_stretch_case_plants_land_in_wave_0():
    c = rc.case_stretch()
    pos = {int(r): p for p, r in enumerate(c["big"])}
    seen = set()
    for cnt in rc.STRETCH_COUNTS:
        at = [pos[int(r)] for r in c["plant"][cnt]]
        assert len(at) == cnt == len(set(at)) and all(p % 256 < 64 for p in at) and not seen & set(at)
        seen |= set(at)
    for dtype in sc.STORAGES:
        lims, _, I = rc.range_search(c["rows"], c["q6"], c["assign"], c["centroids"], rc.STRETCH_RADIUS, 1, dtype)
        assert tuple(np.diff(lims)) == rc.STRETCH_COUNTS
        assert all(np.array_equal(I[lims[u]:lims[u + 1]], c["plant"][cnt]) for u, cnt in enumerate(rc.STRETCH_COUNTS))


def test_range_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "ivf_range_math_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivf_range_math_check.cpp"), "-o", exe])
    for seed in ("1", "20261020"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 1000000


def test_range_search_is_declared_listed_exported_and_bound():
    lib_ = ram._lib
    with open(lib_.HEADER_IVF_RANGE) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", code))
    assert declared == set(lib_.EXPORTS_IVF_RANGE) == {"mips_ivf_range_search", "mips_ivf_range_search_grp"}
    assert len(lib_.EXPORTS_IVF) == len(set(lib_.EXPORTS_IVF)) == 21 and len(lib_.EXPORTS) == 41             # the pinned lists stay
    assert not set(lib_.EXPORTS_IVF_RANGE) & (set(lib_.EXPORTS_IVF) | set(lib_.EXPORTS))
    head = ("mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, const float* radii, int64_t nprobe, int64_t* out_lims, "
            "float* out_scores, int64_t* out_idx, int64_t cap, int64_t idx_offset, int flags, ")
    tail = "const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels, int grp_mode, void* hip_stream"
    for name, rest in (("mips_ivf_range_search", "void* hip_stream"), ("mips_ivf_range_search_grp", tail)):
        m = re.search(rf"int {name}\(([^;]*)\);", code)
        assert m and re.sub(r"\s+", " ", m.group(1)) == head + rest, name
    assert re.search(r"#define MIPS_RADII_DEVICE 256\b", code) and lib_.RADII_DEVICE == 256
    assert "mips_ivf_range_search_sel" not in text                                                        # a bitmap alone is q_labels == NULL
    with open(lib_.HEADER_IVF) as f:
        ivf_text = f.read()
    assert "mips_hip_ivf_range.h" in ivf_text                                                              # the pointer, a comment only:
    assert "mips_ivf_range_search" not in re.sub(r"/\*.*?\*/", "", ivf_text, flags=re.S)                    # no declaration there
    assert lib_.HEADER_IVF_RANGE in lib_._sources()
    lib = lib_.load()
    for name in lib_.EXPORTS_IVF_RANGE:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", lib_.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mips_ivf_range_search$", out, flags=re.M) and re.search(r" T mips_ivf_range_search_grp$", out, flags=re.M)
    par = list(inspect.signature(ram.IvfIndex.range_search_probed).parameters)
    assert par == ["self", "x", "radius", "nprobe", "idx_offset", "selector", "groups", "group_mode", "sel_bit0"]
    assert list(inspect.signature(ram.IvfIndex.range_search_probed_into).parameters) == par[:3] + ["lims", "D", "I"] + par[3:]
    assert ram.IvfIndex.range_search is ram.IvfIndex.search                                                # the faiss-shaped form stays refused


def test_c_consumer_of_the_range_search_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_ivf_range_smoke.c"), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "c_abi_ivf_range_smoke.o")])


def test_range_kernels_registers_and_lds():
    """tools/kernel_regs.py (the code object's notes, no GPU): six range-scan instances (3 storages x filtered or not) with the list
    scan's LDS less its lists and counters -- 45 056 bytes, filtered 47 104 --, the place kernel without LDS, the order kernel with
    its 4096 (row, score) pairs; none with a spill or scratch; and still exactly 24 kernels whose name holds ivf_list_scan."""
    ram.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("llvm tools of the ROCm image not found")
    all_ks = kernel_regs.kernels()
    assert sum("ivf_list_scan" in k["demangled"] for k in all_ks) == 24
    ks = {k["demangled"]: k for k in all_ks if "ivf_range" in k["demangled"]}
    assert len(ks) == 8 and all(k["spill"] == 0 and k["scratch"] == 0 for k in ks.values()), ks
    pairs = ("mips::ElemF32, mips::ElemF32", "mips::ElemU8, mips::ElemBF16", "mips::ElemBF16, mips::ElemBF16")
    for p in pairs:
        assert ks[f"mips::ivf_range_scan_kernel<{p}, false>"]["lds"] == 8192 + 4 * 64 * 9 * 16
        assert ks[f"mips::ivf_range_scan_kernel<{p}, true>"]["lds"] == 8192 + 4 * 64 * 9 * 16 + 4 * 128 * 4
        assert ks[f"mips::ivf_range_scan_kernel<{p}, false>"]["vgpr"] <= 128 and ks[f"mips::ivf_range_scan_kernel<{p}, true>"]["vgpr"] <= 128
    assert ks["mips::ivf_range_place_kernel"]["lds"] == 0 and ks["mips::ivf_range_order_kernel"]["lds"] == rc.SORT_LDS * 8
