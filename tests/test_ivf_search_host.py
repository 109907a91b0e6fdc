"""IVF search, CPU side: the restatement of tests/ivf_search_cases.py agrees with the oracle's brute force over the admitted rows,
its deliberate mistake changes the tie case, csrc/ivf_search_math.hpp -- the text host and kernel compile -- holds its properties
under AddressSanitizer and UBSan and agrees with a Python restatement, mips_ivf_search is declared, listed and exported, and a
plain-C consumer compiles against the header.  The GPU tests are tests/test_gpu_ivf_search.py and test_gpu_ivf_search_graph.py."""
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
import ivf_search_cases as sc  # noqa: E402


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_restatement_equals_bruteforce_on_the_admitted_rows(dtype):
    case = iv.case_planted(40)
    assign = iv.nearest(case["rows"], case["centroids"])[:, 0]
    for k, nprobe in ((1, 1), (5, 2), (29, 3), (5, 8), (2, 100)):
        got = sc.search(case["rows"], case["q"], assign, case["centroids"], k, nprobe, dtype)
        want = sc.bruteforce_on_admitted(case["rows"], case["q"], assign, case["centroids"], k, nprobe, dtype)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    d1, i1 = sc.search(case["rows"], case["q"], assign, case["centroids"], 29, 1, dtype)
    empty = case["qlabels"] == 0                                                          # list 0 is empty: nothing but padding
    assert (i1[empty] == -1).all() and np.isneginf(d1[empty]).all()
    single = case["qlabels"] == 2                                                         # a list of one row: one result, then padding
    assert (i1[single][:, 0] >= 0).all() and (i1[single][:, 1:] == -1).all()
    _, off = sc.search(case["rows"], case["q"], assign, case["centroids"], 5, 2, dtype, idx_offset=1000)
    _, base = sc.search(case["rows"], case["q"], assign, case["centroids"], 5, 2, dtype)
    assert np.array_equal(off, np.where(base >= 0, base + 1000, -1))


def test_every_probed_list_gives_the_flat_result():
    case = iv.case_gauss(700, 24, 5, 6)
    c = iv.train(case["rows"], 6, 2)
    assign = iv.nearest(case["rows"], c)[:, 0]
    d, i = sc.search(case["rows"], case["q"], assign, c, 5, 6, "f32")
    es, ei = iv.orc.search_exact_bruteforce(case["q"], case["rows"], 5)
    assert np.array_equal(i, ei) and np.array_equal(d.view(np.uint32), es.view(np.uint32))


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_breaking_ties_by_list_position_changes_the_tie_case(dtype):
    case = sc.case_ties()
    args = (case["rows"], case["q"], case["assign"], case["centroids"], 29, 3, dtype)
    assert np.array_equal(iv.nearest(case["q"], case["centroids"], 3)[0], [0, 1, 2])
    d, i = sc.search(*args)
    assert np.array_equal(i[0], case["copies"][:29]) and (d[0] == d[0, 0]).all()           # the lowest 29 copies, ascending
    _, bad = sc.search(*args, wrong="list_position")
    assert not np.array_equal(bad, i) and set(bad[0]) <= set(case["copies"])
    # on a case without ties the mistake is invisible: it is the tie rule and nothing else
    plain = iv.case_planted(40)
    pa = iv.nearest(plain["rows"], plain["centroids"])[:, 0]
    a = sc.search(plain["rows"], plain["q"], pa, plain["centroids"], 5, 3, dtype)
    b = sc.search(plain["rows"], plain["q"], pa, plain["centroids"], 5, 3, dtype, wrong="list_position")
    assert np.array_equal(a[1], b[1])


def _segments(nq, p, k, cus):
    S = 1
    while S < 32 and nq * p * S < 2 * cus:
        S *= 2
    while S > 1 and p * S * k > 65536:
        S //= 2
    return S


def test_search_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "ivf_search_math_check"), str(tmp_path / "sizes.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivf_search_math_check.cpp"), "-o", exe])
    rng = np.random.default_rng(17)
    sizes = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(rng.integers(1, 5000, 60), rng.integers(1, 1025, 60), rng.integers(1, 30, 60),
                                                                    rng.choice([1, 64, 256, 304, 50000], 60))]
    lists = [(int(L), int(S)) for L, S in zip(rng.integers(0, 1 << 31, 40), rng.choice([1, 2, 4, 8, 16, 32], 40))] + [(0, 32), (1, 32), (31, 32), (65, 4)]
    with open(inp, "w") as f:
        f.write("".join(f"S {a} {b} {c} {d}\n" for a, b, c, d in sizes) + "".join(f"L {L} {S}\n" for L, S in lists))
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0].split()[0] == "ok" and int(lines[0].split()[1]) > 1000
    for (nq, p, k, cus), line in zip(sizes, lines[1:1 + len(sizes)]):
        assert line.split() == ["S", str(_segments(nq, p, k, cus)), str(min(4096, max(1, (256 << 20) // (p * k * 16))))]
    for (L, S), line in zip(lists, lines[1 + len(sizes):]):
        assert [int(v) for v in line.split()[1:]] == [L * s // S for s in range(S + 1)]


def test_search_is_declared_listed_and_exported():
    lib_ = ram._lib
    with open(lib_.HEADER_IVF) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", code))
    assert "mips_ivf_search" in declared and "mips_ivf_search" in lib_.EXPORTS_IVF
    assert declared == set(lib_.EXPORTS_IVF)
    m = re.search(r"int mips_ivf_search\(([^;]*)\);", code)
    assert m and re.sub(r"\s+", " ", m.group(1)) == ("mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, "
                                                    "int64_t* out_idx, int64_t idx_offset, int flags, void* hip_stream")
    assert "NOT IN THIS HEADER YET" not in text
    assert len(lib_.EXPORTS) == 41 and "MIPS_ABI_VERSION" not in text                   # one ABI version, the first header as it was
    assert hasattr(lib_.load(), "mips_ivf_search")
    assert callable(getattr(ram.IvfIndex, "search_probed"))


def test_c_consumer_of_the_search_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_ivf_search_smoke.c"), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "c_abi_ivf_search_smoke.o")])
