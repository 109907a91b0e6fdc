"""Filtered IVF search, CPU side: the restatement of tests/ivf_filter_cases.py agrees with the oracle's brute force over the admitted
rows, every deliberate mistake (`wrong=`) changes the result of at least one case -- so the cases bite --, csrc/ivf_filter_math.hpp
holds its properties under AddressSanitizer and UBSan, and mips_ivf_search_sel / _grp are declared, listed and bound.  The GPU tests
are tests/test_gpu_ivf_filter.py, test_gpu_ivf_filter_graph.py and test_gpu_ivf_facade.py."""
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
import ivf_search_cases as sc  # noqa: E402


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_restatement_equals_bruteforce_on_the_admitted_rows(dtype):
    c = fc.case_planted(40)
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    for k, nprobe in ((1, 1), (5, 2), (29, 3), (5, 8)):
        for kw in ({"sel": c["sel"]}, {"labels": c["row_labels"], "q_labels": c["q_labels"], "mode": "exclude"},
                   {"labels": c["row_labels"], "q_labels": c["q_labels"], "mode": "only"},
                   {"sel": c["sel_off"], "sel_bit0": 13, "labels": c["row_labels"], "q_labels": c["q_labels"], "mode": "exclude"}):
            assert _same(fc.search(*base, k, nprobe, dtype, **kw), fc.bruteforce_on_admitted(*base, k, nprobe, dtype, **kw)), (k, nprobe, kw.keys())
    assert _same(fc.search(*base, 5, 2, dtype), sc.search(*base, 5, 2, dtype))                       # no filter: the unfiltered restatement
    # a query labelled LABEL_NONE is not filtered
    none = c["q_labels"] == fc.LABEL_NONE
    assert none.any() and not none.all()
    got = fc.search(*base, 5, 2, dtype, labels=c["row_labels"], q_labels=c["q_labels"], mode="only")
    plain = sc.search(*base, 5, 2, dtype)
    assert np.array_equal(got[1][none], plain[1][none]) and not np.array_equal(got[1][~none], plain[1][~none])
    # a group that covers a whole list: excluded, nothing of the list is left; kept, all of it answers
    five = (c["qlabels"] == 5) & ~none
    d1, i1 = fc.search(*base, 29, 1, dtype, labels=c["row_labels"], q_labels=c["q_labels"], mode="exclude")
    assert five.any() and (i1[five] == -1).all() and np.isneginf(d1[five]).all()
    _, i2 = fc.search(*base, 29, 1, dtype, labels=c["row_labels"], q_labels=c["q_labels"], mode="only")
    assert (i2[five] >= 0).all() and (c["assign"][i2[five]] == 5).all()
    single = (c["qlabels"] == 2) & ~none                                                             # the list of one row, its own group
    assert (i1[single] == -1).all() and (i2[single][:, 0] >= 0).all() and (i2[single][:, 1:] == -1).all()


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_ties_under_a_bitmap_give_the_lowest_admitted_copies(dtype):
    c = fc.case_ties()
    d, i = fc.search(c["rows"], c["q"], c["assign"], c["centroids"], 29, 3, dtype, sel=c["sel"])
    assert np.array_equal(i[0], c["admitted_copies"][:29]) and (d[0] == d[0, 0]).all() and len(c["admitted_copies"]) == 30


def _cases_for_wrong():
    """(name, positional arguments, keyword arguments) of restatement calls, small enough for the CPU"""
    p = fc.case_planted(40)
    base = (p["rows"], p["q"], p["assign"], p["centroids"])
    grp = {"labels": p["row_labels"], "q_labels": p["q_labels"]}
    t = fc.case_ties()
    qc = fc.case_queue()
    qbase = (qc["rows"], qc["q"][:1], qc["assign"], qc["centroids"])
    out = [("planted exclude", base + (5, 2, "f32"), dict(grp, mode="exclude")),
           ("planted only", base + (5, 2, "f32"), dict(grp, mode="only")),
           ("planted bit0", base + (5, 2, "f32"), {"sel": p["sel_off"], "sel_bit0": 13}),
           ("ties bitmap", (t["rows"], t["q"], t["assign"], t["centroids"], 29, 3, "f32"), {"sel": t["sel"]})]
    out += [(f"queue {name}", qbase + (5, 1, "f32"), {"sel": m}) for name, m in qc["bitmaps"].items()]
    return out


def test_every_deliberate_mistake_is_rejected_by_a_case():
    cases = _cases_for_wrong()
    right = [fc.search(*a, **kw) for _, a, kw in cases]
    for wrong in fc.WRONG:
        hit = [name for (name, a, kw), want in zip(cases, right) if not _same(fc.search(*a, wrong=wrong, **kw), want)]
        assert hit, wrong
    # and each mistake is the rule it names: without a filter none of them changes anything
    p = fc.case_planted(40)
    plain = fc.search(p["rows"], p["q"], p["assign"], p["centroids"], 5, 2, "f32")
    for wrong in fc.WRONG:
        assert _same(fc.search(p["rows"], p["q"], p["assign"], p["centroids"], 5, 2, "f32", wrong=wrong), plain), wrong


def test_queue_case_counts():
    qc = fc.case_queue()
    big = qc["big"]
    assert len(big) == fc.QUEUE_BIG and len(qc["rows"]) == fc.QUEUE_N
    in_list = {r: t for t, r in enumerate(big)}
    for cnt in fc.QUEUE_COUNTS:
        rows = np.flatnonzero(qc["bitmaps"][f"c{cnt}"])
        assert len(rows) == cnt and all(in_list[r] % 256 < 64 for r in rows)                        # all in wave 0's stretch of one segment
    assert np.array_equal(np.flatnonzero(qc["bitmaps"]["first64"]), np.sort(big[:64]))
    assert fc.segments(512, 1, 5) == 1 and fc.segments(1, 1, 5) == 32
    assert (sc.iv.nearest(qc["q"], qc["centroids"], 1) == 0).all()


def test_filter_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "ivf_filter_math_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivf_filter_math_check.cpp"), "-o", exe])
    for seed in ("1", "20261020"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 100000


def test_filtered_search_is_declared_listed_and_bound():
    lib_ = ram._lib
    with open(lib_.HEADER_IVF) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", code))
    assert {"mips_ivf_search_sel", "mips_ivf_search_grp"} <= declared and declared == set(lib_.EXPORTS_IVF)
    tail = "const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, "
    head = ("mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, float* out_scores, int64_t* out_idx, "
            "int64_t idx_offset, int flags, ")
    for name, rest in (("mips_ivf_search_sel", tail + "void* hip_stream"), ("mips_ivf_search_grp", tail + "const int32_t* q_labels, int grp_mode, void* hip_stream")):
        m = re.search(rf"int {name}\(([^;]*)\);", code)
        assert m and re.sub(r"\s+", " ", m.group(1)) == head + rest, name
    lib = lib_.load()
    assert hasattr(lib, "mips_ivf_search_sel") and hasattr(lib, "mips_ivf_search_grp")
    import inspect

    par = inspect.signature(ram.IvfIndex.search_probed).parameters
    assert list(par)[:8] == ["self", "x", "k", "nprobe", "idx_offset", "selector", "groups", "group_mode"]
    assert all(callable(getattr(ram.IvfIndex, n)) for n in ("set_labels", "labels", "labels_of"))
    assert ram.MipsArgs().mips_nlist == 0
