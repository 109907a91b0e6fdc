"""IVF index, CPU side: the cases of tests/ivf_cases.py are what they claim, its training restatement notices a centroid mean summed
in another order, csrc/ivf_math.hpp -- the text the kernels compile -- holds its properties under AddressSanitizer and UBSan and
agrees with the restatement bit for bit, the new header is additive, a plain-C consumer compiles against it, and the factory
strings still refuse IVF.  The GPU tests are tests/test_gpu_ivf.py."""
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
import ivf_cases as iv  # noqa: E402



def test_cases_cover_what_they_claim():
    case = iv.case_planted(48)
    assign = iv.nearest(case["rows"], case["centroids"])[:, 0]
    assert np.array_equal(assign, case["labels"])                                       # the planted lists are the lists
    assert tuple(np.bincount(assign, minlength=case["nlist"])) == iv.PLANTED_SIZES       # empty, several segments, 1 / 63 / 64 / 65
    assert np.array_equal(iv.nearest(case["q"], case["centroids"])[:, 0], case["qlabels"])
    P = iv.nearest(case["q"], case["centroids"], 3)
    assert (np.sort(P, axis=1)[:, 1:] != np.sort(P, axis=1)[:, :-1]).all()               # a query's probed lists are distinct
    case = iv.case_clustered(400, 64, 12, 4)
    c = iv.train(case["rows"], 4, 10)
    assert np.array_equal(iv.nearest(case["rows"], c)[:, 0], case["labels"])             # k-means finds the well-separated clusters
    assert np.array_equal(iv.nearest(case["q"], c)[:, 0], case["qlabels"])
    dup = iv.case_duplicates(300, 32, 4, 3)["rows"]
    c0 = iv.train(dup, 3, 0)
    assert np.array_equal(c0[0], c0[1]) and (iv.nearest(dup, c0)[:, 0] == 0).all()       # equal centroids: ties go to the lowest list


def test_summing_the_mean_in_another_order_changes_a_centroid():
    case = iv.case_cancel(300, 40)
    good, bad = iv.train(case["rows"], 1, 1), iv.train(case["rows"], 1, 1, wrong="sum_order")
    assert good[0, 0] != bad[0, 0] and np.array_equal(good[0, 1:], bad[0, 1:])


def test_training_restatement_properties():
    case = iv.case_gauss(700, 24, 4, 2)
    x = case["rows"]
    c0 = iv.train(x, 2, 0)
    assert np.array_equal(c0, iv.normalise(x[[0, 350]]))                                 # niter = 0: the normalised initial rows
    sub = iv.training_set(x, 2)
    assert len(sub) == 512 and np.array_equal(sub[3], x[3 * 700 // 512])                 # n > 256 nlist: evenly spaced rows
    z = np.zeros((1, 5), np.float32)
    assert np.array_equal(iv.normalise(z), z)
    off, rows = iv.list_table(np.array([2, 0, 2, 1, 0]), 4)
    assert list(off) == [0, 2, 3, 5, 5] and list(rows) == [1, 4, 3, 0, 2]


def test_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "ivf_math_check"), str(tmp_path / "vectors.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivf_math_check.cpp"), "-o", exe])
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((37, 101)) * np.exp(rng.uniform(-20, 20, (37, 1)))).astype(np.float32)
    x[5] = 0
    x[6, 1:] = 0
    with open(inp, "w") as f:
        f.write(f"{x.shape[0]} {x.shape[1]}\n" + " ".join(f"{v:08x}" for v in x.view(np.uint32).reshape(-1)) + "\n")
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0].split()[0] == "ok" and int(lines[0].split()[1]) >= 5
    bits = lambda line: np.array([int(v, 16) for v in line.split()], dtype=np.uint32)  # noqa: E731
    got = np.stack([bits(line) for line in lines[1:1 + len(x)]])
    assert np.array_equal(got, iv.normalise(x).view(np.uint32))
    pairs = np.arange(len(x) - 1)[:, None] + 1
    want = iv.orc.canonical_pairs(x[:-1], x, pairs).astype(np.float32)[:, 0]
    assert np.array_equal(bits(lines[1 + len(x)]), want.view(np.uint32))
    mean = (np.cumsum(x.astype(np.float64), axis=0)[-1] / np.float64(len(x))).astype(np.float32)
    assert np.array_equal(bits(lines[2 + len(x)]), mean.view(np.uint32))


def test_header_is_additive():
    lib_ = ram._lib
    with open(lib_.HEADER_IVF) as f:
        text = f.read()
    with open(lib_.HEADER) as f:
        main_text = f.read()
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(lib_.EXPORTS_IVF) and len(lib_.EXPORTS_IVF) == len(declared)
    assert {"mips_ivf_create", "mips_ivf_destroy", "mips_ivf_flat", "mips_ivf_train", "mips_ivf_is_trained", "mips_ivf_set_centroids",
            "mips_ivf_get_centroids", "mips_ivf_add", "mips_ivf_probe", "mips_ivf_remove", "mips_ivf_reset",
            "mips_ivf_list_sizes", "mips_ivf_read_assign", "mips_ivf_set_param"} <= declared
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text                 # one version, defined in the first header
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", main_text).group(1)) == lib_.ABI_VERSION == 1
    assert not set(lib_.EXPORTS) & declared and len(lib_.EXPORTS) == 41                       # the first header declares what it did
    assert lib_.HEADER_IVF in lib_._sources()                                                 # a change of the header rebuilds the library
    lib = lib_.load()
    for name in lib_.EXPORTS_IVF:
        assert hasattr(lib, name), name


def test_c_consumer_compiles_against_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_ivf_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "c_abi_ivf_smoke.o")])


def test_factory_strings_still_refuse():
    for bad in ("IVF256,SQ8", "IVF16,Flat", "IVF4096,PQ32"):
        with pytest.raises(NotImplementedError):
            faiss_shim.index_factory(64, bad, faiss_shim.METRIC_INNER_PRODUCT)
        with pytest.raises(NotImplementedError):
            ram.mips.factory_dtype(bad, "f32")
    assert isinstance(ram.IvfIndex, type)
