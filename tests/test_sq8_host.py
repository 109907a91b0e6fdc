"""8-bit scalar-quantised index, CPU side: the NumPy restatement of tests/sq8_cases.py rejects wrong kernels (each deliberate
mistake changes a result on its cases), csrc/sq8_quant.hpp -- the text the kernels compile -- holds its properties under
AddressSanitizer and UBSan and agrees with the restatement byte for byte, the new header is additive, and the Python layers parse
the factory strings.  The GPU tests are tests/test_gpu_sq8.py."""
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
import sq8_cases as sq  # noqa: E402


@pytest.fixture(scope="module")
def references():
    """(name, case, k, vmin, vdiff, codes, D, I) of every host case, computed once"""
    out = []
    for name, case, k in sq.host_cases():
        vmin, vdiff, codes = sq.prepared(case)
        D, I = sq.search(case["q"], codes, vmin, vdiff, k)
        out.append((name, case, k, vmin, vdiff, codes, D, I))
    return out


def test_cases_cover_what_they_claim(references):
    by = {r[0]: r for r in references}
    _, case, _, vmin, vdiff, codes, D, I = by["all_codes"]
    assert all(set(codes[:, j]) == set(range(256)) for j in range(codes.shape[1]))      # all 256 codes in every column
    assert (codes == 255).all(axis=1).any() and (codes == 0).all(axis=1).any()           # whole rows of 255 and of 0
    assert np.array_equal(codes[:256], case["levels"])                                   # decode(c) encodes back as c
    _, case, _, vmin, vdiff, codes, D, I = by["gauss"]
    assert vdiff[3] == 0 and (codes[:, 3] == 0).all()                                    # the constant column
    qp = sq.scaled_queries(case["q"], vdiff)
    assert (qp < 0).any() and (qp[:, 5] == 0).all() and (qp[:, 3] == 0).all()            # negative and zero s_j q_j
    assert (np.diff(D, axis=1) <= 0).all()                                               # D is monotone in S
    _, case, _, vmin, vdiff, codes, D, I = by["outside"]
    raw = sq.encode(case["rows"], vmin, vdiff, wrong="no_clamp")
    assert (raw != codes).mean() > 0.2                                                    # most added rows leave the trained range
    _, case, k, vmin, vdiff, codes, D, I = by["duplicates"]
    for j, copies in ((0, 3), (1, 70)):
        same = np.flatnonzero((codes == codes[I[j, 0]]).all(axis=1))
        assert len(same) == copies and np.array_equal(I[j, :min(k, copies)], same[:min(k, copies)])   # ties: lowest rows first
        assert (D[j, :min(k, copies)] == D[j, 0]).all()
    _, case, k, vmin, vdiff, codes, D, I = by["k_gt_n"]
    assert (I[:, 3:] == -1).all() and np.isneginf(D[:, 3:]).all() and (I[:, :3] >= 0).all()


@pytest.mark.parametrize("mistake", sq.MISTAKES)
def test_every_mistake_changes_a_result(references, mistake):
    changed = []
    for name, case, k, vmin, vdiff, codes, D, I in references:
        c = sq.encode(case["rows"], vmin, vdiff, wrong=mistake) if mistake in ("round_encode", "no_clamp") else codes
        d2, i2 = sq.search(case["q"], c, vmin, vdiff, k, wrong=mistake)
        if not (np.array_equal(i2, I) and np.array_equal(d2, D)):
            changed.append(name)
    assert changed, f"{mistake}: no case notices it"


def test_decode_is_the_inner_product_up_to_the_query_rounding(references):
    """D is <q, decoded row> up to the bf16 rounding of q' (relative 2^-9 per term) and float32 rounding"""
    name, case, k, vmin, vdiff, codes, D, I = references[0]
    dec = sq.decode(codes, vmin, vdiff).astype(np.float64)
    q = case["q"].astype(np.float64)
    s, _ = sq.scale_offset(vmin, vdiff)
    for j in range(len(q)):
        ip = dec[I[j]] @ q[j]
        bound = 2.0 ** -8 * (np.abs(q[j]) * s * 255.0).sum() + 1e-5 * np.abs(ip).max()
        assert np.abs(ip - D[j]).max() <= bound


def test_quant_header_under_asan_and_ubsan(tmp_path, references):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "sq8_quant_check"), str(tmp_path / "triples.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "sq8_quant_check.cpp"), "-o", exe])
    # the header's encode on the cases' own values (and the special values), against the NumPy restatement
    xs, mins, diffs = [], [], []
    for name, case, k, vmin, vdiff, codes, D, I in references:
        rows = case["rows"][:40]
        xs.append(rows.reshape(-1))
        mins.append(np.broadcast_to(vmin, rows.shape).reshape(-1))
        diffs.append(np.broadcast_to(vdiff, rows.shape).reshape(-1))
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30], dtype=np.float32)
    xs.append(special), mins.append(np.full(7, -1.5, np.float32)), diffs.append(np.full(7, 3.25, np.float32))
    x, vm, vd = (np.concatenate(a).astype(np.float32) for a in (xs, mins, diffs))
    with open(inp, "w") as f:
        for a, b, c in zip(x.view(np.uint32), vm.view(np.uint32), vd.view(np.uint32)):
            f.write(f"{a:x} {b:x} {c:x}\n")
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split()
    assert lines[0] == "ok" and int(lines[1]) > 100000
    got = np.array(lines[2:], dtype=np.int64)
    want = np.concatenate([sq.encode(a[None, :], b, c)[0] for a, b, c in zip(xs, mins, diffs)])
    assert np.array_equal(got, want)
    assert list(got[-7:]) == [0, 255, 0, 117, 117, 255, 0]          # NaN, +inf, -inf, +-0 = (1.5 / 3.25) * 255 truncated, the clamps


def test_header_is_additive():
    lib_ = ram._lib
    with open(lib_.HEADER_SQ8) as f:
        text = f.read()
    with open(lib_.HEADER) as f:
        main_text = f.read()
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(lib_.EXPORTS_SQ8) == {"mips_index_sq8_train", "mips_index_sq8_set_params", "mips_index_sq8_get_params",
                                                 "mips_index_sq8_is_trained"}
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text                 # one version, defined in the first header
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", main_text).group(1)) == lib_.ABI_VERSION == 1
    assert int(re.search(r"#define MIPS_DTYPE_SQ8 (\d+)", main_text).group(1)) == lib_.DTYPE_SQ8
    codes = [int(v) for v in re.findall(r"#define MIPS_DTYPE_[A-Z0-9_]+ (\d+)", main_text)]
    assert len(codes) == len(set(codes)) == 5                                                 # a code of its own
    assert not set(lib_.EXPORTS) & declared and len(lib_.EXPORTS) == 41                       # the first header declares what it did
    assert lib_.HEADER_SQ8 in lib_._sources()                                                 # a change of the header rebuilds the library
    lib = lib_.load()
    for name in lib_.EXPORTS_SQ8:
        assert hasattr(lib, name), name


def test_factory_strings():
    ix = faiss_shim.index_factory(64, "SQ8", faiss_shim.METRIC_INNER_PRODUCT)
    assert isinstance(ix, faiss_shim.IndexScalarQuantizer) and ix.d == 64 and ix.ntotal == 0
    assert isinstance(faiss_shim.IndexScalarQuantizer(64, faiss_shim.ScalarQuantizer.QT_8bit, faiss_shim.METRIC_INNER_PRODUCT), faiss_shim.IndexFlat)
    assert type(faiss_shim.index_factory(64, "Flat", faiss_shim.METRIC_INNER_PRODUCT)) is faiss_shim.IndexFlat
    for bad in ("IVF256,SQ8", "HNSW32", "PQ16", "IVF256,Flat", "SQ4", "IVF4096,PQ32"):
        with pytest.raises(NotImplementedError):
            faiss_shim.index_factory(64, bad, faiss_shim.METRIC_INNER_PRODUCT)
    with pytest.raises(NotImplementedError, match="inner product"):
        faiss_shim.index_factory(64, "SQ8", faiss_shim.METRIC_L2)
    with pytest.raises(NotImplementedError):
        faiss_shim.IndexScalarQuantizer(64, 5, faiss_shim.METRIC_INNER_PRODUCT)
    from retrieval_augmented_mds_amd import mips as mips_mod
    assert mips_mod.factory_dtype("SQ8", "f32") == "sq8" and mips_mod.factory_dtype("Flat", "f32") == "f32" and mips_mod.factory_dtype(None, "bf16") == "bf16"
    with pytest.raises(NotImplementedError):
        mips_mod.factory_dtype("IVF256,SQ8", "f32")


def test_sharded_index_refuses_sq8():
    with pytest.raises(NotImplementedError, match="sq8"):
        ram.ShardedMipsIndex(64, dtype="sq8")
