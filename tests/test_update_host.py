"""Rows overwritten in place by id, the parts that need no GPU: the header and its exports, the shared rules of csrc/update_math.hpp
run as a stand-alone program under AddressSanitizer and UBSan on every id set of tests/update_cases.py, and NumPy models showing
that each deliberately wrong restatement of tests/update_cases.py changes the outcome of at least one case -- i.e. that the GPU
tests of tests/test_gpu_update*.py, which compare with a fresh index of the right restatement's rows, can fail."""
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
try:
    import lifecycle_cases as lc
    import update_cases as uc
finally:
    sys.path.pop(0)


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return text, set(re.findall(r"\b(mips_[a-z0-9_]+)\s*\(", text))


# ------------------------------------------------------------------ 1. ABI and surface
def test_header_declares_and_library_exports_the_two_calls():
    lib_ = ram._lib
    text, declared = _declared(lib_.HEADER_WRITE)
    assert declared == set(lib_.EXPORTS_WRITE) == {"mips_index_update", "mips_ivf_update"}
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text       # one version, defined in the first header
    others = set(lib_.EXPORTS) | set(lib_.EXPORTS_UPDATE) | set(lib_.EXPORTS_ROWS) | set(lib_.EXPORTS_IVF) | set(lib_.EXPORTS_IVF_RANGE)
    assert not declared & others
    assert lib_.HEADER_WRITE in lib_._sources()                                     # a change of the header rebuilds the library
    for name in ("update_kernels.hpp", "host_update.hpp", "update_math.hpp"):
        assert os.path.join(lib_.CSRC, name) in lib_._sources()
    lib = lib_.load()
    assert len(lib.mips_index_update.argtypes) == len(lib.mips_ivf_update.argtypes) == 9


def test_python_surface():
    import inspect

    p = inspect.signature(ram.MipsIndex.update_rows).parameters
    assert p["idx_offset"].default == 0 and p["return_count"].default is False
    assert hasattr(ram.IvfIndex, "update_rows") and hasattr(ram.ShardedMipsIndex, "update_rows_global")
    assert hasattr(ram.faiss_shim.IndexFlat, "update_vectors") and hasattr(ram.faiss_shim.IndexScalarQuantizer, "update_vectors")
    assert hasattr(ram.KnowledgeBase, "update_rows") and hasattr(ram.Mips, "refresh_embeddings")


def test_the_math_header_has_no_hip_type_and_the_kernels_are_the_three_passes():
    math = open(os.path.join(ram._lib.CSRC, "update_math.hpp")).read()
    code = re.sub(r"//.*", "", math)
    assert "hip/" not in code and "hipStream" not in code and "__global__" not in code   # plain C++ behind one macro
    kern = open(os.path.join(ram._lib.CSRC, "update_kernels.hpp")).read()
    names = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", kern)
    assert sorted(names) == ["update_finish_kernel", "update_mark_kernel", "update_scatter_kernel"]
    assert "upd::local_row" in kern and "upd::wins" in kern                               # the one text of the id test and the winner rule


# ------------------------------------------------------------------ 2. the shared rules, stand-alone, under the sanitizers
def _id_cases():
    cases = []
    for ntotal in (uc.NTOTAL, 1, 7):
        for off in (0, uc.OFFSET, -5):
            for name, ids in uc.id_sets(uc.NTOTAL, off).items():      # (on the small indexes most ids name no row)
                cases.append((f"{name}-n{ntotal}-o{off}", ntotal, off, ids))
    cases.append(("empty index", 0, 0, np.array([0, -1, 5], np.int64)))
    cases.append(("extremes", 3, np.iinfo(np.int64).min, np.array([np.iinfo(np.int64).min + 2, np.iinfo(np.int64).max, 0], np.int64)))
    return cases


def test_math_program_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "update_math_check"), str(tmp_path / "cases.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "update_math_check.cpp"), "-o", exe])
    cases = _id_cases()
    with open(inp, "w") as f:
        for _, ntotal, off, ids in cases:
            f.write(" ".join(str(v) for v in [ntotal, off, len(ids)] + [int(i) for i in ids]) + "\n")
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ok, ncase, npos, nwin = out.stdout.split()
    want = sum(int(uc.winners(ids, off, ntotal).sum()) for _, ntotal, off, ids in cases)
    assert ok == "ok" and int(ncase) == len(cases) and int(npos) == sum(len(c[3]) for c in cases) and int(nwin) == want > 0
    with open(inp, "w") as f:                                          # the program refuses what is malformed
        f.write("10 0 3 1 2\n")
    assert subprocess.run([exe, inp], capture_output=True, text=True, timeout=60).returncode == 1


# ------------------------------------------------------------------ 3. the id sets are what the issue asks for
def test_id_sets_cover_the_edges():
    for off in (0, uc.OFFSET):
        sets = uc.id_sets(uc.NTOTAL, off)
        assert [len(sets[k]) for k in ("n0", "n1", "n64", "n65", "n1000")] == [0, 1, 64, 65, 1000]
        every = np.concatenate(list(sets.values()))
        local = uc.local_rows(every, off, uc.NTOTAL)
        assert 0 in local and uc.NTOTAL - 1 in local
        for junk in (-1, off + uc.NTOTAL, off + (1 << 32) + 3):
            assert junk in every and junk in sets["n65"]
        assert (every < off).any() and (sets["n1000"] == -1).any()
        for name in ("n65", "n1000"):
            loc = uc.local_rows(sets[name], off, uc.NTOTAL)
            vals, counts = np.unique(loc[loc >= 0], return_counts=True)
            assert counts.max() == 5, name                             # up to 5 copies of one id
        c = sets["n1000"]
        assert c[uc.SCATTER_BLOCK - 1] == c[uc.SCATTER_BLOCK] == c[uc.MARK_BLOCK - 1] == c[uc.MARK_BLOCK] == c[999]   # across both borders
        x = uc.new_rows(1000, 16)
        assert len(np.unique(x, axis=0)) == 1000                       # a row names its position


# ------------------------------------------------------------------ 4. every wrong restatement is rejected by a case
@pytest.mark.parametrize("wrong", uc.WRONG_LOOP)
def test_the_id_sets_reject_the_wrong_loops(wrong):
    base = uc.base_rows(uc.NTOTAL, 16)
    rejected = []
    for off in (0, uc.OFFSET):
        for name, ids in uc.id_sets(uc.NTOTAL, off).items():
            x = uc.new_rows(len(ids), 16)
            right, count = uc.apply_update(base, ids, x, off)
            assert count == int(uc.winners(ids, off, uc.NTOTAL).sum())
            bad, _ = uc.apply_update(base, ids, x, off, wrong)
            if not np.array_equal(right, bad):
                rejected.append((off, name))
    assert rejected, wrong
    if wrong == "offset_ignored":
        assert all(off != 0 for off, _ in rejected)
    if wrong == "truncate32":                                          # 2^32 + 3 was written to row 3
        ids = uc.id_sets(uc.NTOTAL, 0)["n65"]
        bad, _ = uc.apply_update(base, ids, uc.new_rows(65, 16), 0, wrong)
        assert not np.array_equal(bad[3], base[3]) and np.array_equal(uc.apply_update(base, ids, uc.new_rows(65, 16))[0][3], base[3])


def test_a_stale_bf16_image_loses_the_beacon():
    before, ids, x, q = uc.image_case()
    st = uc.State(before)
    right, wrong = st.updated(ids, x), st.updated(ids, x, wrong="image_stale")
    assert np.array_equal(right.rows, wrong.rows) and right.xmax2 == wrong.xmax2
    got, _ = uc.model_search(right, q)
    assert got[0] == ids[0]                                            # the truth: the beacon first
    bad, certified = uc.model_search(wrong, q)
    assert certified and ids[0] not in bad                             # certified without it


def test_a_stale_norm_bound_certifies_the_decoys():
    before, ids, x, queries = uc.norm_case()
    st = uc.State(before)
    right, wrong = st.updated(ids, x), st.updated(ids, x, wrong="xmax2_stale")
    assert right.xmax2 > 400 * wrong.xmax2 and np.array_equal(right.rows, wrong.rows)
    fam = lc.family(128)
    plant = set((lc.N_A + uc.PLACEHOLDERS + fam.b_plant_at).tolist())
    assert np.array_equal(right.rows, np.concatenate([fam.A, fam.R, fam.B]))              # the rows of the lifecycle step
    for q in queries:
        got, certified = uc.model_search(right, q)
        assert not certified and set(got.tolist()) <= plant            # flagged, settled exactly: planted rows only
        bad, certified = uc.model_search(wrong, q)
        assert certified and not set(bad.tolist()) & plant             # the wrong top-5, certified


def test_a_stale_phi_moves_every_distance():
    before, ids, x = uc.phi_case()
    st = uc.State(before)
    right, wrong = st.updated(ids, x), st.updated(ids, x, wrong="phi_stale")
    assert right.phi < wrong.phi / 1000 and right.phi == float(lc.orc.sumsq_canonical(lc.family(128).A).max())   # phi FELL
    fam = lc.family(128)
    ref = lc.Reference(fam.q, right.rows)
    assert (ref.values(1, wrong.phi) != ref.values(1, right.phi)).all()


def test_the_bounds_are_kept_as_upper_bounds():
    """A row that shrinks leaves the bound where it was: still a bound, and a larger e only flags more queries."""
    before, ids, x = uc.phi_case()
    st = uc.State(before)
    after = st.updated(ids, x)
    assert after.xmax2 == st.xmax2 >= lc.scalars(after.rows)[0] and after.dres2 >= lc.scalars(after.rows)[1]
