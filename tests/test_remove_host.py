"""Row removal, the parts that need no GPU: the third header and its export, the native plan run as a stand-alone program under
AddressSanitizer and UBSan on every pattern of tests/remove_cases.py, the shard renumbering, the shim's selectors as removal masks,
and NumPy models on the planted rows of tests/lifecycle_cases.py showing what a removal that forgot to invalidate phi or the bf16
image of an fp32-exact index would answer -- i.e. that the GPU tests of tests/test_gpu_remove.py can fail."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import lifecycle_cases as lc
    import remove_cases as rm
finally:
    sys.path.pop(0)


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return text, set(re.findall(r"\b(mips_[a-z0-9_]+)\s*\(", text))


# ------------------------------------------------------------------ 1. ABI pins
def test_third_header_declares_and_library_exports_the_removal():
    text, declared = _declared(os.path.join(ROOT, "include", "mips_hip_update.h"))
    assert re.search(r"\bint\s+mips_index_remove\s*\(", text)
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text     # one version, defined in the first header
    assert set(ram._lib.EXPORTS_UPDATE) == declared == {"mips_index_remove"}
    _, main_declared = _declared(os.path.join(ROOT, "include", "mips_hip.h"))
    _, sharded_declared = _declared(os.path.join(ROOT, "include", "mips_hip_sharded.h"))
    assert set(ram._lib.EXPORTS) == main_declared and len(ram._lib.EXPORTS) == 41  # the two old headers are as they were
    assert set(ram._lib.EXPORTS_SHARDED) == sharded_declared and len(sharded_declared) == 1
    assert not declared & (main_declared | sharded_declared)
    lib = ram._lib.load()                                                          # builds, loads and binds
    assert len(lib.mips_index_remove.argtypes) == 7
    assert ram._lib.HEADER_UPDATE in ram._lib._sources()                           # a change of the header rebuilds the library
    for name in ("remove_kernels.hpp", "host_remove.hpp", "remove_plan.hpp"):
        assert os.path.join(ram._lib.CSRC, name) in ram._lib._sources()


def test_python_surface():
    import inspect

    assert inspect.signature(ram.MipsIndex.remove_ids).parameters["sel_bit0"].default == 0
    assert hasattr(ram.faiss_shim.IndexFlat, "remove_ids") and hasattr(ram.ShardedMipsIndex, "remove_ids_global")
    assert hasattr(ram.KnowledgeBase, "remove_rows") and hasattr(ram.KnowledgeBase, "drop_near_duplicates")
    assert "shard_offsets" in ram.__all__ and callable(ram.shard_offsets)


def test_gather_kernels_are_not_scan_kernels_and_the_plan_header_has_no_hip():
    import scan_recipes as sr

    text = open(os.path.join(ram._lib.CSRC, "remove_kernels.hpp")).read()
    names = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", text)
    assert sorted(names) == ["remove_gather_kernel", "remove_gather_labels_kernel", "remove_stage_kernel"]
    assert not any(("mips::" + n).startswith(sr.SCAN_PREFIXES) for n in names)
    plan = open(os.path.join(ram._lib.CSRC, "remove_plan.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", plan).lower()                          # plain host code on vectors


# ------------------------------------------------------------------ 2. the plan, stand-alone, under the sanitizers
def _plan_cases():
    lines = []
    for W in (128, 384):
        for n in sorted(set(rm.sizes(W)) | set(rm.sizes())):
            for name, mask in rm.patterns(n, W).items():
                lines.append((f"W{W}-n{n}-{name}", W, n, mask))
    n = 5 * 384 + 37
    for name, mask in rm.patterns(n, 384).items():                                 # one window larger than the index (the default)
        lines.append((f"W43648-n{n}-{name}", 43648, n, mask))
    lines.append(("empty", 128, 0, np.zeros(0, bool)))
    return lines


def test_plan_program_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, inp = str(tmp_path / "remove_plan_check"), str(tmp_path / "cases.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "remove_plan_check.cpp"), "-o", exe])
    cases = _plan_cases()
    with open(inp, "w") as f:
        for _, W, n, mask in cases:
            f.write(f"{W} {n} {''.join('1' if m else '0' for m in mask) or '-'}\n")
    out = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ok, ncase, nmoves, ndirect, nbounce = out.stdout.split()
    assert ok == "ok" and int(ncase) == len(cases)
    assert int(ndirect) > 0 and int(nbounce) > 0 and int(ndirect) + int(nbounce) == int(nmoves)   # both paths were planned
    # the program refuses a plan that is wrong: the same check on a deliberately malformed case
    with open(inp, "w") as f:
        f.write("100 5 00000\n")
    assert subprocess.run([exe, inp], capture_output=True, text=True, timeout=60).returncode == 1


def test_numpy_model_and_counts():
    n, W = 5 * 384 + 37, 384
    x = rm.rows_for(n, 100, "bf16")
    assert len(np.unique(x, axis=0)) == n                                          # every row names itself
    for storage in ("bf16", "fp8_e4m3"):
        y = rm.rows_for(300, 64, storage)
        assert np.array_equal(lc.stored_rows(y, storage), y)                       # exactly representable in every storage
    labels = np.arange(n) % 11
    for name, mask in rm.patterns(n, W).items():
        rows, lab, nlab = rm.expected(x, labels, 1000, mask)
        assert len(rows) == n - mask.sum() == sum(rm.window_counts(mask, W)) and nlab == len(lab) == (~mask[:1000]).sum(), name
        assert np.array_equal(rows, np.array([x[i] for i in range(n) if not mask[i]]).reshape(-1, 100))
    m = rm.patterns(n, W)["run_3w5"]
    assert rm.window_counts(m, W)[1:5] == [11, 0, 0, W - 16]                        # bounce, nothing, nothing, then direct
    bm = rm.bitmap(m, bit0=13, pad_bits=5)
    assert np.array_equal(np.unpackbits(bm, bitorder="little")[13:13 + n].astype(bool), m) and bm[0] == 0xFF


# ------------------------------------------------------------------ 3. the shard renumbering
def test_shard_offsets():
    assert ram.shard_offsets([5, 0, 7], 0) == (0, 5, 12)
    assert ram.shard_offsets([5, 0, 7], 1) == (5, 5, 12)                           # an emptied shard
    assert ram.shard_offsets([5, 0, 7], 2) == (5, 12, 12)
    assert ram.shard_offsets([0], 0) == (0, 0, 0)
    n, world = 1003, 3
    even = [b - a for a, b in (ram.shard_bounds(n, world, r) for r in range(world))]
    for r in range(world):                                                         # before any removal: the even partition
        assert ram.shard_offsets(even, r) == (*ram.shard_bounds(n, world, r), n)
    mask = rm.patterns(n, 128)["random_50pct"]
    left = [int((~mask[a:b]).sum()) for a, b in (ram.shard_bounds(n, world, r) for r in range(world))]
    spans = [ram.shard_offsets(left, r) for r in range(world)]
    assert spans[0][0] == 0 and all(spans[r][1] == spans[r + 1][0] for r in range(world - 1)) and spans[-1][1] == spans[-1][2] == (~mask).sum()
    for bad in ([1, -1], []):
        with pytest.raises(ValueError):
            ram.shard_offsets(bad, 0)
    with pytest.raises(ValueError):
        ram.shard_offsets([1, 2], 2)


# ------------------------------------------------------------------ 4. the shim's selectors as removal masks
def test_id_selectors_become_removal_masks():
    fs = ram.faiss_shim
    n = 50
    m = fs.removal_mask(fs.IDSelectorRange(10, 20), n)
    assert m.dtype == np.bool_ and m.shape == (n,) and np.flatnonzero(m).tolist() == list(range(10, 20))
    ids = np.array([3, 3, 49, 7, -1, 50, 10 ** 9], np.int64)                       # duplicates; ids the index does not hold
    assert np.flatnonzero(fs.removal_mask(ids, n)).tolist() == [3, 7, 49]
    assert np.array_equal(fs.removal_mask(fs.IDSelectorBatch(ids), n), fs.removal_mask(ids, n))
    assert np.array_equal(fs.removal_mask(fs.IDSelectorArray(len(ids), ids), n), fs.removal_mask(ids, n))
    bm = np.packbits(np.arange(n) % 3 == 0, bitorder="little")
    assert np.array_equal(fs.removal_mask(fs.IDSelectorBitmap(bm), n), np.arange(n) % 3 == 0)
    assert np.array_equal(fs.removal_mask(fs.IDSelectorNot(fs.IDSelectorRange(0, 45)), n), np.arange(n) >= 45)
    assert fs.removal_mask(fs.IDSelectorAll(), n).all() and not fs.removal_mask(np.zeros(0, np.int64), n).any()
    ix = fs.IndexFlat(8, fs.METRIC_INNER_PRODUCT)                                  # an index that holds nothing removes nothing
    assert ix.remove_ids(ids) == 0 and ix.remove_ids(fs.IDSelectorAll()) == 0


# ------------------------------------------------------------------ 5. what a forgotten invalidation would answer
def _first_life(fam):
    return np.concatenate([fam.A, fam.R, fam.B])


@pytest.mark.parametrize("d", lc.DIMS)
def test_a_stale_phi_changes_every_l2_score(d):
    """The big rows (block B, norm ~10^3) leave: phi falls by a factor ~S^2 / 2, and an L2 distance computed with the old one
    differs from the true one in its float32 bits for every (query, row) pair the model looks at."""
    fam = lc.family(d)
    for storage in ("bf16", "f32"):
        q = lc.stored_queries(fam.q, storage)
        before = lc.Reference(q, lc.stored_rows(_first_life(fam), storage))
        after = lc.Reference(q, lc.stored_rows(np.concatenate([fam.A, fam.R]), storage))
        assert before.local_phi > 400 * after.local_phi                            # ~ S^2 / 2 >= 512: a big row against an R row
        stale, true = after.values(1, before.local_phi), after.values(1)
        assert (stale.view(np.int32) != true.view(np.int32)).all()
        # removing only the PLANTED big rows leaves the decoys, which are as long: phi must then stay, bit for bit
        gone = np.zeros(len(fam.B), bool)
        gone[fam.b_plant_at] = True
        decoys_left = lc.Reference(q, lc.stored_rows(np.concatenate([fam.A, fam.R, fam.B[~gone]]), storage))
        assert decoys_left.local_phi == before.local_phi


@pytest.mark.parametrize("d", lc.DIMS)
def test_a_stale_bf16_image_ranks_wrong_rows(d):
    """fp32-exact index, stage 1 of the two-stage search: it scans the bf16 image rows_hi.  R's planted rows leave and the rows
    behind them move up; an image that was neither compacted nor converted again still holds, at row i, the bf16 of the row
    that USED to be there.  For the R-planted queries the 32 best candidates of such a scan (the widest pool of search()) miss
    rows of the true top-5, whose scores no exact re-score of the pool can then bring back."""
    fam = lc.family(d)
    old = _first_life(fam)
    gone = np.zeros(len(old), bool)
    gone[len(fam.A) + fam.r_plant_at] = True
    new = old[~gone]
    ref = lc.Reference(fam.q, new)
    _, true_i = ref.topk(lc.K_SEARCH, 0)
    stale = lc.scan_scores(fam.q, old[:len(new)])                                  # what the stale image answers, by position
    fresh = lc.scan_scores(fam.q, new)
    missed = 0
    for j in fam.r_queries:
        pool_stale = set(np.argsort(-stale[j], kind="stable")[:max(lc.POOLS)].tolist())
        pool_fresh = set(np.argsort(-fresh[j], kind="stable")[:max(lc.POOLS)].tolist())
        assert set(true_i[j].tolist()) <= pool_fresh                               # the true image finds them
        missed += len(set(true_i[j].tolist()) - pool_stale)
    assert missed >= len(fam.r_queries)                                            # at least one true result lost per planted query
    # and the rows before the first removed one did not move: converting from there on is enough
    first = int(np.flatnonzero(gone)[0])
    assert np.array_equal(synth.round_to_bf16(old[:first]), synth.round_to_bf16(new[:first]))
