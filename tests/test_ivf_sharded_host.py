"""The row-sharded IVF index, the parts that need no GPU: the new header, its exports and bindings; csrc/ivf_sharded_math.hpp under
AddressSanitizer and UBSan in a stand-alone program; the cases of tests/ivf_sharded_cases.py and their restatements (parts + merge
equal the UNSHARDED restatement bit for bit, every deliberate mistake is rejected, no SQ8 family holds a pair with equal D and
different S); and ShardedIvfIndex on the ranks of a gloo group, world 2 and 3, with the NumPy restatements injected for the local
steps and the merges -- partition, selector bit offsets, pack, all-gather, merge and the training checksum.  Every comparison is bit
for bit, on every rank.  The GPU tests are tests/test_gpu_ivf_sharded.py."""
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
import ivf_range_cases as rg  # noqa: E402
import ivf_sharded_cases as shc  # noqa: E402
import ivf_wide_cases as wc  # noqa: E402
import range_cases as rc  # noqa: E402
import sq8_cases as sq  # noqa: E402


# ------------------------------------------------------------------ 1. ABI pins
def test_header_declares_what_the_binding_lists_and_the_library_exports():
    lib_ = ram._lib
    text = open(lib_.HEADER_IVF_SHARDED).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mips_[a-z0-9_]+)\(", code))
    assert declared == set(lib_.EXPORTS_IVF_SHARDED) == {"mips_ivf_search_part", "mips_ivf_merge_parts"}
    assert '#include "mips_hip_ivf.h"' in text and "MIPS_ABI_VERSION" not in text
    assert len(lib_.EXPORTS_IVF) == 21 and len(lib_.EXPORTS) == 41 and set(lib_.EXPORTS_SHARDED) == {"mips_range_merge_records"}   # the pinned lists stay
    grp = ("const uint8_t* sel_bits, int64_t sel_nbits, int64_t sel_bit0, const int32_t* q_labels, int grp_mode, void* hip_stream")
    m = re.search(r"int mips_ivf_search_part\(([^;]*)\);", code)
    assert m and re.sub(r"\s+", " ", m.group(1)) == ("mips_ivf_t* ivf, const void* q, int q_dtype, int64_t nq, int k, int64_t nprobe, int64_t* out_packed, "
                                                      "double* out_bias, int64_t idx_offset, int flags, " + grp)
    m = re.search(r"int mips_ivf_merge_parts\(([^;]*)\);", code)
    assert m and re.sub(r"\s+", " ", m.group(1)) == ("const int64_t* gathered, int parts, int64_t nq, int k, const double* bias, float* out_scores, "
                                                      "int64_t* out_idx, int device, void* hip_stream")
    assert lib_.HEADER_IVF_SHARDED in lib_._sources()                       # a change of the header rebuilds the library
    lib = lib_.load()                                                       # builds, loads and binds
    assert len(lib.mips_ivf_search_part.argtypes) == 16 and len(lib.mips_ivf_merge_parts.argtypes) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", lib_.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mips_ivf_search_part$", out, flags=re.M) and re.search(r" T mips_ivf_merge_parts$", out, flags=re.M)
    # what mips_ivf_search* accept is unchanged: the refusal of MIPS_OUT_PACKED is still in the text of the wide search
    assert "MIPS_OUT_PACKED is not served on an IVF index" in open(os.path.join(lib_.CSRC, "host_ivf.hpp")).read()


def test_python_surface():
    assert ram.ShardedIvfIndex is ram.sharded_ivf.ShardedIvfIndex and "ShardedIvfIndex" in ram.__all__ and callable(ram.ivf_merge_parts)
    p = inspect.signature(ram.ShardedIvfIndex.__init__).parameters
    assert list(p)[1:6] == ["d", "nlist", "dtype", "group", "device"] and p["dtype"].default == "bf16"
    assert all(p[n].default is None for n in ("local_search", "merge", "local_range_search", "range_merge"))
    p = inspect.signature(ram.ShardedIvfIndex.search_probed).parameters
    assert list(p)[1:] == ["q", "k", "nprobe", "selector", "groups", "group_mode"]
    assert ram.ShardedIvfIndex.search_probed_wide is ram.ShardedIvfIndex.search_probed
    assert list(inspect.signature(ram.ShardedIvfIndex.range_search_probed).parameters)[1:] == ["q", "radius", "nprobe", "selector", "groups", "group_mode"]
    assert "part_cap" in inspect.signature(ram.ShardedIvfIndex.range_search_probed_into).parameters
    for name in ("train_global", "set_trained", "add_global", "set_labels_global", "update_rows_global", "list_sizes_global", "centroids", "save", "load",
                 "reconstruct_batch", "check_trained_global"):
        assert callable(getattr(ram.ShardedIvfIndex, name)), name
    assert not hasattr(ram.ShardedIvfIndex, "remove_ids_global")            # out of scope, and said so
    with pytest.raises(NotImplementedError):
        ram.ShardedMipsIndex(64, dtype="sq8")                               # the flat sharded index still refuses SQ8
    with pytest.raises(ValueError):
        ram.ShardedIvfIndex(64, 4, local_search=lambda *a, **k: None)       # a local step without its merge
    assert ram.sharded_ivf.shard_bounds is ram.shard_bounds
    for n, world in ((1000, 3), (4, 3), (1000, 2), (0, 2)):
        assert shc.bounds(n, world) == [ram.shard_bounds(n, world, r) for r in range(world)]
    assert shc.bounds(1000, 3) == [(0, 334), (334, 668), (668, 1000)] and shc.bounds(4, 3) == [(0, 2), (2, 4), (4, 4)]


def test_training_checksum_sees_every_bit():
    cen = shc.case("tiny")["centroids"]
    a = ram.sharded_ivf.training_checksum(cen)
    assert a == ram.sharded_ivf.training_checksum(cen.copy()) and -(1 << 63) <= a < (1 << 63)
    other = cen.copy()
    other[1, 63] = np.float32(-0.0)                                         # +0.0 -> -0.0: one bit
    assert ram.sharded_ivf.training_checksum(other) != a
    p = (np.zeros(64, np.float32), np.ones(64, np.float32))
    assert ram.sharded_ivf.training_checksum(cen, p) != a
    assert ram.sharded_ivf.training_checksum(cen, (p[0], np.nextafter(p[1], 2).astype(np.float32))) != ram.sharded_ivf.training_checksum(cen, p)


# ------------------------------------------------------------------ 2. the payload arithmetic, sanitised
def test_sharded_math_header_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "ivf_sharded_math_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ivf_sharded_math_check.cpp"), "-o", exe])
    for seed in ("1", "20261021"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) > 500000
    text = open(os.path.join(ram._lib.CSRC, "ivf_sharded_math.hpp")).read()
    assert "constexpr int64_t kPartsMergeLimit = 65536;" in text and "row < 0 ? row : row + idx_offset" in text


def test_c_consumer_of_the_new_header_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "c_abi_ivf_sharded_smoke.c"), "-I",
                           os.path.join(ROOT, "include"), "-o", str(tmp_path / "c_abi_ivf_sharded_smoke.o")])


def test_pack_agrees_with_the_packages_layout():
    import torch

    S = np.array([[1.5, -2.0, -0.0, -np.inf]], np.float32)
    I = np.array([[7, 1 << 40, 3, -1]], np.int64)
    mine = shc.pack(S, I)
    theirs = ram.pack_topk(torch.from_numpy(S), torch.from_numpy(I)).numpy()
    assert (mine[..., 0] >= 0).all() and (theirs[0, 1, 0] < 0)              # zero-extended here, sign-extended there ...
    assert np.array_equal(mine[..., 0] & 0xFFFFFFFF, theirs[..., 0] & 0xFFFFFFFF) and np.array_equal(mine[..., 1], theirs[..., 1])
    for g in (mine, theirs):                                                # ... and one merge reads both: the low 32 bits
        assert shc.same(shc.merge_parts(g[None], 1, 1, 4), (np.array([[1.5, -0.0, -2.0, -np.inf]], np.float32), np.array([[7, 3, 1 << 40, -1]], np.int64)))


# ------------------------------------------------------------------ 3. the cases and their restatements
def test_the_cases_hold_what_they_promise():
    c = shc.case("planted")
    assert np.array_equal(c["assign"], c["planted"])                       # add() assigns what was planted
    assert set(np.flatnonzero(c["assign"] == 7)) == set(shc.SHORT_LIST[1]) and set(np.flatnonzero(c["assign"] == 6)) == set(shc.ONE_SHARD_LIST[1])
    for world in (2, 3):
        b = shc.bounds(shc.PLANTED_N, world)
        owners = lambda rows: {next(r for r, (lo, hi) in enumerate(b) if lo <= i < hi) for i in rows}
        assert owners(shc.ONE_SHARD_LIST[1]) == {world - 1} and owners(shc.SHORT_LIST[1]) == {0}          # a list whose rows all sit in one shard
        assert owners(shc.BORDER_COPIES) == set(range(world))                                             # the copies reach every rank
    assert [hi - lo for lo, hi in shc.bounds(1000, 3)] == [334, 334, 332]
    d, i = shc.expected(c, "f32", 5, 1)
    assert i[0].tolist()[3:] == [-1, -1] and sorted(i[0, :3].tolist()) == [10, 11, 12] and np.isneginf(d[0, 3:]).all()    # padding to survive
    d, i = shc.expected(c, "f32", 5, 1)
    assert i[2].tolist() == list(shc.BORDER_COPIES[:5]) and (d[2] == d[2, 0]).all()                        # ties: the lowest global rows, ascending
    d, i = shc.expected(c, "f32", 5, 1, "selector")
    assert i[2].tolist()[:3] == list(shc.BORDER_COPIES[1::2])                                              # ... and the admitted ones under the selector
    t = shc.case("tiny")
    assert [hi - lo for lo, hi in shc.bounds(4, 3)] == [2, 2, 0] and t["nlist"] == 2 and sorted(np.bincount(t["assign"]).tolist()) == [2, 2]
    assert shc.case("768")["rows"].shape == (300, 768) and shc.case("trained")["rows"].shape == (3000, 64)
    assert all(len(shc.case(n)["q"]) <= 9 and 2 <= shc.case(n)["nlist"] <= 8 for n in ("planted", "trained", "tiny", "768"))


@pytest.mark.parametrize("dtype", shc.STORAGES)
@pytest.mark.parametrize("name,world", [("planted", 2), ("planted", 3), ("tiny", 3), ("trained", 3), ("768", 2)])
def test_parts_and_merge_equal_the_unsharded_restatement(name, world, dtype):
    c = shc.case(name)
    nlist = c["nlist"]
    combos = [(1, 1, "plain"), (5, 1, "plain"), (5, 3, "selector"), (29, 3, "exclude"), (30, nlist, "only"), (100, nlist + 5, "both"), (5, 1, "both")]
    for k, nprobe, flt in combos:
        want = shc.expected(c, dtype, k, nprobe, flt)
        assert shc.same(shc.sharded_search(c, dtype, world, k, nprobe, flt), want), (k, nprobe, flt)
    if name == "tiny":
        assert (want[1][:, 4:] == -1).all()


def test_every_deliberate_mistake_is_rejected_by_a_case():
    c = shc.case("planted")
    hits = {}
    for wrong in shc.WRONG:
        hits[wrong] = [(world, flt) for world in (2, 3) for flt in ("plain", "selector")
                       if not shc.same(shc.sharded_search(c, "f32", world, 5, 3, flt, wrong=wrong), shc.expected(c, "f32", 5, 3, flt))]
    assert set(hits["no_idx_offset"]) == {(2, "plain"), (2, "selector"), (3, "plain"), (3, "selector")}
    assert set(hits["sel_bit0_zero"]) == {(2, "selector"), (3, "selector")}                               # (nothing to misread without a selector)
    assert hits["merge_on_D"] == []                                                                       # (an f32 index has no D)
    # the SQ8 rule: only the pair with equal D and different S tells a merge on D from the merge on S
    t = shc.case("sq8_tie")
    k, nlist = t["tie"]["k"], t["nlist"]
    want = shc.expected(t, "sq8", k, nlist)
    for world in (2, 3):
        assert shc.same(shc.sharded_search(t, "sq8", world, k, nlist), want)
        assert not shc.same(shc.sharded_search(t, "sq8", world, k, nlist, wrong="merge_on_D"), want)
        assert shc.same(shc.sharded_search(t, "sq8", world, t["tie"]["rank"], nlist, wrong="merge_on_D"), shc.expected(t, "sq8", t["tie"]["rank"], nlist))


def test_the_sq8_tie_case_holds_equal_D_with_different_S_across_shards():
    """Two rows with equal D and different S, the higher S at the higher row, on different ranks of 3: what tells a merge on D from
    the merge on S.  sq8_cases.case_gauss produces such pairs at some seeds and widths (this one at 3000 x 768, seed 2); the small
    d = 64 cases of this file hold none, which is why the pair has a case of its own."""
    t = shc.case("sq8_tie")
    j, (hi_row, lo_row), rank, k = t["tie"]["query"], t["tie"]["rows"], t["tie"]["rank"], t["tie"]["k"]
    X, Y, bias = shc.sc.stored(t["rows"], t["q"], "sq8", t["sq8_params"])
    S = shc.orc.canonical_pairs(Y[j:j + 1], X, np.array([[hi_row, lo_row]], np.int64))[0].astype(np.float32)
    D = (S.astype(np.float64) + bias[j]).astype(np.float32)
    assert S[0] > S[1] and D[0] == D[1] and hi_row > lo_row
    assert t["assign"][hi_row] != t["assign"][lo_row]                                                    # different lists
    owner = lambda row, world: next(r for r, (a, b) in enumerate(shc.bounds(3000, world)) if a <= row < b)
    assert (owner(hi_row, 3), owner(lo_row, 3)) == (1, 0)
    d, i = shc.expected(t, "sq8", k, t["nlist"])
    assert i[j, rank:rank + 2].tolist() == [hi_row, lo_row] and d[j, rank] == d[j, rank + 1] and rank + 2 <= k <= 1024
    assert shc.equal_D_different_S_pairs(t["rows"], t["q"], t["sq8_params"]) == 1
    assert [shc.equal_D_different_S_pairs(shc.case(n)["rows"], shc.case(n)["q"], shc.case(n)["sq8_params"]) for n in ("planted", "trained")] == [0, 0]


@pytest.mark.parametrize("dtype", shc.STORAGES)
def test_part_ranges_merge_to_the_unsharded_range_result(dtype):
    c = shc.case("planted")
    nq = len(c["q"])
    for world in (2, 3):
        for nprobe, flt in ((1, "plain"), (3, "both"), (8, "only")):
            radii = shc.radii_for(c, dtype, nprobe, flt)
            want = shc.expected_range(c, dtype, radii, nprobe, flt)
            parts = [shc.part_range(c, dtype, lo, hi, radii, nprobe, flt) for lo, hi in shc.bounds(len(c["rows"]), world)]
            stride = max(int(p[0][-1]) for p in parts) + 1
            got = rc.merge_records(rc.gather(parts, stride), world, nq, stride)
            assert rg.same(got, want) and int(want[0][-1]) > 0, (world, nprobe, flt)


# ------------------------------------------------------------------ 4. gloo ranks, injected steps
def _gloo_worker(rank, world, port, name, ret):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = shc.case(name)
        n, nq, d, nlist = len(c["rows"]), len(c["q"]), c["rows"].shape[1], c["nlist"]
        lo, hi = ram.shard_bounds(n, world, rank)
        tie = c.get("tie")
        for dtype in (("sq8",) if tie else shc.STORAGES):                  # (the tie case is about the SQ8 rule alone)
            calls = []

            def flt_of(kw):
                """the filter of the cases a call's keywords stand for; the selector must be the GLOBAL one, read from bit lo"""
                if "selector" in kw:
                    assert kw["sel_bit0"] == lo and np.array_equal(np.asarray(kw["selector"]), c["sel"])
                if "groups" in kw:
                    assert np.array_equal(np.asarray(kw["groups"]), c["q_labels"])
                    return "both" if "selector" in kw else kw["group_mode"]
                return "selector" if "selector" in kw else "plain"

            def local_search(q, k, nprobe, off, **kw):
                assert off == lo and isinstance(q, np.ndarray) and np.array_equal(q, c["q"])
                calls.append((k, nprobe))
                return shc.part_search(c, dtype, lo, hi, k, nprobe, flt_of(kw))

            def merge(gathered, parts, nq_, k, bias):
                assert parts == world and gathered.shape == (world, nq_, k, 2) and (bias is None) == (dtype != "sq8")
                return shc.merge_parts(gathered, parts, nq_, k, bias)

            def local_range_search(q, radius, nprobe, off, **kw):
                assert off == lo
                return shc.part_range(c, dtype, lo, hi, ram.MipsIndex._radii(radius, len(q)), nprobe, flt_of(kw))

            def range_merge(gathered, parts, nq_, stride):
                return rc.merge_records(gathered, parts, nq_, stride)

            ix = ram.ShardedIvfIndex(d, nlist, dtype=dtype, local_search=local_search, merge=merge, local_range_search=local_range_search,
                                     range_merge=range_merge)
            assert (ix.rank, ix.world) == (rank, world) and ix.local is None and not ix.is_trained
            ix.set_trained(c["centroids"], c["sq8_params"] if dtype == "sq8" else None)
            assert ix.is_trained and np.array_equal(ix.centroids(), c["centroids"])
            assert ix.set_global_size(n) == (lo, hi) and ix.ntotal == n
            kws = {"plain": {}, "selector": {"selector": c["sel"]}, "exclude": {"groups": c["q_labels"], "group_mode": "exclude"},
                   "only": {"groups": c["q_labels"], "group_mode": "only"}, "both": {"selector": c["sel"], "groups": c["q_labels"]}}
            for k, nprobe, flt in ((1, 1, "plain"), (5, 1, "selector"), (5, 3, "both"), (29, 3, "exclude"), (30, nlist, "only"), (100, nlist + 3, "selector")):
                got = ix.search_probed(c["q"], k, nprobe, **kws[flt])
                assert all(isinstance(t, np.ndarray) for t in got) and got[0].dtype == np.float32 and got[1].dtype == np.int64
                assert shc.same(got, shc.expected(c, dtype, k, nprobe, flt)), (rank, dtype, k, nprobe, flt)
            if tie:                                                         # equal D, different S on ranks 1 and 0: the order of S
                d_, i_ = ix.search_probed(c["q"], tie["k"], nlist)
                assert shc.same((d_, i_), shc.expected(c, dtype, tie["k"], nlist)) and i_[tie["query"], tie["rank"]:tie["rank"] + 2].tolist() == list(tie["rows"])
            got = ix.search_probed_wide(torch.from_numpy(c["q"]), 5, 3)    # a tensor in -> tensors out
            assert all(isinstance(t, torch.Tensor) for t in got) and shc.same((got[0].numpy(), got[1].numpy()), shc.expected(c, dtype, 5, 3))
            for nprobe, flt in ((1, "plain"), (3, "both")):
                radii = shc.radii_for(c, dtype, nprobe, flt)
                assert rg.same(ix.range_search_probed(c["q"], radii, nprobe, **kws[flt]), shc.expected_range(c, dtype, radii, nprobe, flt)), (rank, dtype, flt)
            with pytest.raises(ValueError):
                ix.search_probed(c["q"], 0)
            with pytest.raises(NotImplementedError):
                ix.search_probed(c["q"], 1025)
            with pytest.raises(ValueError):
                ix.search_probed(c["q"], 5, selector=np.ones(n - 1, bool))  # shorter than the global index
            with pytest.raises(ValueError):
                ix.update_rows_global(np.array([0]), c["rows"][:1])        # injected steps hold no rows
        # the training checksum: one rank with other centroids (one bit), every rank raises
        bad = ram.ShardedIvfIndex(d, nlist, dtype="f32", local_search=lambda *a, **k: None, merge=lambda *a: None)
        cen = c["centroids"].copy()
        if rank == world - 1:
            cen[0, 0] = np.nextafter(cen[0, 0], np.float32(2))
        with pytest.raises(RuntimeError, match="different centroids"):
            bad.set_trained(cen)
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,name", [(2, "planted"), (3, "planted"), (3, "tiny"), (3, "sq8_tie")])
def test_sharded_ivf_index_over_gloo_with_injected_steps(world, name):
    """world 3 holds 334 / 334 / 332 rows of the planted case and 2 / 2 / 0 -- an empty shard -- of the tiny one."""
    import torch.multiprocessing as mp

    port = 29100 + (os.getpid() % 2000) + 7 * world + len(name)
    ret = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, port, name, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}
