"""The piece loops of the IVF index, CPU side: what tests/test_gpu_ivf_pieces.py relies on holds without a GPU, so that those tests
cannot pass vacuously.  The constants mirrored in tests/ivf_pieces_cases.py are those of the sources; every period is coprime to the
piece it is tiled over and every call is longer than its piece; for every multi-piece case the expectation in which the second
piece is answered from the first piece's queries, labels, radii or rows ("offset dropped") differs from the true one in at least
half of the entries behind the boundary; the true list offsets of 1025 and 2500 lists differ from those of a scan that stops at list
1024; the planted lists of more than 1024 lists hold an empty, a one-row and a long list where the scan's second branch owns them."""
import os
import re
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_cases as iv  # noqa: E402
import ivf_filter_cases as fc  # noqa: E402
import ivf_pieces_cases as pc  # noqa: E402
import ivf_range_cases as rc  # noqa: E402
import ivf_search_cases as sc  # noqa: E402
import ivf_wide_cases as wc  # noqa: E402


def _src(name):
    with open(os.path.join(ram._lib.CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------ the mirrored constants
def test_mirrored_constants_are_those_of_the_sources():
    host = _src("host_ivf.hpp")
    assert "constexpr int64_t kIvfAssignChunk = 65536;" in host and pc.ASSIGN_CHUNK == 65536
    assert host.count("r0 += kIvfAssignChunk") == 1 and "std::min(kIvfAssignChunk, n - r0)" in host
    probe = host[host.index("int mips_ivf_probe("):host.index("int mips_ivf_search(")]
    assert probe.count("for (int64_t s0 = 0; s0 < nq; s0 += 4096)") == 2 and probe.count("std::min<int64_t>(4096, nq - s0)") == 2   # both branches
    assert len(re.findall(r"\b4096\b", probe)) == 4 and pc.PROBE_SLICE == 4096
    math = _src("ivf_search_math.hpp")
    assert "constexpr int64_t kSliceQueries = 4096;" in math and pc.SLICE_QUERIES == 4096
    assert "constexpr int64_t kPartsBudget = (int64_t)256 << 20;" in math and pc.PARTS_BUDGET == 256 << 20
    assert "int64_t ns = kPartsBudget / (p * k * 16);" in math
    kern = _src("ivf_kernels.hpp")
    assert "constexpr int IVF_SCAN_THREADS = 1024;" in kern and pc.SCAN_THREADS == 1024
    assert "constexpr int IVF_MAX_PROBE = 1024;" in kern and pc.MAX_PROBE == 1024
    assert "constexpr int64_t kRangeSlice = 4096;" in _src("ivf_range_math.hpp") and pc.RANGE_SLICE == 4096
    assert "std::min<int64_t>(nq, ivf::kRangeSlice)" in _src("host_ivf_range.hpp")
    assert [pc.slice_queries(p, k) for p, k in ((2, 5), (64, 1024), (1024, 29))] == [4096, 256, 564]
    assert pc.slice_queries(1024, 1024) == 16 and pc.slice_queries(1, 1) == 4096
    assert 64 * 1024 == wc.MAX_K_WIDE * pc.WIDE_NLIST == 65536                                     # case 5 sits exactly at the merge limit
    assert "constexpr int64_t kMergeLimit = 65536;" in math


# ------------------------------------------------------------------ periods and pieces
CALLS = {  # case: (items of the call, piece)
    "1 add": (pc.ADD_N, pc.ASSIGN_CHUNK),
    "2 train": (256 * pc.TRAIN_NLIST, pc.ASSIGN_CHUNK),
    "3 probe": (pc.ROBIN_NQ, pc.PROBE_SLICE),
    "4 search": (pc.ROBIN_NQ, pc.slice_queries(pc.ROBIN_NPROBE, pc.ROBIN_K)),
    "5 wide": (pc.WIDE_NQ, pc.slice_queries(pc.WIDE_NLIST, pc.WIDE_K)),
    "6 narrow at 1024 probes": (pc.LISTS_NQ, pc.slice_queries(pc.MAX_PROBE, 29)),
    "7 range": (pc.ROBIN_NQ, pc.RANGE_SLICE),
    "8 load": (pc.LOAD_N, pc.LOAD_CHUNK),
}


def test_every_call_is_longer_than_its_piece_and_every_period_is_coprime_to_it():
    assert {k: pc.pieces(*v) for k, v in CALLS.items()} == {"1 add": 2, "2 train": 2, "3 probe": 2, "4 search": 2, "5 wide": 2,
                                                           "6 narrow at 1024 probes": 2, "7 range": 2, "8 load": 3}
    assert all(n > piece for n, piece in CALLS.values())
    assert pc.TRAIN_N > 256 * pc.TRAIN_NLIST > pc.ASSIGN_CHUNK                                     # the training set is the 65 792 picked rows
    for piece in (4096, 256, 564):
        assert all(pc.coprime(per, piece) for per in (pc.QP, pc.LP, pc.RP, pc.QP * pc.LP)), piece
    for name in ("3 probe", "4 search", "5 wide", "6 narrow at 1024 probes", "7 range"):
        assert CALLS[name][1] in (4096, 256, 564)
    qi, li, pi = pc.tile(pc.ROBIN_NQ)
    assert len(set(pi)) == 35 and np.array_equal(pi // pc.LP, qi) and np.array_equal(pi % pc.LP, li)
    assert fc.LABEL_NONE in pc.LAB5 and 7 in pc.LAB5 and 7 not in pc.case_robin()["row_labels"]       # LABEL_NONE, and a label no row has
    # the last slice of case 4 runs with another S than the first (on 256 compute units)
    assert fc.segments(4096, pc.ROBIN_NPROBE, pc.ROBIN_K, 256) == 1 and fc.segments(150, pc.ROBIN_NPROBE, pc.ROBIN_K, 256) == 2


def test_expand_is_the_restatement_of_the_tiled_call():
    c = pc.case_robin()
    rows, assign, cen = pc.base(c)
    qi, li, pi = pc.tile(40)
    q35, l35 = pc.pairs(c["q"], pc.LAB5)
    kw = dict(labels=c["row_labels"], mode="only")
    a = pc.expand(fc.search(rows, q35, assign, cen, 5, 2, "f32", q_labels=l35, **kw), pi)
    b = fc.search(rows, c["q"][qi], assign, cen, 5, 2, "f32", q_labels=pc.LAB5[li], **kw)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    radii = pc.radii_for(rc.probed_scores(rows, c["q"], assign, cen, 2, "f32"), pc.ROBIN_COUNTS)
    a = pc.expand(rc.range_search(rows, q35, assign, cen, radii[np.arange(35) // 5], 2, "f32", q_labels=l35, **kw), pi)
    b = rc.range_search(rows, c["q"][qi], assign, cen, radii[qi], 2, "f32", q_labels=pc.LAB5[li], **kw)
    assert rc.same(a, b) and a[0][-1] > 0
    assert rc.same(pc.expand(b, np.zeros(0, np.int64)), (np.zeros(1, np.int64), b[1][:0], b[2][:0]))


# ------------------------------------------------------------------ offset sensitivity
def _behind(nq, piece, period):
    """for the queries j behind the first piece: (j % period, (j - piece) % period) -- what j uses and what it would use with the
    piece's offset dropped"""
    j = np.arange(piece, nq)
    return j % period, (j - piece) % period


def _half(differ):
    return len(differ) > 0 and 2 * int(np.sum(differ)) >= len(differ)


def test_case_1_the_second_chunk_of_an_add_is_not_the_first():
    c = pc.case_add()
    for rows in (c["rows"], c["rows2"], iv.synth.round_to_bf16(c["rows"])):
        assign = iv.nearest(rows, c["centroids"])[:, 0]
        assert _half(assign[pc.ASSIGN_CHUNK:] != assign[:pc.ADD_N - pc.ASSIGN_CHUNK])
        assert (np.bincount(assign, minlength=pc.ADD_NLIST) > 0).all()


def test_case_2_the_second_chunk_of_the_training_set_moves_the_centroids():
    x = pc.case_train()
    T = np.ascontiguousarray(iv.training_set(x, pc.TRAIN_NLIST))
    m = len(T)
    assert m == 256 * pc.TRAIN_NLIST == 65792
    c0 = iv.train(x, pc.TRAIN_NLIST, 0)
    a = iv.nearest(T, c0)[:, 0]
    true = iv.train(x, pc.TRAIN_NLIST, 1)
    assert np.array_equal(pc.train_step(T, c0, a).view(np.uint32), true.view(np.uint32))            # (train_step is iv.train's update)
    first = pc.train_step(T[:pc.ASSIGN_CHUNK], c0, a[:pc.ASSIGN_CHUNK])                            # the first 65 536 training rows alone
    assert not np.array_equal(first, true)
    dropped = a.copy()
    dropped[pc.ASSIGN_CHUNK:] = a[:m - pc.ASSIGN_CHUNK]                                            # the second chunk assigned from the first one's rows
    assert _half(dropped[pc.ASSIGN_CHUNK:] != a[pc.ASSIGN_CHUNK:])
    assert not np.array_equal(pc.train_step(T, c0, dropped), true)


def test_case_3_the_probe_behind_the_boundary_is_not_the_one_before_it():
    c = pc.case_robin()
    for q in (c["q"], iv.synth.round_to_bf16(c["q"])):
        P = iv.nearest(q, c["centroids"], pc.ROBIN_NPROBE)
        u, w = _behind(pc.ROBIN_NQ, pc.PROBE_SLICE, pc.QP)
        assert _half((P[u] != P[w]).any(axis=1))


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_case_4_the_search_behind_the_boundary_is_not_the_one_before_it(dtype):
    c = pc.case_robin()
    rows, assign, cen = pc.base(c)
    piece = pc.slice_queries(pc.ROBIN_NPROBE, pc.ROBIN_K)
    u, w = _behind(pc.ROBIN_NQ, piece, pc.QP)
    lu, lw = _behind(pc.ROBIN_NQ, piece, pc.LP)
    for q in (c["q"], iv.synth.round_to_bf16(c["q"])):
        assert _half(pc.rows_differ(sc.search(rows, q, assign, cen, pc.ROBIN_K, pc.ROBIN_NPROBE, dtype), u, w))
    assert _half(pc.rows_differ(fc.search(rows, c["q"], assign, cen, pc.ROBIN_K, pc.ROBIN_NPROBE, dtype, sel=c["mask"]), u, w))
    q35, l35 = pc.pairs(c["q"], pc.LAB5)
    for mode in ("exclude", "only"):
        for sel in (None, c["mask"]):
            res = fc.search(rows, q35, assign, cen, pc.ROBIN_K, pc.ROBIN_NPROBE, dtype, sel=sel, labels=c["row_labels"], q_labels=l35, mode=mode)
            assert _half(pc.rows_differ(res, u * pc.LP + lu, w * pc.LP + lw)), (mode, "everything from the first slice")
            assert _half(pc.rows_differ(res, u * pc.LP + lu, u * pc.LP + lw)), (mode, "q_labels + s0 dropped alone")


@pytest.mark.parametrize("dtype", sc.STORAGES)
def test_case_5_the_wide_search_behind_the_boundary_is_not_the_one_before_it(dtype):
    c = pc.case_wide()
    rows, assign, cen = pc.base(c)
    piece = pc.slice_queries(pc.WIDE_NLIST, pc.WIDE_K)
    u, w = _behind(pc.WIDE_NQ, piece, pc.QP)
    lu, lw = _behind(pc.WIDE_NQ, piece, pc.LP)
    assert _half(pc.rows_differ(wc.search(rows, c["q"], assign, cen, pc.WIDE_K, pc.WIDE_NLIST, dtype), u, w))
    q35, l35 = pc.pairs(c["q"], pc.LAB5)
    res = wc.search(rows, q35, assign, cen, pc.WIDE_K, pc.WIDE_NLIST, dtype, labels=c["row_labels"], q_labels=l35, mode="exclude")
    assert _half(pc.rows_differ(res, u * pc.LP + lu, w * pc.LP + lw)) and _half(pc.rows_differ(res, u * pc.LP + lu, u * pc.LP + lw))
    assert (res[1][:, -1] >= 0).all()                                                              # 1024 results for every pair: no padding


@pytest.mark.parametrize("dtype", ("bf16", "sq8"))
def test_case_7_the_range_search_behind_the_boundary_is_not_the_one_before_it(dtype):
    c = pc.case_robin()
    rows, assign, cen = pc.base(c)
    u, w = _behind(pc.ROBIN_NQ, pc.RANGE_SLICE, pc.QP)
    lu, lw = _behind(pc.ROBIN_NQ, pc.RANGE_SLICE, pc.LP)
    for q in (c["q"], iv.synth.round_to_bf16(c["q"])):
        per = rc.probed_scores(rows, q, assign, cen, pc.ROBIN_NPROBE, dtype)
        radii = pc.radii_for(per, pc.ROBIN_COUNTS)
        res = rc.range_search(rows, q, assign, cen, radii, pc.ROBIN_NPROBE, dtype)
        assert [int(x) for x in np.diff(res[0])] == [100 if x is None else x for x in pc.ROBIN_COUNTS]
        assert _half(pc.rows_differ(res, u, w))
        # radii + s0 dropped alone: query j with the radius of query j - 4096
        shifted = rc.range_search(rows, q, assign, cen, radii[(np.arange(pc.QP) - pc.RANGE_SLICE) % pc.RP], pc.ROBIN_NPROBE, dtype)
        both = (np.concatenate([res[0], res[0][-1] + shifted[0][1:]]), np.concatenate([res[1], shifted[1]]), np.concatenate([res[2], shifted[2]]))
        assert _half(pc.rows_differ(both, u, pc.QP + u))
    q35, l35 = pc.pairs(c["q"], pc.LAB5)
    radii = pc.radii_for(rc.probed_scores(rows, c["q"], assign, cen, pc.ROBIN_NPROBE, dtype), pc.ROBIN_COUNTS)
    for mode in ("exclude", "only"):
        res = rc.range_search(rows, q35, assign, cen, radii[np.arange(35) // pc.LP], pc.ROBIN_NPROBE, dtype, labels=c["row_labels"], q_labels=l35, mode=mode)
        assert _half(pc.rows_differ(res, u * pc.LP + lu, w * pc.LP + lw)) and _half(pc.rows_differ(res, u * pc.LP + lu, u * pc.LP + lw))
        full = pc.expand(res, pc.tile(pc.ROBIN_NQ)[2])
        assert full[0][pc.RANGE_SLICE] > 0 and full[0][-1] > full[0][pc.RANGE_SLICE]                # hits on both sides of the boundary


def test_case_6_the_narrow_search_of_600_queries_behind_its_boundary():
    c = pc.case_lists(1025)
    rows, assign, cen = pc.base(c)
    piece = pc.slice_queries(pc.MAX_PROBE, 29)
    assert piece == 564 < pc.LISTS_NQ
    u, w = _behind(pc.LISTS_NQ, piece, pc.QP)
    assert _half(pc.rows_differ(sc.search(rows, c["q"], assign, cen, 29, 1024, "f32"), u, w))


# ------------------------------------------------------------------ more than 1024 lists
@pytest.mark.parametrize("nlist", pc.LISTS_NLISTS)
def test_case_6_list_mix_and_the_offsets_of_a_scan_that_stops_at_list_1024(nlist):
    c = pc.case_lists(nlist)
    assign = c["assign"]
    sizes = np.bincount(assign, minlength=nlist)
    off, order = iv.list_table(assign, nlist)
    assert off[-1] == pc.LISTS_N and (sizes == 0).any() and (sizes == 1).any() and sizes.max() >= 64
    assert sizes[nlist - 1] >= 64 and (assign[c["planted"]] == nlist - 1).all()                     # the long list is the last one
    assert iv.nearest(c["q"][:1], c["centroids"])[0, 0] == nlist - 1                                # ... and query 0 probes it first
    cut = pc.offsets_one_list_per_thread(assign, nlist)
    if nlist > pc.SCAN_THREADS:
        assert nlist - 1 >= pc.SCAN_THREADS                                                        # the long list belongs to the scan's second branch
        assert not np.array_equal(off, cut) and cut[-1] < off[-1]
        if nlist >= 2 * pc.SCAN_THREADS:                                                           # 2500: empty and one-row lists there as well
            assert (sizes[pc.SCAN_THREADS:] == 0).any() and (sizes[pc.SCAN_THREADS:] == 1).any()
            per = -(-nlist // pc.SCAN_THREADS)
            assert per == 3                                                                        # a thread owns three lists, the last thread fewer
    else:
        assert np.array_equal(off, cut)
    # radii of the range search: no hit, some hits, every probed row
    per = rc.probed_scores(c["rows"], c["q"], assign, c["centroids"], 40, "f32")
    assert all(len(p[0]) > 8 for p in per)
