"""Grouped search (mips_index_set_labels / mips_search_wide_grp / mips_range_search_grp; groups= on MipsIndex, ShardedMipsIndex,
KnowledgeBase and Mips): one int32 label per row, one per query and a mode decide per (query, row) whether the row may answer.
Wide expectations are the oracle's FULL ranking (orc.search_exact_bruteforce with k = n, once per shape) from which each query's
non-admitted ids are removed, cut to k and padded -- _filter_ranking of tests/test_gpu_filtered.py with a per-query mask; range
expectations are the all-pairs recipe of tests/test_gpu_range.py (orc.canonical_pairs / orc.sumsq_canonical, strict float32 rule;
phi over ALL rows) AND-ed with the per-query mask.  Everything is compared bit for bit, no query is left out."""
import os
import subprocess

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth
from retrieval_augmented_mds_amd.mips import KnowledgeBase

pytestmark = pytest.mark.gpu

GROUPED = "mips::grouped_scan_kernel"
TILE = 128
NONE = ram.LABEL_NONE
ABSENT = 1 << 20   # a label no row of these tests carries


# ------------------------------------------------------------------ expectations
def _admit(labels, qlabels, mode, mask=None):
    """bool [nq, n]: may row i answer query j?  (the group rule, AND-ed with a row mask if one is given)"""
    labels, qlabels = np.asarray(labels, np.int64), np.asarray(qlabels, np.int64)
    eq = labels[None, :] == qlabels[:, None]
    adm = np.where((qlabels == NONE)[:, None], True, eq if mode == "only" else ~eq)
    return adm if mask is None else adm & np.asarray(mask, bool)[None, :]


def _filter_ranking(full, admit, k, metric, idx_offset=0):
    """full = (scores, ids) [nq, n], the oracle's ranking of ALL rows -> the k best admitted rows per query, padded."""
    fs, fi = full
    nq = fs.shape[0]
    s = np.full((nq, k), np.inf if metric else -np.inf, np.float32)
    i = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        keep = np.flatnonzero(admit[j][fi[j]])[:k]
        s[j, :len(keep)] = fs[j, keep]
        i[j, :len(keep)] = fi[j, keep] + idx_offset
    return s, i


def _same(got, exp, what=""):
    s, i = got
    es, ei = exp
    if isinstance(s, torch.Tensor):
        s, i = s.cpu().numpy(), i.cpu().numpy()
    s, i = np.asarray(s, np.float32), np.asarray(i, np.int64)
    bad = np.flatnonzero((i != ei).any(axis=1))
    assert np.array_equal(i, ei), f"{what}: indices differ in {len(bad)} queries, first {bad[:5]}"
    assert np.array_equal(s.view(np.int32), es.view(np.int32)), f"{what}: scores differ"


def _unpack(packed):
    s, i = ram.unpack_gathered(packed[None], 1)
    return s.cpu().numpy(), i.cpu().numpy()


def _tile_counts(mask):
    pad = np.zeros(-len(mask) % TILE, bool)
    return np.concatenate([mask, pad]).reshape(-1, TILE).sum(axis=1)


def _sparse_mask(n, seed=2):
    """The sparse selector of the filtered tests: the first seed (counting up) whose density-1/64 mask leaves one 128-row tile
    empty and one with a single row."""
    for s in range(seed, seed + 1000):
        mask = np.random.default_rng(s).random(n) < 1 / 64
        c = _tile_counts(mask)
        if (c == 0).any() and (c == 1).any():
            return mask
    raise AssertionError("no such mask")


def _values(q, x, metric):
    """float32 canonical output value of every (query, row) pair: the inner product, or |q|^2 + phi - 2 q.x (metric 1)."""
    n = x.shape[0]
    dot = orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1)))
    if metric == 1:
        phi = orc.sumsq_canonical(x).max()
        return (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * dot).astype(np.float32)
    return dot.astype(np.float32)


def _ranking_from_values(vals, metric):
    """The full ranking out of the all-pairs values: (value best first, row ascending), the order search_exact_bruteforce
    itself applies (orc._order_desc).  For shapes whose brute-force ranking (an insertion sort, n^2 / 4 moves per query) would
    take minutes; the callers assert on their first queries that it IS search_exact_bruteforce's ranking, bit for bit."""
    ids = np.tile(np.arange(vals.shape[1], dtype=np.int64), (vals.shape[0], 1))
    order = orc._order_desc(-vals if metric == 1 else vals, ids)
    return np.take_along_axis(vals, order, axis=1), order.astype(np.int64)


_CASES = {}


def _gauss_case(n, nq, d, metric):
    """Gaussian bf16 inputs and the oracle's full ranking: computed once per shape and metric, shared, never modified."""
    key = (n, nq, d, metric)
    if key not in _CASES:
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
        _CASES[key] = (x, q, orc.search_exact_bruteforce(q, x, n, metric=metric))
    return _CASES[key]


def _f32_case(metric):
    """30000 x 768 float32 rows, 40 queries: values of all pairs and the full ranking (checked against the brute force)."""
    key = ("f32", metric)
    if key not in _CASES:
        rng = np.random.default_rng(31)
        n, nq, d = 30000, 40, 768
        x = rng.standard_normal((n, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        vals = _values(q, x, metric)
        full = _ranking_from_values(vals, metric)
        bs, bi = orc.search_exact_bruteforce(q[:2], x, n, metric=metric)
        assert np.array_equal(bi, full[1][:2]) and np.array_equal(bs.view(np.int32), full[0][:2].view(np.int32))
        _CASES[key] = (x, q, vals, full)
    return _CASES[key]


def _labellings(n):
    row = np.arange(n)
    return {"random 7": np.random.default_rng(n).integers(0, 7, n), "row % 5": row % 5, "row // 2": row // 2, "one label": np.full(n, 3)}


def _query_labels(labels, nq):
    """Cycle through (up to five) present labels, one absent label and LABEL_NONE."""
    present = np.unique(labels)
    cyc = [int(v) for v in present[np.linspace(0, len(present) - 1, min(5, len(present))).astype(int)]] + [ABSENT, NONE]
    return np.array([cyc[j % len(cyc)] for j in range(nq)], np.int64)


# ------------------------------------------------------------------ 1. Gaussian bf16, both metrics, both modes
@pytest.mark.parametrize("n,nq,d,k", [(4099, 129, 1024, 100), (777, 5, 100, 64), (9001, 70, 256, 5)])
@pytest.mark.parametrize("metric", [0, 1])
def test_gaussian_bf16_matches_grouped_oracle(n, nq, d, k, metric):
    x, q, full = _gauss_case(n, nq, d, metric)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    plain = ix.search_wide(q, k)
    assert ix.last_kernel.startswith("mips::wide_scan_kernel")
    for name, labels in _labellings(n).items():
        ix.set_labels(labels)
        ql = _query_labels(labels, nq)
        for mode in ("exclude", "only"):
            got = ix.search_wide(q, k, groups=ql, group_mode=mode)
            st = ix.margin_stats()
            print(f"n={n} nq={nq} d={d} k={k} metric={metric} {name} {mode}: {st}")
            assert ix.last_kernel == GROUPED
            assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] >= 0
            _same(got, _filter_ranking(full, _admit(labels, ql, mode), k, metric), f"{name}, {mode}")
            got = ix.search_wide(q, k, groups=np.full(nq, NONE), group_mode=mode)
            assert ix.last_kernel == GROUPED
            _same(got, plain, f"{name}, {mode}: all queries LABEL_NONE against the unfiltered search")
    ix.search_wide(q, k, groups=None)
    assert ix.last_kernel.startswith("mips::wide_scan_kernel")


# ------------------------------------------------------------------ 2. groups on top of a sparse bitmap
@pytest.mark.parametrize("metric", [0, 1])
def test_groups_combine_with_a_sparse_bitmap(metric):
    n, nq, d, k = 9001, 70, 256, 64
    x, q, full = _gauss_case(n, nq, d, metric)
    mask = _sparse_mask(n)
    c = _tile_counts(mask)
    assert (c == 0).any() and (c == 1).any()                       # an empty tile and a tile with a single row
    labels = np.random.default_rng(21).integers(0, 7, n)
    ql = _query_labels(labels, nq)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    ix.set_labels(labels)
    sel = ram.Selector.from_mask(mask)
    qd = torch.from_numpy(q).cuda()
    for mode in ("exclude", "only"):
        exp = _filter_ranking(full, _admit(labels, ql, mode, mask), k, metric, idx_offset=1 << 33)
        got = ix.search_wide(q, k, idx_offset=1 << 33, selector=sel, groups=ql, group_mode=mode)
        st = ix.margin_stats()
        assert ix.last_kernel == GROUPED and st["unresolved"] == 0 and st["flagged"] == st["rescanned"]
        _same(got, exp, f"bitmap and groups, {mode}")
        _same(_unpack(ix.search_wide_packed(qd, k, idx_offset=1 << 33, selector=sel, groups=ql, group_mode=mode)), exp, f"packed, {mode}")
    if metric == 1:
        exp = _filter_ranking(_gauss_case(n, nq, d, 0)[2], _admit(labels, ql, "exclude", mask), k, 0)
        _same(ix.search_wide(q, k, force_ip=True, selector=sel, groups=ql), exp, "force_ip")


# ------------------------------------------------------------------ 3. only mode on groups smaller than k
@pytest.mark.parametrize("metric", [0, 1])
def test_only_mode_on_groups_smaller_than_k_pads_and_is_certified_outright(metric):
    """Groups of 1 .. 50 rows, k = 64: a query's admitted rows all fit in its pool (k' = k + 64), which then IS the admitted set:
    nothing outside it can be a result and no query may be flagged, whatever the scores are."""
    n, nq, d, k = 9001, 70, 256, 64
    x, q, full = _gauss_case(n, nq, d, metric)
    perm = np.random.default_rng(22).permutation(n)
    labels = np.full(n, 1000)
    start = 0
    for g in range(1, 51):
        labels[perm[start:start + g]] = g
        start += g
    ql = 1 + np.arange(nq) % 50
    exp = _filter_ranking(full, _admit(labels, ql, "only"), k, metric)
    for j in range(nq):
        assert (exp[1][j, :ql[j]] >= 0).all() and (exp[1][j, ql[j]:] == -1).all()     # padded after the group size
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    ix.set_labels(labels)
    got = ix.search_wide(q, k, groups=ql, group_mode="only")
    st = ix.margin_stats()
    print(st)
    assert st == {"flagged": 0, "rescanned": 0, "unresolved": 0}
    _same(got, exp, "small groups")


# ------------------------------------------------------------------ 4. exclude mode with every row in the query's group
@pytest.mark.parametrize("metric", [0, 1])
def test_excluding_the_only_group_leaves_nothing(metric):
    n, nq, d, k = 777, 5, 100, 64
    x, q, full = _gauss_case(n, nq, d, metric)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    ix.set_labels(np.full(n, 9, np.int32))
    s, i = ix.search_wide(q, k, groups=np.full(nq, 9))
    assert (i == -1).all() and (s == (np.inf if metric else -np.inf)).all()
    assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}
    packed = _unpack(ix.search_wide_packed(torch.from_numpy(q).cuda(), k, groups=torch.full((nq,), 9, dtype=torch.int32, device="cuda")))
    assert (packed[1] == -1).all() and (packed[0] == (np.inf if metric else -np.inf)).all()
    ql = np.array([9, NONE, 9, ABSENT, 9])                         # and next to queries that exclude nothing
    _same(ix.search_wide(q, k, groups=ql), _filter_ranking(full, _admit(np.full(n, 9), ql, "exclude"), k, metric), "mixed")


# ------------------------------------------------------------------ 5. fp32-exact index
@pytest.mark.parametrize("metric", [0, 1])
def test_f32_exact_index(metric):
    x, q, vals, full = _f32_case(metric)
    n, nq = x.shape[0], q.shape[0]
    labels = np.random.default_rng(23).integers(0, 7, n)
    ql = _query_labels(labels, nq)
    ix = ram.MipsIndex(x.shape[1], metric=metric, dtype="f32")
    ix.add(x)
    ix.set_labels(labels)
    for mode in ("exclude", "only"):
        for k in (5, 100):
            got = ix.search_wide(q, k, groups=ql, group_mode=mode)
            st = ix.margin_stats()
            print(f"f32 k={k} metric={metric} {mode}: {st}")
            assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] and ix.last_kernel == GROUPED
            _same(got, _filter_ranking(full, _admit(labels, ql, mode), k, metric), f"f32 k={k} {mode}")


# ------------------------------------------------------------------ 6. ties
def test_lattice_ties_lowest_admitted_row_wins():
    x = synth.generate(1, 0, 5000, 128, synth.KIND_LATTICE)
    q = synth.generate(2, 0, 19, 128, synth.KIND_LATTICE)
    full = orc.search_exact_bruteforce(q, x, 5000)
    labels = np.random.default_rng(24).integers(0, 3, 5000)
    ql = _query_labels(labels, 19)
    ix = ram.MipsIndex(128)
    ix.add(x)
    ix.set_labels(labels)
    for mode in ("exclude", "only"):
        for k in (30, 200):
            exp = _filter_ranking(full, _admit(labels, ql, mode), k, 0)
            with np.errstate(invalid="ignore"):                           # (the padding of the ABSENT queries: -inf - -inf)
                assert k < 200 or (np.diff(exp[0], axis=1) == 0).sum() > 0    # tied scores inside the results: their order is by row
            _same(ix.search_wide(q, k, groups=ql, group_mode=mode), exp, f"lattice k={k} {mode}")
            assert ix.margin_stats()["unresolved"] == 0


# ------------------------------------------------------------------ 7. the settlement respects labels
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_excluded_near_duplicates_stay_excluded_when_queries_are_settled(dtype):
    """The construction of tests/test_gpu_filtered.py's test of the same name, unchanged (M = 400 / 600 copies of the star row).
    Instead of a bitmap the 100 best copies carry label A, the next 100 label B, every other row C.  Star query 0 excludes A -- its
    result is the next 100 copies, and the copies the pool leaves out lie within the scan's error bound of the k-th -- and star
    query 8 excludes B: both are flagged and settled in ONE pass of the exact kernel, each under its own label, and the brute
    force, which scores every row, must not append what the query's label excludes."""
    rng = np.random.default_rng(11)
    n, d, nq, k = 20000, 768, 16, 100
    M = 400 if dtype == "bf16" else 600
    x = synth.round_to_bf16(rng.standard_normal((n, d)).astype(np.float32))
    q = synth.round_to_bf16(rng.standard_normal((nq, d)).astype(np.float32))
    v = synth.round_to_bf16(rng.standard_normal(d).astype(np.float32))
    rows = 1003 + 16 * np.arange(M)
    x[rows] = v
    x[rows, 5] = (np.arange(M) % 16).astype(np.float32)
    x[rows, 9] = (np.arange(M) // 16).astype(np.float32)
    star = v.copy()
    star[5] = 2.0 ** -12
    star[9] = 2.0 ** -8
    stars = np.arange(0, nq, 8)
    q[stars] = star
    full = orc.search_exact_bruteforce(q, x, n)
    A, B, C = 1, 2, 3
    best, second = rows[M - 100:], rows[M - 200:M - 100]
    assert np.array_equal(np.sort(full[1][stars[0], :100]), best)                    # (the construction does what it says)
    labels = np.full(n, C)
    labels[best] = A
    labels[second] = B
    ql = np.full(nq, NONE)
    ql[0], ql[8] = A, B
    exp = _filter_ranking(full, _admit(labels, ql, "exclude"), k, 0)
    assert np.array_equal(np.sort(exp[1][0]), second)                                # query 0: the next 100 copies
    assert np.array_equal(np.sort(exp[1][8]), best)                                  # query 8 keeps the best 100
    ix = ram.MipsIndex(d, dtype=dtype)
    ix.add(x)
    ix.set_labels(labels)
    for queries, groups in ((q, ql), (torch.from_numpy(q).cuda(), torch.from_numpy(ql).cuda())):   # host-output and stream-ordered form
        got = ix.search_wide(queries, k, groups=groups)
        st = ix.margin_stats()
        print(dtype, type(queries).__name__, st)
        assert st["flagged"] > 0 and st["rescanned"] == st["flagged"] and st["unresolved"] == 0
        ids = got[1].cpu().numpy() if isinstance(got[1], torch.Tensor) else got[1]
        assert not np.isin(ids[0], best).any() and not np.isin(ids[8], second).any(), "an excluded row came back"
        _same(got, exp, "flood")


# ------------------------------------------------------------------ 8. more than one query slice
@pytest.mark.parametrize("mode", ["exclude", "only"])
def test_more_queries_than_one_slice(mode):
    n, nq, d, k = 2000, 4200, 64, 40
    key = ("slices",)
    if key not in _CASES:
        x = synth.generate(3, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(4, 0, nq, d, synth.KIND_GAUSS)
        full = _ranking_from_values(_values(q, x, 0), 0)
        bs, bi = orc.search_exact_bruteforce(q[4090:4100], x, n)
        assert np.array_equal(bi, full[1][4090:4100]) and np.array_equal(bs.view(np.int32), full[0][4090:4100].view(np.int32))
        _CASES[key] = (x, q, full)
    x, q, full = _CASES[key]
    labels = np.arange(n) % 5
    j = np.arange(nq)
    ql = np.where(j < 4096, j % 5, (j + 2) % 5)
    assert (ql[4096:] != ql[:nq - 4096]).all()                     # a slice that read the labels from offset 0 would be found out
    ix = ram.MipsIndex(d)
    ix.add(x)
    ix.set_labels(labels)
    got = ix.search_wide(q, k, groups=ql, group_mode=mode)
    assert ix.margin_stats()["unresolved"] == 0 and ix.last_kernel == GROUPED
    _same(got, _filter_ranking(full, _admit(labels, ql, mode), k, 0), "4200 queries")


# ------------------------------------------------------------------ 9. range search
def _boundary_radii(vals, metric):
    """A third of the queries get the exact float32 score of one of their own rows (that row and its ties are out), a third the
    nextafter of such a score towards the permissive side (they are in), the rest run from "nothing" to "every row", +-inf
    included.  `vals` [nq, n] float32."""
    nq, n = vals.shape
    permissive = np.float32(np.inf if metric == 1 else -np.inf)
    r = np.empty(nq, np.float32)
    for j in range(nq):
        best = np.sort(vals[j]) if metric == 1 else np.sort(vals[j])[::-1]
        own = best[(7 * j) % min(n, 60)]
        if j % 3 == 0:
            r[j] = own
        elif j % 3 == 1:
            r[j] = np.nextafter(own, permissive)
        else:
            r[j] = [best[0], best[min(n - 1, 50)], np.nextafter(best[-1], permissive), -permissive, permissive][(j // 3) % 5]
    return r


def _expected_range(vals, r, metric, admit, idx_offset=0):
    lims, D, I = [0], [], []
    for j in range(vals.shape[0]):
        ids = np.flatnonzero((vals[j] < r[j] if metric == 1 else vals[j] > r[j]) & admit[j])
        lims.append(lims[-1] + len(ids))
        D.append(vals[j][ids])
        I.append(ids + idx_offset)
    return np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def _same_range(got, exp, what=""):
    lims, D, I = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in got)
    el, eD, eI = exp
    assert lims.shape == el.shape and lims[0] == 0
    for j in range(len(el) - 1):
        a, b = int(lims[j]), int(lims[j + 1])
        ea, eb = int(el[j]), int(el[j + 1])
        assert b - a == eb - ea, f"{what}: query {j} has {b - a} hits, expected {eb - ea}"
        assert np.array_equal(I[a:b], eI[ea:eb]), f"{what}: ids of query {j} differ"
        assert np.array_equal(D[a:b], eD[ea:eb]), f"{what}: scores of query {j} differ"
    assert np.array_equal(lims.astype(np.int64), el) and len(D) == len(I) == el[-1]


@pytest.mark.parametrize("n,nq,d", [(4099, 129, 1024), (777, 5, 100)])
@pytest.mark.parametrize("metric", [0, 1])
def test_range_search_matches_grouped_all_pairs(n, nq, d, metric):
    x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
    vals = _values(q, x, metric)
    r = _boundary_radii(vals, metric)
    labels = np.random.default_rng(25).integers(0, 7, n)
    ql = _query_labels(labels, nq)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    ix.set_labels(labels)
    qd = torch.from_numpy(q).cuda()
    for mode in ("exclude", "only"):
        admit = _admit(labels, ql, mode)
        exp = _expected_range(vals, r, metric, admit)
        got = ix.range_search(q, r, groups=ql, group_mode=mode)
        print(f"n={n} nq={nq} d={d} metric={metric} {mode}: {exp[0][-1]} hits")
        _same_range(got, exp, mode)
        assert ix.last_kernel == GROUPED
        assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}
        # cap = 0: a counting call; its counts are the true ones
        lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        none_s, none_i = torch.empty(0, dtype=torch.float32, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda")
        ix.range_search_into(qd, r, lims, none_s, none_i, groups=ql, group_mode=mode)
        assert np.array_equal(lims.cpu().numpy(), exp[0])
        # the non-synchronising form with CUDA tensors (device labels), ids offset
        total = int(exp[0][-1])
        D = torch.empty(total + 3, dtype=torch.float32, device="cuda")
        I = torch.empty(total + 3, dtype=torch.int64, device="cuda")
        ix.range_search_into(qd, r, lims, D, I, idx_offset=1 << 33, groups=torch.from_numpy(ql).cuda(), group_mode=mode)
        _same_range((lims, D[:total], I[:total]), _expected_range(vals, r, metric, admit, idx_offset=1 << 33), mode + ", into")
    # on top of a bitmap
    mask = np.random.default_rng(26).random(n) < 0.5
    _same_range(ix.range_search(q, r, selector=mask, groups=ql), _expected_range(vals, r, metric, _admit(labels, ql, "exclude", mask)), "bitmap")
    ix.range_search(q, r)
    assert ix.last_kernel.startswith("mips::wide_scan_kernel")


@pytest.mark.parametrize("metric", [0, 1])
def test_range_search_f32_exact_index(metric):
    x, q, vals, _ = _f32_case(metric)
    r = _boundary_radii(vals, metric)
    labels = np.random.default_rng(27).integers(0, 7, x.shape[0])
    ql = _query_labels(labels, q.shape[0])
    ix = ram.MipsIndex(x.shape[1], metric=metric, dtype="f32")
    ix.add(x)
    ix.set_labels(labels)
    for mode in ("exclude", "only"):
        _same_range(ix.range_search(q, r, groups=ql, group_mode=mode), _expected_range(vals, r, metric, _admit(labels, ql, mode)), f"f32 {mode}")
        assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}


# ------------------------------------------------------------------ 10. label plumbing
def test_label_plumbing(tmp_path):
    n, nq, d, k = 9001, 70, 256, 64
    x, q, full = _gauss_case(n, nq, d, 0)
    labels = np.random.default_rng(28).integers(-5, 5, n)
    labels[17] = NONE                                              # a row may carry it: a group no query can name
    ql = _query_labels(labels[labels != NONE], nq)
    exp = _filter_ranking(full, _admit(labels, ql, "exclude"), k, 0)
    ix = ram.MipsIndex(d)
    ix.reserve(1000)                                               # small: the rows grow twice below
    ix.add(x[:3000])
    with pytest.raises(ValueError):                                # never labelled
        ix.search_wide(q, k, groups=ql)
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, groups=ql)
    ix.set_labels(labels[:1000])                                   # three batches with row0, int64 NumPy / CUDA int32 / a list
    with pytest.raises(ValueError):
        ix.set_labels(labels[1500:2000], row0=1500)                # a gap
    ix.set_labels(torch.from_numpy(labels[1000:2500].astype(np.int32)).cuda(), row0=1000)
    ix.set_labels([int(v) for v in labels[2400:3000]], row0=2400)  # (overlapping what is labelled is a rewrite)
    with pytest.raises(ValueError):
        ix.set_labels(labels[:3001])                               # more labels than rows
    assert np.array_equal(ix.labels(), labels[:3000]) and ix.labels().dtype == np.int32
    assert np.array_equal(ix.labels(10, 5), labels[10:15])
    _same(ix.search_wide(q, k, groups=ql), _filter_ranking((full[0], full[1]), _admit(labels, ql, "exclude", np.arange(n) < 3000), k, 0), "3000 rows")
    ix.add(x[3000:])                                               # growth: the labels survive it
    with pytest.raises(ValueError):                                # rows added since
        ix.search_wide(q, k, groups=ql)
    assert np.array_equal(ix.labels(), labels[:3000])
    ix.set_labels(labels[3000:], row0=3000)
    assert np.array_equal(ix.labels(), labels)
    host = ix.search_wide(q, k, groups=ql)
    _same(host, exp, "host labels")
    _same(ix.search_wide(q, k, groups=torch.from_numpy(ql).cuda()), exp, "device labels, host queries")
    _same(ix.search_wide(torch.from_numpy(q).cuda(), k, groups=torch.from_numpy(ql).cuda().to(torch.int32)), exp, "device labels, device queries")
    _same(ix.search_wide(torch.from_numpy(q).cuda(), k, groups=[int(v) for v in ql]), exp, "a list, device queries")
    # save / load, whole and one row range
    path = str(tmp_path / "ix")
    ix.save(path)
    back = ram.MipsIndex.load(path)
    assert back.meta.get("labels") is True and np.array_equal(back.labels(), labels)
    _same(back.search_wide(q, k, groups=ql), exp, "loaded")
    lo, hi = 2999, 6003
    part = ram.MipsIndex.load(path, row_range=(lo, hi))
    assert np.array_equal(part.labels(), labels[lo:hi])
    inside = (np.arange(n) >= lo) & (np.arange(n) < hi)
    got = part.search_wide(q, k, idx_offset=lo, groups=ql, group_mode="only")
    _same(got, _filter_ranking(full, _admit(labels, ql, "only", inside), k, 0), "loaded row range")
    plain = ram.MipsIndex(d)
    plain.add(x[:500])
    plain.save(str(tmp_path / "plain"))                            # files without labels load as before
    assert "labels" not in ram.MipsIndex.load(str(tmp_path / "plain")).meta and not os.path.exists(str(tmp_path / "plain" / "labels.i32"))
    ix.reset()                                                     # reset clears the labels
    ix.add(x[:300])
    with pytest.raises(ValueError):
        ix.search_wide(q, k, groups=ql)


# ------------------------------------------------------------------ 11. plain C
def test_c_abi_grp_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_grp_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_grp_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


# ------------------------------------------------------------------ 12. KnowledgeBase and Mips
def test_knowledge_base_and_mips():
    n, nq, d, k = 9001, 70, 256, 5
    x, q, full = _gauss_case(n, nq, d, 0)
    aid = np.array([f"art{r // 3:05d}" for r in range(n)])        # groups of three rows, a string column
    uniq, codes = np.unique(aid, return_inverse=True)
    q_aid = np.array([aid[(97 * j) % n] for j in range(nq)])
    q_aid[3] = "no such article"
    q_codes = np.searchsorted(uniq, q_aid)
    kb = KnowledgeBase({"emb": x, "row": np.arange(n), "aid": aid})
    kb.add_faiss_index("emb", metric_type=0, dtype="bf16")
    kb.set_groups("emb", "aid")
    assert np.array_equal(kb.get_index("emb").faiss_index.labels(), codes)
    for mode in ("exclude", "only"):
        ql = q_codes.copy()
        ql[3] = NONE if mode == "exclude" else len(uniq)
        exp = _filter_ranking(full, _admit(codes, ql, mode), k, 0)
        assert mode == "exclude" or ((exp[1][3] == -1).all() and (exp[1][0, :3] >= 0).all() and (exp[1][0, 3:] == -1).all())
        scores, examples = kb.get_nearest_examples_batch("emb", q, k, groups=q_aid, group_mode=mode)
        for j in range(nq):
            keep = exp[1][j] >= 0
            assert np.array_equal(np.asarray(scores[j]), exp[0][j][keep]) and np.array_equal(np.asarray(examples[j]["row"]), exp[1][j][keep])
            assert mode == "exclude" or all(a == q_aid[j] for a in examples[j]["aid"])
    # Mips: ignore_groups sets the groups of index_column on first use; it combines with ignore_indexes
    args = ram.MipsArgs(mips_topk=k, mips_metric_type=0, mips_normalize=False, mips_index_dtype="bf16")
    m = ram.Mips(args, data={"mips_column": [f"text {r}" for r in range(n)], "aid": list(aid)})
    m.build_index(x)
    ql = q_codes.copy()
    ql[3] = NONE
    admit = _admit(codes, ql, "exclude")
    exp = _filter_ranking(full, admit, k, 0)
    s, i = m.search(q, k=k, ignore_groups=list(q_aid))
    _same((s, i), exp, "Mips.search(ignore_groups)")
    assert m._index().last_kernel == GROUPED
    exp1 = _filter_ranking(full, admit, k + 1, 0)
    banned = exp1[1][:, 1].copy()                                  # each query bans its second hit
    s, i = m.search(q, ignore_indexes=list(banned), k=k, ignore_groups=list(q_aid))
    want_i = np.stack([row[row != b][:k] for row, b in zip(exp1[1], banned)])
    want_s = np.stack([srow[row != b][:k] for srow, row, b in zip(exp1[0], exp1[1], banned)])
    _same((np.asarray(s, np.float32), np.asarray(i, np.int64)), (want_s, want_i), "ignore_groups and ignore_indexes")
    out = m.forward(queries=q.copy(), aid=list(q_aid), k=k, ignore_own_group=True)
    _same((out.scores, out.indices), exp, "forward(ignore_own_group=True)")
    for j in range(nq):
        assert q_aid[j] not in [aid[r] for r in out.indices[j]]
    plain = m.forward(queries=q.copy(), aid=list(q_aid), k=k)    # the default leaves the call as it was
    _same((plain.scores, plain.indices), (full[0][:, :k], full[1][:, :k]), "forward without the flag")


# ------------------------------------------------------------------ 13. the sharded facade
def _rank_worker(rank, world, port, n, nq, d, k, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        rng = np.random.default_rng(3)
        x = synth.round_to_bf16((synth.generate(151, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
        qn = synth.round_to_bf16(synth.generate(152, 0, nq, d, synth.KIND_GAUSS))
        qd = torch.from_numpy(qn).cuda()
        labels = np.random.default_rng(29).integers(0, 7, n)
        ql = _query_labels(labels, nq)
        ok = True
        for metric in (0, 1):
            ix = ram.ShardedMipsIndex(d, metric=metric, device=0)
            ix.add_global(x)
            ix.set_labels_global(labels)
            full = orc.search_exact_bruteforce(qn, x, n, metric=metric)
            for mode in ("exclude", "only"):
                exp = _filter_ranking(full, _admit(labels, ql, mode), k, metric)
                s, i = ix.search_wide(qd, k, groups=torch.from_numpy(ql).cuda(), group_mode=mode)     # device fast path
                ok &= s.is_cuda and bool(np.array_equal(i.cpu().numpy(), exp[1]) and np.array_equal(s.cpu().numpy(), exp[0]))
                ok &= ix.margin_stats()["unresolved"] == 0 and ix.local.last_kernel == GROUPED
                s, i = ix.search_wide(qn, k, groups=ql, group_mode=mode)                                # generic path: NumPy in, NumPy out
                ok &= isinstance(s, np.ndarray) and bool(np.array_equal(i, exp[1]) and np.array_equal(s, exp[0]))
                s, i = ram.index.route_search(ix, qd, 5, groups=ql, group_mode=mode)                    # search() routes to the wide search
                ok &= bool(np.array_equal(i.cpu().numpy(), exp[1][:, :5]) and np.array_equal(s.cpu().numpy(), exp[0][:, :5]))
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_sharded_search_wide_with_groups(tmp_path):
    """Two row shards on processes sharing cuda:0 (the worker of test_gpu_filtered.py): the row labels are global, each shard keeps
    its own; the query labels are replicated like the queries; equal to the grouped oracle on the unsharded index."""
    import torch.multiprocessing as mp

    world, n, k = 2, 20001, 100
    port = 31300 + (os.getpid() % 2000)
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, n, 50, 256, k, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


# ------------------------------------------------------------------ 14. refusals
def test_refusals():
    d = 64
    x = synth.generate(3, 0, 300, d, synth.KIND_GAUSS)
    q = np.zeros((2, d), np.float32)
    ix = ram.MipsIndex(d)
    ix.add(x)
    ix.set_labels(np.arange(300) % 4)
    g = np.array([1, 2])
    with pytest.raises(NotImplementedError):
        ix.search_wide(q, ram.MAX_K_WIDE + 1, groups=g)
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, groups=g, group_mode="without")
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, groups=np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, groups=np.array([1, 1 << 31]))
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, groups=np.array([-(1 << 31) - 1, 0]))
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, groups=np.array([0.5, 1.0]))
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, groups=g, group_mode="both")
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, groups=np.array([1]))
    with pytest.raises(ValueError):
        ix.set_labels(np.array([1 << 40]))
    for dtype in ("fp8_e4m3", "fp8_e4m3_docs"):
        f8 = ram.MipsIndex(d, dtype=dtype)
        f8.add(x)
        f8.set_labels(np.arange(300) % 4)
        with pytest.raises(NotImplementedError):
            f8.search_wide(q, 40, groups=g)
        with pytest.raises(NotImplementedError):
            f8.range_search(q, 0.0, groups=g)
    wide = ram.MipsIndex(1100)
    wide.add(synth.generate(3, 0, 300, 1100, synth.KIND_GAUSS))
    wide.set_labels(np.arange(300) % 4)
    with pytest.raises(NotImplementedError):
        wide.search_wide(np.zeros((2, 1100), np.float32), 40, groups=g)
    # the C ABI itself: the same refusals, by return code
    lib = ram._lib.load()
    out_s = torch.empty((2, 40), dtype=torch.float32, device="cuda")
    out_i = torch.empty((2, 40), dtype=torch.int64, device="cuda")
    qd = torch.from_numpy(q).cuda()
    gd = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    dev = ram._lib.Q_DEVICE | ram._lib.OUT_DEVICE | ram._lib.GRP_DEVICE

    def wide_rc(index, k, mode):
        return lib.mips_search_wide_grp(index._h, qd.data_ptr(), ram._lib.DTYPE_F32, 2, k, out_s.data_ptr(), out_i.data_ptr(), 0, dev,
                                        None, 0, 0, gd.data_ptr(), mode, None)

    assert wide_rc(ix, 40, 0) == 0 and wide_rc(ix, 40, 1) == 0
    assert wide_rc(ix, 40, 2) == -1 and b"grp_mode" in lib.mips_last_error()                 # MIPS_E_INVALID
    assert wide_rc(ix, 40, -1) == -1
    assert wide_rc(ix, ram.MAX_K_WIDE + 1, 0) == -3 and wide_rc(f8, 40, 0) == -3 and wide_rc(wide, 40, 0) == -3   # MIPS_E_UNSUPPORTED
    bare = ram.MipsIndex(d)
    bare.add(x)
    assert wide_rc(bare, 40, 0) == -1 and b"label" in lib.mips_last_error()                  # never labelled
    lims = torch.empty(3, dtype=torch.int64, device="cuda")
    radii = np.zeros(2, np.float32)

    def range_rc(index, flags, mode):
        return lib.mips_range_search_grp(index._h, qd.data_ptr(), ram._lib.DTYPE_F32, 2, radii.ctypes.data, lims.data_ptr(), None, None, 0, 0,
                                         flags, None, 0, 0, gd.data_ptr(), mode, None)

    assert range_rc(ix, dev, 0) == 0 and range_rc(ix, dev, 1) == 0
    assert range_rc(ix, dev | ram._lib.OUT_PACKED, 0) == -1                                   # MIPS_OUT_PACKED on the range call
    assert range_rc(ix, dev, 5) == -1 and range_rc(bare, dev, 0) == -1 and range_rc(f8, dev, 0) == -3
    assert lib.mips_index_set_labels(ix._h, gd.data_ptr(), 299, 2, 1, None) == -1            # past ntotal
    assert lib.mips_index_set_labels(bare._h, gd.data_ptr(), 1, 2, 1, None) == -1            # a gap behind 0 labelled rows
