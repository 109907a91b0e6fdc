"""Wide top-k (mips_search_wide and its filtered and grouped forms) on rows in an ORDER and in a MULTIPLICITY that Gaussian rows in
random order never have (tests/wide_cases.py; tests/test_wide_orders_host.py checks the constructions on the CPU).  Everything is
compared bit for bit with the oracle; no tolerances.

trending   the score climbs with the row number, so for a third of the lanes nearly every row of EVERY chunk passes the threshold
           (share 0.94 per 8192 rows): the register cursor of the scan reaches the segment capacity in the doubled chunks, the
           select kernel is fed by full segments (several sorts per launch, the threshold rising inside one launch, the binary
           search over counters that are all at the capacity), and the neighbour lanes of the same wave append nothing.
floods     400 copies of every vector against pools of 164 (bf16) / 381 (fp32-exact) entries: every query is flagged, so the
           settlement runs second and third rounds of 256 slots, walks more than one row chunk, meets flagged queries in the
           second query slice, and wide_finalize_kernel writes (plain and packed) for slots >= 256.

The shapes are the smallest that reach those paths with the geometry of csrc/host_wide.hpp: 128 splits up to 128 queries and 16
at 4096; 1, 1, 2, 4, 8 tiles per split and chunk; settlement rounds of 256 flagged queries over chunks of at most 2^17 rows."""
import os
import sys
import time

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import wide_cases
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

WIDE = "mips::wide_scan_kernel"
MASKED = "mips::masked_scan_kernel"
GROUPED = "mips::grouped_scan_kernel"
NONE = ram.LABEL_NONE

# (n, d, nq).  782 tiles: chunks of 128, 128, 256 and 270 tiles, up to 4 tiles per split, two query tiles (the second ragged), a
# ragged last row tile / 1094 tiles, one query tile: the last chunk runs 8 tiles per split / two query slices, 16 splits, chunks
# of at most 8192 rows
TREND_FIRST, TREND_DEEP, TREND_SLICES = (100003, 64, 130), (140000, 32, 40), (20000, 64, 4100)
# (R, d, nq) at m = 400 copies.  8000 rows, settlement rounds of 256, 256 and 88 slots / 140000 rows > 2^17: the first round
# (256 slots) walks two row chunks, the second has 44 slots / the second query slice holds 4 flagged queries
FLOOD_ROUNDS, FLOOD_CHUNKS, FLOOD_SLICES = (20, 64, 600), (350, 32, 300), (20, 64, 4100)
COPIES = 400
K = 100
HEAD = 1500      # places of the oracle's ranking the filtered trending expectations are cut from (asserted to be enough)

_CACHE = {}


def _cached(key, make):
    """References and inputs are computed once, shared between the tests that need them, and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _search_exact(q, x, k, metric):
    """orc.search_exact in batches of 1024 queries (its float64 score matrix of 4100 queries would take 0.6 GB per copy)."""
    parts = [orc.search_exact(q[j:j + 1024], x, k, metric=metric) for j in range(0, len(q), 1024)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _trend(shape):
    return _cached(("trend", shape), lambda: wide_cases.trending(*shape)[:2])


def _trend_ref(shape, metric, k):
    """search_exact at K = 100, once per shape and metric; a smaller k is its first k columns (one ranking, (value, row))."""
    x, q = _trend(shape)
    kk = max(k, K)
    es, ei = _cached(("trend ref", shape, metric, kk), lambda: _search_exact(q, x, kk, metric))
    return es[:, :k], ei[:, :k]


def _flood(shape):
    R, d, nq = shape
    return _cached(("flood", shape), lambda: wide_cases.floods(R, COPIES, d, nq)[:2])


def _flood_ref(shape, metric, k=K):
    x, q = _flood(shape)
    return _cached(("flood ref", shape, metric, k), lambda: orc.search_exact_bruteforce(q, x, k, metric=metric))


def _same(got, exp, what=""):
    s, i = got
    es, ei = exp
    if isinstance(s, torch.Tensor):
        s, i = s.cpu().numpy(), i.cpu().numpy()
    bad = np.flatnonzero((i != ei).any(axis=1))
    assert np.array_equal(i, ei), f"{what}: indices differ in {len(bad)} queries, first {bad[:5]}"
    assert np.array_equal(s.view(np.int32), es.view(np.int32)), f"{what}: scores differ"


def _unpack(packed):
    s, i = ram.unpack_gathered(packed[None], 1)
    return s.cpu().numpy(), i.cpu().numpy()


def _admit(nq, n, mask=None, labels=None, qlabels=None, mode="exclude"):
    """bool [nq, n]: may row i answer query j?  A row mask for all queries and / or the group rule per query."""
    adm = np.ones((nq, n), bool)
    if labels is not None:
        labels, qlabels = np.asarray(labels, np.int64), np.asarray(qlabels, np.int64)
        eq = labels[None, :] == qlabels[:, None]
        adm = np.where((qlabels == NONE)[:, None], True, eq if mode == "only" else ~eq)
    return adm if mask is None else adm & np.asarray(mask, bool)[None, :]


def _filter_ranking(head, admit, k, metric):
    """head = (scores, ids) [nq, places], the first places of the oracle's ranking of ALL rows (row numbers, phi and all) -> the k
    best admitted rows per query: the oracle on the admitted rows with the row numbers mapped back.  Every query must find its k
    within the head -- asserted, so cutting the ranking short changes nothing."""
    hs, hi = head
    nq = hs.shape[0]
    s = np.empty((nq, k), np.float32)
    i = np.empty((nq, k), np.int64)
    for j in range(nq):
        keep = np.flatnonzero(admit[j][hi[j]])[:k]
        assert len(keep) == k, f"query {j}: only {len(keep)} admitted rows among the first {hs.shape[1]} places"
        s[j], i[j] = hs[j, keep], hi[j, keep]
    return s, i


def _index(x, metric, dtype):
    ix = ram.MipsIndex(x.shape[1], metric=metric, dtype=dtype)
    ix.add(x)
    return ix


# ------------------------------------------------------------------ 1. trending rows, plain
@pytest.mark.parametrize("shape", [TREND_FIRST, TREND_DEEP, TREND_SLICES], ids=["782tiles", "8tiles-per-split", "2slices"])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_trending_rows_match_oracle(dtype, metric, shape):
    t0 = time.time()
    x, q = _trend(shape)
    k = K if dtype == "bf16" else 64
    exp = _trend_ref(shape, metric, k)
    t1 = time.time()
    ix = _index(x, metric, dtype)
    got = ix.search_wide(q, k)
    st = ix.margin_stats()
    print(f"trending {shape} {dtype} metric={metric} k={k}: {st}; oracle {t1 - t0:.1f} s, index {time.time() - t1:.1f} s")
    assert ix.last_kernel.startswith(WIDE)
    assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] >= 0
    _same(got, exp, "trending")


@pytest.mark.parametrize("metric", [0, 1])
def test_trending_rows_k1024_overflow_the_select_batch(metric):
    """k' = 1088: a select launch that is fed full segments sorts and cuts its 4096-entry buffer once per batch of 2048."""
    x, q = _trend(TREND_FIRST)
    q = q[:40]
    ix = _index(x, metric, "bf16")
    got = ix.search_wide(q, 1024)
    st = ix.margin_stats()
    print(f"trending k=1024 metric={metric}: {st}")
    assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] >= 0
    _same(got, orc.search_exact(q, x, 1024, metric=metric), "trending k = 1024")


# ------------------------------------------------------------------ 2. trending rows, masked and grouped
def _trend_head(metric):
    x, q = _trend(TREND_FIRST)
    return _cached(("trend head", metric), lambda: orc.search_exact(q, x, HEAD, metric=metric))


@pytest.mark.parametrize("metric", [0, 1])
def test_trending_rows_masked_in_runs(metric):
    """Runs of 300 selected / 300 cleared rows: whole tiles are empty (next_tile steps over them, the prefetch crosses them)."""
    n, d, nq = TREND_FIRST
    x, q = _trend(TREND_FIRST)
    mask = wide_cases.run_mask(n)
    exp = _filter_ranking(_trend_head(metric), _admit(nq, n, mask=mask), K, metric)
    ix = _index(x, metric, "bf16")
    got = ix.search_wide(q, K, selector=ram.Selector.from_mask(mask))
    st = ix.margin_stats()
    print(f"trending masked metric={metric}: {st}")
    assert ix.last_kernel == MASKED
    assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] >= 0
    _same(got, exp, "trending, masked")


@pytest.mark.parametrize("mode", ["exclude", "only"])
@pytest.mark.parametrize("metric", [0, 1])
def test_trending_rows_grouped(metric, mode):
    n, d, nq = TREND_FIRST
    x, q = _trend(TREND_FIRST)
    labels = np.arange(n) % 7
    ql = np.arange(nq) % 7                                         # (the query kinds cycle by 3: every kind meets every label)
    exp = _filter_ranking(_trend_head(metric), _admit(nq, n, labels=labels, qlabels=ql, mode=mode), K, metric)
    ix = _index(x, metric, "bf16")
    ix.set_labels(labels)
    got = ix.search_wide(q, K, groups=ql, group_mode=mode)
    st = ix.margin_stats()
    print(f"trending grouped metric={metric} {mode}: {st}")
    assert ix.last_kernel == GROUPED
    assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] >= 0
    _same(got, exp, f"trending, grouped, {mode}")


# ------------------------------------------------------------------ 3. floods, plain: every query is settled
_FLOOD_CASES = [(s, dt, m) for s in (FLOOD_ROUNDS, FLOOD_SLICES) for dt in ("bf16", "f32") for m in (0, 1)]
_FLOOD_CASES += [(FLOOD_CHUNKS, "bf16", 0), (FLOOD_CHUNKS, "bf16", 1), (FLOOD_CHUNKS, "f32", 1)]   # (bounds the oracle's time)


@pytest.mark.parametrize("shape,dtype,metric", _FLOOD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_floods_settle_every_query(shape, dtype, metric):
    """margin_stats counts per CALL (the flagged word is cleared once per call and summed over the query slices), so flagged ==
    nq also holds for the 4100 queries of two slices."""
    t0 = time.time()
    R, d, nq = shape
    x, q = _flood(shape)
    exp = _flood_ref(shape, metric)
    t1 = time.time()
    assert (exp[0] == exp[0][:, :1]).all() and (np.diff(exp[1], axis=1) == R).all()    # (the construction does what it says)
    ix = _index(x, metric, dtype)
    got = ix.search_wide(q, K)
    st = ix.margin_stats()
    print(f"floods {shape} {dtype} metric={metric}: {st}; oracle {t1 - t0:.1f} s, index {time.time() - t1:.1f} s")
    assert st == {"flagged": nq, "rescanned": nq, "unresolved": 0}
    _same(got, exp, "floods")
    if shape == FLOOD_ROUNDS:
        qd = torch.from_numpy(q).cuda()                            # stream-ordered form
        dev = ix.search_wide(qd, K)
        assert dev[0].is_cuda and dev[1].is_cuda
        _same(dev, exp, "floods, device")
        assert ix.margin_stats() == {"flagged": nq, "rescanned": nq, "unresolved": 0}
        packed = _unpack(ix.search_wide_packed(qd, K))           # wide_finalize_kernel's packed writer, slots >= 256 included
        _same(packed, got, "floods, packed against plain")
        assert ix.margin_stats() == {"flagged": nq, "rescanned": nq, "unresolved": 0}


# ------------------------------------------------------------------ 4. floods, masked and grouped
def _flood_head(metric):
    """The first 400 places of every query's ranking: the 400 copies of its best vector, in row order."""
    return _flood_ref(FLOOD_ROUNDS, metric, COPIES)


@pytest.mark.parametrize("metric", [0, 1])
def test_floods_masked_settle_every_query(metric):
    """The selector clears the lowest 150 copies of every vector: 250 > k' remain, every query is still flagged, and the answer
    starts at copy 150 -- the settlement (three rounds) must not bring a cleared copy back."""
    R, d, nq = FLOOD_ROUNDS
    x, q = _flood(FLOOD_ROUNDS)
    n = len(x)
    mask = np.arange(n) // R >= 150
    head = _flood_head(metric)
    _same((head[0][:, :K], head[1][:, :K]), _flood_ref(FLOOD_ROUNDS, metric), "the head's first k places")
    exp = _filter_ranking(head, _admit(nq, n, mask=mask), K, metric)
    assert np.array_equal(exp[1], head[1][:, :1] + R * (150 + np.arange(K))[None, :])
    ix = _index(x, metric, "bf16")
    got = ix.search_wide(q, K, selector=ram.Selector.from_mask(mask))
    st = ix.margin_stats()
    print(f"floods masked metric={metric}: {st}")
    assert ix.last_kernel == MASKED
    assert st == {"flagged": nq, "rescanned": nq, "unresolved": 0}
    _same(got, exp, "floods, masked")


@pytest.mark.parametrize("metric", [0, 1])
def test_floods_grouped_settle_every_query(metric):
    """Row label = copy number mod 4, exclude mode, query labels cycling 0 .. 3 with one query in ten LABEL_NONE: 300 (400) > k'
    admitted copies of the best vector, every query flagged, each settled under its own label."""
    R, d, nq = FLOOD_ROUNDS
    x, q = _flood(FLOOD_ROUNDS)
    n = len(x)
    labels = (np.arange(n) // R) % 4
    ql = np.arange(nq) % 4
    ql[::10] = NONE
    exp = _filter_ranking(_flood_head(metric), _admit(nq, n, labels=labels, qlabels=ql, mode="exclude"), K, metric)
    assert (exp[0] == exp[0][:, :1]).all()
    ix = _index(x, metric, "bf16")
    ix.set_labels(labels)
    got = ix.search_wide(q, K, groups=ql, group_mode="exclude")
    st = ix.margin_stats()
    print(f"floods grouped metric={metric}: {st}")
    assert ix.last_kernel == GROUPED
    assert st == {"flagged": nq, "rescanned": nq, "unresolved": 0}
    _same(got, exp, "floods, grouped")


# ------------------------------------------------------------------ 5. floods whose first pass is wrong: only the settlement can be right
@pytest.mark.parametrize("metric", [0, 1])
def test_graded_floods_are_put_right_by_the_settlement(metric):
    """In the floods above the pool already holds the answer (the lowest copies) and the settlement merely confirms it.  Here
    (wide_cases.floods_graded, fp32-exact index) the copies of a vector share one bf16 image, so the scan keeps the 381 LOWEST,
    while the canonical score grows with the copy number: the answer is the 100 HIGHEST copies, 19 of them outside every pool.
    A settlement round that did not run, ran on the wrong slot or wrote the wrong output row leaves a wrong result in place:
    600 queries, rounds of 256, 256 and 88 slots."""
    R, d, nq = FLOOD_ROUNDS
    x, q, _ = _cached(("graded",), lambda: wide_cases.floods_graded(R, COPIES, d, nq))
    exp = _cached(("graded ref", metric), lambda: orc.search_exact_bruteforce(q, x, K, metric=metric))
    # every result row is a copy the 381 lowest cannot include for at least 19 places (a query whose two best vectors lie within
    # 400 * 2^-19 of each other draws on both: more such places, never fewer)
    assert (exp[1] // R >= COPIES - K).all() and ((exp[1] // R >= 381).sum(axis=1) >= COPIES - 381).all()
    ix = _index(x, metric, "f32")
    got = ix.search_wide(q, K)
    st = ix.margin_stats()
    print(f"graded floods metric={metric}: {st}")
    assert st == {"flagged": nq, "rescanned": nq, "unresolved": 0}
    _same(got, exp, "graded floods")
    qd = torch.from_numpy(q).cuda()
    _same(_unpack(ix.search_wide_packed(qd, K)), exp, "graded floods, packed")
