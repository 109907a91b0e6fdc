"""The range search over the probed lists (include/mips_hip_ivf_range.h: mips_ivf_range_search / _grp) restated in NumPy, and its
cases, on top of tests/ivf_cases.py (nearest), tests/ivf_search_cases.py (stored) and tests/ivf_filter_cases.py (admitted).

Row i is a hit of query j iff its list lies in P(q_j), it is admitted for j, and the score the search would REPORT for (j, i) -- the
storage's canonical score; sq8: D = (float)((double)S + B_q) -- is strictly above radii[j] as float32.  The result is CSR: lims int64
[nq + 1], the hits of query j at [lims[j], lims[j + 1]) in ascending row order, scores the reported values, ids row + idx_offset.

`wrong=` switches ONE deliberate mistake on; tests/test_ivf_range_host.py shows that every one of them changes the result of a named
case, so a kernel that makes it cannot pass:
    "non_strict"    >= in place of >
    "rule_on_S"     sq8 compared on S instead of D
    "list_order"    the hits in probe order (the concatenation of the probed lists) instead of ascending row
    "first_radius"  radii[0] used for every query
    "all_rows"      unprobed rows returned
    "post_count"    lims counted before the filter
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ivf_cases as iv  # noqa: E402
import ivf_filter_cases as fc  # noqa: E402
import ivf_search_cases as sc  # noqa: E402
from oracle import mips_oracle as orc  # noqa: E402

F = np.float32
WRONG = ("non_strict", "rule_on_S", "list_order", "first_radius", "all_rows", "post_count")
SORT_LDS = 4096          # kRangeSortLds of csrc/ivf_range_math.hpp: the longest stretch the ordering step sorts in LDS
SLICE = 4096             # kRangeSlice: queries of one pass


def sort_class(n):
    """range_sort_class of csrc/ivf_range_math.hpp: the smallest power of two >= n"""
    P = 1
    while P < n:
        P *= 2
    return P


def probed_scores(rows, q, assign, centroids, nprobe, dtype, sq8_params=None, sel=None, labels=None, q_labels=None, mode="exclude", sel_bit0=0,
                  wrong=None):
    """-> per query (ids int64 ascending [probe order under "list_order"], S float32, reported float32, admitted bool): the probed rows of
    the query (all rows under "all_rows"), their ranking keys, the scores a search reports for them, and the filter's verdict"""
    q = np.asarray(q, dtype=F)
    assign = np.asarray(assign)
    P = iv.nearest(q, centroids, min(int(nprobe), len(centroids)))
    X, Y, bias = sc.stored(rows, q, dtype, sq8_params)
    out = []
    for j in range(len(q)):
        if wrong == "all_rows":
            ids = np.arange(len(assign), dtype=np.int64)
        elif wrong == "list_order":
            ids = np.concatenate([np.flatnonzero(assign == l) for l in P[j]] + [np.zeros(0, np.int64)]).astype(np.int64)
        else:
            ids = np.flatnonzero(np.isin(assign, P[j])).astype(np.int64)
        ok = fc.admitted(ids, j, sel, sel_bit0, labels, q_labels, mode)
        if wrong != "post_count":                          # (only that mistake looks at a row the filter refuses)
            ids, ok = ids[ok], ok[ok]
        key = orc.canonical_pairs(Y[j:j + 1], X, ids[None, :])[0].astype(F) if len(ids) else np.zeros(0, F)
        rep = key
        if bias is not None:
            with np.errstate(invalid="ignore"):
                rep = np.where(np.isfinite(key), (key.astype(np.float64) + bias[j]).astype(F), key).astype(F)
        out.append((ids, key, rep, ok))
    return out


def range_search(rows, q, assign, centroids, radii, nprobe, dtype, sq8_params=None, sel=None, labels=None, q_labels=None, mode="exclude",
                 idx_offset=0, sel_bit0=0, wrong=None):
    """-> (lims int64 [nq + 1], D float32 [lims[-1]], I int64 [lims[-1]])"""
    assert wrong is None or wrong in WRONG
    nq = len(q)
    radii = np.broadcast_to(np.asarray(radii, dtype=F), (nq,))
    per = probed_scores(rows, q, assign, centroids, nprobe, dtype, sq8_params, sel, labels, q_labels, mode, sel_bit0, wrong)
    lims = np.zeros(nq + 1, np.int64)
    Ds, Is = [np.zeros(0, F)], [np.zeros(0, np.int64)]
    for j, (ids, key, rep, ok) in enumerate(per):
        r = radii[0] if wrong == "first_radius" else radii[j]
        val = key if wrong == "rule_on_S" else rep
        with np.errstate(invalid="ignore"):
            above = (val >= r) if wrong == "non_strict" else (val > r)
        hit = above & ok
        lims[j + 1] = lims[j] + int((above if wrong == "post_count" else hit).sum())
        Ds.append(rep[hit])
        Is.append(ids[hit] + idx_offset)
    return lims, np.concatenate(Ds).astype(F), np.concatenate(Is).astype(np.int64)


def bruteforce(rows, q, assign, centroids, radii, nprobe, dtype, sq8_params=None, sel=None, labels=None, q_labels=None, mode="exclude", sel_bit0=0):
    """the same result row by row: the oracle's exact brute force over every probed and admitted row (k = all of them), the reported
    scores tested against the radius one by one, the survivors put into ascending row order"""
    q = np.asarray(q, dtype=F)
    radii = np.broadcast_to(np.asarray(radii, dtype=F), (len(q),))
    lims, Ds, Is = [0], [], []
    for j in range(len(q)):
        d, i = fc.bruteforce_on_admitted(rows, q[j:j + 1], assign, centroids, len(rows), nprobe, dtype, sq8_params, sel=sel, labels=labels,
                                         q_labels=None if q_labels is None else q_labels[j:j + 1], mode=mode, sel_bit0=sel_bit0)
        hits = sorted((int(i[0, t]), d[0, t]) for t in range(len(rows)) if i[0, t] >= 0 and d[0, t] > radii[j])
        lims.append(lims[-1] + len(hits))
        Is += [h[0] for h in hits]
        Ds += [h[1] for h in hits]
    return np.array(lims, np.int64), np.array(Ds, F), np.array(Is, np.int64)


def radius_for_count(reported, c):
    """a radius with exactly c hits among `reported` (float32 scores): the (c + 1)-th largest of them, -inf when c takes them all;
    None when the c-th and the (c + 1)-th are equal"""
    s = np.sort(np.asarray(reported, dtype=F))[::-1]
    if c >= len(s):
        return F(-np.inf) if c == len(s) else None
    if c > 0 and s[c - 1] == s[c]:
        return None
    return F(s[c])


def same(a, b):
    return all(x.shape == y.shape for x, y in zip(a, b)) and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and \
        np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ------------------------------------------------------------------ cases
def case_round_robin(n, d, nq, nlist, seed=12):
    """Gaussian rows assigned round-robin by PLANTED assignments (row i in list i % nlist), so that the probed lists interleave
    maximally in row order; planted centroids e_l, Gaussian queries"""
    rng = np.random.default_rng(seed * 9973 + n + d)
    cen = np.zeros((nlist, d), F)
    cen[np.arange(nlist), np.arange(nlist)] = 1
    return {"rows": rng.standard_normal((n, d)).astype(F), "q": rng.standard_normal((nq, d)).astype(F), "nlist": nlist, "centroids": cen,
            "assign": (np.arange(n) % nlist).astype(np.int32)}


def case_equal(seed=13):
    """case_round_robin(600, 32, 4, 4) in which rows 7, 300 and 599 are copies of one row: on an f32 index the radius of query 0 is
    EXACTLY their score, so the strict rule leaves all three out and `>=` takes them in"""
    c = case_round_robin(600, 32, 4, 4, seed)
    c["rows"][[300, 599]] = c["rows"][7]
    c["copies"] = np.array([7, 300, 599])
    return c


STRETCH_COUNTS = (63, 64, 65, 127, 128, 129)
STRETCH_RADIUS = 50.0


def case_stretch(seed=14):
    """fc.case_queue's geometry without its bitmaps: 24 000 rows of d = 32, 20 000 of them in list 0 by PLANTED assignments, the
    centroids e_0 .. e_3, nprobe = 1.  Searched with so many queries that the list is ONE segment, wave 0 of a workgroup walks the
    positions p with p % 256 < 64.  plant[c] (c of STRETCH_COUNTS, disjoint sets) names c rows of wave 0's stretch, scattered over
    its windows; the rows of the u-th set carry 100 in column 4 + u, every other row 0 there.  q6[u] = 2 e_0 + noise + e_(4 + u) (zero
    in the other planted columns) scores ~100 on its set and below ~15 on every other row, so at STRETCH_RADIUS wave 0 sees exactly
    c hits over its stretch -- in passes of no, one or several hits -- and the other waves none.  A test repeats q6 with period 6."""
    c = fc.case_queue(seed)
    rng = np.random.default_rng(seed + 1)
    pos = np.arange(fc.QUEUE_BIG)
    wave0 = rng.permutation(pos[(pos % 256) < 64])
    rows = c["rows"].copy()
    rows[:, 4:4 + len(STRETCH_COUNTS)] = 0
    q6 = c["q"][:len(STRETCH_COUNTS)].copy()
    q6[:, 4:4 + len(STRETCH_COUNTS)] = 0
    plant, at = {}, 0
    for u, cnt in enumerate(STRETCH_COUNTS):
        plant[cnt] = c["big"][np.sort(wave0[at:at + cnt])]
        at += cnt
        rows[plant[cnt], 4 + u] = 100
        q6[u, 4 + u] = 1
    return {"rows": rows, "q6": q6, "nlist": 4, "centroids": c["centroids"], "assign": c["assign"], "plant": plant, "big": c["big"]}
