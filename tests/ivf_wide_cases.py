"""The wide IVF search (include/mips_hip_ivf.h: mips_ivf_search_wide / _grp) restated in NumPy, and its cases, on top of
tests/ivf_filter_cases.py and tests/ivf_search_cases.py -- whose restatements take any k: the definition of the wide search IS the
definition of the search over the probed lists, with 1 <= k <= 1024.

`wrong=` switches ONE deliberate mistake of a wider selection on; tests/test_ivf_wide_host.py shows that each of them changes the
result of at least one case, so a kernel that makes it cannot pass:
    "arrival_ties"        ties inside the selection broken by arrival (the position in the concatenation of the probed lists)
                          instead of by the row
    "key_only_threshold"  a selection that fills with the first k candidates in arrival order and then admits only a candidate
                          whose KEY beats the k-th key: the row half of the order is dropped, a tie with a lower row is lost
    "capacity_for_k"      the pool's capacity KP (64, 256 or 1024, the smallest >= k) used where k belongs: the k-th result is
                          taken from slot KP - 1
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
MAX_K_WIDE = 1024
WRONG = ("arrival_ties", "key_only_threshold", "capacity_for_k")
KS = (1, 29, 30, 64, 65, 256, 257, 1024)


def pool_class(k):
    """KP of csrc/ivf_wide_math.hpp"""
    return 64 if k <= 64 else 256 if k <= 256 else 1024


def search(rows, q, assign, centroids, k, nprobe, dtype, sq8_params=None, sel=None, labels=None, q_labels=None, mode="exclude", wrong=None,
           idx_offset=0, sel_bit0=0):
    """-> (D float32 [nq, k], I int64 [nq, k]); wrong=None: fc.search, the restatement of the definition"""
    if wrong is None:
        return fc.search(rows, q, assign, centroids, k, nprobe, dtype, sq8_params, sel=sel, labels=labels, q_labels=q_labels, mode=mode,
                         idx_offset=idx_offset, sel_bit0=sel_bit0)
    assert wrong in WRONG
    q = np.asarray(q, dtype=F)
    assign = np.asarray(assign)
    P = iv.nearest(q, centroids, min(int(nprobe), len(centroids)))
    X, Y, bias = sc.stored(rows, q, dtype, sq8_params)
    D = np.full((len(q), k), -np.inf, F)
    I = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        ids = np.concatenate([np.flatnonzero(assign == l) for l in P[j]] + [np.zeros(0, np.int64)]).astype(np.int64)   # arrival order
        ids = ids[fc.admitted(ids, j, sel, sel_bit0, labels, q_labels, mode)]
        if len(ids) == 0:
            continue
        key = orc.canonical_pairs(Y[j:j + 1], X, ids[None, :])[0].astype(F)
        if wrong == "arrival_ties":
            order = np.argsort(-key, kind="stable")[:k]
        elif wrong == "key_only_threshold":
            keep = list(range(min(k, len(ids))))
            for c in range(k, len(ids)):
                worst = max(keep, key=lambda u: (-key[u], ids[u]))                       # the k-th of the pool, by the right order
                if key[c] > key[worst]:                                                  # ... but admission looks at the key only
                    keep[keep.index(worst)] = c
            keep = np.array(keep, np.int64)
            order = keep[np.lexsort((ids[keep], -key[keep]))]
        else:
            order = np.lexsort((ids, -key))
            kp = pool_class(k)
            if len(order) >= kp > k:
                order = np.concatenate([order[:k - 1], order[kp - 1:kp]])
            order = order[:k]
        out = key[order]
        if bias is not None:
            out = (out.astype(np.float64) + bias[j]).astype(F)
        D[j, :len(order)] = out
        I[j, :len(order)] = ids[order] + idx_offset
    return D, I


def prefix(res, k):
    return res[0][:, :k], res[1][:, :k]


# ------------------------------------------------------------------ cases
def case_gauss():
    """3000 x 64 Gaussian rows, 16 trained lists, 12 queries: on a 256-CU device S = 32 -- segments of a few rows, pools that never
    fill, partials that are mostly padding"""
    return iv.case_gauss(3000, 64, 12, 16)


FILL_SIZES = (4095, 4096, 4097, 12000)


def queries_for_one_segment(p, cus):
    """the fewest queries for which choose_segments (csrc/ivf_search_math.hpp) gives S = 1: nq p >= 2 cus"""
    return -(-2 * int(cus) // int(p))


def case_fill(nq, seed=11):
    """d = 64, four lists of 4095, 4096, 4097 and 12 000 rows by PLANTED assignments, shuffled; nprobe = 4 probes them all.  Searched
    with S = 1 (nq from queries_for_one_segment(4, cus)) the four waves of a workgroup take 64-position windows in turn, so the waves
    of the first three lists see 1023 / 1024 (wave 3: 1023), exactly 1024, and 1024 / 1025 (wave 0) positions, those of the long list
    3000: at k = 1024 a pool that stays one short, pools that fill exactly at the last row, one that meets one row after its sort."""
    rng = np.random.default_rng(seed)
    n = sum(FILL_SIZES)
    assign = rng.permutation(np.repeat(np.arange(4), FILL_SIZES)).astype(np.int32)
    rows = rng.standard_normal((n, 64)).astype(F)
    cen = np.zeros((4, 64), F)
    cen[np.arange(4), np.arange(4)] = 1
    return {"rows": rows, "q": rng.standard_normal((nq, 64)).astype(F), "nlist": 4, "centroids": cen, "assign": assign}


ORDERED_L = 6000


def case_ordered(nq):
    """Two lists of 6000 rows, d = 64, PLANTED assignments (rows alternate between the lists).  Row i carries (s // 128, s % 128, 0,
    ...) and every query is 2^e (128, 1, 0, ...): the score 2^e s is exact on every storage (an 'sq8' index takes vmin = 0, vdiff =
    255, so its codes are the values: it ranks on S = 2^e s and reports D = S + B_q, B_q = 2^e 64.5).  List 0: s ascends with the row number -- every row beats the threshold, the maximum of
    insertions; list 1: s descends -- none after the fill.  Scores repeat ACROSS the lists (ties for the merge)."""
    n = 2 * ORDERED_L
    assign = (np.arange(n) % 2).astype(np.int32)
    pos = np.arange(n) // 2
    s = np.where(assign == 0, pos, ORDERED_L - 1 - pos)
    rows = np.zeros((n, 64), F)
    rows[:, 0], rows[:, 1] = s // 128, s % 128
    q = np.zeros((nq, 64), F)
    scale = (2.0 ** (np.arange(nq) % 4)).astype(F)
    q[:, 0], q[:, 1] = 128 * scale, scale
    cen = np.zeros((2, 64), F)
    cen[0, 0], cen[1, 1] = 1, 1
    return {"rows": rows, "q": q, "nlist": 2, "centroids": cen, "assign": assign, "score": s, "distinct_queries": 4,
            "sq8_params": (np.zeros(64, F), np.full(64, 255, F))}


FLOOD_COPIES = 1100


def case_flood(n=3000, d=32, seed=7):
    """sc.case_ties with 1100 copies: one vector stored 1100 times at scattered rows, copy c in list c mod 3 by PLANTED assignments,
    the other rows over all four lists; the one query is that vector and P(q) = (0, 1, 2).  nprobe = 3, k = 1024: the lowest 1024 of
    those rows, ascending."""
    rng = np.random.default_rng(seed * 65537 + n + d)
    rows = rng.standard_normal((n, d)).astype(F)
    v = (4 * rng.standard_normal(d)).astype(F)
    at = np.sort(rng.choice(n, FLOOD_COPIES, replace=False))
    rows[at] = v
    assign = rng.integers(0, 4, n).astype(np.int32)
    assign[at] = rng.permutation(FLOOD_COPIES) % 3
    u = iv.normalise(v)[0]
    cen = np.stack([u, (F(0.9) * u).astype(F), (F(0.8) * u).astype(F), -u]).astype(F)
    return {"rows": rows, "q": v[None, :].copy(), "nlist": 4, "centroids": cen, "assign": assign, "copies": at}
