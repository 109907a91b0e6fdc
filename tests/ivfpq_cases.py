"""Inputs and the NumPy restatement of the IVF index over PQ codes (include/mips_hip_ivfpq.h has the definition): train, assign,
residual, encode, the coarse term T, score, search, reconstruct and the scores by id.  The coarse quantiser is the restatement of
tests/ivf_cases.py, the sub-quantisers, the table and the ranking are those of tests/pq_cases.py: imported, not copied.  float32
steps are NumPy float32 operations.  `wrong=` switches ONE deliberate mistake on --
    "coarse_last"   the coarse term added behind the table entries instead of in front of them
    "no_coarse"     the coarse term left out
    "raw_codes"     the row coded as it is instead of its residual
    "fp64"          the sum taken in fp64 and rounded once
    "tie_high"      ties to the highest row
    "one_list_less" one probed list too few
    "no_centroid"   reconstruct without the centroid
-- and tests/test_ivfpq_host.py shows that each changes the bits of a D, an I, a code or a row on a named case, so a kernel that
makes it cannot pass.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_cases as ic  # noqa: E402
import pq_cases as pc  # noqa: E402
from oracle import mips_oracle as orc  # noqa: E402

F = np.float32
KSUB = pc.KSUB
MISTAKES = ("coarse_last", "no_coarse", "raw_codes", "fp64", "tie_high", "one_list_less", "no_centroid")


# ------------------------------------------------------------------ the arithmetic
def probe(q, centroids, nprobe, wrong=None):
    """-> (lists int64 [nq, p], T float32 [nq, p]): the p = min(nprobe, nlist) nearest lists of every query, nearest first (highest
    canonical score, ties to the lowest list), and their canonical scores"""
    p = min(int(nprobe), len(centroids))
    T, L = orc.search_exact_bruteforce(np.asarray(q, dtype=F), np.asarray(centroids, dtype=F), p)
    if wrong == "one_list_less" and p > 1:
        return L[:, :p - 1].astype(np.int64), T[:, :p - 1].astype(F)
    return L.astype(np.int64), T.astype(F)


def assign(x, centroids):
    """int32 [n]: the nearest list of every float32 row"""
    return ic.nearest(x, centroids)[:, 0]


def residuals(x, centroids, a, by_residual=True, wrong=None):
    """r = x - c[a]: one float32 subtraction per column"""
    x = np.asarray(x, dtype=F)
    if not by_residual or wrong == "raw_codes":
        return x
    with np.errstate(over="ignore", invalid="ignore"):
        return (x - centroids[a]).astype(F)


def train(x, nlist, M, niter=10, pq_niter=10, by_residual=True):
    """-> (centroids [nlist, d], codebook [M, 256, dsub]): ic.train on x; pc.train on the residuals of the PQ subsample of x"""
    x = np.asarray(x, dtype=F)
    cen = ic.train(x, nlist, niter)
    R = training_residuals(x, cen, by_residual)
    if not np.isfinite(R).all():
        raise ValueError("a residual overflows")
    return cen, pc.train(R, M, pq_niter)


def training_residuals(x, cen, by_residual=True):
    T = np.ascontiguousarray(pc.training_set(np.asarray(x, dtype=F)))
    return residuals(T, cen, assign(T, cen), by_residual)


def encode(x, cen, cb, by_residual=True, wrong=None):
    """-> (codes uint8 [n, M], assign int32 [n])"""
    a = assign(x, cen)
    return pc.encode(residuals(x, cen, a, by_residual, wrong=wrong), cb), a.astype(np.int32)


def row_scores(T_row, table, codes, by_residual=True, wrong=None):
    """T_row [nq, n] (the coarse term of every row's list for every query), table [nq, M, 256], codes [n, M] -> D float32 [nq, n]:
    acc = T; acc = acc + LUT[m][code_m] in ascending m, float32"""
    nq, M, _ = table.shape
    flat = table.reshape(nq, M * KSUB)
    terms = flat[:, np.arange(M, dtype=np.int64)[None, :] * KSUB + codes.astype(np.int64)]      # [nq, n, M]
    if not by_residual:
        return pc.scores(table, codes, wrong=wrong if wrong == "fp64" else None)
    with np.errstate(over="ignore", invalid="ignore"):
        if wrong == "fp64":
            return (T_row.astype(np.float64) + np.cumsum(terms.astype(np.float64), axis=2)[..., -1]).astype(F)
        if wrong == "no_coarse":
            return pc.scores(table, codes)
        if wrong == "coarse_last":
            return (pc.scores(table, codes) + T_row).astype(F)
        acc = T_row.astype(F).copy()
        for m in range(M):
            acc = (acc + terms[..., m]).astype(F)
        return acc


def coarse_of_rows(q, cen, a):
    """T [nq, n]: the canonical score of every query and the centroid of every row's list"""
    T, L = orc.search_exact_bruteforce(np.asarray(q, dtype=F), np.asarray(cen, dtype=F), len(cen))
    full = np.empty((len(q), len(cen)), F)
    np.put_along_axis(full, L.astype(np.int64), T.astype(F), axis=1)
    return full[:, np.asarray(a, dtype=np.int64)]


def all_scores(q, cen, cb, codes, a, by_residual=True, wrong=None):
    """D [nq, n] of every row with the coarse term of its own list (what score_subset returns)"""
    table = pc.lut(q, cb)
    if len(codes) == 0:
        return np.zeros((len(table), 0), F)
    return row_scores(coarse_of_rows(q, cen, a), table, codes, by_residual, wrong=wrong)


def search(q, cen, cb, codes, a, k, nprobe, idx_offset=0, by_residual=True, wrong=None):
    """-> (D float32 [nq, k], I int64 [nq, k])"""
    q = np.asarray(q, dtype=F)
    D = all_scores(q, cen, cb, codes, a, by_residual, wrong=wrong)
    L, _ = probe(q, cen, nprobe, wrong=wrong)
    out_d = np.full((len(q), k), -np.inf, F)
    out_i = np.full((len(q), k), -1, np.int64)
    a = np.asarray(a, dtype=np.int64)
    for j in range(len(q)):
        rows = np.flatnonzero(np.isin(a, L[j]))
        order = np.lexsort((-rows if wrong == "tie_high" else rows, -D[j, rows].astype(np.float64)))[:k]
        out_d[j, :len(order)] = D[j, rows[order]]
        out_i[j, :len(order)] = rows[order] + idx_offset
    return out_d, out_i


def reconstruct(codes, a, cen, cb, by_residual=True, wrong=None):
    """row i = c[assign_i] + decode(code_i): one float32 addition per column"""
    dec = pc.reconstruct(codes, cb)
    if not by_residual or wrong == "no_centroid":
        return dec
    return (cen[np.asarray(a, dtype=np.int64)] + dec).astype(F)


# ------------------------------------------------------------------ cases
GEOMETRY = ((32, 4), (32, 16), (48, 24), (80, 40), (128, 128))   # (d, M): a partial 16-byte chunk, exactly one, one and a partial one, the 16-wave instance, the largest table
NLISTS = (1, 8, 33)
NTOTALS = (0, 1, 1000, 4097)
NQS = (1, 3, 17)
KS = (1, 5, 29)


def waves(M):
    return 16 if M > 32 else 4


def list_sizes(nlist, n, M):
    """sizes [nlist] that sum to n: 0, 1, 63, 64, 65 and 64 * WAVES +- 1 where they fit, the rest in the last list"""
    w = 64 * waves(M)
    want = [0, 1, 63, 64, 65, w - 1, w + 1]
    sizes = [0] * nlist
    left = n
    for l in range(nlist - 1):
        s = want[l % len(want)]
        if s <= left:
            sizes[l] = s
            left -= s
    sizes[-1] += left
    return np.asarray(sizes, np.int64)


def case_planted(d, M, nlist, n, nq, seed=1, one_list=None, scale=1.0):
    """random centroids, codebook, codes and a shuffled assignment with the sizes of list_sizes (one_list: every row in that list):
    the scan alone (set_centroids / set_codebook / add_codes)"""
    rng = np.random.default_rng(seed * 1000003 + d * 131 + M * 7 + nlist * 17 + n)
    cen = (rng.standard_normal((nlist, d)) * scale).astype(F)
    cb = (rng.standard_normal((M, KSUB, d // M)) * 0.3 * scale).astype(F)
    sizes = list_sizes(nlist, n, M)
    a = np.full(n, one_list, np.int64) if one_list is not None else rng.permutation(np.repeat(np.arange(nlist), sizes))
    return {"d": d, "M": M, "nlist": nlist, "centroids": cen, "codebook": cb, "codes": pc.random_codes(rng, n, M), "assign": a.astype(np.int32),
            "q": rng.standard_normal((nq, d)).astype(F)}


def case_sum_order(seed=2):
    """the coarse term is ~2^12 times the table entries and the entries of sub-quantiser m are scaled by 2^(6 (m mod 4)): T + (a + b)
    and (T + a) + b round differently, and so does every other order of the float32 sum"""
    c = case_planted(32, 8, 8, 1000, 3, seed)
    c["codebook"] = (c["codebook"] * (2.0 ** (6 * (np.arange(8) % 4) - 12))[:, None, None]).astype(F)
    return c


def case_ties(seed=3):
    """the same codes in every row and the same centroid in every list: every probed row scores the same, the best k are the k
    lowest probed rows"""
    c = case_planted(32, 4, 8, 600, 2, seed)
    c["codes"] = np.ascontiguousarray(np.tile(c["codes"][:1], (600, 1)))
    c["centroids"] = np.ascontiguousarray(np.tile(c["centroids"][:1], (8, 1)))
    return c


def case_train(n=1000, d=32, M=4, nlist=8, seed=5):
    """clustered rows: residual coding has something to remove"""
    rng = np.random.default_rng(seed * 7919 + n + d)
    cen = ic.normalise(rng.standard_normal((nlist, d)).astype(F))
    x = (cen[rng.integers(0, nlist, n)] + 0.2 * rng.standard_normal((n, d))).astype(F)
    return {"d": d, "M": M, "nlist": nlist, "x": x, "q": (cen[rng.integers(0, nlist, 5)] + 0.2 * rng.standard_normal((5, d))).astype(F)}
