"""Inputs and the NumPy restatement of the IVF index (include/mips_hip_ivf.h has the definition): train, assign, list table and
probe.  Canonical scores and rankings come from the oracle's exact brute force (sequential fp64 sums, ties to the lowest list);
sums that the definition spells out are np.cumsum (sequential).  train(wrong="sum_order") switches ONE deliberate mistake on;
tests/test_ivf_host.py shows that it changes a centroid, so a kernel that makes it cannot pass.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mips_oracle as orc  # noqa: E402
from oracle import synth  # noqa: E402

F = np.float32


# ------------------------------------------------------------------ the arithmetic
def normalise(v):
    """rows of v [.., d] float32: t = sequential fp64 sum of squares; t == 0 stays; else (float)((double)v / sqrt(t))"""
    v = np.atleast_2d(np.asarray(v, dtype=F))
    v64 = v.astype(np.float64)
    t = np.cumsum(v64 * v64, axis=1)[:, -1]
    r = np.sqrt(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (v64 / r[:, None]).astype(F)
    return np.where((t == 0)[:, None], v, out).astype(F)


def nearest(x, centroids, p=1):
    """int32 [n, p]: the p nearest lists of every float32 row of x -- highest canonical score, ties to the lowest list"""
    _, i = orc.search_exact_bruteforce(np.asarray(x, dtype=F), np.asarray(centroids, dtype=F), int(p))
    return i.astype(np.int32)


def training_set(x, nlist):
    n = len(x)
    m = 256 * nlist if n > 256 * nlist else n
    return x if m == n else x[(np.arange(m, dtype=np.int64) * n) // m]


def train(x, nlist, niter=10, wrong=None):
    """-> centroids float32 [nlist, d]"""
    T = np.ascontiguousarray(training_set(np.asarray(x, dtype=F), nlist))
    m = len(T)
    c = normalise(T[(np.arange(nlist, dtype=np.int64) * m) // nlist])
    for _ in range(niter):
        a = nearest(T, c)[:, 0]
        for l in np.unique(a):
            mem = T[a == l].astype(np.float64)            # ascending i
            if wrong == "sum_order":
                mem = mem[::-1]
            s = np.cumsum(mem, axis=0)[-1]
            c[l] = normalise((s / np.float64(len(mem))).astype(F))[0]
    return c


def list_table(assign, nlist):
    """-> (offsets int64 [nlist + 1], rows int64 [n] ascending inside each list)"""
    assign = np.asarray(assign)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    return off, np.argsort(assign, kind="stable").astype(np.int64)


# ------------------------------------------------------------------ cases: dict(rows, q, nlist[, centroids])
def case_gauss(n, d, nq, nlist, seed=1):
    rng = np.random.default_rng(seed * 1000003 + n * 31 + d)
    return {"rows": rng.standard_normal((n, d)).astype(F), "q": rng.standard_normal((nq, d)).astype(F), "nlist": nlist}


def case_clustered(n, d, nq, nlist, seed=2, noise=0.01):
    """nlist well-separated centres (random unit vectors, pairwise cosines ~ d^-1/2), rows = centre + small noise in contiguous
    blocks (the evenly spaced initial rows then fall into different clusters), queries near centres"""
    rng = np.random.default_rng(seed * 7919 + n + d)
    cen = normalise(rng.standard_normal((nlist, d)).astype(F))
    m = 256 * nlist if n > 256 * nlist else n
    starts = (np.arange(nlist, dtype=np.int64) * m) // nlist          # the initial rows of train(), as rows of x:
    starts = starts if m == n else (starts * n) // m                  # cluster l begins at the l-th of them
    lab = np.searchsorted(starts, np.arange(n), side="right") - 1
    rows = (cen[lab] + noise * rng.standard_normal((n, d))).astype(F)
    ql = rng.integers(0, nlist, nq)
    q = (cen[ql] + noise * rng.standard_normal((nq, d))).astype(F)
    return {"rows": rows, "q": q, "nlist": nlist, "labels": lab, "qlabels": ql}


def case_duplicates(n, d, nq, nlist, seed=3):
    """every vector stored three times"""
    c = case_gauss((n + 2) // 3, d, nq, nlist, seed)
    c["rows"] = np.ascontiguousarray(np.tile(c["rows"], (3, 1))[:n])
    return c


def case_cancel(n, d, seed=5):
    """One list whose column 0 holds 2^30, -2^30 and then values near 1e-9: summed in ascending row order the two large values
    cancel first and the small ones survive; in any order that meets a large value late they are absorbed.  The order of the
    centroid mean's sum shows in the float32 result."""
    rng = np.random.default_rng(seed * 31337 + n + d)
    rows = rng.standard_normal((n, d)).astype(F)
    rows[:, 0] = (1e-9 * rng.uniform(1, 2, n)).astype(F)
    rows[0, 0], rows[1, 0] = F(2.0 ** 30), F(-(2.0 ** 30))
    return {"rows": rows, "q": rng.standard_normal((3, d)).astype(F), "nlist": 1}


PLANTED_SIZES = (0, 2500, 1, 63, 64, 65, 200, 100)   # an empty list, one of several segments, the sizes around a wave


def case_planted(d, nq=24, seed=4):
    """Planted centroids e_l (set_centroids): rows of list l are 3 e_l + noise, shuffled; list 0 is empty.  Queries 2 e_l + noise
    cycle over the lists.  Rows 2 q_j sit at row 0, at row n - 1, and as the first and the last member of the large list."""
    rng = np.random.default_rng(seed * 104729 + d)
    nlist = len(PLANTED_SIZES)
    cen = np.zeros((nlist, d), F)
    cen[np.arange(nlist), np.arange(nlist)] = 1
    lab = rng.permutation(np.repeat(np.arange(nlist), PLANTED_SIZES))
    n = len(lab)
    rows = (3 * cen[lab] + 0.05 * rng.standard_normal((n, d))).astype(F)
    ql = np.arange(nq) % nlist
    q = (2 * cen[ql] + 0.05 * rng.standard_normal((nq, d))).astype(F)
    big = np.flatnonzero(lab == 1)
    for row, want in ((0, lab[0]), (n - 1, lab[n - 1]), (big[0], 1), (big[-1], 1)):
        j = np.flatnonzero(ql == want)[1 if row in (n - 1, big[-1]) else 0]   # (two different queries per list)
        rows[row] = 2 * q[j]
    return {"rows": rows, "q": q, "nlist": nlist, "centroids": cen, "labels": lab, "qlabels": ql}


def centroids_of(case, niter=10):
    return case["centroids"] if "centroids" in case else train(case["rows"], case["nlist"], niter)
