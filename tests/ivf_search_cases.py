"""The NumPy restatement of the IVF search (include/mips_hip_ivf.h: mips_ivf_search) and its cases, on top of tests/ivf_cases.py.

For query j: P(q_j) = iv.nearest(q_j, centroids, p) on the float32 query; the admitted rows A_j are those whose assignment lies in
P(q_j); their keys are the flat storage's canonical scores (bf16: rounded rows and queries; f32: as given; sq8: S on the codes and
q', from tests/sq8_cases.py, reported as D = (float)((double)S + B_q)); np.lexsort on (row, -key) gives the order; -1 / -inf pad.
`wrong="list_position"` switches ONE deliberate mistake on: ties are broken by the position in the concatenation of the probed
lists instead of by the row.  tests/test_ivf_search_host.py shows that it changes the result of case_ties.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ivf_cases as iv  # noqa: E402
import sq8_cases as sq  # noqa: E402
from oracle import mips_oracle as orc  # noqa: E402
from oracle import synth  # noqa: E402

F = np.float32
STORAGES = ("bf16", "f32", "sq8")


def stored(rows, q, dtype, sq8_params=None):
    """-> (X, Y, bias): float32 rows and queries the ranking key is the canonical score of, and B_q (sq8) or None"""
    rows, q = np.asarray(rows, dtype=F), np.asarray(q, dtype=F)
    if dtype == "f32":
        return rows, q, None
    if dtype == "bf16":
        return synth.round_to_bf16(rows), synth.round_to_bf16(q), None
    vmin, vdiff = sq8_params if sq8_params is not None else sq.train(rows)
    vmin, vdiff = np.asarray(vmin, dtype=F), np.asarray(vdiff, dtype=F)
    return sq.encode(rows, vmin, vdiff).astype(F), sq.scaled_queries(q, vdiff), sq.bias(q, vmin, vdiff)


def search(rows, q, assign, centroids, k, nprobe, dtype, sq8_params=None, idx_offset=0, wrong=None):
    """-> (D float32 [nq, k], I int64 [nq, k])"""
    q = np.asarray(q, dtype=F)
    assign = np.asarray(assign)
    nlist = len(centroids)
    P = iv.nearest(q, centroids, min(int(nprobe), nlist))
    X, Y, bias = stored(rows, q, dtype, sq8_params)
    D = np.full((len(q), k), -np.inf, F)
    I = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        if wrong == "list_position":   # the candidates in the order the probed lists hold them
            ids = np.concatenate([np.flatnonzero(assign == l) for l in P[j]] + [np.zeros(0, np.int64)]).astype(np.int64)
        else:
            ids = np.flatnonzero(np.isin(assign, P[j])).astype(np.int64)
        if len(ids) == 0:
            continue
        key = orc.canonical_pairs(Y[j:j + 1], X, ids[None, :])[0].astype(F)
        if wrong == "list_position":
            order = np.argsort(-key, kind="stable")
        else:
            order = np.lexsort((ids, -key))
        order = order[:k]
        out = key[order]
        if bias is not None:
            out = (out.astype(np.float64) + bias[j]).astype(F)
        D[j, :len(order)] = out
        I[j, :len(order)] = ids[order] + idx_offset
    return D, I


def bruteforce_on_admitted(rows, q, assign, centroids, k, nprobe, dtype, sq8_params=None):
    """the same result from the oracle's exact brute force over the admitted rows alone, row numbers mapped back"""
    q = np.asarray(q, dtype=F)
    P = iv.nearest(q, centroids, min(int(nprobe), len(centroids)))
    X, Y, bias = stored(rows, q, dtype, sq8_params)
    D = np.full((len(q), k), -np.inf, F)
    I = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        ids = np.flatnonzero(np.isin(assign, P[j]))
        if len(ids) == 0:
            continue
        s, i = orc.search_exact_bruteforce(Y[j:j + 1], np.ascontiguousarray(X[ids]), k)
        ok = i[0] >= 0
        I[j, ok] = ids[i[0, ok]]
        D[j, ok] = s[0, ok] if bias is None else (s[0, ok].astype(np.float64) + bias[j]).astype(F)
    return D, I


# ------------------------------------------------------------------ cases
TIE_COPIES = 40


def case_ties(n=600, d=32, seed=6):
    """One vector stored 40 times at scattered rows; PLANTED assignments (mips_ivf_set_assign) spread the copies over the lists 0, 1, 2
    (copy c in list c mod 3), the other rows over all four lists.  The planted centroids make P(q) = (0, 1, 2) for the one query,
    which is the copied vector: with nprobe = 3 and k = 29 the result is the lowest 29 rows among the copies, ascending."""
    rng = np.random.default_rng(seed * 65537 + n + d)
    rows = rng.standard_normal((n, d)).astype(F)
    v = (4 * rng.standard_normal(d)).astype(F)
    at = np.sort(rng.choice(n, TIE_COPIES, replace=False))
    rows[at] = v
    assign = rng.integers(0, 4, n).astype(np.int32)
    assign[at] = np.arange(TIE_COPIES) % 3
    u = iv.normalise(v)[0]
    cen = np.stack([u, (F(0.9) * u).astype(F), (F(0.8) * u).astype(F), -u]).astype(F)
    return {"rows": rows, "q": v[None, :].copy(), "nlist": 4, "centroids": cen, "assign": assign, "copies": at}
