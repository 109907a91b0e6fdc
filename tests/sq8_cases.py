"""Inputs and NumPy references of the 8-bit scalar-quantised index (dtype "sq8"; include/mips_hip_sq8.h has the definition).

The quantiser is restated here in float32 NumPy -- every operation one IEEE float32 operation, as csrc/sq8_quant.hpp performs it --
and the ranking comes from the oracle's exact search on (codes as float32, q'), the way the e4m3-documents tests use it.  The
`wrong` argument of the functions switches ONE deliberate mistake on; tests/test_sq8_host.py shows that each of them changes a
result on the cases below, so a kernel that makes it cannot pass.
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
MISTAKES = ("signed_decode", "no_bias", "round_encode", "no_clamp", "f32_query", "ties_high")


# ------------------------------------------------------------------ the quantiser, float32
def train(x):
    """-> (vmin, vdiff) float32 [d]"""
    x = np.asarray(x, dtype=F)
    vmin = x.min(axis=0)
    return vmin, (x.max(axis=0) - vmin).astype(F)


def encode(x, vmin, vdiff, wrong=None):
    x = np.asarray(x, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(vdiff != 0, ((x - vmin).astype(F) / vdiff).astype(F), F(0)).astype(F)
    if wrong == "no_clamp":
        return (F(255) * t).astype(F).astype(np.int64).astype(np.uint8)      # (wraps modulo 256 outside the range)
    t = np.fmin(np.fmax(t, F(0)), F(1)).astype(F)
    v = (F(255) * t).astype(F)
    if wrong == "round_encode":
        v = np.rint(v)
    return v.astype(np.int32).astype(np.uint8)                                # the cast truncates


def decode(codes, vmin, vdiff):
    c = np.asarray(codes).astype(F)
    return (vmin + (((c + F(0.5)).astype(F) / F(255)).astype(F) * vdiff).astype(F)).astype(F)


def scale_offset(vmin, vdiff):
    s = (vdiff / F(255)).astype(F)
    return s, (vmin + (F(0.5) * s).astype(F)).astype(F)


def scaled_queries(q, vdiff, wrong=None):
    """q' = bf16(q s) as float32 values"""
    s, _ = scale_offset(np.zeros_like(vdiff), vdiff)
    qs = (np.asarray(q, dtype=F) * s).astype(F)
    return qs if wrong == "f32_query" else synth.round_to_bf16(qs)


def bias(q, vmin, vdiff):
    """B_q: the sequential fp64 sum over ascending j of q_j o_j (cumsum is sequential)"""
    _, o = scale_offset(vmin, vdiff)
    return np.cumsum(np.asarray(q, dtype=F).astype(np.float64) * o.astype(np.float64), axis=1)[:, -1]


def search(q, codes, vmin, vdiff, k, wrong=None):
    """The reference result (D float32 [nq, k], I int64 [nq, k]) of an sq8 index holding `codes` for float32 queries q."""
    q = np.asarray(q, dtype=F)
    rows = np.asarray(codes)
    rows = (rows.astype(np.int8) if wrong == "signed_decode" else rows).astype(F)
    qp = scaled_queries(q, vdiff, wrong)
    n = rows.shape[0]
    if wrong == "ties_high":   # the same search over the rows in reverse order prefers the HIGHEST row among equals
        s, i = orc.search_exact_bruteforce(qp, rows[::-1], k)
        i = np.where(i >= 0, n - 1 - i, -1)
    else:
        s, i = orc.search_exact_bruteforce(qp, rows, k)   # S: sequential fp64 sum, (score desc, row asc)
    if wrong == "no_bias":
        return s, i
    d = (s.astype(np.float64) + bias(q, vmin, vdiff)[:, None]).astype(F)
    return np.where(i >= 0, d, F(-np.inf)).astype(F), i


def subset_scores(q, codes, vmin, vdiff, ids):
    """D of the pairs (q[j], row ids[j, t]); ids < 0 score -inf"""
    qp = scaled_queries(q, vdiff)
    s = orc.canonical_pairs(qp, np.asarray(codes).astype(F), ids).astype(F)
    d = (s.astype(np.float64) + bias(q, vmin, vdiff)[:, None]).astype(F)
    return np.where(np.asarray(ids) >= 0, d, F(-np.inf)).astype(F)


# ------------------------------------------------------------------ cases: -> dict(train, rows, q)
def _columns(rng, d):
    """per-column offsets and scales; column 3 (when there is one) is CONSTANT: vdiff = 0"""
    off = rng.uniform(-2.0, 2.0, d).astype(F)
    sc = rng.uniform(0.05, 3.0, d).astype(F)
    if d > 3:
        sc[3] = 0
    return off, sc


def _queries(rng, nq, d):
    """signed queries; column 5 is zero (a zero s_j q_j), and so is every product with the constant column"""
    q = rng.standard_normal((nq, d)).astype(F)
    if d > 5:
        q[:, 5] = 0
    return q


def case_gauss(n, d, nq, seed=1):
    """(a) + (c) + (g): Gaussian rows whose columns have different offsets and scales, one constant column"""
    rng = np.random.default_rng(seed * 1000003 + n * 31 + d)
    off, sc = _columns(rng, d)
    x = (rng.standard_normal((n, d)).astype(F) * sc + off).astype(F)
    return {"train": x, "rows": x, "q": _queries(rng, nq, d)}


def case_all_codes(d, nq, seed=2):
    """(b): 258 rows that produce all 256 codes in every column, among them a whole row of 255 and a whole row of 0"""
    rng = np.random.default_rng(seed * 7919 + d)
    vmin = rng.uniform(-1.0, 1.0, d).astype(F)
    vdiff = rng.uniform(0.5, 2.0, d).astype(F)
    lv = (np.arange(256)[:, None] + 37 * np.arange(d)[None, :]) % 256          # row r, column j: code (r + 37 j) mod 256
    # (the level rows' maximum, decode(255), is the top of the TRAINED range: that row is the whole row of 255)
    x = np.concatenate([decode(lv, vmin, vdiff), decode(np.full((1, d), 255), vmin, vdiff), vmin[None, :]])
    return {"train": x, "rows": x, "q": _queries(rng, nq, d), "levels": lv}


def case_outside(n, d, nq, seed=3):
    """(d): trained on half the range of the rows that are added afterwards (they clamp)"""
    c = case_gauss(n, d, nq, seed)
    c["train"] = (c["rows"][: max(2, n // 4)] * F(0.5)).astype(F)
    return c


def case_duplicates(n, d, nq, seed=4):
    """(e): 3 copies of the best row of query 0 and 70 of the best row of query 1, spread over the index"""
    c = case_gauss(n, d, nq, seed)
    vmin, vdiff = train(c["train"])
    _, best = search(c["q"][:2], encode(c["rows"], vmin, vdiff), vmin, vdiff, 1)
    x = np.concatenate([c["rows"], np.repeat(c["rows"][best[0, 0]][None], 2, axis=0), np.repeat(c["rows"][best[1, 0]][None], 69, axis=0)])
    perm = np.random.default_rng(seed).permutation(len(x))
    c["rows"] = np.ascontiguousarray(x[perm])
    return c


def prepared(case):
    """-> (vmin, vdiff, codes) of a case"""
    vmin, vdiff = train(case["train"])
    return vmin, vdiff, encode(case["rows"], vmin, vdiff)


def host_cases():
    """The small set tests/test_sq8_host.py runs every mistake against: (name, case, k)"""
    return [("gauss", case_gauss(300, 100, 9), 5), ("all_codes", case_all_codes(40, 6), 7), ("outside", case_outside(200, 64, 5), 5),
            ("duplicates", case_duplicates(400, 48, 4), 5), ("k_gt_n", case_gauss(3, 40, 4), 5)]
