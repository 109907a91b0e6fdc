"""Inputs and NumPy restatements of the row-sharded IVF index (include/mips_hip_ivf_sharded.h; ShardedIvfIndex), on top of the
restatements of the UNSHARDED index: tests/ivf_search_cases.py, ivf_filter_cases.py, ivf_wide_cases.py and ivf_range_cases.py.

The expectation of every test is the unsharded restatement applied to ALL the rows in global order (`expected`, `expected_range`).
What is restated here is only what sharding adds:
    part_search   one shard's search cut behind its merge: the rows [lo, hi) with the global centroids and SQ8 range, the GLOBAL
                  selector read from bit lo, the shard's own labels; -> the RANKING scores (sq8: S, not D), the global rows
                  (row + lo, -1 padding) and B_q
    pack          the payload int64 [nq, k, 2] = {float32 bits, zero-extended; row}
    merge_parts   the merge of the gathered payloads: order (score descending, row ascending, padding last; then part, position),
                  the best k, S -> D = (float)((double)S + B_q) on the entries that name a row
    part_range    one shard's range result with idx_offset = sel_bit0 = lo (the records and their merge: tests/range_cases.py)
`wrong=` switches ONE deliberate mistake on; tests/test_ivf_sharded_host.py shows that each of them changes the result of a case:
    "no_idx_offset"   the part returns its local row numbers
    "sel_bit0_zero"   every part reads the global selector from bit 0 instead of bit lo
    "merge_on_D"      an sq8 part applies B_q itself and hands over D; the parts are merged on D.  It shows only on two rows with
                      equal D and different S: case_sq8_tie holds such a pair (sq8_cases.case_gauss produces it), the higher S at the
                      higher row, so a merge on D puts the two rows the other way round
One further mistake CANNOT be told apart from the right result, and is therefore not in WRONG: ties broken by shard order instead of
by row.  The shards are contiguous row ranges in rank order and every part list is in row order among equals, so "part, then
position" IS "ascending global row".
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
import ivf_range_cases as rg  # noqa: E402
import ivf_search_cases as sc  # noqa: E402
import ivf_wide_cases as wc  # noqa: E402
import sq8_cases as sq  # noqa: E402
from oracle import mips_oracle as orc  # noqa: E402

F = np.float32
LABEL_NONE = fc.LABEL_NONE
WRONG = ("no_idx_offset", "sel_bit0_zero", "merge_on_D")
STORAGES = sc.STORAGES
FILTERS = ("plain", "selector", "exclude", "only", "both")
KS = (1, 5, 29, 30, 100)


def shard_bounds(n, world, rank):
    """ShardedMipsIndex's partition: ceil(n / world) rows per rank"""
    per = -(-int(n) // int(world))
    return min(n, rank * per), min(n, (rank + 1) * per)


def bounds(n, world):
    return [shard_bounds(n, world, r) for r in range(world)]


# ------------------------------------------------------------------ cases: dict(rows, q, nlist, centroids, assign, row_labels, q_labels, sel, sq8_params)
def _finish(c, seed):
    """the derived parts of a case: assignments by the definition, the GLOBAL SQ8 range, labels, query labels and a global bitmap"""
    rng = np.random.default_rng(seed)
    n, nq = len(c["rows"]), len(c["q"])
    c["assign"] = iv.nearest(c["rows"], c["centroids"])[:, 0].astype(np.int32)
    c["sq8_params"] = sq.train(c["rows"])
    c["row_labels"] = rng.integers(0, 5, n).astype(np.int32)
    ql = rng.integers(0, 5, nq).astype(np.int32)
    ql[nq // 2] = LABEL_NONE
    c["q_labels"] = ql
    c["sel"] = rng.random(n) < 0.6
    return c


PLANTED_N = 1000
BORDER_COPIES = (333, 334, 499, 500, 667, 668)      # both sides of the borders of 2 ranks (500) and of 3 ranks (334, 668)
ONE_SHARD_LIST = (6, range(900, 940))               # list 6: 40 rows, all of them in the last shard of 2 and of 3 ranks
SHORT_LIST = (7, range(10, 13))                     # list 7: 3 rows, all of them in the first shard: fewer than k = 5 at nprobe = 1


def case_planted(seed=41):
    """1000 x 64 rows, 8 lists, 9 queries; 3 ranks hold 334 / 334 / 332 rows.  Planted centroids e_l; row i is 3 e_l + noise for its
    list l, so the assignment add() computes IS the planted one.  Lists 0 .. 5 are spread over all rows; list 6 lives in rows 900 ..
    939 only (one shard) and list 7 in rows 10 .. 12 only: query 0 = 2 e_7 + noise finds 3 rows at nprobe = 1, and the padding of its
    result must survive the merge.  Six copies of one vector of list 0 sit on both sides of every shard border and query 2 IS that
    vector: equal scores on different ranks, resolved to the lowest global row.  Query 1 = 2 e_6 + noise."""
    rng = np.random.default_rng(seed)
    n, d, nlist, nq = PLANTED_N, 64, 8, 9
    cen = np.zeros((nlist, d), F)
    cen[np.arange(nlist), np.arange(nlist)] = 1
    lab = rng.integers(0, 6, n)
    lab[list(ONE_SHARD_LIST[1])] = ONE_SHARD_LIST[0]
    lab[list(SHORT_LIST[1])] = SHORT_LIST[0]
    rows = (3 * cen[lab] + 0.05 * rng.standard_normal((n, d))).astype(F)
    v = (4 * cen[0] + 0.05 * rng.standard_normal(d)).astype(F)   # (longer than its list's rows: its copies score highest)
    rows[list(BORDER_COPIES)] = v
    lab[list(BORDER_COPIES)] = 0
    ql = np.array([7, 6, 0, 1, 2, 3, 4, 5, 0])
    q = (2 * cen[ql] + 0.05 * rng.standard_normal((nq, d))).astype(F)
    q[2] = v
    c = _finish({"rows": rows, "q": q, "nlist": nlist, "centroids": cen, "planted": lab.astype(np.int32)}, seed)
    c["sel"][list(BORDER_COPIES)[::2]] = False      # the selector takes one copy of every border pair out ...
    c["sel"][list(BORDER_COPIES)[1::2]] = True      # ... and keeps the other
    return c


def case_trained(seed=42):
    """3000 x 64 Gaussian rows, 8 lists trained by the definition (2 iterations), 9 Gaussian queries: lists that interleave in every
    shard"""
    c = iv.case_gauss(3000, 64, 9, 8, seed)
    c["centroids"] = iv.train(c["rows"], 8, 2)
    return _finish(c, seed)


def case_tiny(seed=43):
    """4 x 64 rows, 2 lists, 3 queries: 3 ranks hold 2 / 2 / 0 rows -- an EMPTY shard -- and every k > 4 leaves padding"""
    rng = np.random.default_rng(seed)
    cen = np.zeros((2, 64), F)
    cen[0, 0], cen[1, 1] = 1, 1
    lab = np.array([0, 1, 1, 0])
    rows = (3 * cen[lab] + 0.05 * rng.standard_normal((4, 64))).astype(F)
    q = (2 * cen[[0, 1, 0]] + 0.05 * rng.standard_normal((3, 64))).astype(F)
    return _finish({"rows": rows, "q": q, "nlist": 2, "centroids": cen}, seed)


def case_768(seed=44):
    """300 x 768 rows, 4 planted lists, 3 queries: the row pitch of the flagship workload"""
    rng = np.random.default_rng(seed)
    n, d = 300, 768
    cen = np.zeros((4, d), F)
    cen[np.arange(4), np.arange(4)] = 1
    lab = rng.integers(0, 4, n)
    rows = (cen[lab] + 0.05 * rng.standard_normal((n, d))).astype(F)
    q = (cen[[0, 1, 3]] + 0.05 * rng.standard_normal((3, d))).astype(F)
    return _finish({"rows": rows, "q": q, "nlist": 4, "centroids": cen}, seed)


SQ8_TIE = {"query": 8, "rows": (1213, 24), "rank": 646, "k": 700}


def case_sq8_tie():
    """sq8_cases.case_gauss(3000, 768, 9, seed=2) -- Gaussian rows with per-column offsets and scales -- over 4 planted lists (e_0 ..
    e_3; list 2 stays empty), the SQ8 range trained on all the rows.  For query 8, rows 1213 and 24 are neighbours at ranks 646 and
    647 of the S order with S = 11.948988 and 11.948987 and ONE D = 28.949942: equal D, different S, the higher S at the HIGHER row.
    They lie in different lists, and on different ranks of 3 (borders 1000 / 2000; on one rank of 2, where a merge that orders by
    (D, row) still swaps them).  Every list probed and k = 700 reach the pair; ranked and merged on S the result has 1213 before 24."""
    c = sq.case_gauss(3000, 768, 9, seed=2)
    cen = np.zeros((4, 768), F)
    cen[np.arange(4), np.arange(4)] = 1
    c = _finish({"rows": c["rows"], "q": c["q"], "nlist": 4, "centroids": cen}, 45)
    c["tie"] = SQ8_TIE
    return c


_CASES = {}


def case(name):
    """the case `name`, computed once and shared: nobody modifies it"""
    if name not in _CASES:
        _CASES[name] = {"planted": case_planted, "trained": case_trained, "tiny": case_tiny, "768": case_768, "sq8_tie": case_sq8_tie}[name]()
    return _CASES[name]


def filter_kw(c, flt):
    """the filter of FILTERS as keywords of the unsharded restatements: sel / labels / q_labels / mode over ALL the rows"""
    kw = {}
    if flt in ("selector", "both"):
        kw["sel"] = c["sel"]
    if flt in ("exclude", "only", "both"):
        kw.update(labels=c["row_labels"], q_labels=c["q_labels"], mode="only" if flt == "only" else "exclude")
    return kw


def sq8_of(c, dtype):
    return c["sq8_params"] if dtype == "sq8" else None


# ------------------------------------------------------------------ the unsharded expectations
def expected(c, dtype, k, nprobe, flt="plain"):
    return wc.search(c["rows"], c["q"], c["assign"], c["centroids"], k, nprobe, dtype, sq8_of(c, dtype), **filter_kw(c, flt))


def expected_range(c, dtype, radii, nprobe, flt="plain"):
    return rg.range_search(c["rows"], c["q"], c["assign"], c["centroids"], radii, nprobe, dtype, sq8_of(c, dtype), **filter_kw(c, flt))


def radii_for(c, dtype, nprobe, flt="plain", count=20):
    """per query a radius with about `count` hits among the probed, admitted rows (-inf: all of them)"""
    per = rg.probed_scores(c["rows"], c["q"], c["assign"], c["centroids"], nprobe, dtype, sq8_of(c, dtype), **filter_kw(c, flt))
    out = []
    for ids, key, rep, ok in per:
        r = rg.radius_for_count(rep, count + len(out) % 3)
        out.append(F(-np.inf) if r is None else r)
    return np.array(out, F)


# ------------------------------------------------------------------ what sharding adds
def part_search(c, dtype, lo, hi, k, nprobe, flt="plain", wrong=None):
    """-> (S float32 [nq, k] RANKING scores, I int64 [nq, k] global rows, bias float64 [nq] or None) of the shard [lo, hi)"""
    q = np.asarray(c["q"], dtype=F)
    nq = len(q)
    kw = filter_kw(c, flt)
    S = np.full((nq, k), -np.inf, F)
    I = np.full((nq, k), -1, np.int64)
    bias = sq.bias(q, *c["sq8_params"]) if dtype == "sq8" else None
    if hi == lo:
        return S, I, bias
    X, Y, _ = sc.stored(c["rows"][lo:hi], q, dtype, sq8_of(c, dtype))   # (the GLOBAL range: the shard never trains its own)
    assign = c["assign"][lo:hi]
    P = iv.nearest(q, c["centroids"], min(int(nprobe), c["nlist"]))
    labels = kw["labels"][lo:hi] if "labels" in kw else None
    for j in range(nq):
        ids = np.flatnonzero(np.isin(assign, P[j])).astype(np.int64)
        ids = ids[fc.admitted(ids, j, kw.get("sel"), 0 if wrong == "sel_bit0_zero" else lo, labels, kw.get("q_labels"), kw.get("mode", "exclude"))]
        if len(ids) == 0:
            continue
        key = orc.canonical_pairs(Y[j:j + 1], X, ids[None, :])[0].astype(F)
        order = np.lexsort((ids, -key))[:k]
        S[j, :len(order)] = key[order]
        I[j, :len(order)] = ids[order] + (0 if wrong == "no_idx_offset" else lo)
    if wrong == "merge_on_D" and bias is not None:                          # the part finishes S -> D itself and hands over no bias
        real = (I >= 0) & np.isfinite(S)
        S = np.where(real, (S.astype(np.float64) + bias[:, None]).astype(F), S).astype(F)
        bias = None
    return S, I, bias


def pack(S, I):
    """-> int64 [nq, k, 2]: {the float32 bits, zero-extended; the row}"""
    out = np.empty(S.shape + (2,), np.int64)
    out[..., 0] = np.ascontiguousarray(S, dtype=F).view(np.uint32).astype(np.int64)
    out[..., 1] = I
    return out


def merge_parts(gathered, parts, nq, k, bias=None):
    """gathered int64 [parts, nq, k, 2] -> (D float32 [nq, k], I int64 [nq, k]); reads the LOW 32 bits of word 0, as the kernel does
    (pack_topk of the package sign-extends them, the part search zero-extends)"""
    g = np.asarray(gathered, dtype=np.int64).reshape(parts, nq, k, 2)
    D = np.full((nq, k), -np.inf, F)
    I = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        s = (g[:, j, :, 0] & 0xFFFFFFFF).astype(np.uint32).view(F).reshape(-1)
        ids = g[:, j, :, 1].reshape(-1)
        rank_id = np.where(ids < 0, np.iinfo(np.int64).max, ids)
        order = np.lexsort((np.arange(parts * k), rank_id, -s))[:k]          # (score desc, id asc, part-major position)
        out, oi = s[order].copy(), ids[order]
        if bias is not None:
            real = (oi >= 0) & np.isfinite(out)
            out[real] = (out[real].astype(np.float64) + bias[j]).astype(F)
        D[j], I[j] = out, oi
    return D, I


def sharded_search(c, dtype, world, k, nprobe, flt="plain", wrong=None):
    """parts -> payloads -> merge, all in NumPy: what ShardedIvfIndex computes"""
    ps = [part_search(c, dtype, lo, hi, k, nprobe, flt, wrong) for lo, hi in bounds(len(c["rows"]), world)]
    g = np.stack([pack(S, I) for S, I, _ in ps])
    return merge_parts(g, world, len(c["q"]), k, ps[0][2])


def part_range(c, dtype, lo, hi, radii, nprobe, flt="plain"):
    """-> (lims, D, I) of the shard [lo, hi): idx_offset = sel_bit0 = lo"""
    kw = filter_kw(c, flt)
    nq = len(c["q"])
    if hi == lo:
        return np.zeros(nq + 1, np.int64), np.zeros(0, F), np.zeros(0, np.int64)
    if "labels" in kw:
        kw["labels"] = kw["labels"][lo:hi]
    return rg.range_search(c["rows"][lo:hi], c["q"], c["assign"][lo:hi], c["centroids"], radii, nprobe, dtype, sq8_of(c, dtype), idx_offset=lo,
                           sel_bit0=lo, **kw)


def same(a, b):
    """(D, I) pairs equal bit for bit"""
    return a[0].shape == b[0].shape and np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and \
        np.array_equal(np.asarray(a[0], dtype=F).view(np.uint32), np.asarray(b[0], dtype=F).view(np.uint32))


def equal_D_different_S_pairs(rows, q, sq8_params):
    """how many neighbours in the S order of any query have different S and equal D on an sq8 index over `rows`"""
    X, Y, bias = sc.stored(rows, q, "sq8", sq8_params)
    n, count = len(rows), 0
    for j in range(len(q)):
        S = orc.canonical_pairs(Y[j:j + 1], X, np.arange(n, dtype=np.int64)[None, :])[0].astype(F)
        D = (S.astype(np.float64) + bias[j]).astype(F)
        o = np.argsort(-S, kind="stable")
        count += int(((D[o][1:] == D[o][:-1]) & (S[o][1:] != S[o][:-1])).sum())
    return count
