"""Inputs and the NumPy restatement of the two-stage search on PQ codes (include/mips_hip_refine.h has the definition): the candidate
search for k <= 1024 on a PqIndex / IvfPqIndex and the exact re-ranking of candidate ids.  The scores are those of tests/pq_cases.py and
tests/ivfpq_cases.py, imported, not copied.

    candidates_pq / candidates_ivfpq   the definition: every row (of the probed lists) scored, fully sorted by (score descending, row
                                       ascending), cut at k
    rerank                             the set of valid ids, their canonical scores, a sort by (score descending, id ascending), the
                                       duplicate drop, the cut at k
    pool_candidates                    the same result the way the scan kernels reach it -- 64-row tiles dealt round robin to P pools,
                                       fill, one sort, threshold and insertion, the final rank over the sorted pools -- so that the
                                       mistakes such a kernel can make are stated next to the definition.  `wrong=` switches ONE on:
        "threshold_at_k"   the threshold read at slot k instead of k - 1.  A slot nobody wrote is modelled as +inf: LDS is not cleared,
                           and at k = KP the slot behind a pool is the best entry of the next one
        "tie_high"         ties to the highest row
        "unsorted_short"   a pool that ends below k is never sorted
        "four_pools"       the final rank counted over the first four pools only
    and rerank has
        "keep_duplicate"   a repeated id kept
        "pad_as_row"       the -1 padding ranked as row -1 (the last row, as an unchecked index reads it)
tests/test_refine_host.py shows that pool_candidates without a mistake IS the definition and that each mistake changes an I or a D on
a named case, so a kernel that makes it cannot pass tests/test_gpu_refine.py.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivfpq_cases as vc  # noqa: E402
import pq_cases as pc  # noqa: E402

F = np.float32
MAX_K, MAX_K_WIDE = 29, 1024
NO_ROW = 0x7FFFFFFF
MISTAKES = ("threshold_at_k", "tie_high", "unsorted_short", "four_pools", "keep_duplicate", "pad_as_row")

KS = (1, 29, 30, 63, 64, 65, 255, 256, 257, 1023, 1024)
NQS = (1, 3, 17)
GEOMETRY = ((32, 4), (80, 40))             # (d, M): the four-wave class, the sixteen-wave class
WORST = dict(d=128, M=128, nlist=1024, n=5000)   # nprobe = 1024: the largest table beside the longest prefix


def ntotals(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 4097})


# ------------------------------------------------------------------ the definition
def candidates_pq(q, cb, codes, k, idx_offset=0):
    return pc.search(q, cb, codes, k, idx_offset)


def candidates_ivfpq(q, cen, cb, codes, a, k, nprobe, idx_offset=0, by_residual=True):
    return vc.search(q, cen, cb, codes, a, k, nprobe, idx_offset, by_residual)


def rerank(score_of, ids, k, ntotal, idx_offset=0, wrong=None):
    """score_of(local [nq, kc] int64 with -1 for "no row") -> float32 [nq, kc] (the store's canonical scores); ids int64 [nq, kc]
    -> (D float32 [nq, k], I int64 [nq, k])"""
    ids = np.asarray(ids, dtype=np.int64)
    nq, kc = ids.shape
    local = np.array([[int(v) - int(idx_offset) for v in row] for row in ids], dtype=object).reshape(nq, kc)
    valid = np.array([[0 <= v < ntotal for v in row] for row in local], dtype=bool).reshape(nq, kc)
    loc = np.where(valid, local, -1).astype(np.int64)
    if wrong == "pad_as_row" and ntotal > 0:
        pad = ids == -1
        loc = np.where(pad, ntotal - 1, loc)
        valid = valid | pad
    S = np.asarray(score_of(loc), dtype=F)
    out_d = np.full((nq, k), -np.inf, F)
    out_i = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        seen, ent = set(), []
        for t in range(kc):
            g = int(ids[j, t])
            if not valid[j, t] or np.isnan(S[j, t]):
                continue
            if g in seen and wrong != "keep_duplicate":
                continue
            seen.add(g)
            ent.append((-float(S[j, t]), g, S[j, t]))
        ent.sort(key=lambda e: (e[0], e[1]))
        for u, e in enumerate(ent[:k]):
            out_d[j, u], out_i[j, u] = e[2], e[1]
    return out_d, out_i


def refined(cand_i, score_of, k, ntotal, idx_offset=0):
    """RefinedIndex.search: the re-ranking of the candidates' ids"""
    return rerank(score_of, cand_i, k, ntotal, idx_offset)


# ------------------------------------------------------------------ the pools, as the kernels keep them
def pool_class(k):
    return 64 if k <= 64 else 256 if k <= 256 else 1024


def pools_of(M, k, p=0):
    """adcw::pools of csrc/adc_wide_math.hpp"""
    KP = pool_class(k)
    fixed = M * 1024 + 16 * 4 + ((3 * p + 1) * 4 if p > 0 else 0)
    fit = (160 * 1024 - fixed) // (KP * 8)
    return max(1, min(fit, 16 if M > 32 else 4))


def _before(k1, r1, k2, r2, wrong=None):
    if wrong == "tie_high":
        return k1 > k2 or (k1 == k2 and r1 > r2)
    return k1 > k2 or (k1 == k2 and r1 < r2)


def _count_before(pk, pr, n, key, row, wrong):
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) >> 1
        if _before(pk[mid], pr[mid], key, row, wrong):
            lo = mid + 1
        else:
            hi = mid
    return lo


class _Pool:
    def __init__(self, k, wrong):
        self.k, self.wrong, self.cnt = k, wrong, 0
        KP = pool_class(k)
        self.pk = [np.inf] * (KP + 1)          # (a slot nobody wrote; slot KP stands for what lies behind the pool)
        self.pr = [0] * (KP + 1)

    def sort(self):
        ent = sorted(zip(self.pk[:self.cnt], self.pr[:self.cnt]), key=lambda e: (-e[0], -e[1] if self.wrong == "tie_high" else e[1]))
        n = 2
        while n < self.cnt:
            n *= 2
        ent += [(-np.inf, NO_ROW)] * (n - self.cnt)
        for u, (a, b) in enumerate(ent):
            self.pk[u], self.pr[u] = a, b

    def take(self, keys, rows):
        """one scoring pass: up to 64 candidates in lane order"""
        k, w = self.k, self.wrong
        cand = list(zip(keys, rows))
        if self.cnt < k:
            room = k - self.cnt
            for a, b in cand[:room]:
                self.pk[self.cnt], self.pr[self.cnt] = a, b
                self.cnt += 1
            cand = cand[room:]
            if self.cnt < k:
                return
            self.sort()
        ts = k if w == "threshold_at_k" else k - 1
        for a, b in cand:
            if not _before(a, b, self.pk[ts], self.pr[ts], w):
                continue
            at = _count_before(self.pk, self.pr, k, a, b, w)
            if at >= k:
                continue
            self.pk[at + 1:k] = self.pk[at:k - 1]
            self.pr[at + 1:k] = self.pr[at:k - 1]
            self.pk[at], self.pr[at] = a, b

    def finish(self):
        if 1 < self.cnt < self.k and self.wrong != "unsorted_short":
            self.sort()


def flat_tiles(n, P):
    """(pool, rows) of the flat scan of one segment: wave w takes rows [64 (w + P i), +64)"""
    return [((t0 // 64) % P, np.arange(t0, min(n, t0 + 64))) for t0 in range(0, n, 64)]


def list_tiles(lists, P):
    """(pool, rows) of the list scan of one segment: lists = the probed lists' rows in probe order; 64-row tiles go round robin
    across list boundaries"""
    out, t = [], 0
    for rows in lists:
        for t0 in range(0, len(rows), 64):
            out.append((t % P, np.asarray(rows[t0:t0 + 64])))
            t += 1
    return out


def pool_select(D_row, tiles, k, P, wrong=None):
    """one query, one segment: -> (float32 [k], int64 [k])"""
    pools = [_Pool(k, wrong) for _ in range(P)]
    for w, rows in tiles:
        pools[w].take([float(D_row[r]) for r in rows], [int(r) for r in rows])
    for p in pools:
        p.finish()
    out_d = np.full(k, -np.inf, F)
    out_i = np.full(k, -1, np.int64)
    for w, p in enumerate(pools):
        for u in range(p.cnt):
            rank = u
            for w2, p2 in enumerate(pools):
                if w2 != w and not (wrong == "four_pools" and w2 >= 4):
                    rank += _count_before(p2.pk, p2.pr, p2.cnt, p.pk[u], p.pr[u], wrong)
            if rank < k:
                out_d[rank], out_i[rank] = F(p.pk[u]), p.pr[u]
    return out_d, out_i


def pool_candidates_pq(q, cb, codes, k, wrong=None):
    D = pc.scores(pc.lut(q, cb), codes) if len(codes) else np.zeros((len(q), 0), F)
    P = pools_of(cb.shape[0], k)
    res = [pool_select(D[j], flat_tiles(len(codes), P), k, P, wrong) for j in range(len(q))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def pool_candidates_ivfpq(q, cen, cb, codes, a, k, nprobe, by_residual=True, wrong=None):
    D = vc.all_scores(q, cen, cb, codes, a, by_residual)
    L, _ = vc.probe(q, cen, nprobe)
    P = pools_of(cb.shape[0], k, L.shape[1])
    a = np.asarray(a, dtype=np.int64)
    res = []
    for j in range(len(q)):
        lists = [np.flatnonzero(a == l) for l in L[j]]
        res.append(pool_select(D[j], list_tiles(lists, P), k, P, wrong))
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ------------------------------------------------------------------ cases
def case_flood(n=1100, flood=300, seed=11):
    """an IVFPQ case (d = 32, M = 4, 8 lists) in which `flood` rows of ONE list carry the codes of query 0's best row of that list:
    a cut inside the flood is decided by the row number alone"""
    c = vc.case_planted(32, 4, 8, n, 3, seed)
    c["q"][0] = 3 * c["centroids"][7]                                         # list 7 is query 0's nearest: its rows lead
    rows = np.flatnonzero(c["assign"] == 7)
    assert len(rows) >= flood
    D = vc.all_scores(c["q"], c["centroids"], c["codebook"], c["codes"], c["assign"])
    best = rows[int(np.argmax(D[0, rows]))]
    c["flood"] = rows[-flood:]
    c["codes"][c["flood"]] = c["codes"][best]
    return c


def case_ordered(n, M=4, d=32, nq=2, ascending=True, seed=12):
    """a PQ case whose rows score in strictly ascending (descending) order for EVERY query: code column 0 alone decides, through a
    codebook whose sub-quantiser 0 is c * e_0 with c rising in the code, queries with q_0 > 0, every other sub-quantiser zero; rows
    come in blocks of equal code, so inside a block the order is by row"""
    c = pc.case_planted(d, M, n, nq, seed)
    cb = np.zeros_like(c["codebook"])
    cb[0, :, 0] = np.arange(256, dtype=F)
    c["codebook"] = cb
    c["q"][:, 0] = np.abs(c["q"][:, 0]) + F(1)
    codes = np.zeros((n, M), np.uint8)
    ramp = (np.arange(n, dtype=np.int64) * 256) // max(n, 1)
    codes[:, 0] = ramp if ascending else 255 - ramp
    c["codes"] = codes
    return c


def rerank_ids(ntotal, nq, kc, seed=13, idx_offset=0):
    """ids [nq, kc] with -1 padding, ids past the index, INT64_MIN and repeats among valid ids"""
    rng = np.random.default_rng([seed, ntotal, kc])
    ids = rng.integers(0, max(ntotal, 1), (nq, kc)).astype(np.int64) + idx_offset
    junk = rng.random((nq, kc))
    ids[junk < 0.15] = -1
    ids[(junk >= 0.15) & (junk < 0.2)] = ntotal + idx_offset
    ids[(junk >= 0.2) & (junk < 0.23)] = (1 << 40) + 3
    ids[(junk >= 0.23) & (junk < 0.25)] = -(1 << 63)
    if kc >= 4:
        ids[:, kc - 1] = ids[:, 0]               # a repeat at the two ends
        ids[:, kc // 2] = ids[:, 1]
    return ids
