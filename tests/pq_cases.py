"""Inputs and the NumPy restatement of the product-quantised index (include/mips_hip_pq.h has the definition): train, encode, lookup
table, score, search and reconstruct.  Sums that the definition spells out are np.cumsum (sequential); float32 steps are NumPy
float32 operations.  `wrong=` switches ONE deliberate mistake on -- the score summed in fp64 then rounded ("fp64"), summed pairwise
("pairwise"), codes read as signed bytes ("signed"), the table rounded to bf16 ("bf16_table"), ties to the highest row ("tie_high"),
the nearest centroid taken with <= ("le"), the centroid mean summed in another order ("sum_order") -- and tests/test_pq_host.py shows
that each changes the bits of a score, a code or the codebook on a named case, so a kernel that makes it cannot pass.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import synth  # noqa: E402

F = np.float32
KSUB = 256
TRAIN_ROWS = 65536
MAX_K = 29


def widen_bf16(bits):
    """uint16 bf16 bit patterns -> the float32 values they are, exactly"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F)


# ------------------------------------------------------------------ the arithmetic
def seq_sum(a, axis):
    """the sequential fp64 sum along axis, started from +0.0 as the definition starts it (np.cumsum starts from the first addend, so
    a sum of -0.0 alone would come out as -0.0; adding +0.0 changes nothing else)"""
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis) + 0.0


def distances(x, cb):
    """x [n, dsub] float32, cb [256, dsub] float32 -> e [n, 256] float64: u = x - c is one float32 subtraction, e the sequential
    fp64 sum of u^2 over ascending column"""
    with np.errstate(over="ignore", invalid="ignore"):
        u = (x[:, None, :] - cb[None, :, :]).astype(F).astype(np.float64)
        return seq_sum(u * u, 2)


def nearest(x, cb, wrong=None):
    """-> int64 [n]: scan j = 0 .. 255 with best = 0; j replaces best iff e_j < e_best (strict: ties to the lowest j, a NaN never wins)"""
    x = np.asarray(x, dtype=F)
    out = np.empty(len(x), np.int64)
    for r0 in range(0, len(x), 2048):
        e = distances(x[r0:r0 + 2048], cb)
        best = np.zeros(len(e), np.int64)
        e_best = e[:, 0].copy()
        for j in range(1, KSUB):
            with np.errstate(invalid="ignore"):
                win = e[:, j] <= e_best if wrong == "le" else e[:, j] < e_best
            best[win] = j
            e_best[win] = e[win, j]
        out[r0:r0 + 2048] = best
    return out


def training_set(x):
    n = len(x)
    return x if n <= TRAIN_ROWS else x[(np.arange(TRAIN_ROWS, dtype=np.int64) * n) // TRAIN_ROWS]


def _tree_sum(mem):
    """the shared-memory tree of a parallel reduction: s[i] += s[i + stride], stride halving -- NOT the defined order"""
    s = list(mem)
    size = 1
    while size < len(s):
        size *= 2
    s += [np.zeros_like(s[0])] * (size - len(s))
    stride = size // 2
    while stride >= 1:
        for i in range(stride):
            s[i] = s[i] + s[i + stride]
        stride //= 2
    return s[0]


def train(x, M, niter=10, wrong=None, stats=None):
    """-> codebook float32 [M, 256, dsub].  stats (a dict): counts the (sub-quantiser, centroid, iteration) updates without members."""
    T = np.ascontiguousarray(training_set(np.asarray(x, dtype=F)))
    n, d = T.shape
    dsub = d // M
    first = (np.arange(KSUB, dtype=np.int64) * n) // KSUB
    cb = np.ascontiguousarray(T[first].reshape(KSUB, M, dsub).transpose(1, 0, 2))
    empty = 0
    for _ in range(niter):
        for m in range(M):
            sub = T[:, m * dsub:(m + 1) * dsub]
            a = nearest(sub, cb[m], wrong=wrong)
            present = np.unique(a)
            empty += KSUB - len(present)
            new = cb[m].copy()
            for j in present:
                mem = sub[a == j].astype(np.float64)            # ascending i
                s = _tree_sum(mem) if wrong == "sum_order" else seq_sum(mem, 0)
                new[j] = (s / np.float64(len(mem))).astype(F)
            cb[m] = new
    if stats is not None:
        stats["empty_updates"] = empty
    return cb


def encode(x, cb, wrong=None):
    """x [n, d] float32 -> codes uint8 [n, M]"""
    x = np.asarray(x, dtype=F)
    M, _, dsub = cb.shape
    return np.stack([nearest(x[:, m * dsub:(m + 1) * dsub], cb[m], wrong=wrong) for m in range(M)], axis=1).astype(np.uint8)


def lut(q, cb, wrong=None):
    """q [nq, d] float32 -> LUT float32 [nq, M, 256]: the canonical score of q^m and C[m][c]"""
    q = np.asarray(q, dtype=F)
    M, _, dsub = cb.shape
    q64 = q.reshape(len(q), M, 1, dsub).astype(np.float64)
    out = seq_sum(q64 * cb.astype(np.float64)[None], 3).astype(F)
    return synth.round_to_bf16(out) if wrong == "bf16_table" else out


def scores(table, codes, wrong=None):
    """table [nq, M, 256] float32, codes [n, M] uint8 -> D float32 [nq, n]: float32 additions in ascending m"""
    nq, M, _ = table.shape
    flat = table.reshape(nq, M * KSUB)
    if wrong == "signed":   # the byte read as a signed char: index m * 256 + (int8)code, wrapped into the table
        idx = (np.arange(M, dtype=np.int64)[None, :] * KSUB + codes.view(np.int8).astype(np.int64)) % (M * KSUB)
    else:
        idx = np.arange(M, dtype=np.int64)[None, :] * KSUB + codes.astype(np.int64)
    terms = flat[:, idx]                                        # [nq, n, M]
    if wrong == "fp64":
        return np.cumsum(terms.astype(np.float64), axis=2)[..., -1].astype(F)
    if wrong == "pairwise":
        t = [terms[..., m] for m in range(M)]
        while len(t) > 1:
            t = [(t[i] + t[i + 1]).astype(F) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0]
    acc = terms[..., 0].copy()
    for m in range(1, M):
        acc = (acc + terms[..., m]).astype(F)
    return acc


def top_k(D, k, idx_offset=0, wrong=None):
    """D [nq, n] -> (float32 [nq, k], int64 [nq, k]): (D descending, row ascending), -1 / -inf padding, idx_offset added"""
    nq, n = D.shape
    rows = np.arange(n, dtype=np.int64)
    out_d = np.full((nq, k), -np.inf, F)
    out_i = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        order = np.lexsort((-rows if wrong == "tie_high" else rows, -D[j].astype(np.float64)))[:k]
        out_d[j, :len(order)] = D[j, order]
        out_i[j, :len(order)] = order + idx_offset
    return out_d, out_i


def search(q, cb, codes, k, idx_offset=0, wrong=None):
    table = lut(q, cb, wrong=wrong)
    D = scores(table, codes, wrong=wrong) if len(codes) else np.zeros((len(table), 0), F)
    return top_k(D, k, idx_offset, wrong=wrong)


def reconstruct(codes, cb):
    """codes [n, M] -> float32 [n, d]: the concatenation of C[m][code[i][m]]"""
    M = cb.shape[0]
    return np.concatenate([cb[m][codes[:, m].astype(np.int64)] for m in range(M)], axis=1)


# ------------------------------------------------------------------ cases
GEOMETRY = ((32, 4), (24, 8), (16, 1), (16, 16), (256, 128), (768, 96))   # (d, M): plain, odd dsub, one sub-quantiser, dsub = 1, largest table, the shape it is for
NTOTALS = (0, 1, 63, 64, 65, 1000, 4097)
NQS = (1, 3, 17)
KS = (1, 5, 29)


def random_codes(rng, n, M):
    """uniform over 0 .. 255, with 0 and 255 present in every column (n >= 2)"""
    codes = rng.integers(0, KSUB, (n, M), dtype=np.uint8)
    if n >= 2:
        for m in range(M):
            r = rng.choice(n, 2, replace=False)
            codes[r[0], m], codes[r[1], m] = 0, 255
    return codes


def case_planted(d, M, n, nq, seed=1):
    """a random codebook and random codes: the scan alone (set_codebook / add_codes)"""
    rng = np.random.default_rng(seed * 1000003 + d * 131 + M * 7 + n)
    cb = rng.standard_normal((M, KSUB, d // M)).astype(F)
    return {"d": d, "M": M, "codebook": cb, "codes": random_codes(rng, n, M), "q": rng.standard_normal((nq, d)).astype(F)}


def case_sum_order(d=32, M=8, n=1000, nq=3, seed=2):
    """sub-quantiser m's codebook scaled by 2^(6 (m mod 4)): the addends of a score differ by up to 2^18, so every order of the
    float32 sum other than ascending m rounds differently"""
    c = case_planted(d, M, n, nq, seed)
    c["codebook"] = (c["codebook"] * (2.0 ** (6 * (np.arange(M) % 4)))[:, None, None]).astype(F)
    return c


def case_ties(d=32, M=4, n=300, nq=2, seed=3):
    """n identical rows: the best k are rows 0 .. k - 1"""
    c = case_planted(d, M, n, nq, seed)
    c["codes"] = np.ascontiguousarray(np.tile(c["codes"][:1], (n, 1)))
    return c


def case_duplicates(d=32, M=4, n=4097, nq=3, seed=4):
    """query j's best row planted at rows that straddle the wave (64), workgroup (256, 1024) and segment boundaries"""
    c = case_planted(d, M, n, nq, seed)
    D = scores(lut(c["q"], c["codebook"]), c["codes"])
    top = int(np.argmax(D[0]))
    best = c["codes"][top].copy()
    where = sorted({r for r in (0, 63, 64, 65, 255, 256, 1023, 1024, 1025, 2048, 2049, n // 2, n - 1, top) if r < n})
    c["codes"][where] = best
    c["planted"] = where
    return c


def case_train_gauss(n=700, d=32, M=4, seed=5):
    rng = np.random.default_rng(seed * 7919 + n + d)
    return {"d": d, "M": M, "x": rng.standard_normal((n, d)).astype(F)}


def case_train_distinct(n=320, distinct=40, d=24, M=8, seed=6):
    """n rows made of `distinct` different ones: most centroids have no members (they keep their value) and equal centroids tie
    (the lowest j wins)"""
    rng = np.random.default_rng(seed * 104729 + n)
    base = rng.standard_normal((distinct, d)).astype(F)
    return {"d": d, "M": M, "x": np.ascontiguousarray(base[rng.integers(0, distinct, n)])}


def case_train_cancel(seed=7):
    """d = 2, M = 2, 512 rows, one iteration: the initial centroids are the even rows.  In column 0 centroid 0 is 0, centroid j is
    10 + j; the odd rows are 2^70 (row 1), 1 (row 3), -2^70 (row 5) and 10.25 + j.  The two huge rows are equally far from every
    centroid (the float32 difference is 2^70 whichever centroid), so they go to the lowest, centroid 0, and so does 1: its members
    in ascending row order are 0, 2^70, 1, -2^70 -- summed in that order the 1 is absorbed and the mean is 0; a tree reduction adds
    0 + 1 and 2^70 - 2^70 first and gives 1 / 4."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((512, 2)).astype(F)
    j = np.arange(256)
    x[0::2, 0] = 10.0 + j
    x[1::2, 0] = 10.25 + j
    x[0, 0], x[1, 0], x[3, 0], x[5, 0] = 0.0, 2.0 ** 70, 1.0, -(2.0 ** 70)
    return {"d": 2, "M": 2, "x": x}


def case_train_subsample(seed=8):
    """n = 65536 + 37 rows: the trainer looks at x[floor(i n / 65536)]"""
    rng = np.random.default_rng(seed)
    return {"d": 4, "M": 2, "x": rng.standard_normal((TRAIN_ROWS + 37, 4)).astype(F)}


def case_encode(n=500, d=24, M=8, seed=9):
    """rows to encode against a random codebook; row 3 holds a NaN, row 5 a +inf, row 7 is all NaN, row 9 all +inf"""
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((M, KSUB, d // M)).astype(F)
    x = rng.standard_normal((n, d)).astype(F)
    x[3, 4] = np.nan
    x[5, 10] = np.inf
    x[7] = np.nan
    x[9] = np.inf
    return {"d": d, "M": M, "codebook": cb, "x": x}
