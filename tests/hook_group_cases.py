"""Inputs and expectations of the grouped one-launch hook search (mips_search_fused_grp, MipsIndex.search_fused(groups=)), shared by
tests/test_hook_group_host.py (CPU: the builders do what they say, and the wrong kernels they are meant to catch ARE wrong on
them) and tests/test_gpu_hook_groups.py (GPU: the library against the expectations).  Pure NumPy + the oracle, no GPU.

Expectations are the oracle's FULL ranking of all rows, filtered per query by the admission matrix, cut to k and padded --
_admit / _filter_ranking of tests/test_gpu_grouped.py.  Where the brute-force ranking (an insertion sort) would take minutes the
ranking comes from the canonical values of all pairs (orc.canonical_pairs) ordered by orc._order_desc, the order the brute force
applies; test_hook_group_host.py checks on a small shape that the two are the same ranking, bit for bit."""
import numpy as np

from oracle import mips_oracle as orc
from oracle import synth

NONE = -(1 << 31)  # MIPS_LABEL_NONE
ABSENT = 1 << 20   # a label no row of these cases carries


# ------------------------------------------------------------------ expectations
def admit(labels, qlabels, mode):
    """bool [nq, n]: may row i answer query j under the group rule?"""
    labels, qlabels = np.asarray(labels, np.int64), np.asarray(qlabels, np.int64)
    eq = labels[None, :] == qlabels[:, None]
    return np.where((qlabels == NONE)[:, None], True, eq if mode == "only" else ~eq)


def filter_ranking(full, adm, k, metric, idx_offset=0):
    """full = (values, ids) [nq, n], the ranking of ALL rows -> the k best admitted rows per query, padded (-+inf, -1)."""
    fs, fi = full
    nq = fs.shape[0]
    s = np.full((nq, k), np.inf if metric else -np.inf, np.float32)
    i = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        keep = np.flatnonzero(adm[j][fi[j]])[:k]
        s[j, :len(keep)] = fs[j, keep]
        i[j, :len(keep)] = fi[j, keep] + idx_offset
    return s, i


def dots(q, x):
    """float64 [nq, n]: the canonical inner product (sequential fp64 sum) of every pair."""
    n = x.shape[0]
    return orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1)))


def values(q, x, metric, dot=None):
    """float32 [nq, n]: the output value of every pair -- the inner product, or |q|^2 + phi - 2 q.x (metric 1, phi over ALL rows)."""
    dot = dots(q, x) if dot is None else dot
    if metric == 1:
        phi = orc.sumsq_canonical(x).max()
        return (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * dot).astype(np.float32)
    return dot.astype(np.float32)


def ranking(vals, metric):
    """(values best first, rows) [nq, n] out of the all-pairs values: (value best first, row ascending)."""
    ids = np.tile(np.arange(vals.shape[1], dtype=np.int64), (vals.shape[0], 1))
    order = orc._order_desc(-vals if metric == 1 else vals, ids)
    return np.take_along_axis(vals, order, axis=1), order.astype(np.int64)


def drop_banned(exp1, banned, k, metric):
    """The ignore filter on a (k + 1)-wide result: the entry equal to banned[j] leaves, the rest is cut to k (padding stays)."""
    s1, i1 = exp1
    nq = s1.shape[0]
    s = np.full((nq, k), np.inf if metric else -np.inf, np.float32)
    i = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        keep = np.flatnonzero(i1[j] != banned[j])[:k]
        s[j, :len(keep)] = s1[j, keep]
        i[j, :len(keep)] = i1[j, keep]
    return s, i


def pick_banned(exp1, absent=(1 << 40)):
    """One id per query to ban: its second hit, else its first, else an id nothing has (never -1: that is the padding)."""
    i1 = exp1[1]
    second = i1[:, 1] if i1.shape[1] > 1 else i1[:, 0]
    return np.where(second >= 0, second, np.where(i1[:, 0] >= 0, i1[:, 0], absent)).astype(np.int64)


def labellings(n):
    row = np.arange(n)
    return {"row % 5": row % 5, "row // 2": row // 2, "random 7": np.random.default_rng(n).integers(0, 7, n), "one label": np.full(n, 3)}


def query_labels(labels, nq):
    """Cycle through (up to five) present labels, one absent label and LABEL_NONE."""
    present = np.unique(labels)
    cyc = [int(v) for v in present[np.linspace(0, len(present) - 1, min(5, len(present))).astype(int)]] + [ABSENT, NONE]
    return np.array([cyc[j % len(cyc)] for j in range(nq)], np.int64)


# ------------------------------------------------------------------ case "own group on top"
OWN_M = 40     # rows of a labelled query's own group
OWN_POOL = 8   # the re-score pool of the one-launch kernel


def own_group_on_top(n=5003, d=256, nq=8, seed=41, f32=False):
    """-> (x [n, d], q [nq, d], labels [n], qlabels [nq]).  Query j < nq - 1 carries label 100 + j, and the OWN_M rows of that
    group are its own direction, q_j scaled by 1 .. 2 (distinct factors): they out-score every other row, so its unfiltered top
    OWN_POOL is entirely own-group.  Every other row is Gaussian and labelled row % 7; the last query is LABEL_NONE.
    f32: rows and queries keep float32 values (fp32-exact index), otherwise everything is rounded to bf16."""
    rng = np.random.default_rng(seed)
    rnd = (lambda a: np.ascontiguousarray(a, dtype=np.float32)) if f32 else synth.round_to_bf16
    x = rnd(rng.standard_normal((n, d)).astype(np.float32))
    q = rnd(rng.standard_normal((nq, d)).astype(np.float32))
    labels = (np.arange(n) % 7).astype(np.int64)
    spots = rng.permutation(n)[:(nq - 1) * OWN_M].reshape(nq - 1, OWN_M)
    for j in range(nq - 1):
        scale = (1.0 + (1 + np.arange(OWN_M)) / OWN_M).astype(np.float32)
        x[spots[j]] = rnd(q[j][None, :] * scale[:, None])
        labels[spots[j]] = 100 + j
    qlabels = np.array([100 + j for j in range(nq - 1)] + [NONE], np.int64)
    return x, q, labels, qlabels


def ignore_labels(full, k):
    """A wrong kernel: the labels are dropped."""
    return full[0][:, :k].copy(), full[1][:, :k].copy()


def filter_after_pool(full, adm, k, metric, pool=OWN_POOL):
    """A wrong kernel: the pool of `pool` candidates is selected first, the group rule applied to the pool."""
    return filter_ranking((full[0][:, :pool], full[1][:, :pool]), adm, k, metric)


# ------------------------------------------------------------------ case "ties at the k-th"
TIE_COPIES = 150   # rows tied with the k-th admitted score of the chosen queries
TIE_A, TIE_B, TIE_C = 7, 8, 9
TIE_CHOSEN = (0, 3)


def ties_at_kth(n=3000, d=128, nq=6, seed=5, graded=False):
    """-> (x, q, labels, qlabels, copies, twice): the last two are the row numbers of the copies of u (ascending) and of the two
    2 u rows.  Lattice rows and queries (synth.KIND_LATTICE: integers / 64, exact in bf16).  The chosen
    queries TIE_CHOSEN are one lattice vector u; TIE_COPIES scattered rows are copies of u (every third labelled TIE_A, the
    others TIE_B) and two rows are 2 u (one TIE_A, one TIE_B; integers up to 254 / 64 are bf16 values too).  By Cauchy-Schwarz
    the 2 u rows and then the copies out-score every other row of the lattice for u; all copies tie, so with k = 5 the k-th
    admitted score of a chosen query is the tie's, reached by TIE_COPIES rows of which some are admitted and some are not.
    Query 0 is labelled TIE_A, query 3 TIE_B; the others cycle through row % 5 labels (the rest of the rows), ABSENT and NONE.
    graded (the fp32-exact index, floods_graded of tests/wide_cases.py): copy c is float32(u (1 + c 2^-19)) -- the same bf16
    image for every copy, so the scan scores them alike, while the canonical score grows with c: nothing ties any more, the
    best admitted rows are the HIGHEST admitted copies, and only the settlement can find them.  The graded copies lie in ONE run
    of rows from row 1000 on: the fp32-exact kernel re-scores each workgroup's pool of 8 on the fp32 rows, so copies spread thinly
    over the workgroups would all reach the final selection and be ranked right without a settlement."""
    x = synth.generate(seed, 0, n, d, synth.KIND_LATTICE)
    q = synth.generate(seed + 1, 0, nq, d, synth.KIND_LATTICE)
    u = synth.generate(seed + 2, 0, 1, d, synth.KIND_LATTICE)[0]
    rng = np.random.default_rng(seed)
    spots = np.sort(rng.permutation(n)[:TIE_COPIES + 2])
    if graded:  # one run of rows: a workgroup of the one-launch kernel (128 rows) then holds far more copies than its pool of 8
        spots = 1000 + np.arange(TIE_COPIES + 2)
    twice, copies = spots[[40, 90]], np.delete(spots, [40, 90])
    labels = (np.arange(n) % 5).astype(np.int64)
    x[copies] = u
    if graded:
        c = np.arange(TIE_COPIES, dtype=np.float64)
        x[copies] = (u.astype(np.float64)[None, :] * (1.0 + c * 2.0 ** -19)[:, None]).astype(np.float32)
        assert np.array_equal(synth.round_to_bf16(x[copies]), np.tile(u, (TIE_COPIES, 1)))
    labels[copies] = np.where(np.arange(TIE_COPIES) % 3 == 0, TIE_A, TIE_B)
    x[twice] = 2.0 * u
    labels[twice] = (TIE_A, TIE_B)
    for j in TIE_CHOSEN:
        q[j] = u
    cyc = [0, 1, ABSENT, NONE]
    qlabels = np.array([cyc[j % len(cyc)] for j in range(nq)], np.int64)
    qlabels[TIE_CHOSEN[0]], qlabels[TIE_CHOSEN[1]] = TIE_A, TIE_B
    return np.ascontiguousarray(x), q, labels, qlabels, copies, twice
