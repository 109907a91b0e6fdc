"""Inputs, references and deliberate mistakes of tests/test_magnitude_cases_host.py and tests/test_gpu_magnitudes.py: every search
path away from zero-mean Gaussian data at unit scale.  NumPy only; no GPU is needed to import this module.

Families (a family transforms the Gaussian base inputs of oracle.synth; `family(name, n, nq)` describes one):
    scaled(a, b)      T1  rows x 2^a, queries x 2^b, the pairs of T1_PAIRS; (0, 0) is the baseline
    ragged_queries    T2  query j x 2^(12 (j mod 5) - 24): norms that differ by 2^48 inside one batch
    ragged_rows       T3  row i x 2^(6 (i mod 5) - 12)
    loud_row          T4  one mid-stream row x 2^12 (no edge row of a document block); the even queries are the Gaussian query
                          PLUS that row (it is their first result), the odd ones the query MINUS it (it is their last)
    all_negative      T5  rows |g| + 2^-6, queries -|g|: every score of the call is negative
    zero_queries      T6a the first and the last query are all-zero
    zero_rows         T6b every 7th row is all-zero, row 0 and row n - 1 among them
    zero_index        T6c 300 all-zero rows, Gaussian queries, one zero query

A power of two scales a float32 or bf16 value exactly, and an fp64 product or sum of such values likewise (nothing comes near the
ends of fp64), so the canonical dots of T1, T2, T3, T6a and T6b are those of their base inputs, scaled entry by entry -- `derive()`
does that from ONE all-pairs matrix per base, and tests/test_magnitude_cases_host.py shows that the derivation equals
orc.canonical_pairs on the transformed inputs bit for bit.

References.  All-pairs (`topk`, `in_range` on `keys`): the canonical fp64 dot of EVERY (query, row) pair, the float32 key (inner
product, or |q|^2 + phi - 2 q.x), order by (key, row).  orc.search_exact_bruteforce re-ranks an L2 result among the k + 16 best rows by
inner product only: too few where hundreds of rows share one float32 distance (T4: phi is 2^24 times a quiet row's norm).
search_wide, range_search and search_fused are always held to it (4099 rows of at most 250 columns, or 16 queries); a search()
case is where `needs_all_pairs` says that rows tie (T3, T4, T6; L2 under T1 with a != b and under T2), on N_ALL_PAIRS rows, and is
held to orc.search_exact on N_DEFAULT rows otherwise -- on those families the two agree (checked on the host).  sq8: the trained
quantiser and the search of tests/sq8_cases.py; the IVF paths: the restatements of tests/ivf_*_cases.py.

The window: every non-zero product |x_ij q_j|, every non-zero squared norm, phi and every non-zero finite key of a case lies in
[2^-110, 2^110] (`assert_window`), so no float32 subnormal or overflow arises and the flush-to-zero behaviour of the matrix pipe is
not what is tested.

The certificate's flagged count under T1.  Every bound the searches decide by is a product of the data: e = err_c |q| max|x|
(rank_flag_write, the wide scan's tau, range_tau_kernel), the key-rounding slack 2^-20 (|need| + |qq + phi|) of the exact pass, the
factors 1 + 1e-12 (tiny_search.hpp, aux_kernels.hpp: squared norms as upper bounds) and 1.000000001.  Three absolute constants
remain: + 1e-30 in resolve_kernels.hpp (the pre-filter of the exact pass, which runs AFTER the flags are set: it decides how many
rows a flagged query re-scores, never whether it is flagged) and -+ 1e-300 in range_kernels.hpp and scan_kernel_wide.hpp (added to
an fp64 bound B + e: inside the window B + e is either exactly 0 -- zero rows or queries, where the term makes the bound strict --
or at least 2^-110, and 1e-300 is far below half an fp64 ulp of that, so the sum does not change).  All three only widen a bound.
Hence nothing that sets a flag changes when rows and queries are scaled by powers of two inside the window, and the GPU file
asserts flagged(T1 pair) == flagged(baseline) wherever the result is the baseline's, scaled: inner product under every pair, L2
under a = b.
The exception is L2 under a != b, and it is the data's, not a constant's.  The key is float32(|q|^2 + phi - 2 q.x) with the three
terms at 2^(2b) d, 2^(2a) d and 2^(a+b) sqrt(d) times a few: for |a - b| >= 30 the largest term is 2^30 sqrt(d) / (a few) times the
last, one float32 ulp of it (2^-23 of it) exceeds the whole spread of 2 q.x over the rows, and every row of the index gets one
of at most a few float32 keys -- measured on the Gaussian base: 3 - 4 distinct distances per query under one loud row, one or two
here.  The k-th key is then shared by more rows than the widest pool (K' = 32) holds, so no certificate can vouch for WHICH of
them are the lowest rows: every such query must be flagged and settled by the exact pass.  `tied_beyond_pool` counts these
queries on the reference's keys; the GPU file asserts that they are at least nine in ten of the call (on an MI355X: 129 or 130 of
130, and exactly as many flagged), that flagged >= that count, and -- as under T3 and T4 -- that rescanned == flagged and nothing
stays unresolved.
"""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import ivf_cases as iv  # noqa: E402
    import scan_recipes as sr  # noqa: E402
    import sq8_cases as sq  # noqa: E402
finally:
    sys.path.pop(0)
from oracle import mips_oracle as orc  # noqa: E402
from oracle import synth  # noqa: E402

F = np.float32
WINDOW = (2.0 ** -110, 2.0 ** 110)
T1_PAIRS = ((30, 0), (-30, 0), (0, 30), (0, -30), (30, 30), (-30, -30), (30, -30))
N_DEFAULT = 4099                   # 32 blocks of 128 rows and a ragged one of 3
N_ZERO_INDEX = 300
LOUD_EXP = 12
RADIUS_FLOOR = F(2.0 ** -100)      # what stands in for a radius one subnormal step away from 0

# name, base ("gauss" | "neg" | "loud" | "zero"), row / query exponents, zero masks
Family = namedtuple("Family", "name base n nq rexp qexp rzero qzero")


def scaled_name(a, b):
    return f"scaled({a},{b})"


BASELINE = scaled_name(0, 0)
T1_NAMES = tuple(scaled_name(a, b) for a, b in T1_PAIRS)
T2, T3, T4, T5, T6A, T6B, T6C = "ragged_queries", "ragged_rows", "loud_row", "all_negative", "zero_queries", "zero_rows", "zero_index"
ALL_FAMILIES = (BASELINE,) + T1_NAMES + (T2, T3, T4, T5, T6A, T6B, T6C)
QUERY_SIDE = (BASELINE, scaled_name(0, 30), scaled_name(0, -30), T2, T5, T6A, T6B, T6C)   # what e4m3 rows x bf16 queries take (a = 0)
UNSCALED = (BASELINE, T5, T6A, T6B, T6C)                                                   # what an all-e4m3 index takes


def loud_row(n):
    """a mid-stream row that is neither the first nor the last row of a document block of any size in use"""
    row = (n // 2) // 128 * 128 + 37
    assert 0 < row < n - 1 and all(row % b not in (0, b - 1) for b in sr.DOC_BLOCKS)
    return row


def family(name, n, nq):
    rexp, qexp = np.zeros(n, np.int64), np.zeros(nq, np.int64)
    rzero, qzero = np.zeros(n, bool), np.zeros(nq, bool)
    base = "gauss"
    if name.startswith("scaled("):
        a, b = (int(t) for t in name[7:-1].split(","))
        rexp[:], qexp[:] = a, b
    elif name == T2:
        qexp[:] = 12 * (np.arange(nq) % 5) - 24
    elif name == T3:
        rexp[:] = 6 * (np.arange(n) % 5) - 12
    elif name == T4:
        base = "loud"
        rexp[loud_row(n)] = LOUD_EXP
    elif name == T5:
        base = "neg"
    elif name == T6A:
        qzero[[0, nq - 1]] = True
    elif name == T6B:
        rzero[::7] = True
        rzero[n - 1] = True
    elif name == T6C:
        base, n = "zero", N_ZERO_INDEX
        rexp, rzero = np.zeros(n, np.int64), np.ones(n, bool)
        qzero[nq // 2] = True
    else:
        raise KeyError(name)
    return Family(name, base, n, nq, rexp, qexp, rzero, qzero)


def scale_of(name):
    """(a, b) of a T1 family"""
    return tuple(int(t) for t in name[7:-1].split(","))


# ------------------------------------------------------------------ inputs
_GAUSSIAN = {}      # generated once per shape, read-only


def gaussian(storage, d, n, nq):
    """Gaussian rows and queries of oracle.synth (bf16-exact); storages that keep float32 values (f32, sq8) get a per-row float32
    factor, as tests/scan_recipes.py gives them, so that their values need all 24 mantissa bits"""
    key = (storage in ("f32", "sq8"), d, n, nq)
    if key not in _GAUSSIAN:
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
        if key[0]:
            rng = np.random.default_rng(d)
            x = (x * rng.uniform(0.75, 1.25, (n, 1)).astype(F)).astype(F)
            q = (q * rng.uniform(0.75, 1.25, (nq, 1)).astype(F)).astype(F)
        x.setflags(write=False)
        q.setflags(write=False)
        _GAUSSIAN[key] = (x, q)
    return _GAUSSIAN[key]


def base_inputs(base, storage, d, n, nq):
    """float32 (x, q) of a base, before the family's exponents and zeros"""
    x, q = gaussian(storage, d, n, nq)
    if base == "neg":
        return (np.abs(x) + F(2.0 ** -6)).astype(F), (-np.abs(q)).astype(F)
    if base == "loud":
        sign = np.where(np.arange(nq) % 2 == 0, F(1), F(-1))[:, None]
        return x, (q + sign * x[loud_row(n)][None, :]).astype(F)
    if base == "zero":
        return np.zeros((n, d), F), q
    return x, q


def apply(fam, x, q):
    """the family's exponents and zeros on float32 rows and queries (exact)"""
    x = np.ldexp(x, fam.rexp[:, None].astype(np.int32)).astype(F)
    q = np.ldexp(q, fam.qexp[:, None].astype(np.int32)).astype(F)
    x[fam.rzero] = 0
    q[fam.qzero] = 0
    return x, q


def inputs(name, storage, d, n, nq):
    """-> (fam, x, q): float32 rows and queries as a test adds and asks them"""
    fam = family(name, n, nq)
    x, q = apply(fam, *base_inputs(fam.base, storage, d, fam.n, nq))
    return fam, x, q


def stored(storage, x, q):
    """what the index multiplies (sq8 has its own reference: sq8_reference)"""
    return sr.storage_values(storage, x), sr.query_values(storage, q)


# ------------------------------------------------------------------ all-pairs canonical dots
Pairs = namedtuple("Pairs", "dot xx qq")     # fp64: [nq, n], [n], [nq]


def pairs_direct(xs, qs):
    """canonical dots of every pair and the canonical squared norms of stored values xs, qs"""
    n = xs.shape[0]
    cand = np.tile(np.arange(n, dtype=np.int64), (qs.shape[0], 1))
    return Pairs(orc.canonical_pairs(qs, xs, cand), orc.sumsq_canonical(xs), orc.sumsq_canonical(qs))


_BASE_PAIRS = {}


def base_pairs(base, storage, d, n, nq):
    """the all-pairs matrix of a base's STORED values: computed once, read-only"""
    key = (base, storage, d, n, nq)
    if key not in _BASE_PAIRS:
        p = pairs_direct(*stored(storage, *base_inputs(base, storage, d, n, nq)))
        for a in p:
            a.setflags(write=False)
        _BASE_PAIRS[key] = p
    return _BASE_PAIRS[key]


def derive(fam, bp):
    """the family's pairs from its base's: exponents add, zeroed rows and queries give + 0"""
    e = (fam.rexp[None, :] + fam.qexp[:, None]).astype(np.int32)
    dot = np.ldexp(bp.dot, e)
    xx = np.ldexp(bp.xx, (2 * fam.rexp).astype(np.int32))
    qq = np.ldexp(bp.qq, (2 * fam.qexp).astype(np.int32))
    dot[fam.qzero, :] = 0.0
    dot[:, fam.rzero] = 0.0
    xx[fam.rzero] = 0.0
    qq[fam.qzero] = 0.0
    return Pairs(dot, xx, qq)


def pairs(name, storage, d, n, nq):
    fam = family(name, n, nq)
    return derive(fam, base_pairs(fam.base, storage, d, fam.n, nq))


def keys(p, metric):
    """float32 [nq, n]: the value a search reports and ranks by"""
    if metric == 1:
        phi = p.xx.max() if len(p.xx) else 0.0
        return (p.qq[:, None] + phi - 2.0 * p.dot).astype(F)
    return p.dot.astype(F)


# ------------------------------------------------------------------ references on a key matrix
def _mask_of(mask, j):
    return None if mask is None else (mask if mask.ndim == 1 else mask[j])


def topk(key, k, metric, mask=None):
    """(D float32 [nq, k], I int64 [nq, k]): the best k by (key, row) -- inner product descending, distance ascending, ties to the
    lowest row; mask (bool [n] or [nq, n]): the rows that may answer; -1 / -+inf padding"""
    nq, n = key.shape
    D = np.full((nq, k), np.inf if metric == 1 else -np.inf, F)
    I = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        m = _mask_of(mask, j)
        ids = np.arange(n, dtype=np.int64) if m is None else np.flatnonzero(m).astype(np.int64)
        kj = key[j, ids]
        order = np.lexsort((ids, kj if metric == 1 else -kj))[:k]
        D[j, :len(order)] = kj[order]
        I[j, :len(order)] = ids[order]
    return D, I


WIDEST_POOL = 32      # K' of the deepest candidate pool of MipsIndex.search (csrc/host_launch.hpp, pool_policy)


def tied_beyond_pool(key, k, metric):
    """the number of queries whose k-th best key is shared by more than WIDEST_POOL rows: no pool can hold them all, so the
    certificate cannot vouch for WHICH of them are the lowest rows"""
    kth = (np.sort(key, axis=1)[:, k - 1] if metric == 1 else -np.sort(-key, axis=1)[:, k - 1])[:, None]
    return int(((key == kth).sum(axis=1) > WIDEST_POOL).sum())


RANGE_COUNTS = (0, 1, 7, 50, None)     # None: every row


def radii_for_counts(key, metric, mask=None, counts=RANGE_COUNTS):
    """float32 [nq]: query j gets the radius that admits counts[j mod len] of its (admitted) rows -- the key of the next best one,
    so that row and its ties stay out under the strict rule; None: one step beyond the worst key.  A radius that would be a
    subnormal step away from 0 is -+2^-100 instead.  (the `radius_for_count` of tests/ivf_range_cases.py, for both metrics)"""
    nq = key.shape[0]
    permissive = F(np.inf) if metric == 1 else F(-np.inf)
    r = np.empty(nq, F)
    for j in range(nq):
        m = _mask_of(mask, j)
        kj = key[j] if m is None else key[j, m]
        best = np.sort(kj) if metric == 1 else np.sort(kj)[::-1]
        c = counts[j % len(counts)]
        if len(best) and best[0] == best[-1]:          # every row ties: even queries take them all, odd ones sit ON the value (none)
            c = None if j % 2 == 0 else 0
        if c is None or c >= len(best):
            r[j] = np.nextafter(best[-1], permissive) if len(best) else F(0)
        else:
            r[j] = best[c]
        if r[j] != 0 and abs(float(r[j])) < WINDOW[0]:
            r[j] = RADIUS_FLOOR if metric == 1 else -RADIUS_FLOOR
    return r


def in_range(key, r, metric, mask=None):
    """(lims, D, I) in CSR form: the rows strictly inside the radius, ascending"""
    lims, D, I = [0], [np.zeros(0, F)], [np.zeros(0, np.int64)]
    for j in range(key.shape[0]):
        hit = key[j] < r[j] if metric == 1 else key[j] > r[j]
        m = _mask_of(mask, j)
        if m is not None:
            hit = hit & m
        ids = np.flatnonzero(hit)
        lims.append(lims[-1] + len(ids))
        D.append(key[j][ids])
        I.append(ids.astype(np.int64))
    return np.asarray(lims, np.int64), np.concatenate(D).astype(F), np.concatenate(I)


def group_mask(labels, q_labels, mode="exclude"):
    """bool [nq, n]: the rows the group rule admits for every query"""
    same = np.asarray(labels)[None, :] == np.asarray(q_labels)[:, None]
    return ~same if mode == "exclude" else same


def selector_mask(n):
    """a bitmap that keeps about 5 rows in 8, with runs of refused rows over the first block boundary and the ragged tail"""
    keep = (np.arange(n) * 2654435761 % 8) < 5
    keep[120:140] = False
    keep[n - 2:] = False
    return keep


def row_labels(n):
    return (np.arange(n) // 3 % 11).astype(np.int32)


def query_labels(nq):
    return (np.arange(nq) % 11).astype(np.int32)


# ------------------------------------------------------------------ sq8
def sq8_reference(x, q, k):
    """(D, I, vmin, vdiff, codes): the quantiser trained on the rows it then holds, tests/sq8_cases.py's search"""
    vmin, vdiff = sq.train(x)
    codes = sq.encode(x, vmin, vdiff)
    D, I = sq.search(q, codes, vmin, vdiff, k)
    return D, I, vmin, vdiff, codes


# ------------------------------------------------------------------ the window
def _nonzero_range(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    nz = a[(a != 0) & np.isfinite(a)]
    return (nz.min(), nz.max()) if nz.size else None


def _inside(rng, what):
    if rng is not None:
        assert WINDOW[0] <= rng[0] and rng[1] <= WINDOW[1], f"{what}: [2^{np.log2(rng[0]):.1f}, 2^{np.log2(rng[1]):.1f}] leaves the window"


def assert_products(xs, qs, what=""):
    """every non-zero |x_ij q_j| lies inside WINDOW"""
    ax, aq = np.abs(xs.astype(np.float64)), np.abs(qs.astype(np.float64))
    xlo, qlo = np.where(ax > 0, ax, np.inf).min(axis=0), np.where(aq > 0, aq, np.inf).min(axis=0)
    lo, hi = xlo * qlo, ax.max(axis=0) * aq.max(axis=0)
    lo, hi = lo[np.isfinite(lo)], hi[hi > 0]
    if lo.size:
        _inside((lo.min(), hi.max()), f"{what}: products")


def assert_window(xs, qs, p=None, what=""):
    """every non-zero |x_ij q_j|, every non-zero squared norm, phi and every non-zero finite key (both metrics) of the stored values
    xs, qs lies inside WINDOW.  The products are bounded column by column: the smallest and largest non-zero magnitude of a column of
    xs times those of the same column of qs are the extremes over all pairs."""
    assert_products(xs, qs, what)
    if p is None:      # (an fp64 matrix product stands in for the canonical dots: the window is 2^20 wide of anything here)
        p = Pairs(qs.astype(np.float64) @ xs.astype(np.float64).T, orc.sumsq_canonical(xs), orc.sumsq_canonical(qs))
    _inside(_nonzero_range(p.xx), f"{what}: row norms (phi among them)")
    _inside(_nonzero_range(p.qq), f"{what}: query norms")
    if p.dot.size:
        for metric in (0, 1):
            _inside(_nonzero_range(keys(p, metric)), f"{what}: keys of metric {metric}")


# ------------------------------------------------------------------ deliberate mistakes (restated on a key matrix)
MISTAKES = ("zero_init", "pad_scores_zero", "abs_eps", "neighbour_norm", "ip_prefilter_only", "zero_row_is_padding")


def wrong_topk(wrong, p, k, metric):
    """top-k as a kernel making the named mistake would return it (inner product unless the mistake is about L2)"""
    key = keys(p, metric)
    nq, n = key.shape
    if wrong == "zero_init":          # the pool starts with k entries (0, no row): only positive scores get in
        D, I = topk(key, k, 0, mask=key > 0)
        return np.where(I < 0, F(0), D).astype(F), I
    if wrong == "pad_scores_zero":    # the rows n .. roundup(n, 128) take part with score 0
        pad = -n % 128
        return topk(np.concatenate([key, np.zeros((nq, pad), F)], axis=1), k, 0)
    if wrong == "zero_row_is_padding":
        return topk(key, k, metric, mask=p.xx > 0)
    if wrong == "ip_prefilter_only":  # L2 re-ranked among the k + 16 best rows by inner product
        _, cand = topk(p.dot.astype(F), min(n, k + 16), 0)
        mask = np.zeros((nq, n), bool)
        np.put_along_axis(mask, cand, True, axis=1)
        return topk(key, k, 1, mask=mask)
    raise KeyError(wrong)


def wrong_range(wrong, p, r, metric):
    key = keys(p, metric)
    if wrong == "abs_eps":            # an absolute 1e-6 between the key and the radius
        shifted = (r.astype(np.float64) + (-1e-6 if metric == 1 else 1e-6))
        return in_range(key.astype(np.float64), shifted, metric)[0::2]
    if wrong == "neighbour_norm":     # the L2 image of every query is built with query 0's norm
        phi = p.xx.max()
        return in_range((p.qq[0] + phi - 2.0 * p.dot).astype(F), r, 1)[0::2]
    if wrong == "zero_row_is_padding":
        return in_range(key, r, metric, mask=p.xx > 0)[0::2]
    if wrong == "zero_init":          # the threshold starts at 0: a negative radius admits nothing below 0
        return in_range(key, np.maximum(r, F(0)), 0)[0::2]
    raise KeyError(wrong)


# ------------------------------------------------------------------ what tests/test_gpu_magnitudes.py runs (the host file checks the window of all of it)
STD = (BASELINE,) + T1_NAMES + (T2, T5, T6A, T6B, T6C)
FULL = STD + (T3, T4)
# kernel: the instance of tests/scan_recipes.py whose recipe (storage, d, k, knobs) the case borrows; nq may be smaller than there
SearchCase = namedtuple("SearchCase", "kernel storage d nq k knobs families metrics")
SQ8_KERNEL = "mips::sq8_scan_kernel"


def _recipe(name, families, nq=None):
    r = sr.RECIPES[name]
    return SearchCase(name, r.storage, r.d, nq or r.nq, r.k, r.knobs, families, (0, 1))


def search_cases():
    out = [
        _recipe("mips::scan_kernel_v3<8, 16, 1, 2, true, 0, 2, 8, 3, true, true, 8>", STD),
        _recipe("mips::scan_kernel_v4<6, 24, 2, 0, true, 1>", FULL),                          # the large-kernel recipe of T3 / T4
        _recipe("mips::scan_kernel_v4<6, 16, 2, 0, true, 4>", FULL),                          # stage 1 of the "f32" two-stage search
        _recipe("mips::scan_kernel_k3<4, 32, 2, 0, 1>", STD, nq=260),                         # (beyond 256 queries)
        _recipe("mips::scan_kernel_k3<4, 32, 2, 0, 4>", STD, nq=260),                         # pools of 32 at k = 12: queries ARE flagged at unit scale
        _recipe("mips::scan_kernel<8>", FULL),                                                # "f32" with f32_fast = 0
        _recipe("mips::scan_kernel_e8<6, 256, 4, 3, false, 1, true, 4>", QUERY_SIDE),
        _recipe("mips::scan_kernel_f8x<6, 256, 2, 0, true>", UNSCALED),
        _recipe("mips::scan_kernel_f8<10, 512, 2, true>", UNSCALED),
    ]
    for l2 in (False, True):
        for f32 in (False, True):
            name = f"mips::tiny_search_kernel<{'true' if l2 else 'false'}, {'true' if f32 else 'false'}>"
            out.append(_recipe(name, FULL)._replace(metrics=(int(l2),)))
    out.append(SearchCase(SQ8_KERNEL, "sq8", 250, 40, 5, (), FULL, (0,)))       # (its reference scores every pair: a 64-query tile, ragged)
    return out


WIDE_K = 64
WIDE_SHAPES = (("bf16", 250, 130), ("f32", 100, 130))       # (storage, d, nq) of search_wide and range_search: bases shared with search_cases
FUSED_SHAPES = (("bf16", 700, 16), ("f32", 500, 16))        # search_fused: the one-launch shapes
FUSED_K = 5
IVF_SHAPE = (100, 2053, 24)                                 # (d, n, nq)
IVF_STORAGES = ("bf16", "f32", "sq8")


N_ALL_PAIRS = 2039          # 15 blocks of 128 rows and a ragged one: the rows of a search() case whose reference is all-pairs


def needs_all_pairs(name, metric):
    """Is the result of a family tie-free, so that orc.search_exact's k + 16 candidates hold it?  Not where rows or queries are
    zero (everything ties), not under T3 / T4, and not under L2 once |q|^2, phi and q.x differ by many powers of two (T1 with a != b,
    T2): whole stretches of rows then share one float32 distance."""
    if name in (T3, T4, T6A, T6B, T6C):
        return True
    if metric == 1 and (name == T2 or (name.startswith("scaled(") and len(set(scale_of(name))) == 2)):
        return True
    return False


def search_rows(name, metric):
    """rows of a search() case: N_DEFAULT where orc.search_exact is the reference, N_ALL_PAIRS where every pair is scored"""
    return N_ALL_PAIRS if needs_all_pairs(name, metric) else N_DEFAULT


def search_reference(name, storage, d, nq, k, metric):
    """-> (D, I) of MipsIndex.search on the family at search_rows(name, metric) rows (sq8: sq8_reference on the inputs instead)"""
    n = search_rows(name, metric)
    if needs_all_pairs(name, metric):
        return topk(keys(pairs(name, storage, d, n, nq), metric), k, metric)
    _, x, q = inputs(name, storage, d, n, nq)
    xs, qs = stored(storage, x, q)
    return orc.search_exact(qs, xs, k, metric=metric)


def flat_window_cases():
    """(what, family name, storage, d, n, nq) of every flat call of the GPU file"""
    seen = {}
    for c in search_cases():
        for f in c.families:
            for metric in c.metrics:
                seen[(f, c.storage, c.d, N_DEFAULT if c.storage == "sq8" else search_rows(f, metric), c.nq)] = c.kernel
    for storage, d, nq in WIDE_SHAPES + FUSED_SHAPES:
        for f in FULL if (storage, d, nq) in WIDE_SHAPES else STD:
            seen.setdefault((f, storage, d, N_DEFAULT, nq), "wide / range / fused")
    return [(what,) + key for key, what in seen.items()]


# ------------------------------------------------------------------ IVF
IVF_NLIST = 8


def ivf_centroids(d, exp=0):
    """planted centroids (IvfIndex.set_centroids): normalised Gaussian directions x 2^exp; the lists they cut out of Gaussian or
    positive rows are of ragged length"""
    rng = np.random.default_rng(7 * d + 1)
    c = iv.normalise(rng.standard_normal((IVF_NLIST, d)).astype(F))
    return np.ldexp(c, np.int32(exp)).astype(F)


def ivf_case(name, storage, d, n, nq, centroid_exp=None):
    """-> dict(rows, q, centroids, assign, par): a family on an IVF index.  The centroids scale with the rows of a T1 family
    (centroid_exp=0 leaves them at unit scale under rows x 2^30: the "unscaled_centroids" case); assign and the probed lists come from the probe
    restatement of tests/ivf_cases.py; par: the sq8 range trained on the rows"""
    fam, x, q = inputs(name, storage, d, n, nq)
    if centroid_exp is None:
        centroid_exp = scale_of(name)[0] if name.startswith("scaled(") else 0
    c = ivf_centroids(d, centroid_exp)
    par = sq.train(x) if storage == "sq8" else None
    return {"rows": x, "q": q, "centroids": c, "assign": iv.nearest(x, c)[:, 0], "par": par, "fam": fam}
