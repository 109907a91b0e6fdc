"""Inputs, references and bound models of tests/test_lifecycle_cases_host.py and tests/test_gpu_lifecycle.py: searches on an index
that CHANGES between the calls (add, growth, reset, phi override, add_synthetic).  Not a test file; NumPy only, no GPU is needed
to import it.

Why planted data.  The native host caches max |x|^2 (xmax2), max |x - bf16 x|^2 (dres2), phi and the bf16 image of an fp32-exact
index between calls (csrc/host_state.hpp) and every search trusts them.  A cached scalar that survives an add is TOO SMALL; a
bound that is too small never crashes, it certifies a wrong top-k or drops range members -- but only where the scan's score and
the exact score disagree by more than the stale bound, which Gaussian rows never do.  The blocks below make them disagree by a
known, exactly representable amount:

  block A  "plain"     rows of bf16 values with norm ~1: dres2 = 0, xmax2 ~ 1.
  block R  "residual"  PLANTED rows x = h + rho: h = the +-1 pattern g of the R-planted queries, rho = sign(g) 2^-9 (under half a
                       bf16 ulp at 1: bf16(x) = h).  The scan of an fp32-exact index sees h . q, the exact score is larger by
                       rho . q = 2^-9 sum |q_i| =: shift.  DECOY rows are bf16 values whose scan score is ABOVE the planted rows' and
                       whose exact score is BELOW: stage 1 ranks NDECOY decoys in front of every planted row, the truth has the
                       planted rows first.
  block B  "big"       PLANTED rows of norm ~10^3, S ph on one half M of the columns; the B-planted queries are ph (1 + 2^-9) on M
                       -- q = bf16(q) + delta with delta sign-aligned to the big rows -- and ph on the other half N, where the
                       decoys S ph live (delta = 0 there: their scan and exact scores agree).  Again the scan ranks NDECOY decoys
                       first and the truth the planted rows; here the term (x_max + d_res) |q - bf16 q| of the bound decides, so
                       a stale xmax2 does.  One such row moves phi by ~10^6.

Scores inside a family are spaced by LEVELS: the last LEVEL_COLS columns of the planted queries hold 2^-3 and those of the rows
small multiples of a power of two, so that row "level L" scores L units more; planted rows have levels 0 .. NPLANT - 1, decoys
the plan of decoy_levels() (the best TOP, a gap of LEVEL_GAP units, then one unit apart), all below the planted rows' shift.  The
two families are orthogonal on purpose (g = ph r with sum_M r = sum_N r = 0), so neither disturbs the other's ranking.  Every
product and every partial sum of a planted pair is a small multiple of a power of two: the MFMA scan is exact on them whatever
its summation order, which is what lets a CPU model say what the scan sees.

References: the oracle's canonical arithmetic over ALL pairs (orc.canonical_pairs / orc.sumsq_canonical), ranked by (value best
first, row ascending) -- what orc.search_exact_bruteforce returns, asserted by the host test -- and the strict float32 rule of
tests/test_gpu_range.py for range search.  phi is an argument (the maximum over the rows the index should hold, or an override)."""
import math

import numpy as np

from oracle import mips_oracle as orc
from oracle import synth

F32 = np.float32
F64 = np.float64
SEED = 20240907

DIMS = (64, 128, 1024)   # 64: row pitch 64, never the one-launch kernel; 128: the smallest pitch it takes; 1024: the largest
LEVEL_COLS = 4
QSMALL = 2.0 ** -3       # the planted queries' value in the level columns
RHO = 2.0 ** -9          # residual of the R rows and delta of the B-planted queries, relative to the +-1 pattern
NPLANT = 8               # planted rows per family (> k of search())
NDECOY = 360             # decoys per family: more than the widest pool (k' = 64 + 256 + 16 on the fp32-exact index)
TOP = 5                  # decoys above the gap: the wrong top-5
LEVEL_T = 470            # decoy levels lie below it
LEVEL_GAP = 100          # units between the TOP best decoys and the rest (wider than any stale bound: asserted by the host test)
N_A = 2048 + 37
NQ = 40
NQ_TINY = 8
K_SEARCH = 5
K_WIDE = 64
POOLS = (8, 16, 32)      # candidate pools of search() (csrc/mips_hip.hip, search_impl: K' = 8 / 16 / 32)
PHI_OVERRIDE = 8.0e6     # above every local maximum of these cases

STORAGES = ("bf16", "f32", "fp8_e4m3", "fp8_e4m3_docs")


def stored_rows(x, storage):
    """What an index of that storage makes of float32 rows."""
    x = np.ascontiguousarray(x, dtype=F32)
    if storage == "f32":
        return x
    return synth.round_to_bf16(x) if storage == "bf16" else synth.round_to_e4m3(x)


def stored_queries(q, storage):
    q = np.ascontiguousarray(q, dtype=F32)
    if storage == "f32":
        return q
    return synth.round_to_e4m3(q) if storage == "fp8_e4m3" else synth.round_to_bf16(q)


def _balanced(n, rng):
    assert n % 2 == 0
    r = np.concatenate([np.ones(n // 2), -np.ones(n // 2)])
    rng.shuffle(r)
    return r


def decoy_levels():
    """Level of decoy m, best first: LEVEL_T - 1 .. LEVEL_T - TOP, the gap, then one unit apart."""
    m = np.arange(NDECOY)
    return np.where(m < TOP, LEVEL_T - 1 - m, LEVEL_T - TOP - LEVEL_GAP - (m - TOP)).astype(np.int64)


def _unit(shift):
    """The largest power of two u with shift / u >= 475 (> LEVEL_T: every decoy's exact score stays below the planted rows')."""
    return 2.0 ** math.floor(math.log2(shift / 475.0))


class Family:
    """Everything of one dimension d: the patterns, the two planted queries, blocks A, R, B, the extra row and the query set."""

    def __init__(self, d):
        assert d in DIMS
        self.d = d
        rng = np.random.default_rng([SEED, d])
        body = self.body = d - LEVEL_COLS
        half = self.half = body // 2
        perm = rng.permutation(body)
        self.M, self.N = np.sort(perm[:half]), np.sort(perm[half:])
        self.ph = rng.choice([-1.0, 1.0], size=body)
        r = np.empty(body)
        r[self.M], r[self.N] = _balanced(half, rng), _balanced(half, rng)
        self.g_body = self.ph * r
        self.S = 2.0 ** 7 if d <= 128 else 2.0 ** 5
        self.shift_r = body * RHO                       # rho . g
        self.shift_b = self.S * half * RHO              # (big row) . delta
        self.unit_r, self.unit_b = _unit(self.shift_r), _unit(self.shift_b)
        self.base_r = float(body)                       # h . g
        self.base_b = self.S * half                     # (big row) . bf16(p) = (B decoy) . p
        lv = decoy_levels()
        assert lv.min() > NPLANT and lv.max() < LEVEL_T and len(set(lv.tolist())) == NDECOY

        # ---- planted queries
        self.g = np.concatenate([self.g_body, np.full(LEVEL_COLS, QSMALL)]).astype(F32)
        p = self.ph.copy()
        p[self.M] *= 1.0 + RHO
        self.p = np.concatenate([p, np.full(LEVEL_COLS, QSMALL)]).astype(F32)

        # ---- blocks (planted rows and decoys shuffled together: the candidate lists of the scans see them mixed)
        def levels(L, unit):
            out = np.zeros((len(L), LEVEL_COLS))
            left = np.asarray(L, dtype=np.int64).copy()
            for c in range(LEVEL_COLS):
                a = np.minimum(left, 255)
                out[:, c] = a * (unit / QSMALL)
                left -= a
            assert (left == 0).all()
            return out

        plant_l = np.arange(NPLANT)
        r_plant = np.concatenate([np.tile(self.g_body * (1.0 + RHO), (NPLANT, 1)), levels(plant_l, self.unit_r)], axis=1)
        r_decoy = np.concatenate([np.tile(self.g_body, (NDECOY, 1)), levels(lv, self.unit_r)], axis=1)
        big = np.zeros(body)
        big[self.M] = self.S * self.ph[self.M]
        dec = np.zeros(body)
        dec[self.N] = self.S * self.ph[self.N]
        b_plant = np.concatenate([np.tile(big, (NPLANT, 1)), levels(plant_l, self.unit_b)], axis=1)
        b_decoy = np.concatenate([np.tile(dec, (NDECOY, 1)), levels(lv, self.unit_b)], axis=1)
        order_r, order_b = rng.permutation(NPLANT + NDECOY), rng.permutation(NPLANT + NDECOY)
        self.R = np.ascontiguousarray(np.concatenate([r_plant, r_decoy])[order_r].astype(F32))
        self.B = np.ascontiguousarray(np.concatenate([b_plant, b_decoy])[order_b].astype(F32))
        # position inside the block of planted row m / decoy m
        inv_r, inv_b = np.argsort(order_r), np.argsort(order_b)
        self.r_plant_at, self.r_decoy_at = inv_r[:NPLANT], inv_r[NPLANT:]
        self.b_plant_at, self.b_decoy_at = inv_b[:NPLANT], inv_b[NPLANT:]
        a = rng.standard_normal((N_A, d)) / math.sqrt(d)
        self.A = synth.round_to_bf16(a.astype(F32))
        self.A2 = synth.round_to_bf16((rng.standard_normal((N_A, d)) / math.sqrt(d)).astype(F32))   # what a reset index is refilled with
        extra = np.zeros(d)
        extra[self.M] = 2.0 * self.S * self.ph[self.M]            # twice a big row: the new maximum norm, phi x 4
        self.extra = extra.astype(F32)[None, :]

        # ---- queries: j % 5 == 1 R-planted, j % 5 == 3 B-planted (scaled by powers of two), the others Gaussian float32
        q = rng.standard_normal((NQ, d)).astype(F32)
        self.r_queries, self.b_queries, self.scale = [], [], np.ones(NQ)
        for j in range(NQ):
            s = 2.0 ** ((j // 5) % 4 - 1)
            if j % 5 == 1:
                q[j], self.scale[j] = self.g * F32(s), s
                self.r_queries.append(j)
            elif j % 5 == 3:
                q[j], self.scale[j] = self.p * F32(s), s
                self.b_queries.append(j)
        self.q = np.ascontiguousarray(q)
        # 80 copies of the R-planted query: with block R in an fp32-exact index every one of them is flagged (what arms the
        # stage-1 skip of csrc/host_search.hpp, scan_and_finish: >= 64 flagged and more than an eighth of the call)
        self.q_arm = np.ascontiguousarray(np.stack([self.g * F32(2.0 ** (j % 6 - 2)) for j in range(80)]))

    def block(self, name):
        return {"A": self.A, "R": self.R, "B": self.B, "X": self.extra, "A2": self.A2}[name]


_CACHE = {}


def cached(key, make):
    """Cases and references are built once per process, shared by the tests, and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def family(d):
    return cached(("family", d), lambda: Family(d))


# ------------------------------------------------------------------ references
def all_dots(q, x):
    """float64 canonical dot of every (query, row) pair."""
    n = x.shape[0]
    if n == 0:
        return np.zeros((q.shape[0], 0))
    return orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1)))


class Reference:
    """The canonical values of `q` (as the index stores queries) against `rows` (as it stores rows); every expectation of a
    step is taken from a PREFIX-free copy: build one per row set (cached by the callers under the row set's name)."""

    def __init__(self, q, rows):
        self.q, self.rows = np.ascontiguousarray(q, F32), np.ascontiguousarray(rows, F32)
        self.n = rows.shape[0]
        self.dot = all_dots(self.q, self.rows)
        self.qq = orc.sumsq_canonical(self.q)
        self.local_phi = float(orc.sumsq_canonical(self.rows).max()) if self.n else 0.0

    def values(self, metric, phi=None):
        """float32 [nq, n]: the inner product, or |q|^2 + phi - 2 q.x (metric 1; phi None: the maximum over the rows)."""
        if metric == 1:
            phi = self.local_phi if phi is None else float(phi)
            return (self.qq[:, None] + phi - 2.0 * self.dot).astype(F32)
        return self.dot.astype(F32)

    def ranking(self, metric, phi=None):
        vals = self.values(metric, phi)
        ids = np.tile(np.arange(self.n, dtype=np.int64), (vals.shape[0], 1))
        order = orc._order_desc(-vals if metric == 1 else vals, ids)
        return np.take_along_axis(vals, order, axis=1), order.astype(np.int64)

    def topk(self, k, metric, phi=None, admit=None):
        """(scores, ids) [nq, k] of the k best (admitted) rows, padded with -1 / -+inf."""
        fs, fi = self.ranking(metric, phi)
        nq = fs.shape[0]
        s = np.full((nq, k), np.inf if metric == 1 else -np.inf, F32)
        i = np.full((nq, k), -1, np.int64)
        for j in range(nq):
            keep = np.arange(self.n)[:k] if admit is None else np.flatnonzero(admit[j][fi[j]])[:k]
            s[j, :len(keep)] = fs[j, keep]
            i[j, :len(keep)] = fi[j, keep]
        return s, i

    def range(self, radii, metric, phi=None, admit=None):
        """(lims, D, I) of the strict float32 rule: value > radius (inner product), value < radius (L2); rows ascending."""
        vals = self.values(metric, phi)
        lims, D, I = [0], [np.zeros(0, F32)], [np.zeros(0, np.int64)]
        for j in range(vals.shape[0]):
            hit = vals[j] < radii[j] if metric == 1 else vals[j] > radii[j]
            if admit is not None:
                hit &= admit[j]
            ids = np.flatnonzero(hit)
            lims.append(lims[-1] + len(ids))
            D.append(vals[j][ids])
            I.append(ids)
        return np.asarray(lims, np.int64), np.concatenate(D).astype(F32), np.concatenate(I).astype(np.int64)


def boundary_radii(vals, metric):
    """The radii of tests/test_gpu_range.py: a third of the queries the exact float32 score of one of their own rows (it and its
    ties are out), a third the nextafter of such a score towards the permissive side, the rest from nothing to everything,
    +-inf included."""
    nq, n = vals.shape
    permissive = F32(np.inf if metric == 1 else -np.inf)
    r = np.empty(nq, F32)
    for j in range(nq):
        best = np.sort(vals[j]) if metric == 1 else np.sort(vals[j])[::-1]
        own = best[(7 * j) % min(n, 60)]
        if j % 3 == 0:
            r[j] = own
        elif j % 3 == 1:
            r[j] = np.nextafter(own, permissive)
        else:
            r[j] = [best[0], best[min(n - 1, 50)], np.nextafter(best[-1], permissive), -permissive, permissive][(j // 3) % 5]
    return r


RADIUS_LEVEL = LEVEL_T - 129.5  # planted radii sit here: the planted rows and the decoys above it are members


def planted_dot_radius(fam, j, which):
    """The radius of planted query j in the DOT domain: between every planted row's scan score and its exact score."""
    s = fam.scale[j]
    if which == "R":
        return s * (fam.base_r + RADIUS_LEVEL * fam.unit_r)
    return s * (fam.base_b + RADIUS_LEVEL * fam.unit_b)


def radii_for(fam, ref, metric, phi, have_r, have_b):
    """float32 radii of one step: the boundary radii, and for the planted queries whose family is in the index the planted
    radius (L2: its image |q|^2 + phi - 2 r, rounded to float32)."""
    vals = ref.values(metric, phi)
    r = boundary_radii(vals, metric)
    phi = ref.local_phi if phi is None else float(phi)
    for which, have, qs in (("R", have_r, fam.r_queries), ("B", have_b, fam.b_queries)):
        if not have:
            continue
        for j in qs:
            if j >= len(r):
                continue
            t = planted_dot_radius(fam, j, which)
            r[j] = F32(ref.qq[j] + phi - 2.0 * t) if metric == 1 else F32(t)
    return r


# ------------------------------------------------------------------ the filters of the filtered / grouped searches
def row_mask(n):
    """The selector of the lifecycle tests: two rows of three, a pattern that cuts through every block."""
    return np.arange(n) % 3 != 0


def row_labels(n):
    return (np.arange(n) % 7).astype(np.int64)


def query_labels(nq):
    """Labels 0 .. 6, one absent label and LABEL_NONE (-1 << 31, retrieval_augmented_mds_amd.LABEL_NONE; checked by the GPU test)."""
    cyc = [0, 1, 2, 3, 4, 5, 6, 1 << 20, -(1 << 31)]
    return np.array([cyc[j % len(cyc)] for j in range(nq)], np.int64)


def admit_groups(labels, qlabels, mode="exclude", none=-(1 << 31)):
    eq = np.asarray(labels)[None, :] == np.asarray(qlabels)[:, None]
    return np.where((np.asarray(qlabels) == none)[:, None], True, eq if mode == "only" else ~eq)


# ------------------------------------------------------------------ the host's cached scalars and the bounds built on them
def scalars(rows_f32):
    """(xmax2, dres2) of the rows an fp32-exact index holds: max |x|^2 (ensure_xmax2, csrc/host_state.hpp) and
    max |x - bf16 x|^2 (ensure_hi), in float64."""
    x = np.asarray(rows_f32, F32).astype(F64)
    if x.shape[0] == 0:
        return 0.0, 0.0
    res = x - synth.round_to_bf16(np.asarray(rows_f32, F32)).astype(F64)
    return float((x * x).sum(1).max()), float((res * res).sum(1).max())


def err_c(d, f32x):
    """The constant in front of |q| max|x|: d 2^-23, x 1.01 where the scan multiplied bf16(q) . bf16(x) of an fp32-exact index.
    csrc/host_range.hpp:71 (range threshold), csrc/host_wide.hpp:163 (wide certificate), csrc/host_search.hpp:107 (the one-launch
    kernel) and :239 (the exact pass), and csrc/host_launch.hpp:371-374 for the scan launches of search(): STAGE 1 of the
    two-stage search views the index as the bf16 index rows_hi (scan_and_finish sets plane = 0 for the launch, so f32x of
    launch_search is false there and fast_f32 multiplies d 2^-23 by 1.01) -- the same number.  The other branch of that line is
    err_c_three_segment below."""
    return d * 1.1920928955078125e-07 * (1.01 if f32x else 1.0)


def err_c_three_segment(d):
    """csrc/host_launch.hpp:371, f32x: the one-stage scan of the fp32-exact index over the [hi | lo] planes (three segments, the
    lo . lo term dropped).  That launch sets neither dres2 nor qerr2 (:373-377 belong to fast_f32 alone): its e is
    err_c |q| max|x| and nothing else, so a stale dres2 cannot reach it, and a stale xmax2 shrinks it like any other e."""
    return 3.0 * d * 1.1920928955078125e-07 + 1.52587890625e-05


def bound_e(d, qq, xmax2, dres2=None, qerr2=None):
    """e of rank_flag_write (csrc/aux_kernels.hpp:604-608; merge_select_kernel supplies the bound it is added to),
    wide_rescore_kernel (csrc/scan_kernel_wide.hpp:505-510) and range_tau_kernel (csrc/range_kernels.hpp:79-84):
    e = err_c |q| max|x|, and where the scan saw bf16(x) . bf16(q) of an fp32-exact index (qerr2 given)
    + d_res |q| + (max|x| + d_res) |q - bf16 q|."""
    f32x = qerr2 is not None
    qn, xm = np.sqrt(qq), math.sqrt(xmax2)
    e = err_c(d, f32x) * qn * xm
    if f32x:
        dr = math.sqrt(dres2)
        e = e + dr * qn + (xm + dr) * np.sqrt(qerr2)
    return e


def range_tau(radius, qq, phi, l2, e):
    """range_tau_kernel (csrc/range_kernels.hpp:69-89): the scan's threshold, float32, rounded down."""
    rf = F32(radius)
    if np.isinf(rf):
        return F32(-np.inf) if (rf > 0) == bool(l2) else F32(np.inf)
    r = float(rf)
    c = qq + phi
    image = 0.5 * (c - r) if l2 else r
    slack = 1.1920928955078125e-07 * (abs(c) + abs(r) if l2 else abs(r))
    t = image - slack - e * 1.000000001 - 1e-300
    tau = F32(t)
    if float(tau) > t:
        tau = np.nextafter(tau, F32(-np.inf))
    return tau


def wide_certified(B, e, outk, qq, phi, l2):
    """The certificate of wide_rescore_kernel (csrc/scan_kernel_wide.hpp:504-514): B the pool's worst approximate score, outk the
    k-th float32 result.  True: nothing outside the pool can enter."""
    ub = B + e * 1.000000001 + 1e-300
    if l2:
        return bool(F32(qq + phi - 2.0 * ub) > outk)
    return bool(F32(ub) < outk)


def search_certified(bnd, e, tk, qq=0.0, phi=0.0, l2=False):
    """The margin check of rank_flag_write (csrc/aux_kernels.hpp:609, margin_key_worse :538-544): bnd bounds the scan score of every row
    outside the pool, tk is the exact dot of the k-th result.  True: not flagged -- the float32 key of a row with inner product
    bnd + e is STRICTLY worse than the k-th result's (rows whose dots differ can share a float32 key; the row number then ranks
    them, so a tie must not be certified)."""
    ub = float(F32(bnd)) + e
    if l2:
        return bool(F32(qq + phi - 2.0 * ub) > F32(qq + phi - 2.0 * tk))
    return bool(F32(ub) < F32(tk))


def wide_pool(k, f32x):
    """k' of wide_search (csrc/host_wide.hpp:17 and :100)."""
    return min(2048, k + (256 + k // 4 if f32x else 64))


def scan_scores(q_f32, rows_f32):
    """What stage 1 of an fp32-exact index multiplies: bf16(q) . bf16(x), here in float64 (exact for the planted pairs: see the
    module docstring).  [nq, n]"""
    return synth.round_to_bf16(q_f32).astype(F64) @ synth.round_to_bf16(rows_f32).astype(F64).T


def query_err2(q_f32):
    """|q - bf16 q|^2 per query (query_resid_kernel)."""
    r = np.asarray(q_f32, F32).astype(F64) - synth.round_to_bf16(q_f32).astype(F64)
    return (r * r).sum(1)


# ------------------------------------------------------------------ the sequences (what the GPU test replays step by step)
# A step is a list of adds, each (block name, lo, hi) -- rows lo .. hi of that block -- after which the index is searched.
# Sequence 1: everything reserved; no search step leaves ntotal on a multiple of 128, the first add ends on one.
SEQ_PLAIN = [[("A", 0, 1024), ("A", 1024, N_A)],
             [("R", 0, NPLANT + NDECOY)],
             [("B", 0, 100), ("B", 100, NPLANT + NDECOY)],
             [("X", 0, 1)]]
# Sequence 2: reserve(1000) -> capacity 1024.  Growth 1 happens in the second add (no hi row converted yet, hi_rows = 0 < ntotal
# = 900); the first search converts all 1037.  R fits (capacity 1536) and is not searched, so growth 2 (inside the add of B)
# copies hi_rows = 1037 < ntotal = 1405 converted rows; growth 3 (the rest of A) finds hi_rows == ntotal.
SEQ_GROWTH_RESERVE = 1000
SEQ_GROWTH = [[("A", 0, 900), ("A", 900, 1037)],
              [("R", 0, NPLANT + NDECOY), ("B", 0, NPLANT + NDECOY)],
              [("A", 1037, N_A)]]
# Sequence 4: the first life of the index.  Rows 1037 .. 1404 are block B: after reset() and 1037 new rows, what lies behind
# ntotal in the last 128-row tile (rows 1037 .. 1151) are big rows, 10^3 times the norm of the new ones.
SEQ_RESET_FIRST = [("A", 0, 1037), ("B", 0, NPLANT + NDECOY), ("A", 1037, N_A), ("R", 0, NPLANT + NDECOY)]
SEQ_RESET_SECOND = [("A2", 0, 1000), ("A2", 1000, 1037)]
SYNTH_ROWS, SYNTH_ROW0, SYNTH_SEED = 500, 7, 11


def rows_of(fam, adds):
    return np.ascontiguousarray(np.concatenate([fam.block(b)[lo:hi] for b, lo, hi in adds])) if adds else np.zeros((0, fam.d), F32)


def block_offset(adds, name):
    """Row number at which block `name` starts (it is added in one piece or in consecutive pieces)."""
    at = 0
    for b, lo, hi in adds:
        if b == name:
            assert lo == 0
            return at
        at += hi - lo
    raise KeyError(name)


def has_block(adds, name):
    """Is the WHOLE block `name` among the adds?"""
    got = sorted((lo, hi) for b, lo, hi in adds if b == name)
    at = 0
    for lo, hi in got:
        if lo != at:
            return False
        at = hi
    return at == NPLANT + NDECOY
