"""Inputs, float64 references and derived error bounds of tests/test_hook_cases_host.py and tests/test_gpu_hook_kernels.py: the
kernels of the retriever scoring hook and of the facade (csrc/aux_kernels.hpp: cosine re-score forward and backward, row
normalisation, maximum row norm, ignore filter, storage rounding).  Not a test file; NumPy only, no GPU is needed to import it.

What is here, per kernel:
  inputs      deterministic builders.  Rows are SPIKED: a Gaussian row hides a dropped or an extra element (the cosine moves by
              about 1e-9), so every probed column P(d) carries, in at least one pair / row, an element 4 times the norm of the
              rest of the row, and every row carries one at column 0 (what a read one element past a row picks up).
  reference   plain float64 NumPy of the operation, from the exact input values.
  bound       derived from the number of float32 roundings of the kernel's summation order (u = 2^-24, m(x) = ceil(x / 64)); the
              derivations stand next to the functions.  Nothing here is tuned against what a kernel returns.
  compare_*   the comparison the GPU test applies to the kernel's output: EVERY element, non-finite reference values demand
              a non-finite result, everything else obeys the bound.  They return the worst error / bound ratio and raise
              AssertionError otherwise.
  model_*     NumPy models of the kernels' summation order (lane-strided partial sums, xor tree, sequential j) with deliberately
              wrong variants; the host test shows that compare_* accepts the model and rejects every variant."""
import math

import numpy as np

from oracle import mips_oracle as orc

U = 2.0 ** -24
F32 = np.float32
F64 = np.float64

SEED = 20240701


def m(x):
    """ceil(x / 64): the number of elements a lane of a 64-wide wave sums sequentially."""
    return -(-int(x) // 64)


# ------------------------------------------------------------------ bf16, written independently of oracle/synth.py
def bf16_round_bits(x):
    """float32 array -> uint16 bf16 bit patterns: the NEAREST bf16 value by exact comparison in float64, ties to the even
    mantissa.  The two neighbours are the truncated pattern and the next one in magnitude (0x7f80, the pattern of infinity, stands
    for 2^128: what IEEE rounding measures the overflow against).  NaN -> 0x7fc0 with the input's sign; infinities stay."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    sign = ((u >> np.uint32(16)) & np.uint32(0x8000)).astype(np.uint16)
    a = u & np.uint32(0x7FFFFFFF)
    lo = (a >> np.uint32(16)).astype(np.uint32)
    hi = lo + np.uint32(1)

    def value(p):
        with np.errstate(invalid="ignore"):
            v = (np.minimum(p, np.uint32(0x7F7F)) << np.uint32(16)).view(F32).astype(F64)
        return np.where(p >= 0x7F80, 2.0 ** 128, v)

    av = np.where(a >= np.uint32(0x7F800000), 2.0 ** 128, (np.minimum(a, np.uint32(0x7F7FFFFF))).view(F32).astype(F64))
    down, up = av - value(lo), value(hi) - av
    take_hi = (up < down) | ((up == down) & ((lo & np.uint32(1)) == 1))
    out = np.where(take_hi, hi, lo).astype(np.uint16)
    out = np.where(a >= np.uint32(0x7F800000), np.uint16(0x7F80), out)        # infinities stay
    out = np.where(a > np.uint32(0x7F800000), np.uint16(0x7FC0), out)         # NaN
    return (out | sign).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def to_bf16(x):
    """float32 values rounded to bf16, as float32."""
    return bf16_to_f32(bf16_round_bits(x))


def model_bf16_bits(x, half_up=False):
    """The kernel's integer rounding (f32_to_bf16_rne); half_up: ties away from zero instead of to the even mantissa."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    add = np.uint32(0x8000) if half_up else np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    r = ((u.astype(np.uint64) + add) >> np.uint64(16)).astype(np.uint16)
    return np.where(nan, (np.uint16(0x7FC0) | ((u >> np.uint32(16)) & np.uint32(0x8000)).astype(np.uint16)), r).astype(np.uint16)


# ------------------------------------------------------------------ e4m3, a table search
def e4m3_table():
    """The 127 non-negative finite e4m3 values decoded in float64 (code c: exponent c >> 3, mantissa c & 7; exponent 0 is
    subnormal, m 2^-9; otherwise (1 + m / 8) 2^(e - 7)), ascending, code = position."""
    tab = np.empty(127, dtype=F64)
    for c in range(127):
        e, mm = c >> 3, c & 7
        tab[c] = mm * 2.0 ** -9 if e == 0 else (1.0 + mm / 8.0) * 2.0 ** (e - 7)
    assert (np.diff(tab) > 0).all() and tab[-1] == 448.0
    return tab


def e4m3_nearest_bits(x):
    """float32 array -> uint8 e4m3 codes: nearest of the 127 finite values to min(|x|, 448), ties to the even code; the sign
    bit is the input's; +-inf -> +-448; NaN -> 0x7f with the input's sign."""
    f = np.ascontiguousarray(x, dtype=F32)
    u = f.view(np.uint32)
    sign = ((u >> np.uint32(24)) & np.uint32(0x80)).astype(np.uint8)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    tab = e4m3_table()
    with np.errstate(invalid="ignore"):
        a = np.minimum(np.abs(f.astype(F64)), 448.0)
    a = np.where(nan, 0.0, a)
    hi = np.clip(np.searchsorted(tab, a, side="left"), 0, 126)
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = np.abs(a - tab[lo]), np.abs(tab[hi] - a)
    code = np.where(dhi < dlo, hi, lo)
    code = np.where(dhi == dlo, np.where(hi % 2 == 0, hi, lo), code)
    code = np.where(nan, 0x7F, code)
    return (sign | code.astype(np.uint8)).astype(np.uint8)


def model_e4m3_bits(x, half_up=False, saturate=True):
    """The kernel's integer algorithm (f32_to_e4m3), with two wrong variants: ties rounded up, and no saturation (values from
    464 on run into the NaN code and beyond)."""
    f = np.ascontiguousarray(x, dtype=F32)
    u = f.view(np.uint32)
    sign = ((u >> np.uint32(24)) & np.uint32(0x80)).astype(np.int64)
    a = (u & np.uint32(0x7FFFFFFF)).astype(np.int64)
    e = (a >> 23) - 127
    m3 = (a >> 20) & 7
    rem = a & 0xFFFFF
    up = (rem >= 0x80000) if half_up else ((rem > 0x80000) | ((rem == 0x80000) & ((m3 & 1) == 1)))
    m3 = m3 + up
    ee = e + 7 + (m3 == 8)
    m3 = np.where(m3 == 8, 0, m3)
    normal = (ee << 3) | m3
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.abs(f) * F32(512.0)
        sub = np.floor(s.astype(F64) + 0.5) if half_up else np.rint(s)
        sub = np.where(np.isfinite(sub), sub, 0).astype(np.int64)
    code = np.where(e < -6, sub, normal)
    if saturate:
        code = np.where(a >= 0x43E00000, 0x7E, code)
    else:
        code = np.where(a >= 0x7F800000, 0x7E, code) & 0x7F
    code = np.where(a > 0x7F800000, 0x7F, code)
    return (sign | code).astype(np.uint8)


def rounding_inputs_bf16():
    """float32 [512, 768]: every 16-bit upper half x the lower halves that decide a rounding."""
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    u = (np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)) | lows[None, :]
    return np.ascontiguousarray(u.reshape(512, 768)).view(F32)


def rounding_inputs_e4m3_from_bf16():
    """uint16 [86, 768]: all 65536 bf16 patterns (the last row is filled up with +0)."""
    b = np.zeros(86 * 768, dtype=np.uint16)
    b[:65536] = np.arange(65536, dtype=np.uint16)
    return b.reshape(86, 768)


def rounding_inputs_e4m3_from_f32():
    """float32 [256, 768]: every upper half x lower halves {0x0000, 0x0001, 0xFFFF}."""
    lows = np.array([0x0000, 0x0001, 0xFFFF], dtype=np.uint32)
    u = (np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)) | lows[None, :]
    return np.ascontiguousarray(u.reshape(256, 768)).view(F32)


def compare_codes(got, want, nan_mask, nan_low, sign_bit):
    """Stored codes against the reference: bit-exact, except that a NaN input need only come back as a NaN (all bits of
    nan_low set in the magnitude: 0x7f80 and a non-zero mantissa for bf16, 0x7f for e4m3) of the same sign."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    plain = ~nan_mask
    bad = np.flatnonzero((got != want).ravel() & plain.ravel())
    assert bad.size == 0, f"{bad.size} stored codes differ, first at {bad[:5]}: got {got.ravel()[bad[:5]]}, want {want.ravel()[bad[:5]]}"
    g, w = got[nan_mask].astype(np.int64), want[nan_mask].astype(np.int64)
    assert ((g & sign_bit) == (w & sign_bit)).all(), "a NaN changed its sign"
    if nan_low == 0x7F:
        assert ((g & 0x7F) == 0x7F).all(), "a NaN input is stored as a number"
    else:
        assert (((g & 0x7F80) == 0x7F80) & ((g & 0x007F) != 0)).all(), "a NaN input is stored as a number"


# ------------------------------------------------------------------ spiked rows
def probed_columns(d):
    """P(d): the columns at which a 64-lane stride, its first and last pass and the row end can go wrong."""
    cand = [0, 1, 62, 63, 64, 65, 127, 128, d - 65, d - 64, d - 2, d - 1, 64 * ((d - 1) // 64)]
    return sorted({c for c in cand if 0 <= c < d})


def _spike(rows, cols_per_row, rng):
    """rows [n, d] float64 Gaussian; cols_per_row[i] = columns of row i that get a spike of 4 |rest of the row| (random sign;
    1 stands in for the norm of an empty rest)."""
    n, d = rows.shape
    for i in range(n):
        cols = sorted(cols_per_row[i])
        if not cols:
            continue
        rest = rows[i].copy()
        rest[cols] = 0.0
        r = math.sqrt(float(rest @ rest)) or 1.0
        rows[i, cols] = 4.0 * r * rng.choice([-1.0, 1.0], size=len(cols))
    return rows


def spiked_matrix(n, d, rng):
    """[n, d] float64: column i-th of P(d) is spiked in row i % n, and column 0 in every row."""
    cols = [{0} for _ in range(n)]
    for i, p in enumerate(probed_columns(d)):
        cols[i % n].add(p)
    return _spike(rng.standard_normal((n, d)), cols, rng), cols


FORWARD_SHAPES = [(1, 1, 1, 0), (1, 1, 1, 1), (3, 1, 63, 63), (1, 3, 64, 64), (2, 5, 65, 65), (5, 29, 100, 37), (2, 64, 769, 131),
                  (1, 65, 128, 2), (1, 1024, 96, 1), (3, 7, 4099, 64), (17, 5, 1024, 16)]
BACKWARD_SHAPES = [s for s in FORWARD_SHAPES if s[1] <= 64] + [(2, 63, 70, 3), (2, 4, 256, 65)]
BACKWARD_MODES = ("scores", "bias", "both")
DTYPES = ("f32", "bf16")
# the two zero-norm rows: (shape, what, index) -- neither is a row that alone carries a probed column (pairs 0 .. 12 do)
ZERO_CLS = ((5, 29, 100, 37), (2, 7))
ZERO_QUERY = ((17, 5, 1024, 16), 11)


class CosineCase:
    """q [b, d], c [b, k, d] as float32 holding the exact input values (bf16 cases: values of bf16), spike map, upstream
    gradients gs [b, k] (Gaussian) and gb [b, k, L] (from {+-1, +-2}), and the float64 references."""

    def __init__(self, shape, dtype):
        b, k, d, L = shape
        self.shape, self.dtype = shape, dtype
        self.b, self.k, self.d, self.L = b, k, d, L
        rng = np.random.default_rng([SEED, b, k, d, L, DTYPES.index(dtype)])
        pairs = b * k
        ccols = [{0} for _ in range(pairs)]
        qcols = [{0} for _ in range(b)]
        self.carrier = {}                                    # probed column -> pair that carries it on both sides
        for i, p in enumerate(probed_columns(d)):
            pr = i % pairs
            ccols[pr].add(p)
            qcols[pr // k].add(p)
            self.carrier[p] = pr
        q = _spike(rng.standard_normal((b, d)), qcols, rng)
        c = _spike(rng.standard_normal((pairs, d)), ccols, rng).reshape(b, k, d)
        if shape == ZERO_CLS[0]:
            c[ZERO_CLS[1]] = 0.0
        if shape == ZERO_QUERY[0]:
            q[ZERO_QUERY[1]] = 0.0
        q, c = q.astype(F32), c.astype(F32)
        if dtype == "bf16":
            q, c = to_bf16(q), to_bf16(c)
        self.q, self.c = np.ascontiguousarray(q), np.ascontiguousarray(c)
        self.gs = rng.standard_normal((b, k)).astype(F32)
        self.gb = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=F32), size=(b, k, L)).astype(F32)

    # ---- forward
    def scores_ref(self, q=None, c=None):
        return cosine_ref(self.q if q is None else q, self.c if c is None else c)

    def bias_ref_bits(self, score_bits):
        """memory_bias [b, k L] as bit patterns from the kernel's own scores: score (b, j) at [b][j L + t]."""
        return np.repeat(np.asarray(score_bits).reshape(self.b, self.k, 1), self.L, axis=2).reshape(self.b, self.k * self.L)

    # ---- backward
    def grads(self, mode):
        """(gs or None, gb or None, L) of a backward mode."""
        if mode == "scores":
            return self.gs, None, 0
        if mode == "bias":
            return None, self.gb, self.L
        return self.gs, self.gb, self.L

    def backward_ref(self, mode):
        gs, gb, L = self.grads(mode)
        return backward_ref(self.q, self.c, gs, gb if L > 0 else None)


def tol_f(d):
    """Absolute bound of one cosine.  Each of the three sums is 64 lane-strided partial sums -- at most m(d) roundings each,
    product included (a fused multiply-add only removes one) -- and 6 shuffle additions: relative error (m(d) + 6) u, for the
    numerator relative to sum |a b| <= |q| |c|, i.e. (m + 6) u of the cosine's scale 1.  The two norms' errors are halved by the
    square roots and there are two of them: another (m + 6) u.  Two roots, their product and the division: <= 5 u with the
    final rounding.  Total (2 (m(d) + 6) + 5) u, and 1 % for the second-order terms."""
    return 1.01 * (2 * (m(d) + 6) + 5) * U


def cosine_ref(q, c):
    """float64 [b, k] = q_b . c_bj / (|q_b| |c_bj|) from float32 (or bf16-valued float32) inputs."""
    q6, c6 = np.asarray(q, dtype=F64), np.asarray(c, dtype=F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        num = np.einsum("bd,bkd->bk", q6, c6)
        return num / (np.sqrt((q6 * q6).sum(1))[:, None] * np.sqrt((c6 * c6).sum(2)))


def _ratio(err, bound, ref, got, what):
    """Shared rule of every numeric comparison.  Where ref is non-finite got must be non-finite; everywhere else err <= bound.
    -> worst err / bound over the finite part (0 where the bound and the error are both 0)."""
    ref, got = np.asarray(ref), np.asarray(got)
    assert got.shape == ref.shape, f"{what}: shape {got.shape}, expected {ref.shape}"
    fin = np.isfinite(ref)
    wrong = np.flatnonzero((~fin & np.isfinite(got)).ravel())
    assert wrong.size == 0, f"{what}: {wrong.size} finite values where the reference is non-finite, first at {wrong[:5]}"
    err, bound = np.broadcast_to(err, ref.shape)[fin], np.broadcast_to(bound, ref.shape)[fin]
    ok = err <= bound                                            # (NaN and inf in got fail here)
    if not ok.all():
        at = np.flatnonzero(~ok)
        w = at[np.argmax(np.nan_to_num(err[at] / np.maximum(bound[at], 1e-300), nan=np.inf))]
        raise AssertionError(f"{what}: {at.size} of {ok.size} elements outside the bound; worst |err| = {err[w]:.4g} against "
                             f"{bound[w]:.4g} at finite element {w} (got {got[fin][w]!r}, reference {ref[fin][w]!r})")
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def compare_scores(case, got):
    """float32 scores [b, k] of the kernel against the float64 reference; -> worst error / bound."""
    ref = case.scores_ref()
    got = np.asarray(got)
    assert got.dtype == F32
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(F64) - ref)
    return _ratio(err, tol_f(case.d), ref, got, f"cosine scores {case.shape} {case.dtype}")


def eps_w(d, L):
    """Relative error of w = g / (|q| |c|) against G = (|gs| + sum |gb|) / (|q| |c|): the g sum (m(L) + 6 roundings of the lane
    sums and the tree, one for adding gs), the two norm sums halved by their roots ((m(d) + 6) u together), and the roots, their
    product and the division (5 u)."""
    return (m(L) + 7 + m(d) + 6 + 5) * U


def backward_ref(q, c, gs, gb):
    """float64 (gq [b, d], gc [b, k, d], G [b, k]) with the norms held constant."""
    q6, c6 = np.asarray(q, dtype=F64), np.asarray(c, dtype=F64)
    b, k, d = c6.shape
    g = np.zeros((b, k)) if gs is None else np.asarray(gs, dtype=F64).copy()
    ga = np.abs(g)
    if gb is not None:
        gb6 = np.asarray(gb, dtype=F64).reshape(b, k, -1)
        g = g + gb6.sum(2)
        ga = ga + np.abs(gb6).sum(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.sqrt((q6 * q6).sum(1))[:, None] * np.sqrt((c6 * c6).sum(2))
        w, G = g / nn, ga / nn
        gq = np.zeros((b, d))
        for j in range(k):                                       # (not einsum: inf * 0 must come out as NaN, not be skipped)
            gq = gq + w[:, j, None] * c6[:, j, :]
        gc = w[:, :, None] * q6[:, None, :]
    return gq, gc, G


def backward_bounds(case, mode, G, cast_slack=0.0, ref=None):
    """Elementwise bounds (bq [b, d], bc [b, k, d]).  gc_jt = w_j q_t: the error of w and one product.  gq_t = sum_j w_j c_jt
    summed sequentially in j: the error of w, one product and at most k additions per term.  cast_slack (2^-8 when the gradient is
    cast to bf16) is relative to the reference value."""
    _, _, L = case.grads(mode)
    ew = eps_w(case.d, L)
    q6, c6 = case.q.astype(F64), case.c.astype(F64)
    with np.errstate(invalid="ignore"):
        bc = 1.01 * (ew + U) * G[:, :, None] * np.abs(q6)[:, None, :]
        bq = 1.01 * ((ew + (case.k + 1) * U) * G[:, :, None] * np.abs(c6)).sum(1)
        if cast_slack:
            bq = bq + cast_slack * np.abs(ref[0])
            bc = bc + cast_slack * np.abs(ref[1])
    return bq, bc


def compare_backward(case, mode, got_gq, got_gc, cast_slack=0.0):
    """-> (worst ratio of grad_query, worst ratio of grad_cls); a gradient passed as None is not compared (ratio 0)."""
    gq, gc, G = case.backward_ref(mode)
    bq, bc = backward_bounds(case, mode, G, cast_slack, (gq, gc))
    what = f"cosine backward {case.shape} {case.dtype} {mode}"
    out = []
    # a bound that is itself non-finite (a zero-norm row in the same batch row) bounds nothing: the reference is non-finite
    # there as well, which _ratio demands of the result
    for got, ref, bound, name in ((got_gq, gq, bq, " grad_query"), (got_gc, gc, bc, " grad_cls")):
        if got is None:
            out.append(0.0)
            continue
        with np.errstate(invalid="ignore"):
            err = np.abs(np.asarray(got, dtype=F64) - ref)
        out.append(_ratio(err, np.nan_to_num(bound, nan=0.0, posinf=0.0), ref, got, what + name))
    return tuple(out)


# ------------------------------------------------------------------ models of the kernels' summation order
def wave_sum(p, dtype=F32):
    """p [rows, n] -> [rows]: lane l sums p[l], p[l + 64], ... sequentially, then the xor tree 32, 16, ... 1 (lane 0)."""
    p = np.asarray(p, dtype=dtype)
    rows, n = p.shape
    lanes = np.zeros((rows, 64), dtype=dtype)
    for t in range(0, n, 64):
        seg = p[:, t:t + 64]
        lanes[:, :seg.shape[1]] = (lanes[:, :seg.shape[1]] + seg).astype(dtype)
    off = 32
    while off:                       # lane l < off adds lane l ^ off = l + off; the later steps read lanes below off only
        lanes = (lanes[:, :off] + lanes[:, off:2 * off]).astype(dtype)
        off >>= 1
    return lanes[:, 0]


VARIANTS_COLUMNS = ("drop_last", "drop_stride_col", "extra")


def _columns(flat, d, variant):
    """flat [rows * d (+ guard)] -> [rows, d'] as a wrong kernel would read row r: without its last column, without column
    64 floor((d - 1) / 64) (lane 0's last pass), or with the element behind it (the next row's first; NaN behind the last)."""
    flat = np.asarray(flat, dtype=F32).ravel()
    rows = flat.size // d
    x = flat[:rows * d].reshape(rows, d)
    if variant == "drop_last":
        return x[:, :d - 1]
    if variant == "drop_stride_col":
        keep = np.ones(d, dtype=bool)
        keep[64 * ((d - 1) // 64)] = False
        return x[:, keep]
    if variant == "extra":
        nxt = np.append(flat[d::d][:rows - 1], F32(np.nan)) if rows > 0 else np.zeros(0, F32)
        return np.concatenate([x, nxt[:, None].astype(F32)], axis=1)
    return x


def model_scores(case, variant=None):
    """The forward kernel in NumPy float32 (products rounded, then summed: one rounding more per term than a fused
    multiply-add).  variant: one of VARIANTS_COLUMNS, or "wrong_norm" (|c| of the previous pair)."""
    b, k, d = case.b, case.k, case.d
    q = _columns(case.q, d, variant)
    c = _columns(case.c, d, variant)
    qr = np.repeat(q, k, axis=0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qc = wave_sum((qr * c).astype(F32))
        qq = wave_sum((qr * qr).astype(F32))
        cc = wave_sum((c * c).astype(F32))
        if variant == "wrong_norm":
            cc = np.roll(cc, 1)
        return (qc / (np.sqrt(qq) * np.sqrt(cc)).astype(F32)).astype(F32).reshape(b, k)


def model_backward(case, mode, variant=None):
    """The backward kernel in NumPy float32.  variant: VARIANTS_COLUMNS (in the norm sums and in the column loop), "skip_j_tail"
    (j >= 4 floor(k / 4) never computed: w stays 0), "mem_past_64" (gb terms t >= 64 dropped), "wrong_norm"."""
    b, k, d = case.b, case.k, case.d
    gs, gb, L = case.grads(mode)
    qn = _columns(case.q, d, variant if variant in VARIANTS_COLUMNS else None)
    cn = _columns(case.c, d, variant if variant in VARIANTS_COLUMNS else None)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qq = wave_sum((qn * qn).astype(F32))
        cc = wave_sum((cn * cn).astype(F32)).reshape(b, k)
        if variant == "wrong_norm":
            cc = np.roll(cc.ravel(), 1).reshape(b, k)
        g = np.zeros((b, k), dtype=F32)
        if gb is not None and L > 0:
            terms = gb.reshape(b * k, L)
            if variant == "mem_past_64":
                terms = terms[:, :64]
            g = wave_sum(terms).reshape(b, k)
        g = ((gs if gs is not None else F32(0)) + g).astype(F32)
        w = (g / (np.sqrt(qq)[:, None] * np.sqrt(cc)).astype(F32)).astype(F32)
        if variant == "skip_j_tail":
            w[:, 4 * (k // 4):] = 0
        gq = np.zeros((b, d), dtype=F32)
        gc = np.zeros((b, k, d), dtype=F32)
        cols = slice(0, d - 1) if variant == "drop_last" else slice(0, d)   # (a column loop that stops one short)
        for j in range(k):
            gq[:, cols] = (gq[:, cols] + (w[:, j, None] * case.c[:, j, cols]).astype(F32)).astype(F32)
            gc[:, j, cols] = (w[:, j, None] * case.q[:, cols]).astype(F32)
    return gq, gc


# ------------------------------------------------------------------ l2_normalize_
L2_N = (1, 3, 5, 513)
L2_D = (1, 63, 64, 65, 769)
L2_NORM_WINDOW = (1e-15, 1e15)
L2_ZERO_ROW, L2_UNDERFLOW_ROW, L2_OVERFLOW_ROW = 1, 2, 3          # in the cases with n >= 5


class L2Case:
    def __init__(self, n, d):
        self.n, self.d = n, d
        rng = np.random.default_rng([SEED, 3, n, d])
        x, self.cols = spiked_matrix(n, d, rng)
        scale = 10.0 ** ((np.arange(n) * 7) % 25 - 12.0)          # row norms spread over the window, every decade
        x = (x * scale[:, None]).astype(F32)
        self.edge = {}
        if n >= 5:
            x[L2_ZERO_ROW] = 0.0
            x[L2_ZERO_ROW, d // 2] = -0.0
            x[L2_UNDERFLOW_ROW] = (rng.uniform(1e-27, 9e-26, d) * rng.choice([-1.0, 1.0], d)).astype(F32)
            x[L2_OVERFLOW_ROW] = (rng.uniform(1e20, 2e20, d) * rng.choice([-1.0, 1.0], d)).astype(F32)
            big = x[L2_OVERFLOW_ROW:L2_OVERFLOW_ROW + 1].copy()
            with np.errstate(over="ignore"):
                big = orc.l2_normalization(big)
            self.edge = {L2_ZERO_ROW: x[L2_ZERO_ROW].copy(), L2_UNDERFLOW_ROW: x[L2_UNDERFLOW_ROW].copy(), L2_OVERFLOW_ROW: big[0]}
        self.x = np.ascontiguousarray(x)
        self.plain = np.array([i for i in range(n) if i not in self.edge], dtype=np.int64)

    def ref(self):
        x6 = self.x[self.plain].astype(F64)
        return x6 / np.sqrt((x6 * x6).sum(1))[:, None]


def tol_l2(d):
    """Relative bound of one normalised element: the sum of squares has relative error (m(d) + 6) u, halved by the root; the
    root, the reciprocal, the product and second-order terms: 4 u."""
    return 1.01 * ((m(d) + 6) / 2.0 + 4) * U


def compare_l2(case, got):
    """The [n, d] matrix after the call.  Edge rows bit for bit; the others elementwise relative.  -> worst ratio."""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == case.x.shape
    for r, want in case.edge.items():
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), f"l2_normalize ({case.n}, {case.d}): edge row {r} differs"
    ref = case.ref()
    g = got[case.plain]
    with np.errstate(invalid="ignore"):
        err = np.abs(g.astype(F64) - ref)
    return _ratio(err, tol_l2(case.d) * np.abs(ref), ref, g, f"l2_normalize ({case.n}, {case.d})")


def model_l2(case, variant=None):
    x = case.x.copy()
    cols = _columns(x, case.d, variant)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        nr = wave_sum((cols * cols).astype(F32))
        if variant == "wrong_norm":
            nr = np.roll(nr, 1)
        inv = (F32(1.0) / np.sqrt(nr)).astype(F32)
        out = np.where((nr > 0)[:, None], (x * inv[:, None]).astype(F32), x)
    return out.astype(F32)


# ------------------------------------------------------------------ rows_max_sumsq
MAX_N = (1, 3, 4, 5, 16383, 16384, 16385, 16384 * 2 + 5)
MAX_D = (1, 3, 65)
MAX_STRIDE = 16384                     # rows one pass of the kernel's grid covers (4096 workgroups of 4 rows)
MAX_GUARD = 1e30                       # what the rows before and after the window hold


def max_plants(n):
    """Rows at which the maximum is planted in turn: first, last, first of the second stride, last of the second stride."""
    return sorted({r for r in (0, n - 1, MAX_STRIDE, 2 * MAX_STRIDE - 1) if 0 <= r < n})


def max_matrix(n, d, plant=None, top=2.25, seed=0):
    """float32 [n, d] Gaussian; row `plant` is scaled so that its sum of squares is `top` times the largest of the others
    (plant None: no row stands out on purpose)."""
    rng = np.random.default_rng([SEED, 4, n, d, seed])
    x = rng.standard_normal((n, d)).astype(F32)
    if plant is not None:
        ss = (x.astype(F64) ** 2).sum(1)
        others = np.delete(ss, plant).max() if n > 1 else 1.0
        v = rng.standard_normal(d) + 0.5
        x[plant] = (v * math.sqrt(top * others / float(v @ v))).astype(F32)
    return x


def max_ref(x):
    """max_i |x_i|^2 in float64, correctly rounded: the products are exact in float64 and math.fsum adds them exactly; the row
    is the one NumPy's own sum ranks first or within 1e-9 of it."""
    x6 = np.asarray(x, dtype=F64)
    if x6.shape[0] == 0:
        return 0.0
    ss = (x6 * x6).sum(1)
    best = 0.0
    for r in np.flatnonzero(ss >= ss.max() * (1 - 1e-9)):
        best = max(best, math.fsum((x6[r] * x6[r]).tolist()))
    return best


def tol_max(d):
    """Relative: exact products, at most m(d) + 6 float64 additions."""
    return 1.01 * (m(d) + 6) * 2.0 ** -53


def compare_max(d, got, ref):
    got = float(got)
    assert math.isfinite(got), f"rows_max_sumsq: {got!r}"
    err, bound = abs(got - ref), tol_max(d) * abs(ref)
    assert err <= bound, f"rows_max_sumsq (d = {d}): {got!r} against {ref!r}, |err| = {err:.4g} > {bound:.4g}"
    return err / bound if bound > 0 else 0.0


def model_max(x, variant=None):
    """The kernel in float64: lane-strided sums, xor tree, maximum over rows.  Variants: "drop_last", "drop_stride_col", "extra"
    and "no_stride" (rows from MAX_STRIDE on never visited)."""
    x = np.asarray(x, dtype=F32)
    n, d = x.shape
    cols = _columns(x, d, variant).astype(F64)
    if variant == "extra":
        cols[-1, -1] = MAX_GUARD                                   # (behind the last row lies the guard)
    if variant == "no_stride":
        cols = cols[:MAX_STRIDE]
    return float(wave_sum(cols * cols, dtype=F64).max()) if cols.size else 0.0


# ------------------------------------------------------------------ filter_ignore
FILTER_NQ = (1, 255, 256, 257, 1000)
FILTER_K = ((2, 1), (6, 5), (11, 10), (30, 29), (30, 1), (5, 5))
ID_OFFSET = 1 << 33
PAD_SCORE_BITS = 0xFF800000            # -inf


class FilterCase:
    """scores (as uint32 bit patterns: they are only copied) and ids [nq, kf], ignore [nq], and the expected [nq, k] outputs:
    oracle.filter_ignore's lists, padded with id -1 / score -inf where the hits run out."""

    def __init__(self, nq, kf, k):
        self.nq, self.kf, self.k = nq, kf, k
        rng = np.random.default_rng([SEED, 5, nq, kf, k])
        ids = np.empty((nq, kf), dtype=np.int64)
        for j in range(nq):
            ids[j] = ID_OFFSET + rng.choice(100000, size=kf, replace=False)
        s = -np.sort(-rng.standard_normal((nq, kf)).astype(F32), axis=1)
        bits = s.view(np.uint32).copy()
        bits[::9, 0] = 0x7FC12345                                    # a NaN with a payload and a -0.0: copies, not arithmetic
        bits[4::9, kf - 1] = 0x80000000
        ignore = np.empty(nq, dtype=np.int64)
        self.dup = np.zeros(nq, dtype=bool)
        for j in range(nq):
            if j % 5 == 3:                                          # the row ends in padding
                npad = min(kf, 1 + j % 3)
                ids[j, kf - npad:] = -1
                bits[j, kf - npad:] = PAD_SCORE_BITS
            pos = j % (kf + 1)
            ignore[j] = ids[j, pos] if pos < kf else ID_OFFSET + 200000 + j        # (the last value: absent)
            if j % 11 == 7:
                ignore[j] = -1
            if j % 6 == 4 and pos < kf and kf > 1 and ignore[j] >= 0:               # the banned id twice
                ids[j, (pos + 1) % kf] = ignore[j]
                self.dup[j] = True
        self.ids, self.score_bits, self.ignore = ids, bits, ignore
        ks, ki = orc.filter_ignore(bits, ids, ignore, k)
        self.survivors = np.array([len(r) for r in ki], dtype=np.int64)
        self.want_i = np.full((nq, k), -1, dtype=np.int64)
        self.want_s = np.full((nq, k), PAD_SCORE_BITS, dtype=np.uint32)
        for j in range(nq):
            self.want_i[j, :len(ki[j])] = ki[j]
            self.want_s[j, :len(ks[j])] = ks[j]


def compare_filter(case, got_score_bits, got_ids):
    got_score_bits, got_ids = np.asarray(got_score_bits), np.asarray(got_ids)
    assert got_ids.dtype == np.int64 and got_score_bits.dtype == np.uint32
    assert got_ids.shape == case.want_i.shape and got_score_bits.shape == case.want_s.shape
    bad = np.flatnonzero((got_ids != case.want_i).any(1) | (got_score_bits != case.want_s).any(1))
    assert bad.size == 0, (f"filter_ignore (nq {case.nq}, k_fetched {case.kf}, k {case.k}): {bad.size} rows differ, first {bad[0]}: ids "
                           f"{got_ids[bad[0]]} / {case.want_i[bad[0]]}, {case.survivors[bad[0]]} survivors")


def model_filter(case, sentinel_i, sentinel_s, pad=True):
    """The kernel; pad False: the version that wrote only the survivors and left the rest of the buffer as it was."""
    out_i = np.full((case.nq, case.k), sentinel_i, dtype=np.int64)
    out_s = np.full((case.nq, case.k), sentinel_s, dtype=np.uint32)
    for j in range(case.nq):
        w = 0
        for t in range(case.kf):
            if w >= case.k:
                break
            if case.ids[j, t] != case.ignore[j]:
                out_i[j, w], out_s[j, w] = case.ids[j, t], case.score_bits[j, t]
                w += 1
        if pad:
            out_i[j, w:], out_s[j, w:] = -1, PAD_SCORE_BITS
    return out_s, out_i


_CACHE = {}


def cached(key, make):
    """Cases and references are built once per process, shared by the tests, and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cosine_case(shape, dtype):
    return cached(("cos", shape, dtype), lambda: CosineCase(shape, dtype))


def l2_case(n, d):
    return cached(("l2", n, d), lambda: L2Case(n, d))


def filter_case(nq, kf, k):
    return cached(("flt", nq, kf, k), lambda: FilterCase(nq, kf, k))
