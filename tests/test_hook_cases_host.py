"""CPU proof that tests/test_gpu_hook_kernels.py can fail: the cases of tests/hook_cases.py are as sharp as they claim, a NumPy
model of every kernel's summation order stays inside the derived bounds, and deliberately wrong variants of that model are
REJECTED by the very comparison functions the GPU test applies to the kernels' output.  No GPU.

Worst model error / bound ratios (printed by the tests; run with -s): cosine forward 0.24, backward grad_query 0.14 and grad_cls
0.20, l2_normalize 0.43, rows_max_sumsq 0.22."""
import os
import sys

import numpy as np
import pytest

from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import hook_cases as hc
finally:
    sys.path.pop(0)

COSINE = [(s, t) for s in hc.FORWARD_SHAPES for t in hc.DTYPES]
BACKWARD = [(s, t) for s in hc.BACKWARD_SHAPES for t in hc.DTYPES]
_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def _moved(a, b, by):
    """Did any element move by more than `by` (or leave the finite numbers)?"""
    with np.errstate(invalid="ignore"):
        return bool((~np.isfinite(b) | (np.abs(a - b) > by))[np.isfinite(a)].any())


# ------------------------------------------------------------------ 1. the inputs are sharp
def test_shape_lists_are_what_the_kernels_branch_on():
    assert len(hc.FORWARD_SHAPES) == 11 and len(hc.BACKWARD_SHAPES) == 11
    assert all(k <= 64 for _, k, _, _ in hc.BACKWARD_SHAPES) and (2, 63, 70, 3) in hc.BACKWARD_SHAPES and (2, 4, 256, 65) in hc.BACKWARD_SHAPES
    assert hc.probed_columns(1) == [0] and hc.probed_columns(65) == [0, 1, 62, 63, 64]
    assert hc.probed_columns(769) == [0, 1, 62, 63, 64, 65, 127, 128, 704, 705, 767, 768]
    assert abs(hc.tol_f(769) - 2.6e-6) < 1e-7


@pytest.mark.parametrize("shape,dtype", COSINE, ids=_ID)
def test_spikes_make_every_probed_column_and_the_next_element_visible(shape, dtype):
    case = hc.cosine_case(shape, dtype)
    b, k, d, _ = shape
    ref = case.scores_ref()
    big = 1000 * hc.tol_f(d)
    if dtype == "bf16":
        assert np.array_equal(hc.to_bf16(case.q), case.q) and np.array_equal(hc.to_bf16(case.c), case.c)
    for p in hc.probed_columns(d):
        pr = case.carrier[p]
        q, c = case.q.copy(), case.c.copy()
        q[:, p], c[:, :, p] = 0, 0
        assert _moved(ref.ravel()[pr:pr + 1], case.scores_ref(q, c).ravel()[pr:pr + 1], big), f"column {p} is invisible"
    # one element too many: row r read together with the first element of row r + 1
    if b * k > 1:
        q = np.concatenate([case.q, np.append(case.q[1:, 0], 0)[:, None]], axis=1)
        cf = case.c.reshape(b * k, d)
        c = np.concatenate([cf, np.append(cf[1:, 0], 0)[:, None]], axis=1).reshape(b, k, d + 1)
        assert _moved(ref, case.scores_ref(q, c), big)
    # the zero rows give non-finite references, and only there
    bad = ~np.isfinite(ref)
    want = np.zeros((b, k), dtype=bool)
    if shape == hc.ZERO_CLS[0]:
        want[hc.ZERO_CLS[1]] = True
    if shape == hc.ZERO_QUERY[0]:
        want[hc.ZERO_QUERY[1]] = True
    assert np.array_equal(bad, want)


@pytest.mark.parametrize("shape,dtype", BACKWARD, ids=_ID)
def test_bias_gradient_terms_keep_their_share(shape, dtype):
    case = hc.cosine_case(shape, dtype)
    L = case.L
    if L:
        a = np.abs(case.gb.astype(np.float64))
        assert set(np.unique(a)) <= {1.0, 2.0}
        share = (a.min(2) / a.sum(2)).min()
        assert share >= 1.0 / (2 * L) and share > 1000 * hc.eps_w(case.d, L)


@pytest.mark.parametrize("n", hc.L2_N)
@pytest.mark.parametrize("d", hc.L2_D)
def test_l2_rows_stay_where_float32_and_float64_agree(n, d):
    case = hc.l2_case(n, d)
    x6 = case.x[case.plain].astype(np.float64)
    norms = np.sqrt((x6 * x6).sum(1))
    assert (norms >= hc.L2_NORM_WINDOW[0]).all() and (norms <= hc.L2_NORM_WINDOW[1]).all()
    nz = np.abs(x6[x6 != 0])
    assert nz.min() >= 1e-18 and nz.max() <= 1e15 and (np.abs(case.ref()[x6 != 0]) > 1e-9).all()   # no float32 subnormal anywhere
    if n >= 5:
        z, uf, of = (case.x[r] for r in (hc.L2_ZERO_ROW, hc.L2_UNDERFLOW_ROW, hc.L2_OVERFLOW_ROW))
        assert not z.any() and np.signbit(z).sum() == 1
        assert (np.abs(uf) < 1e-25).all() and uf.all() and not (uf * uf).any()
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(of[0]) * np.float32(of[0])) and not case.edge[hc.L2_OVERFLOW_ROW].any()
    # every probed column is a spike somewhere
    plain = set(case.plain.tolist())
    if n < 5:
        assert set().union(*[case.cols[i] for i in plain]) == set(hc.probed_columns(d))


# ------------------------------------------------------------------ 2. + 3. the model passes, its wrong variants do not
_WORST = {}


def _note(key, r):
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    print(f"model error / bound, {key}: {r:.3f} (worst so far {_WORST[key]:.3f})")
    assert r <= 1.0


@pytest.mark.parametrize("shape,dtype", COSINE, ids=_ID)
def test_forward_model_within_bound_and_mutations_rejected(shape, dtype):
    case = hc.cosine_case(shape, dtype)
    b, k, d, _ = shape
    _note("cosine forward", hc.compare_scores(case, hc.model_scores(case)))
    for variant in hc.VARIANTS_COLUMNS + ("wrong_norm",):
        if variant == "wrong_norm" and b * k == 1:
            continue                                             # (there is no other row)
        with pytest.raises(AssertionError):
            hc.compare_scores(case, hc.model_scores(case, variant))


@pytest.mark.parametrize("shape,dtype", BACKWARD, ids=_ID)
def test_backward_model_within_bound_and_mutations_rejected(shape, dtype):
    case = hc.cosine_case(shape, dtype)
    b, k, d, L = shape
    for mode in hc.BACKWARD_MODES:
        if mode == "bias" and L == 0:
            gq, gc = hc.model_backward(case, mode)
            assert not gq.any() and not gc.any()                    # nothing flows: exact zeros
        rq, rc = hc.compare_backward(case, mode, *hc.model_backward(case, mode))
        _note("cosine backward grad_query", rq)
        _note("cosine backward grad_cls", rc)
        variants = list(hc.VARIANTS_COLUMNS)
        if b * k > 1:
            variants.append("wrong_norm")
        if k % 4:
            variants.append("skip_j_tail")
        if L > 64 and mode != "scores":
            variants.append("mem_past_64")
        if mode == "bias" and L == 0:
            variants = []
        for variant in variants:
            with pytest.raises(AssertionError):
                hc.compare_backward(case, mode, *hc.model_backward(case, mode, variant))


def test_backward_mutations_all_occur():
    """Every variant the issue names is live in at least one shape."""
    assert any(k % 4 for _, k, _, _ in hc.BACKWARD_SHAPES) and any(L > 64 for _, _, _, L in hc.BACKWARD_SHAPES)
    assert any(k == 63 for _, k, _, _ in hc.BACKWARD_SHAPES) and any(k == 64 for _, k, _, _ in hc.BACKWARD_SHAPES)


@pytest.mark.parametrize("n", hc.L2_N)
@pytest.mark.parametrize("d", hc.L2_D)
def test_l2_model_within_bound_and_mutations_rejected(n, d):
    case = hc.l2_case(n, d)
    _note("l2_normalize", hc.compare_l2(case, hc.model_l2(case)))
    for variant in hc.VARIANTS_COLUMNS + ("wrong_norm",):
        if variant == "wrong_norm" and n == 1:
            continue
        with pytest.raises(AssertionError):
            hc.compare_l2(case, hc.model_l2(case, variant))
    if n >= 5:                                                       # a rule other than faiss's on the edge rows
        wrong = hc.model_l2(case)
        wrong[hc.L2_UNDERFLOW_ROW] = 0
        with pytest.raises(AssertionError):
            hc.compare_l2(case, wrong)
        wrong = hc.model_l2(case)
        wrong[hc.L2_ZERO_ROW] = 0.0                                   # (+0 where -0 stood)
        with pytest.raises(AssertionError):
            hc.compare_l2(case, wrong)


@pytest.mark.parametrize("n", hc.MAX_N)
@pytest.mark.parametrize("d", hc.MAX_D)
def test_max_model_within_bound_and_mutations_rejected(n, d):
    for plant in hc.max_plants(n):
        x = hc.max_matrix(n, d, plant)
        ref = hc.max_ref(x)
        x6 = x.astype(np.float64)
        ss = (x6 ** 2).sum(1)
        assert ss.argmax() == plant and abs(ss.max() - ref) <= 8 * 2.0 ** -53 * ref    # the issue's expression, correctly rounded
        if n > 1:
            assert ss[plant] > 2 * np.delete(ss, plant).max()
        _note("rows_max_sumsq", hc.compare_max(d, hc.model_max(x), ref))
        variants = ["drop_last", "drop_stride_col"]
        if plant == n - 1:
            variants.append("extra")                                  # (the guard behind the window)
        if plant >= hc.MAX_STRIDE:
            variants.append("no_stride")
        for variant in variants:
            with pytest.raises(AssertionError):
                hc.compare_max(d, hc.model_max(x, variant), ref)
    assert hc.max_ref(np.zeros((n, d), np.float32)) == 0.0


@pytest.mark.parametrize("kf,k", hc.FILTER_K)
@pytest.mark.parametrize("nq", hc.FILTER_NQ)
def test_filter_cases_run_short_and_the_unpadded_kernel_is_rejected(nq, kf, k):
    case = hc.filter_case(nq, kf, k)
    assert (case.ids[case.ids >= 0] >= hc.ID_OFFSET).all()
    for si, ss in ((0x5A5A5A5A5A5A5A5A, 0x7FC0BEEF), (-1, hc.PAD_SCORE_BITS)):
        hc.compare_filter(case, *hc.model_filter(case, si, ss))
    short = case.survivors < k
    if nq >= 255:
        assert (case.survivors == k).any()
        assert short.any() or kf - k > 1                             # (30 fetched for 1 never runs short: the plain path)
        assert (case.ignore == -1).any() and ((case.ids[:, -1] == -1) & (case.ignore == -1)).any()
        if kf > 2:
            assert case.dup.any()
        if kf == k:
            assert short.sum() > nq // 2
    if short.any():
        # stale memory cannot pass: each of two different sentinels fails on its own
        for si, ss in ((0x5A5A5A5A5A5A5A5A, 0x7FC0BEEF), (7, 0x3F800000)):
            with pytest.raises(AssertionError):
                hc.compare_filter(case, *hc.model_filter(case, si, ss, pad=False))


# ------------------------------------------------------------------ storage rounding
def _nan32(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def test_bf16_reference_is_independent_and_half_up_is_rejected():
    x = hc.rounding_inputs_bf16()
    assert x.shape == (512, 768) and len(np.unique(x.view(np.uint32))) == 512 * 768
    want = hc.bf16_round_bits(x)
    nan = _nan32(x)
    fin = np.isfinite(x)
    with np.errstate(over="ignore"):
        assert np.array_equal(synth.bf16_bits(synth.round_to_bf16(x))[fin], want[fin])     # two algorithms, one answer
    inf = np.isinf(x)
    assert inf.sum() == 2 and np.array_equal(want[inf] & 0x7FFF, [0x7F80, 0x7F80])
    assert (np.abs(hc.bf16_to_f32(want)[fin & (np.abs(x) > 3.39e38)]) == np.inf).any()       # overflow rounds to infinity
    hc.compare_codes(hc.model_bf16_bits(x), want, nan, 0x7F80, 0x8000)
    with pytest.raises(AssertionError):
        hc.compare_codes(hc.model_bf16_bits(x, half_up=True), want, nan, 0x7F80, 0x8000)
    with pytest.raises(AssertionError):                                                       # a NaN that lost its sign
        hc.compare_codes(np.where(nan, np.uint16(0x7FC0), want), want, nan, 0x7F80, 0x8000)


def test_e4m3_reference_is_a_table_search_and_wrong_roundings_are_rejected():
    bits = np.arange(65536, dtype=np.uint16)
    x = hc.bf16_to_f32(bits)
    fin = np.isfinite(x)
    assert fin.sum() == 65280
    want = hc.e4m3_nearest_bits(x)
    assert np.array_equal(synth.e4m3_bits(x)[fin], want[fin])
    assert np.array_equal(want[np.isinf(x)], [0x7E, 0xFE])
    for x in (hc.bf16_to_f32(hc.rounding_inputs_e4m3_from_bf16()), hc.rounding_inputs_e4m3_from_f32()):
        want, nan = hc.e4m3_nearest_bits(x), _nan32(x)
        hc.compare_codes(hc.model_e4m3_bits(x), want, nan, 0x7F, 0x80)
        hc.compare_codes(synth.e4m3_bits(x), want, nan, 0x7F, 0x80)
        with pytest.raises(AssertionError):
            hc.compare_codes(hc.model_e4m3_bits(x, half_up=True), want, nan, 0x7F, 0x80)
        with pytest.raises(AssertionError):
            hc.compare_codes(hc.model_e4m3_bits(x, saturate=False), want, nan, 0x7F, 0x80)
