"""The cases of tests/magnitude_cases.py do what tests/test_gpu_magnitudes.py relies on (no GPU): the derived all-pairs dots are the
direct ones, the references are exactly scale-equivariant, every case the GPU file uses stays inside the window, every listed
mistake changes a result of the family named for it, and the absolute constants the module's docstring speaks of are the ones
the sources carry."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import ivf_range_cases as rc
    import ivf_search_cases as sc
    import magnitude_cases as mc
finally:
    sys.path.pop(0)
from oracle import mips_oracle as orc  # noqa: E402

F = np.float32
CSRC = os.path.join(ROOT, "retrieval-augmented-mds_amd", "csrc")
N, NQ, D = 777, 23, 100          # small shapes of this file: 6 blocks of 128 rows and a ragged one


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))


def _direct(name, storage, d=D, n=N, nq=NQ):
    fam, x, q = mc.inputs(name, storage, d, n, nq)
    xs, qs = mc.stored(storage, x, q)
    return fam, xs, qs, mc.pairs_direct(xs, qs)


# ------------------------------------------------------------------ the derivation
@pytest.mark.parametrize("storage,names", [("bf16", mc.ALL_FAMILIES), ("f32", mc.ALL_FAMILIES), ("fp8_e4m3_docs", mc.QUERY_SIDE),
                                           ("fp8_e4m3", mc.UNSCALED)])
def test_derived_pairs_are_the_direct_ones(storage, names):
    """dots and squared norms scaled entry by entry from the base's == orc.canonical_pairs / sumsq_canonical on the transformed,
    stored inputs, as fp64 bit patterns"""
    for name in names:
        fam, xs, qs, direct = _direct(name, storage)
        derived = mc.pairs(name, storage, D, N, NQ)
        for a, b, what in zip(derived, direct, ("dot", "xx", "qq")):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (storage, name, what)
        if name == mc.T5:
            assert (direct.dot < 0).all()
        if name == mc.T4:
            L = mc.loud_row(N)
            k0, k1 = mc.keys(direct, 0), mc.keys(direct, 1)
            assert (k0.argmax(axis=1)[0::2] == L).all() and (k0.argmin(axis=1)[1::2] == L).all()
            assert (k1.argmin(axis=1)[0::2] == L).all() and (k1.argmax(axis=1)[1::2] == L).all()
            assert max(len(np.unique(k1[j])) for j in range(NQ)) <= 8       # the float32 distances collapse


def test_all_pairs_reference_is_the_oracle_on_tie_free_data():
    for storage in ("bf16", "f32"):
        fam, xs, qs, p = _direct(mc.BASELINE, storage)
        assert _same(mc.topk(mc.keys(p, 0), 7, 0), orc.search_exact(qs, xs, 7))
        assert _same(mc.topk(mc.keys(p, 1), 7, 1), orc.search_exact(qs, xs, 7, metric=1))
        assert _same(mc.topk(mc.keys(p, 0), 7, 0), orc.search_exact_bruteforce(qs, xs, 7))
        for name in mc.STD:                                   # wherever the GPU file takes orc.search_exact as the reference
            for metric in (0, 1):
                if not mc.needs_all_pairs(name, metric):
                    fam, xs, qs, p = _direct(name, storage)
                    assert _same(mc.topk(mc.keys(p, metric), 7, metric), orc.search_exact(qs, xs, 7, metric=metric)), (name, metric)


# ------------------------------------------------------------------ scale equivariance of the references
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_references_are_scale_equivariant(storage):
    _, xs0, qs0, p0 = _direct(mc.BASELINE, storage)
    d0, i0 = orc.search_exact(qs0, xs0, 9)
    l0, li0 = mc.topk(mc.keys(p0, 1), 9, 1)
    r0 = mc.radii_for_counts(mc.keys(p0, 0), 0)
    for a, b in mc.T1_PAIRS:
        _, xs, qs, p = _direct(mc.scaled_name(a, b), storage)
        d, i = orc.search_exact(qs, xs, 9)
        assert np.array_equal(i, i0) and np.array_equal(_bits(d), _bits(np.ldexp(d0, np.int32(a + b)))), (a, b)
        assert _same(mc.topk(mc.keys(p, 0), 9, 0), (d, i))
        r = mc.radii_for_counts(mc.keys(p, 0), 0)
        assert np.array_equal(_bits(r), _bits(np.ldexp(r0, np.int32(a + b))))               # the radii scale with the data
        if a == b:
            l, li = mc.topk(mc.keys(p, 1), 9, 1)
            assert np.array_equal(li, li0) and np.array_equal(_bits(l), _bits(np.ldexp(l0, np.int32(2 * a))))
            assert _same(orc.search_exact(qs, xs, 9, metric=1), (l, li))


def test_sq8_reference_is_scale_equivariant():
    _, x0, q0 = mc.inputs(mc.BASELINE, "sq8", D, N, NQ)
    d0, i0, vmin0, vdiff0, codes0 = mc.sq8_reference(x0, q0, 5)
    for a, b in mc.T1_PAIRS:
        _, x, q = mc.inputs(mc.scaled_name(a, b), "sq8", D, N, NQ)
        d, i, vmin, vdiff, codes = mc.sq8_reference(x, q, 5)
        assert np.array_equal(codes, codes0), (a, b)
        assert np.array_equal(_bits(vmin), _bits(np.ldexp(vmin0, np.int32(a)))) and np.array_equal(_bits(vdiff), _bits(np.ldexp(vdiff0, np.int32(a))))
        assert np.array_equal(i, i0) and np.array_equal(_bits(d), _bits(np.ldexp(d0, np.int32(a + b)))), (a, b)


def test_normalised_queries_do_not_depend_on_their_scale():
    _, _, q0 = mc.inputs(mc.BASELINE, "f32", D, N, NQ)
    want = orc.l2_normalization(q0.copy())
    for name in (mc.scaled_name(0, 30), mc.scaled_name(0, -30), mc.T2):
        _, _, q = mc.inputs(name, "f32", D, N, NQ)
        assert np.array_equal(_bits(orc.l2_normalization(q.copy())), _bits(want)), name
    _, _, qz = mc.inputs(mc.T6A, "f32", D, N, NQ)
    assert not orc.l2_normalization(qz.copy())[[0, NQ - 1]].any()                          # a zero query stays zero


def test_ivf_reference_is_scale_equivariant():
    d, n, nq = 40, 600, 9
    for storage in mc.IVF_STORAGES:
        c0 = mc.ivf_case(mc.BASELINE, storage, d, n, nq)
        want = sc.search(c0["rows"], c0["q"], c0["assign"], c0["centroids"], 5, 3, storage, c0["par"])
        for a, b in mc.T1_PAIRS:
            for cexp in (None, 0):                                                       # centroids scaled with the rows / left alone
                c = mc.ivf_case(mc.scaled_name(a, b), storage, d, n, nq, centroid_exp=cexp)
                assert np.array_equal(c["assign"], c0["assign"])
                got = sc.search(c["rows"], c["q"], c["assign"], c["centroids"], 5, 3, storage, c["par"])
                assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(np.ldexp(want[0], np.int32(a + b)))), (storage, a, b)
        neg = mc.ivf_case(mc.T5, storage, d, n, nq)
        sizes = np.bincount(neg["assign"], minlength=mc.IVF_NLIST)
        assert len(set(sizes[sizes > 0])) > 1 and (sizes % 64 != 0).any()                 # ragged lists: padded tails exist
        per = rc.probed_scores(neg["rows"], neg["q"], neg["assign"], neg["centroids"], mc.IVF_NLIST, storage, neg["par"])
        assert all((rep < 0).all() for _, _, rep, _ in per)


# ------------------------------------------------------------------ the window
def test_every_gpu_case_is_inside_the_window():
    cases = mc.flat_window_cases()
    assert {c[1] for c in cases} == set(mc.ALL_FAMILIES)
    for what, name, storage, d, n, nq in cases:
        fam, x, q = mc.inputs(name, storage, d, n, nq)
        if storage == "sq8":       # norms and products of the values given; the scan's own products are code x q', the score adds the bias
            D_, _, vmin, vdiff, codes = mc.sq8_reference(x, q, 5)
            mc.assert_window(x, q, what=f"{what} {name} sq8")
            mc.assert_products(codes.astype(F), mc.sq.scaled_queries(q, vdiff), what=f"{what} {name} sq8 codes")
            mc._inside(mc._nonzero_range(D_), f"{what} {name} sq8: reported scores")
            mc._inside(mc._nonzero_range(vdiff), f"{what} {name} sq8: vdiff")
            continue
        xs, qs = mc.stored(storage, x, q)
        mc.assert_window(xs, qs, what=f"{what} {name} {storage} d={d} n={n}")
    d, n, nq = mc.IVF_SHAPE
    for storage in mc.IVF_STORAGES:
        for name in mc.FULL:
            c = mc.ivf_case(name, storage, d, n, nq)
            X, Y, bias = sc.stored(c["rows"], c["q"], storage, c["par"])
            if storage == "sq8":
                mc.assert_window(c["rows"], c["q"], what=f"ivf {name} sq8")
                mc.assert_products(X, Y, what=f"ivf {name} sq8 codes")
            else:
                mc.assert_window(X, Y, what=f"ivf {name} {storage}")
            mc._inside(mc._nonzero_range(c["centroids"].astype(np.float64) ** 2), "centroids")


def test_the_window_assertion_bites():
    _, xs, qs, _ = _direct(mc.scaled_name(-30, -30), "bf16")
    with pytest.raises(AssertionError, match="leaves the window"):
        mc.assert_window(np.ldexp(xs, np.int32(-30)).astype(F), qs, what="2^-60 rows")
    with pytest.raises(AssertionError, match="leaves the window"):
        mc.assert_window(np.ldexp(xs, np.int32(90)).astype(F), np.ldexp(qs, np.int32(90)).astype(F), what="2^60 x 2^60")


# ------------------------------------------------------------------ the cases reject wrong kernels
def _changed(a, b):
    """queries whose (ids, score bits) differ"""
    return int(sum(not (np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[0]), _bits(y[0]))) for x, y in
                   zip(zip(a[0], a[1]), zip(b[0], b[1]))))


def _csr_changed(a, b):
    (la, ia), (lb, ib) = a, b
    return int(sum(not np.array_equal(ia[la[j]:la[j + 1]], ib[lb[j]:lb[j + 1]]) for j in range(len(la) - 1)))


def _range_ref(p, metric):
    key = mc.keys(p, metric)
    r = mc.radii_for_counts(key, metric)
    return r, mc.in_range(key, r, metric)[0::2]


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_every_mistake_is_caught_by_its_family(storage):
    k = 5
    base = mc.pairs(mc.BASELINE, storage, D, N, NQ)
    neg = mc.pairs(mc.T5, storage, D, N, NQ)
    assert N % 128 != 0
    # zero_init / pad_scores_zero: invisible on Gaussian data, fatal when every score is negative
    for wrong in ("zero_init", "pad_scores_zero"):
        assert _changed(mc.wrong_topk(wrong, base, k, 0), mc.topk(mc.keys(base, 0), k, 0)) == 0, wrong
        assert _changed(mc.wrong_topk(wrong, neg, k, 0), mc.topk(mc.keys(neg, 0), k, 0)) == NQ, wrong
    r, want = _range_ref(neg, 0)
    assert (r < 0).all() and _csr_changed(mc.wrong_range("zero_init", neg, r, 0), want) > 0
    # abs_eps: harmless at unit scale, caught at (-30, -30) and by the all-tied zero query
    r, want = _range_ref(base, 0)
    assert _csr_changed(mc.wrong_range("abs_eps", base, r, 0), want) == 0
    for name in (mc.scaled_name(-30, -30), mc.T6A):
        p = mc.pairs(name, storage, D, N, NQ)
        r, want = _range_ref(p, 0)
        assert _csr_changed(mc.wrong_range("abs_eps", p, r, 0), want) > 0, name
    # neighbour_norm: equal norms hide it; T2's differ by 2^48
    p = mc.pairs(mc.T2, storage, D, N, NQ)
    r, want = _range_ref(p, 1)
    assert _csr_changed(mc.wrong_range("neighbour_norm", p, r, 1), want) >= NQ // 2
    # ip_prefilter_only: right on Gaussian data (it IS orc.search_exact_bruteforce's L2), wrong where the distances collapse
    assert _changed(mc.wrong_topk("ip_prefilter_only", base, k, 1), mc.topk(mc.keys(base, 1), k, 1)) == 0
    p = mc.pairs(mc.T4, storage, D, N, NQ)
    assert _changed(mc.wrong_topk("ip_prefilter_only", p, 29, 1), mc.topk(mc.keys(p, 1), 29, 1)) > 0
    # zero_row_is_padding
    p = mc.pairs(mc.T6B, storage, D, N, NQ)
    r, want = _range_ref(p, 0)
    assert _csr_changed(mc.wrong_range("zero_row_is_padding", p, r, 0), want) > 0
    assert _changed(mc.wrong_topk("zero_row_is_padding", p, mc.WIDE_K, 1), mc.topk(mc.keys(p, 1), mc.WIDE_K, 1)) >= 0
    pz = mc.pairs(mc.T6C, storage, D, N, NQ)
    assert _changed(mc.wrong_topk("zero_row_is_padding", pz, k, 0), mc.topk(mc.keys(pz, 0), k, 0)) == NQ
    assert set(mc.MISTAKES) == {"zero_init", "pad_scores_zero", "abs_eps", "neighbour_norm", "ip_prefilter_only", "zero_row_is_padding"}


def test_zero_cases_tie_every_row():
    p = mc.pairs(mc.T6C, "bf16", D, N, NQ)
    d, i = mc.topk(mc.keys(p, 0), 5, 0)
    assert (i == np.arange(5)).all() and not _bits(d).any()                               # + 0, the lowest rows
    p = mc.pairs(mc.T6A, "bf16", D, N, NQ)
    d, i = mc.topk(mc.keys(p, 1), 5, 1)
    assert (i[[0, NQ - 1]] == np.arange(5)).all() and (d[[0, NQ - 1]] == F(p.xx.max())).all()


# ------------------------------------------------------------------ what the module says about the sources
def test_pinned_constants_and_block_sizes():
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    # the absolute constants the module's docstring (and DESIGN.md, "Magnitudes") names are where it says, and are the only ones
    assert len(re.findall(r"\+ 1e-30;", src("resolve_kernels.hpp"))) == 1
    assert len(re.findall(r"- 1e-300;", src("range_kernels.hpp"))) == 1
    assert len(re.findall(r"\+ 1e-300;", src("scan_kernel_wide.hpp"))) == 1
    assert len(re.findall(r"\* \(1\.0 \+ 1e-12\)", src("tiny_search.hpp"))) == 2
    assert len(re.findall(r"\* \(1\.0 \+ 1e-12\)", src("aux_kernels.hpp"))) == 1
    tiny = re.compile(r"(?<![\w.])\d(?:\.\d+)?e-(?:[2-9]\d|\d{3})\b")                      # a literal below 1e-19
    found = {f: tiny.findall(src(f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip"))}
    found = {f: v for f, v in found.items() if v}
    assert found == {"resolve_kernels.hpp": ["1e-30"], "range_kernels.hpp": ["1e-300"], "scan_kernel_wide.hpp": ["1e-300"]}, found
    # the loud row avoids the block edges of every size the recipes name
    assert mc.sr.DOC_BLOCKS == (16, 32, 64, 128)
    for n in (mc.N_DEFAULT, N, mc.IVF_SHAPE[1]):
        row = mc.loud_row(n)
        assert all(row % b not in (0, b - 1) for b in (16, 32, 64, 128)) and n // 4 < row < 3 * n // 4
    assert mc.N_DEFAULT % 128 != 0 and all(f.n <= 4099 for f in (mc.family(name, mc.N_DEFAULT, 16) for name in mc.ALL_FAMILIES))
    assert mc.WINDOW == (2.0 ** -110, 2.0 ** 110)
