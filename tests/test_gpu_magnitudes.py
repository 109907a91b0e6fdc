"""Every search path across magnitudes, signs and zero vectors (tests/magnitude_cases.py has the families, the references and the
window): rows x 2^a and queries x 2^b, queries and rows of ragged magnitude inside one call, one loud row, calls in which every
score is negative, zero queries, zero rows and an all-zero index -- on MipsIndex.search (one recipe per scan-kernel family, the
family asserted through last_kernel), search_wide (plain, selector, groups), range_search, search_fused (plain, normalize=True,
groups=), compute_distance_subset, and IvfIndex.search_probed / search_probed_wide / range_search_probed.

Per call: I equals the reference and D equals it bit for bit; under T1 and T2 the result is the baseline call's, scaled exactly;
index.check() passes and nothing stays unresolved; under T1 the certificate flags as many queries as at unit scale (it is built from
relative terms: a higher count would mean that an absolute constant widens it); under T3 and T4 whatever is flagged is settled."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import ivf_filter_cases as fc
    import ivf_range_cases as rc
    import ivf_wide_cases as wc
    import magnitude_cases as mc
    import scan_recipes as sr
finally:
    sys.path.pop(0)
from oracle import synth  # noqa: E402

F = np.float32
MASKED, GROUPED, HOOK = "mips::masked_scan_kernel", "mips::grouped_scan_kernel", "mips::hook_grouped_kernel"
KNOB_DEFAULTS = (("nsplit", 0), ("variant", 0), ("optimistic", 1), ("tiny", 1), ("f32_fast", 1))


def _ram():
    import retrieval_augmented_mds_amd as ram

    return ram


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=F).view(np.uint32)


def _same(got, want, what):
    """the suite's convention: ids exactly, scores as bit patterns; the first difference names its query"""
    gd, gi, wd, wi = _np(got[0]), _np(got[1]), _np(want[0]), _np(want[1])
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert not len(bad), f"{what}: ids differ in queries {bad[:8]} ({len(bad)} of {len(gi)}): {gi[bad[0]]} != {wi[bad[0]]}"
    bad = np.flatnonzero((_bits(gd) != _bits(wd)).any(axis=1))
    assert not len(bad), f"{what}: scores differ in queries {bad[:8]} ({len(bad)} of {len(gi)}): {gd[bad[0]]} != {wd[bad[0]]}"


def _same_csr(got, want, what):
    lims, D, I = (_np(t) for t in got)
    el, eD, eI = want
    assert lims.shape == el.shape and lims[0] == 0, what
    for j in range(len(el) - 1):
        a, b, ea, eb = int(lims[j]), int(lims[j + 1]), int(el[j]), int(el[j + 1])
        assert b - a == eb - ea, f"{what}: query {j} has {b - a} hits, expected {eb - ea}"
        assert np.array_equal(I[a:b], eI[ea:eb]), f"{what}: ids of query {j} differ"
        assert np.array_equal(_bits(D[a:b]), _bits(eD[ea:eb])), f"{what}: scores of query {j} differ"
    assert len(D) == len(I) == el[-1]


def _scaled(D, e):
    """float32 D x 2^e, exactly (e: an int or one per query)"""
    e = np.asarray(e, dtype=np.int32)
    return np.ldexp(_np(D), e if e.ndim == 0 else e[:, None]).astype(F)


def _flat(storage, d, metric, x):
    """an index over x, added through the public surface; it holds what the references multiply"""
    ram = _ram()
    ix = ram.MipsIndex(d, metric=metric, dtype=storage)
    if storage == "sq8":
        ix.train(x)
    ix.add(x)
    if storage != "sq8":
        raw = ix.rows_raw()
        held = synth.bf16_bits_to_f32(raw) if storage == "bf16" else raw if storage == "f32" else synth.e4m3_bits_to_f32(raw)
        assert np.array_equal(held.view(np.uint32), sr.storage_values(storage, x).view(np.uint32)), "the index does not hold what the reference multiplies"
    return ix


def _collapsed(name, metric):
    """L2 under T1 with a != b: |q|^2, phi and q.x lie 2^30 or more apart, one float32 ulp of the largest exceeds every gap between
    two rows' keys, and the rows tie at the k-th place by the hundred (tests/magnitude_cases.py, needs_all_pairs)"""
    return metric == 1 and name.startswith("scaled(") and len(set(mc.scale_of(name))) == 2


def _settled(ix, name, what, metric):
    """checks 3 and 5; -> the flagged count (check 4 compares it).  Where many queries are rightly flagged -- T3, T4, and the
    collapsed L2 keys -- every one of them is settled"""
    ix.check()
    st = ix.margin_stats()
    assert st["unresolved"] == 0, (what, st)
    if name in (mc.T3, mc.T4) or _collapsed(name, metric):
        assert st["rescanned"] == st["flagged"], (what, st)
    return st["flagged"]


def _baseline_relation(name, metric, fam):
    """-> None, or the exponent(s) e with D(name) == D(baseline) x 2^e and I(name) == I(baseline)"""
    if name.startswith("scaled("):
        a, b = mc.scale_of(name)
        if metric == 0:
            return a + b
        return 2 * a if a == b else None
    if name == mc.T2 and metric == 0:
        return fam.qexp
    return None


# ------------------------------------------------------------------ MipsIndex.search: one recipe per scan-kernel family
_SEARCH_BASE = {}
SEARCH_PARAMS = [(c, m, f) for c in mc.search_cases() for m in c.metrics for f in c.families]


def _search_id(p):
    c, m, f = p
    return f"{c.kernel.replace('mips::', '').replace(' ', '')}-{c.storage}-d{c.d}-{'l2' if m else 'ip'}-{f}"


def _run_search(c, metric, name):
    """-> (D, I, flagged, last_kernel) of the case's search on the family, every check of the call made"""
    n = mc.N_DEFAULT if c.storage == "sq8" else mc.search_rows(name, metric)
    fam, x, q = mc.inputs(name, c.storage, c.d, n, c.nq)
    what = f"{c.kernel} {c.storage} metric {metric} {name}"
    ix = _flat(c.storage, c.d, metric, x)
    for knob, value in KNOB_DEFAULTS + c.knobs:
        ix.set_param(knob, value)
    D, I = ix.search(q, c.k)
    kernel = ix.last_kernel
    flagged = _settled(ix, name, what, metric)
    if c.storage == "sq8":
        wd, wi, vmin, vdiff, codes = mc.sq8_reference(x, q, c.k)
        assert np.array_equal(ix.rows_raw(), codes), what
        want = (wd, wi)
    else:
        want = mc.search_reference(name, c.storage, c.d, c.nq, c.k, metric)
    _same((D, I), want, what)
    _same((ix.compute_distance_subset(q, I), I), (D, I), what + ": compute_distance_subset")
    return D, I, flagged, kernel, fam


@pytest.mark.parametrize("p", SEARCH_PARAMS, ids=_search_id)
def test_search(p):
    c, metric, name = p
    D, I, flagged, kernel, fam = _run_search(c, metric, name)
    family_of = c.kernel if "tiny_search_kernel" in c.kernel else c.kernel.split("<")[0]
    print(f"{_search_id(p)}: {kernel}, flagged {flagged} of {c.nq}")
    if name == mc.BASELINE:
        assert kernel.startswith(c.kernel), f"dispatched to {kernel}"
    assert kernel.startswith(family_of), f"{name}: dispatched to {kernel}, not to {family_of}"
    e = _baseline_relation(name, metric, fam)
    if e is not None:
        key = (c.kernel, metric)
        if key not in _SEARCH_BASE:
            _SEARCH_BASE[key] = _run_search(c, metric, mc.BASELINE)[:3]
        D0, I0, flagged0 = _SEARCH_BASE[key]
        _same((D, I), (_scaled(D0, e), I0), f"{_search_id(p)} against the baseline call")
        if name.startswith("scaled("):
            assert flagged == flagged0, f"{name}: {flagged} queries flagged, {flagged0} at unit scale"
    elif _collapsed(name, metric) and c.storage != "sq8":
        # the one exception to "as many flagged as at unit scale", derived in tests/magnitude_cases.py: a query whose k-th key is
        # shared by more rows than the widest pool holds cannot be certified -- it is flagged, and settled (_settled)
        tied = mc.tied_beyond_pool(mc.keys(mc.pairs(name, c.storage, c.d, mc.search_rows(name, metric), c.nq), metric), c.k, metric)
        assert 10 * tied >= 9 * c.nq and flagged >= tied, f"{name}: {flagged} of {c.nq} queries flagged, {tied} with a k-th key tied beyond any pool"


# ------------------------------------------------------------------ search_wide and range_search
WIDE_PARAMS = [(s, d, nq, m, f) for s, d, nq in mc.WIDE_SHAPES for m in (0, 1) for f in mc.FULL]
_WIDE_BASE, _RANGE_BASE = {}, {}


def _wide_id(p):
    s, d, nq, m, f = p
    return f"{s}-d{d}-{'l2' if m else 'ip'}-{f}"


def _flat_case(storage, d, nq, metric, name):
    fam, x, q = mc.inputs(name, storage, d, mc.N_DEFAULT, nq)
    ix = _flat(storage, d, metric, x)
    ix.set_labels(mc.row_labels(fam.n))
    key = mc.keys(mc.pairs(name, storage, d, mc.N_DEFAULT, nq), metric)
    return fam, q, ix, key


def _run_wide(storage, d, nq, metric, name):
    fam, q, ix, key = _flat_case(storage, d, nq, metric, name)
    k = mc.WIDE_K
    out = {}
    sel, qlab = mc.selector_mask(fam.n), mc.query_labels(nq)
    for mode, kw, mask, kernel in (("plain", {}, None, "mips::wide_scan_kernel"), ("selector", {"selector": sel}, sel, MASKED),
                                   ("groups", {"groups": qlab, "group_mode": "exclude"}, mc.group_mask(mc.row_labels(fam.n), qlab), GROUPED)):
        what = f"search_wide {mode} {_wide_id((storage, d, nq, metric, name))}"
        D, I = ix.search_wide(q, k, **kw)
        assert ix.last_kernel.startswith(kernel), (what, ix.last_kernel)
        flagged = _settled(ix, name, what, metric)
        _same((D, I), mc.topk(key, k, metric, mask), what)
        _same((ix.compute_distance_subset(q, I), I), (D, I), what + ": compute_distance_subset")
        out[mode] = (D, I, flagged)
    print(f"search_wide {_wide_id((storage, d, nq, metric, name))}: flagged {[v[2] for v in out.values()]} of {nq}")
    return out, fam


@pytest.mark.parametrize("p", WIDE_PARAMS, ids=_wide_id)
def test_search_wide(p):
    storage, d, nq, metric, name = p
    out, fam = _run_wide(*p)
    e = _baseline_relation(name, metric, fam)
    if e is not None:
        if p[:4] not in _WIDE_BASE:
            _WIDE_BASE[p[:4]] = _run_wide(storage, d, nq, metric, mc.BASELINE)[0]
        for mode, (D, I, flagged) in out.items():
            D0, I0, flagged0 = _WIDE_BASE[p[:4]][mode]
            _same((D, I), (_scaled(D0, e), I0), f"search_wide {mode} {_wide_id(p)} against the baseline call")
            if name.startswith("scaled("):
                assert flagged == flagged0, f"{mode} {name}: {flagged} queries flagged, {flagged0} at unit scale"


def _run_range(storage, d, nq, metric, name):
    fam, q, ix, key = _flat_case(storage, d, nq, metric, name)
    r = mc.radii_for_counts(key, metric)
    assert np.isfinite(r).all()
    what = f"range_search {_wide_id((storage, d, nq, metric, name))}"
    got = ix.range_search(q, r)
    flagged = _settled(ix, name, what, metric)
    _same_csr(got, mc.in_range(key, r, metric), what)
    sel = mc.selector_mask(fam.n)
    rs = mc.radii_for_counts(key, metric, mask=sel)
    _same_csr(ix.range_search(q, rs, selector=sel), mc.in_range(key, rs, metric, sel), what + " selector")
    _settled(ix, name, what + " selector", metric)
    return got, r, flagged


@pytest.mark.parametrize("p", WIDE_PARAMS, ids=_wide_id)
def test_range_search(p):
    storage, d, nq, metric, name = p
    (lims, D, I), r, flagged = _run_range(*p)
    if name.startswith("scaled(") and (metric == 0 or len(set(mc.scale_of(name))) == 1):
        a, b = mc.scale_of(name)
        e = a + b if metric == 0 else 2 * a
        if p[:4] not in _RANGE_BASE:
            _RANGE_BASE[p[:4]] = _run_range(storage, d, nq, metric, mc.BASELINE)
        (l0, D0, I0), r0, flagged0 = _RANGE_BASE[p[:4]]
        assert np.array_equal(_bits(r), _bits(_scaled(r0, e))), "the radii scale with the data"
        _same_csr((lims, D, I), (l0, _scaled(D0, e), I0), f"range_search {_wide_id(p)} against the baseline call")
        assert flagged == flagged0, f"{name}: {flagged} queries flagged, {flagged0} at unit scale"


# ------------------------------------------------------------------ search_fused: the one-launch hook search
FUSED_PARAMS = [(s, d, nq, m, f) for s, d, nq in mc.FUSED_SHAPES for m in (0, 1) for f in mc.STD]
_FUSED_BASE = {}


def _run_fused(storage, d, nq, metric, name):
    import torch

    fam, q, ix, key = _flat_case(storage, d, nq, metric, name)
    k = mc.FUSED_K
    what = f"search_fused {_wide_id((storage, d, nq, metric, name))}"
    qd = torch.from_numpy(q).cuda()
    out = {}
    D, I = ix.search_fused(qd, k)
    assert ix.last_kernel.startswith("mips::tiny_search_kernel"), (what, ix.last_kernel)
    out["plain"] = (_np(D), _np(I), _settled(ix, name, what, metric))
    _same((D, I), mc.topk(key, k, metric), what)
    _same((ix.compute_distance_subset(qd, I), I), (D, I), what + ": compute_distance_subset")
    qlab = mc.query_labels(nq)
    D, I = ix.search_fused(qd, k, groups=qlab)
    assert ix.last_kernel.startswith(HOOK), (what, ix.last_kernel)
    out["groups"] = (_np(D), _np(I), _settled(ix, name, what + " groups", metric))
    _same((D, I), mc.topk(key, k, metric, mc.group_mask(mc.row_labels(fam.n), qlab)), what + " groups")
    if metric == 0:      # normalize=True: the queries the index multiplies are the normalised ones, whatever their scale
        D, I = ix.search_fused(qd, k, normalize=True)
        out["normalize"] = (_np(D), _np(I), _settled(ix, name, what + " normalize", metric))
        assert np.array_equal(_np(qd), q), "search_fused(normalize=True) changed the caller's queries"
        # the normalised rows are the library's own (l2_normalize_: a float32 sum whose order is the kernel's, so only it has
        # their bits; tests/test_gpu_hook_kernels.py holds it to fp64) -- within (d + 3) 2^-24 of the fp64 ones, zero rows kept
        from retrieval_augmented_mds_amd.index import l2_normalize_

        qn = _np(l2_normalize_(qd.clone()))
        q64 = q.astype(np.float64)
        norm = np.sqrt((q64 * q64).sum(axis=1, keepdims=True))
        exact = np.divide(q64, norm, out=np.zeros_like(q64), where=norm > 0)
        assert np.all(np.abs(qn - exact) <= (d + 3) * 2.0 ** -24 * np.abs(exact)), what + ": l2_normalize_"
        xs = sr.storage_values(storage, ix.reconstruct_n())
        _same((D, I), mc.topk(mc.keys(mc.pairs_direct(xs, sr.query_values(storage, qn)), 0), k, 0), what + " normalize")
    return out, fam


@pytest.mark.parametrize("p", FUSED_PARAMS, ids=_wide_id)
def test_search_fused(p):
    storage, d, nq, metric, name = p
    out, fam = _run_fused(*p)
    e = _baseline_relation(name, metric, fam)
    if e is not None:
        if p[:4] not in _FUSED_BASE:
            _FUSED_BASE[p[:4]] = _run_fused(storage, d, nq, metric, mc.BASELINE)[0]
        base = _FUSED_BASE[p[:4]]
        for mode, (D, I, flagged) in out.items():
            D0, I0, flagged0 = base[mode]
            if mode == "normalize":      # bit for bit the baseline's for every b; the rows still scale the scores
                e_mode = mc.scale_of(name)[0] if name.startswith("scaled(") else 0
            else:
                e_mode = e
            _same((D, I), (_scaled(D0, e_mode), I0), f"search_fused {mode} {_wide_id(p)} against the baseline call")
            if name.startswith("scaled("):
                assert flagged == flagged0, f"{mode} {name}: {flagged} queries flagged, {flagged0} at unit scale"


# ------------------------------------------------------------------ the IVF index
IVF_PARAMS = [(s, f) for s in mc.IVF_STORAGES for f in mc.FULL + ("unscaled_centroids",)]
_IVF_BASE = {}


def _run_ivf(storage, name):
    ram = _ram()
    d, n, nq = mc.IVF_SHAPE
    fname = mc.scaled_name(30, 0) if name == "unscaled_centroids" else name
    c = mc.ivf_case(fname, storage, d, n, nq, centroid_exp=0 if name == "unscaled_centroids" else None)
    rows, q, cen, assign, par, fam = (c[t] for t in ("rows", "q", "centroids", "assign", "par", "fam"))
    ix = ram.IvfIndex(d, mc.IVF_NLIST, dtype=storage)
    ix.set_centroids(cen)
    if storage == "sq8":
        ix.set_sq8_params(*par)
    ix.add(rows)
    assert np.array_equal(ix.assignments(), assign), f"{name}: the rows went to other lists than the restatement's"
    sel, labels, qlab = mc.selector_mask(fam.n), mc.row_labels(fam.n), mc.query_labels(nq)
    ix.set_labels(labels)
    out = {}
    for nprobe in (3, mc.IVF_NLIST):
        what = f"ivf {storage} {name} nprobe {nprobe}"
        args = (rows, q, assign, cen)
        got = ix.search_probed(q, 5, nprobe)
        _same(got, fc.search(*args, 5, nprobe, storage, par), what + ": search_probed")
        out[("search", nprobe)] = got
        if name not in (mc.T3, mc.T4):
            got = ix.search_probed_wide(q, mc.WIDE_K, nprobe)
            _same(got, wc.search(*args, mc.WIDE_K, nprobe, storage, par), what + ": search_probed_wide")
            out[("wide", nprobe)] = got
            per = rc.probed_scores(*args, nprobe, storage, par)
            r = np.array([_radius(rep, j) for j, (_, _, rep, _) in enumerate(per)], F)
            _same_csr(ix.range_search_probed(q, r, nprobe), rc.range_search(*args, r, nprobe, storage, par), what + ": range_search_probed")
    # one filtered call each
    what = f"ivf {storage} {name} filtered"
    args = (rows, q, assign, cen)
    _same(ix.search_probed(q, 5, 3, selector=sel), fc.search(*args, 5, 3, storage, par, sel=sel), what + ": search_probed")
    if name not in (mc.T3, mc.T4):
        kw = dict(labels=labels, q_labels=qlab, mode="exclude")
        _same(ix.search_probed_wide(q, mc.WIDE_K, 3, groups=qlab), wc.search(*args, mc.WIDE_K, 3, storage, par, **kw), what + ": search_probed_wide")
        per = rc.probed_scores(*args, 3, storage, par, sel=sel)
        r = np.array([_radius(rep[ok], j) for j, (_, _, rep, ok) in enumerate(per)], F)
        _same_csr(ix.range_search_probed(q, r, 3, selector=sel), rc.range_search(*args, r, 3, storage, par, sel=sel), what + ": range_search_probed")
    ix.flat.check()
    return out, fam


def _radius(reported, j):
    """tests/ivf_range_cases.py's radius_for_count per target count; where the boundary ties, or nothing is probed, the radius sits
    ON a score (or at - 2^-100): the strict rule decides"""
    if len(reported) == 0:
        return -mc.RADIUS_FLOOR
    c = (0, 1, 7, 50, len(reported))[j % 5]
    r = rc.radius_for_count(reported, min(c, len(reported)))
    if r is None or not np.isfinite(r):
        s = np.sort(np.asarray(reported, dtype=F))
        r = s[0] if j % 2 else np.nextafter(s[0], F(-np.inf))
    if r != 0 and abs(float(r)) < mc.WINDOW[0]:
        r = -mc.RADIUS_FLOOR
    return F(r)


@pytest.mark.parametrize("p", IVF_PARAMS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_ivf(p):
    storage, name = p
    out, fam = _run_ivf(storage, name)
    fname = mc.scaled_name(30, 0) if name == "unscaled_centroids" else name
    e = _baseline_relation(fname, 0, fam)
    if e is not None:
        if storage not in _IVF_BASE:
            _IVF_BASE[storage] = _run_ivf(storage, mc.BASELINE)[0]
        for key, got in out.items():
            D0, I0 = _IVF_BASE[storage][key]
            _same(got, (_scaled(D0, e), I0), f"ivf {storage} {name} {key} against the baseline call")
