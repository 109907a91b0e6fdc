"""The range search over the probed lists on the GPU (mips_ivf_range_search / _grp, IvfIndex.range_search_probed / _into): everything
bit for bit, on all three storages, no tolerance anywhere -- against the NumPy restatement (tests/ivf_range_cases.py) and against the
identities of the definition tested AS identities: every list probed (flat.range_search), scores by id
(flat.compute_distance_subset), against the top-k (search_probed_wide), no filter (the _grp entry).

Cases: Gaussian rows assigned round-robin, so that the probed lists interleave maximally in row order, with per-query radii that give
no, one, many and all hits, empty queries between full ones; -inf and +inf; a planted list scanned as ONE segment whose wave 0 sees
exactly 63, 64, 65, 127, 128 and 129 hits over its stretch; N - 1, N and N + 1 hits around every size class of the ordering step, 4096
-> 4097 (where it leaves LDS) included; empty lists and an empty index; capacities of the total, one less and 0 with guard elements;
the filters of tests/ivf_filter_cases.py, its queue case with a radius every admitted row passes; a call that crosses a query slice;
idx_offset; host radii with a NaN, device radii; the refusals by return code; a plain-C caller."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_cases as iv  # noqa: E402
import ivf_filter_cases as fc  # noqa: E402
import ivf_range_cases as rc  # noqa: E402
import ivf_search_cases as sc  # noqa: E402
import ivf_wide_cases as wc  # noqa: E402

STORAGES = sc.STORAGES
NONE = fc.LABEL_NONE
INF = np.float32(np.inf)


def _ram():
    import retrieval_augmented_mds_amd as ram

    return ram


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _same(got, want):
    gl, gd, gi = (_np(t) for t in got)
    assert np.array_equal(gl, want[0]), (gl[:12], want[0][:12])
    assert gi.shape == want[2].shape and gd.shape == want[1].shape
    assert np.array_equal(gi, want[2]), (np.flatnonzero(gi != want[2])[:5], gi[gi != want[2]][:5], want[2][gi != want[2]][:5])
    assert np.array_equal(gd.view(np.uint32), want[1].view(np.uint32))


def _bitmap(mask):
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def _cus():
    import torch

    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _plant(case, dtype, assign=None, labels=None):
    """an index over case["rows"] with planted centroids (and planted assignments) -> (index, sq8 parameters or None)"""
    ram = _ram()
    from retrieval_augmented_mds_amd.index import _stream_handle

    rows = case["rows"]
    ix = ram.IvfIndex(rows.shape[1], case["nlist"], dtype=dtype)
    ix.set_centroids(case["centroids"])
    par = None
    if dtype == "sq8":
        par = sc.sq.train(rows)
        ix.set_sq8_params(*par)
    ix.add(rows)
    if assign is not None:
        a = np.ascontiguousarray(assign, dtype=np.int32)
        ram._lib.check(ix._lib.mips_ivf_set_assign(ix._h, a.ctypes.data, len(a), _stream_handle(ix.device)), "mips_ivf_set_assign")
        assert np.array_equal(ix.assignments(), a)
    if labels is not None:
        ix.set_labels(labels)
    return ix, par


def _radii_for(per, counts):
    """radii that give query j exactly counts[j] hits among its probed rows (per: rc.probed_scores); `None` in counts: all of them"""
    out = []
    for (ids, _, rep, _), c in zip(per, counts):
        r = rc.radius_for_count(rep, len(rep) if c is None else c)
        assert r is not None, c
        out.append(r)
    return np.array(out, np.float32)


_cache = {}
NQ, N, NLIST = 12, 6000, 8


def robin(dtype):
    """6000 x 32 Gaussian rows, row i in list i % 8 (planted), 12 queries; filled once per storage, the probed rows' scores of every
    nprobe computed once"""
    if dtype not in _cache:
        c = rc.case_round_robin(N, 32, NQ, NLIST)
        rng = np.random.default_rng(3)
        c.update(row_labels=rng.integers(0, 40, N).astype(np.int32), mask=rng.random(N) < 0.5, q_labels=rng.integers(0, 40, NQ).astype(np.int32))
        c["q_labels"][5] = NONE
        ix, par = _plant(c, dtype, assign=c["assign"], labels=c["row_labels"])
        c["par"] = par
        c["base"] = (c["rows"], c["q"], c["assign"], c["centroids"])
        c["per"] = {nprobe: rc.probed_scores(*c["base"], nprobe, dtype, par) for nprobe in (1, 3, 8)}
        _cache[dtype] = (c, ix)
    return _cache[dtype]


# ------------------------------------------------------------------ interleaved lists, per-query radii, the identities
@pytest.mark.parametrize("dtype", STORAGES)
def test_round_robin_radii_and_the_identities(dtype):
    c, ix = robin(dtype)
    q = c["q"]
    qd = _dev(q)
    for nprobe in (1, 3, 8, 100):
        p = min(nprobe, NLIST)
        per = c["per"][p]
        probed = N * p // NLIST
        assert all(len(ids) == probed for ids, _, _, _ in per)
        # no, all, no, one, many, all, no, a few ... hits: empty queries between full ones
        counts = [0, None, 0, 1, probed // 3, None, 0, 5, 64, 0, min(1000, probed - 1), 2]
        radii = _radii_for(per, counts)
        want = rc.range_search(*c["base"], radii, nprobe, dtype, c["par"])
        assert [int(x) for x in np.diff(want[0])] == [probed if x is None else x for x in counts]
        got = ix.range_search_probed(q, radii, nprobe)                                               # host in, host out
        assert all(isinstance(t, np.ndarray) for t in got) and got[0].dtype == np.int64 and got[2].dtype == np.int64
        _same(got, want)
        dev = ix.range_search_probed(qd, _dev(radii), nprobe, idx_offset=1 << 40)                     # device in and out, device radii, an offset
        assert all(t.is_cuda for t in dev)
        _same((dev[0], dev[1], _np(dev[2]) - (1 << 40)), want)
        lims, D, I = got
        for j in (1, 4, 10):                                                                         # identity: scores by id
            again = ix.flat.compute_distance_subset(q[j:j + 1], I[None, lims[j]:lims[j + 1]])
            assert np.array_equal(again[0].view(np.uint32), D[lims[j]:lims[j + 1]].view(np.uint32))
        if p == NLIST and dtype != "sq8":                                                            # identity: every list probed
            _same(got, ix.flat.range_search(q, radii))
        # identity: against the top-k, for radii with fewer than 1024 hits per query
        few = _radii_for(per, [min(x, probed) for x in (0, 1, 2, 29, 30, 64, 65, 100, 500, 1000, 1023, 7)])
        lims, D, I = ix.range_search_probed(q, few, nprobe)
        wd, wi = ix.search_probed_wide(q, 1024, nprobe)
        for j in range(NQ):
            d, i = D[lims[j]:lims[j + 1]], I[lims[j]:lims[j + 1]]
            order = np.lexsort((i, -d))
            keep = wd[j] > few[j]
            assert np.array_equal(i[order], wi[j][keep]) and np.array_equal(d[order].view(np.uint32), wd[j][keep].view(np.uint32))
        for r in (-INF, INF):                                                                        # every probed row / none
            _same(ix.range_search_probed(q, r, nprobe), rc.range_search(*c["base"], r, nprobe, dtype, c["par"]))
        assert ix.range_search_probed(q, -INF, nprobe)[0][-1] == NQ * probed and ix.range_search_probed(qd, INF, nprobe)[0][-1].item() == 0


def test_no_filter_the_grp_entry_is_the_unfiltered_call():
    ram = _ram()
    c, ix = robin("f32")
    lib, qc = ix._lib, np.ascontiguousarray(c["q"])
    radii = _radii_for(c["per"][3], [0, 7, None, 300] * 3)
    out = [(np.empty(NQ + 1, np.int64), np.empty(20000, np.float32), np.empty(20000, np.int64)) for _ in range(2)]
    assert lib.mips_ivf_range_search(ix._h, qc.ctypes.data, ram.DTYPE_F32, NQ, radii.ctypes.data, 3, out[0][0].ctypes.data, out[0][1].ctypes.data,
                                     out[0][2].ctypes.data, 20000, 0, 0, None) == 0
    assert lib.mips_ivf_range_search_grp(ix._h, qc.ctypes.data, ram.DTYPE_F32, NQ, radii.ctypes.data, 3, out[1][0].ctypes.data, out[1][1].ctypes.data,
                                         out[1][2].ctypes.data, 20000, 0, 0, None, 0, 0, None, 0, None) == 0
    total = int(out[0][0][-1])
    want = rc.range_search(*c["base"], radii, 3, "f32")
    assert total == want[0][-1] == 3 * (7 + 2250 + 300)
    for o in out:
        _same((o[0], o[1][:total], o[2][:total]), want)


# ------------------------------------------------------------------ a wave that sees exactly 63 .. 129 hits over its stretch
@pytest.mark.parametrize("dtype", STORAGES)
def test_wave_stretches_of_63_to_129_hits_in_one_segment(dtype):
    nq = wc.queries_for_one_segment(1, _cus())
    assert fc.segments(nq, 1, 1, _cus()) == 1
    c = rc.case_stretch()
    ix, par = _plant(c, dtype, assign=c["assign"])
    six = rc.range_search(c["rows"], c["q6"], c["assign"], c["centroids"], rc.STRETCH_RADIUS, 1, dtype, par)
    assert tuple(np.diff(six[0])) == rc.STRETCH_COUNTS
    rep = np.arange(nq) % 6                                                                          # the queries repeat with period 6
    cnt = np.diff(six[0])[rep]
    want = (np.concatenate([[0], np.cumsum(cnt)]), np.concatenate([six[1][six[0][u]:six[0][u + 1]] for u in rep]),
            np.concatenate([six[2][six[0][u]:six[0][u + 1]] for u in rep]))
    _same(ix.range_search_probed(_dev(c["q6"][rep]), rc.STRETCH_RADIUS, 1), want)                     # one segment: wave 0 owns every hit
    _same(ix.range_search_probed(c["q6"], rc.STRETCH_RADIUS, 1), six)                                 # 32 segments


# ------------------------------------------------------------------ the size classes of the ordering step
@pytest.mark.parametrize("dtype", STORAGES)
def test_hit_counts_around_every_size_class_of_the_ordering_step(dtype):
    c, ix = robin(dtype)
    classes = [2 ** e for e in range(1, 13)]
    assert classes[-1] == rc.SORT_LDS and rc.sort_class(rc.SORT_LDS + 1) == 2 * rc.SORT_LDS
    counts = sorted({n + s for n in classes for s in (-1, 0, 1)}) + [N]                               # 1 .. 4097 (the first stretch beyond LDS), all
    rng = np.random.default_rng(21)
    q = rng.standard_normal((len(counts), 32)).astype(np.float32)
    per = rc.probed_scores(c["rows"], q, c["assign"], c["centroids"], NLIST, dtype, c["par"])
    radii = _radii_for(per, counts)
    want = rc.range_search(c["rows"], q, c["assign"], c["centroids"], radii, NLIST, dtype, c["par"])
    assert [int(x) for x in np.diff(want[0])] == counts and 4095 in counts and 4096 in counts and 4097 in counts
    _same(ix.range_search_probed(_dev(q), _dev(radii), NLIST), want)
    _same(ix.range_search_probed(q[::-1].copy(), radii[::-1].copy(), NLIST), rc.range_search(c["rows"], q[::-1], c["assign"], c["centroids"], radii[::-1],
                                                                                            NLIST, dtype, c["par"]))


# ------------------------------------------------------------------ capacities: the total, one less, none
@pytest.mark.parametrize("dtype", STORAGES)
def test_capacity_of_the_total_one_less_and_zero(dtype):
    import torch

    c, ix = robin(dtype)
    radii = _radii_for(c["per"][3], [40, 0, 700, 1, None, 0, 0, 5000 // 3, 3, 64, 65, 0])
    want = rc.range_search(*c["base"], radii, 3, dtype, c["par"])
    total = int(want[0][-1])
    qd, rd = _dev(c["q"]), _dev(radii)
    for cap in (total, total - 1, 0, total + 9):
        lims = torch.full((NQ + 1,), -1, dtype=torch.int64, device="cuda")
        Dg = torch.full((cap + 16,), -7.0, dtype=torch.float32, device="cuda")
        Ig = torch.full((cap + 16,), -7, dtype=torch.int64, device="cuda")
        ix.range_search_probed_into(qd, rd, lims, Dg[8:8 + cap], Ig[8:8 + cap], nprobe=3)
        assert np.array_equal(_np(lims), want[0]), cap                                                # the true counts, whatever the capacity
        D, I = _np(Dg), _np(Ig)
        assert (D[:8] == -7).all() and (D[8 + cap:] == -7).all() and (I[:8] == -7).all() and (I[8 + cap:] == -7).all()   # the guards
        if cap >= total:
            assert np.array_equal(I[8:8 + total], want[2]) and np.array_equal(D[8:8 + total].view(np.uint32), want[1].view(np.uint32))
            assert (I[8 + total:8 + cap] == -7).all()                                                # nothing behind the last hit either
    lims = np.empty(NQ + 1, np.int64)                                                                # the counting call of the C ABI: NULL arrays
    ram = _ram()
    qc = np.ascontiguousarray(c["q"])
    assert ix._lib.mips_ivf_range_search(ix._h, qc.ctypes.data, ram.DTYPE_F32, NQ, radii.ctypes.data, 3, lims.ctypes.data, None, None, 0, 0, 0, None) == 0
    assert np.array_equal(lims, want[0])


# ------------------------------------------------------------------ filters
@pytest.mark.parametrize("dtype", STORAGES)
def test_round_robin_filters(dtype):
    ram = _ram()
    c, ix = robin(dtype)
    q, ql, lab, mask = c["q"], c["q_labels"], c["row_labels"], c["mask"]
    off = np.concatenate([np.zeros(13, bool), mask, np.ones(3, bool)])
    sel = ram.Selector.from_mask(mask)
    for nprobe in (3, 8):
        radii = _radii_for(c["per"][nprobe], [300, None, 0, 2000, 50, 700, None, 1, 64, 0, 129, 500])
        for mode in ("exclude", "only"):
            want = rc.range_search(*c["base"], radii, nprobe, dtype, c["par"], labels=lab, q_labels=ql, mode=mode)
            _same(ix.range_search_probed(q, radii, nprobe, groups=ql, group_mode=mode), want)         # host labels, a LABEL_NONE query among them
            both = rc.range_search(*c["base"], radii, nprobe, dtype, c["par"], sel=mask, labels=lab, q_labels=ql, mode=mode)
            got = ix.range_search_probed(_dev(q), _dev(radii), nprobe, selector=sel, groups=_dev(ql), group_mode=mode)   # everything on the device
            assert got[0].is_cuda
            _same(got, both)
            assert both[0][-1] < want[0][-1] < rc.range_search(*c["base"], radii, nprobe, dtype, c["par"])[0][-1]
            if nprobe == NLIST and dtype != "sq8":                                                   # every list probed, the same filter
                _same(got, ix.flat.range_search(q, radii, selector=sel, groups=ql, group_mode=mode))
        want = rc.range_search(*c["base"], radii, nprobe, dtype, c["par"], sel=off, sel_bit0=13, idx_offset=77)
        _same(ix.range_search_probed(q, radii, nprobe, idx_offset=77, selector=_bitmap(off), sel_bit0=13), want)   # a host bitmap, bit 13 + i decides row i
        assert not np.array_equal(want[0], rc.range_search(*c["base"], radii, nprobe, dtype, c["par"], sel=off[:N])[0])
    three = np.zeros(N, bool)
    three[[5, 1700, 5999]] = True
    lims, D, I = ix.range_search_probed(q, -INF, 8, selector=_bitmap(three))                          # three rows admitted
    assert np.array_equal(lims, 3 * np.arange(NQ + 1)) and np.array_equal(I, np.tile([5, 1700, 5999], NQ))
    assert ix.range_search_probed(q, -INF, 8, selector=_bitmap(np.zeros(N, bool)))[0][-1] == 0


@pytest.mark.parametrize("dtype", STORAGES)
def test_planted_lists_with_an_empty_one_under_every_filter(dtype):
    ram = _ram()
    c = fc.case_planted(40)
    ix, par = _plant(c, dtype, labels=c["row_labels"])
    assert np.array_equal(ix.assignments(), c["assign"]) and ix.list_sizes()[0] == 0                  # list 0 is empty
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    q, ql, lab = c["q"], c["q_labels"], c["row_labels"]
    for nprobe in (1, 2, 8):
        per = rc.probed_scores(*base, nprobe, dtype, par)
        mid = np.array([np.sort(rep)[len(rep) // 2] if len(rep) else 0.0 for _, _, rep, _ in per], np.float32)
        for radii in (mid, np.full(len(q), -INF)):
            _same(ix.range_search_probed(q, radii, nprobe), rc.range_search(*base, radii, nprobe, dtype, par))
            _same(ix.range_search_probed(q, radii, nprobe, selector=_bitmap(c["sel"])), rc.range_search(*base, radii, nprobe, dtype, par, sel=c["sel"]))
            for mode in ("exclude", "only"):
                want = rc.range_search(*base, radii, nprobe, dtype, par, labels=lab, q_labels=ql, mode=mode)
                _same(ix.range_search_probed(q, radii, nprobe, groups=ql, group_mode=mode), want)
                both = rc.range_search(*base, radii, nprobe, dtype, par, sel=c["sel_off"], sel_bit0=13, labels=lab, q_labels=ql, mode=mode)
                _same(ix.range_search_probed(_dev(q), radii, nprobe, selector=ram.Selector.from_mask(c["sel_off"]), sel_bit0=13, groups=_dev(ql),
                                             group_mode=mode), both)
    if dtype == "f32":                                                                               # queries of the empty list hit nothing at nprobe = 1
        lims = ix.range_search_probed(q, -INF, 1)[0]
        assert all(lims[j + 1] == lims[j] for j in np.flatnonzero(c["qlabels"] == 0))


@pytest.mark.parametrize("dtype", STORAGES)
def test_queue_case_with_a_radius_every_admitted_row_passes(dtype):
    ram = _ram()
    c = fc.case_queue()
    ix, par = _plant(c, dtype, assign=c["assign"], labels=c["row_labels"])
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    one = (c["rows"], c["q"][:1], c["assign"], c["centroids"])
    qd = _dev(c["q"])
    for name, m in c["bitmaps"].items():
        sel = ram.Selector.from_mask(m)
        want = rc.range_search(*base, -INF, 1, dtype, par, sel=m)
        assert want[0][-1] == len(c["q"]) * int(m[c["big"]].sum())
        _same(ix.range_search_probed(qd[:1], -INF, 1, selector=sel), rc.range_search(*one, -INF, 1, dtype, par, sel=m))   # 32 segments
        _same(ix.range_search_probed(qd, -INF, 1, selector=sel), want)                                # one segment per workgroup


# ------------------------------------------------------------------ a call that crosses a query slice; an empty index
def test_more_queries_than_one_slice_on_a_tiny_index():
    c = rc.case_round_robin(200, 32, 7, 4)
    ix, _ = _plant(c, "f32", assign=c["assign"])
    nq = rc.SLICE + 150
    rep = np.arange(nq) % 7
    per = rc.probed_scores(c["rows"], c["q"], c["assign"], c["centroids"], 2, "f32")
    radii7 = _radii_for(per, [3, 0, None, 1, 50, 0, 17])
    seven = rc.range_search(c["rows"], c["q"], c["assign"], c["centroids"], radii7, 2, "f32")
    cnt = np.diff(seven[0])[rep]
    want = (np.concatenate([[0], np.cumsum(cnt)]), np.concatenate([seven[1][seven[0][u]:seven[0][u + 1]] for u in rep]),
            np.concatenate([seven[2][seven[0][u]:seven[0][u + 1]] for u in rep]))
    assert want[0][rc.SLICE] > 0 and want[0][-1] > want[0][rc.SLICE]                                  # hits on both sides of the boundary
    _same(ix.range_search_probed(_dev(c["q"][rep]), _dev(radii7[rep]), 2), want)
    _same(ix.range_search_probed(c["q"][rep], radii7[rep], 2, idx_offset=5), (want[0], want[1], want[2] + 5))


def test_empty_index_and_no_queries():
    ram = _ram()
    x = iv.case_gauss(600, 64, 3, 16)
    ix = ram.IvfIndex(64, 16, dtype="bf16")
    ix.niter = 1
    ix.train(x["rows"])
    lims, D, I = ix.range_search_probed(x["q"], -INF, 4)                                              # an empty index: all-zero lims
    assert np.array_equal(lims, np.zeros(4, np.int64)) and len(D) == 0 and len(I) == 0
    ix.add(x["rows"])
    lims, D, I = ix.range_search_probed(np.zeros((0, 64), np.float32), 0.0, 4)                        # nq = 0
    assert np.array_equal(lims, [0]) and len(D) == 0
    cen = ix.centroids()
    assign = iv.nearest(x["rows"], cen)[:, 0]                                                        # trained lists, some of them empty or short
    _same(ix.range_search_probed(x["q"], 1.5, 5), rc.range_search(x["rows"], x["q"], assign, cen, 1.5, 5, "bf16"))


# ------------------------------------------------------------------ radii: host NaN refused, device radii
def test_host_nan_is_refused_and_device_radii_are_read_on_the_device():
    import torch

    ram = _ram()
    c, ix = robin("f32")
    q = c["q"]
    radii = _radii_for(c["per"][3], [10, 0, 300, 1, None, 0, 0, 77, 3, 64, 65, 0])
    bad = radii.copy()
    bad[4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ix.range_search_probed(q, bad, 3)
    qc = np.ascontiguousarray(q)
    lims = np.full(NQ + 1, -5, np.int64)
    assert ix._lib.mips_ivf_range_search(ix._h, qc.ctypes.data, ram.DTYPE_F32, NQ, bad.ctypes.data, 3, lims.ctypes.data, None, None, 0, 0, 0, None) == -1
    assert b"NaN" in ix._lib.mips_last_error() and (lims == -5).all()                                 # MIPS_E_INVALID, nothing written
    got = ix.range_search_probed(_dev(q), _dev(bad), 3)                                               # on the device: that query hits nothing
    quiet = radii.copy()
    quiet[4] = INF
    _same(got, rc.range_search(*c["base"], quiet, 3, "f32"))
    lims_t = torch.empty(NQ + 1, dtype=torch.int64, device="cuda")                                    # host queries with device radii, and the reverse
    D, I = torch.empty(9000, dtype=torch.float32, device="cuda"), torch.empty(9000, dtype=torch.int64, device="cuda")
    want = rc.range_search(*c["base"], radii, 3, "f32")
    total = int(want[0][-1])
    for qq, rr in ((q, _dev(radii)), (_dev(q), radii), (_dev(q), list(radii))):
        ix.range_search_probed_into(qq, rr, lims_t, D, I, nprobe=3)
        _same((lims_t, D[:total], I[:total]), want)
    ix.range_search_probed_into(_dev(q), float(radii[2]), lims_t, D[:0], I[:0], nprobe=3)             # a scalar, a counting call
    assert np.array_equal(_np(lims_t), rc.range_search(*c["base"], radii[2], 3, "f32")[0])
    with pytest.raises(ValueError, match="radii"):
        ix.range_search_probed(q, _dev(radii[:5]), 3)
    with pytest.raises(ValueError, match="lims"):
        ix.range_search_probed_into(_dev(q), radii, lims_t[:-1], D, I, nprobe=3)


# ------------------------------------------------------------------ refusals, by return code
def test_refusals():
    ram = _ram()
    x = iv.case_gauss(600, 64, 3, 128)
    ix = ram.IvfIndex(64, 128, dtype="f32")
    lib = ix._lib
    q = np.ascontiguousarray(x["q"])
    radii = np.zeros(3, np.float32)
    lims, od, oi = np.empty(4, np.int64), np.empty(2000, np.float32), np.empty(2000, np.int64)

    def rng_(nprobe=2, nq=3, dt=ram.DTYPE_F32, outs=(od.ctypes.data, oi.ctypes.data), cap=2000, flags=0, lp=lims.ctypes.data, rp=radii.ctypes.data):
        return lib.mips_ivf_range_search(ix._h, q.ctypes.data, dt, nq, rp, nprobe, lp, outs[0], outs[1], cap, 0, flags, None)

    def grp(sel=None, nbits=0, bit0=0, lab=None, mode=0):
        return lib.mips_ivf_range_search_grp(ix._h, q.ctypes.data, ram.DTYPE_F32, 3, radii.ctypes.data, 2, lims.ctypes.data, od.ctypes.data, oi.ctypes.data, 2000, 0, 0,
                                             sel, nbits, bit0, lab, mode, None)

    assert rng_() == -1 and b"not trained" in lib.mips_last_error()                                   # untrained (MIPS_E_INVALID)
    with pytest.raises(RuntimeError, match="not trained"):
        ix.range_search_probed(x["q"], 0.0)
    ix.niter = 1
    ix.train(x["rows"])
    ix.add(x["rows"])
    assert rng_() == 0 and lims[0] == 0 and lims[3] <= 2000
    assert rng_(flags=ram._lib.OUT_PACKED) == -1 and rng_(flags=ram._lib.OUT_PACKED | ram._lib.OUT_DEVICE) == -1
    assert rng_(outs=(od.ctypes.data, None)) == -1 and rng_(outs=(None, oi.ctypes.data)) == -1 and rng_(lp=None) == -1 and rng_(rp=None) == -1
    assert rng_(cap=-1) == -1 and rng_(nprobe=0) == -1 and rng_(dt=ram.DTYPE_SQ8) == -1
    assert rng_(nq=0, outs=(None, None), cap=0, rp=None) == 0 and lims[0] == 0                          # nq = 0
    bits = np.full(80, 255, np.uint8)
    ql = np.zeros(3, np.int32)
    assert grp(sel=bits.ctypes.data, nbits=599) == -1 and grp(sel=bits.ctypes.data, nbits=640, bit0=41) == -1   # what mips_ivf_search_grp refuses
    assert grp(sel=bits.ctypes.data, nbits=640, bit0=-1) == -1 and grp(sel=bits.ctypes.data, nbits=640, bit0=40) == 0
    assert grp(lab=ql.ctypes.data) == -1 and b"label" in lib.mips_last_error()                         # no labels yet
    ix.set_labels(np.arange(600, dtype=np.int32) // 8)
    assert grp(lab=ql.ctypes.data) == 0 and grp(lab=ql.ctypes.data, mode=2) == -1
    big = ram.IvfIndex(32, 1100, dtype="f32")                                                         # p > 1024 (MIPS_E_UNSUPPORTED)
    big.set_centroids(np.random.default_rng(1).standard_normal((1100, 32)).astype(np.float32))
    q32 = np.zeros((3, 32), np.float32)
    assert lib.mips_ivf_range_search(big._h, q32.ctypes.data, ram.DTYPE_F32, 3, radii.ctypes.data, 1025, lims.ctypes.data, od.ctypes.data, oi.ctypes.data, 2000, 0,
                                     0, None) == -3 and b"1024" in lib.mips_last_error()
    assert lib.mips_ivf_range_search(big._h, q32.ctypes.data, ram.DTYPE_F32, 3, radii.ctypes.data, 1024, lims.ctypes.data, od.ctypes.data, oi.ctypes.data, 2000, 0,
                                     0, None) == 0 and (lims == 0).all()                              # ... and at it, on an empty index
    with pytest.raises(ValueError, match="group_mode"):
        ix.range_search_probed(x["q"], 0.0, 1, groups=ql, group_mode="without")
    with pytest.raises(NotImplementedError, match="search_probed"):                                  # the faiss-shaped form stays refused
        ix.range_search(x["q"], 0.0)
    cen = ix.centroids()                                                                             # afterwards the index answers as before
    assign = iv.nearest(x["rows"], cen)[:, 0]
    _same(ix.range_search_probed(x["q"], 2.0, 5), rc.range_search(x["rows"], x["q"], assign, cen, 2.0, 5, "f32"))
    d, i = ix.search_probed(x["q"], 29, 5)
    want = sc.search(x["rows"], x["q"], assign, cen, 29, 5, "f32")
    assert np.array_equal(i, want[1]) and np.array_equal(d.view(np.uint32), want[0].view(np.uint32))


# ------------------------------------------------------------------ the C ABI from plain C
def test_c_abi_ivf_range_from_plain_c(tmp_path):
    ram = _ram()
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_ivf_range_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_ivf_range_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
