"""The filtered IVF search on the GPU (mips_ivf_search_sel / _grp, IvfIndex.search_probed(selector=, groups=, group_mode=)): everything
bit for bit against the NumPy restatement of tests/ivf_filter_cases.py, on all three storages, no tolerance anywhere.

Cases: the planted lists (an empty list, a list of one row, a group that covers a whole list) under a bitmap, under groups in both
modes and under both, at nprobe 1, 2, 3, 8 and k 1, 5, 29, with host and CUDA inputs and idx_offset; ties under a bitmap; the queue
case, whose bitmaps leave exactly 0, 1, 63, 64, 65, 127, 128 and 129 rows in one wave's stretch of a 20 000-row list (the compacting
queue of the list scan: empty, one pass less one, exactly one pass, one pass and a remainder, two passes ...), searched as 32 segments
(one query) and as one segment (512 queries); a mixed batch with LABEL_NONE; nothing admitted; fewer than k admitted; the three
identities of the definition; the index as it changes; the refusals of the C ABI by return code; Gaussian rows at d = 1, 64, 768, 1024."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_cases as iv  # noqa: E402
import ivf_filter_cases as fc  # noqa: E402
import ivf_search_cases as sc  # noqa: E402

STORAGES = sc.STORAGES
NONE = fc.LABEL_NONE


def _ram():
    import retrieval_augmented_mds_amd as ram

    return ram


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _same(got, want):
    gd, gi = _np(got[0]), _np(got[1])
    assert np.array_equal(gi, want[1]), (gi, want[1])
    assert np.array_equal(gd.view(np.uint32), want[0].view(np.uint32))


def _bitmap(mask):
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


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
    if labels is not None:
        ix.set_labels(labels)
    return ix, par


_cache = {}


def planted(dtype):
    if ("planted", dtype) not in _cache:
        c = fc.case_planted(40)
        ix, par = _plant(c, dtype, labels=c["row_labels"])
        assert np.array_equal(ix.assignments(), c["assign"])
        _cache[("planted", dtype)] = (c, ix, par)
    return _cache[("planted", dtype)]


# ------------------------------------------------------------------ planted lists: bitmap alone, groups alone, both
@pytest.mark.parametrize("dtype", STORAGES)
def test_planted_lists_under_every_filter(dtype):
    ram = _ram()
    c, ix, par = planted(dtype)
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    q, ql, lab = c["q"], c["q_labels"], c["row_labels"]
    sel = ram.Selector.from_mask(c["sel"])
    for nprobe in (1, 2, 3, 8):
        for k in (1, 5, 29):
            _same(ix.search_probed(q, k, nprobe, selector=_bitmap(c["sel"])), fc.search(*base, k, nprobe, dtype, par, sel=c["sel"]))      # host bitmap
            for mode in ("exclude", "only"):
                want = fc.search(*base, k, nprobe, dtype, par, labels=lab, q_labels=ql, mode=mode)
                _same(ix.search_probed(q, k, nprobe, groups=ql, group_mode=mode), want)                                                  # host labels
                both = fc.search(*base, k, nprobe, dtype, par, sel=c["sel"], labels=lab, q_labels=ql, mode=mode)
                _same(ix.search_probed(q, k, nprobe, selector=sel, groups=ql, group_mode=mode), both)                                    # Selector + host labels
        got = ix.search_probed(_dev(q), 29, nprobe, selector=sel, groups=_dev(ql), group_mode="only")                                    # everything on the device
        assert got[0].is_cuda and got[1].is_cuda
        _same(got, both)
    # bit sel_bit0 + i decides row i; idx_offset is added to the rows
    off = fc.search(*base, 5, 2, dtype, par, sel=c["sel_off"], sel_bit0=13, labels=lab, q_labels=ql, idx_offset=1 << 40)
    _same(ix.search_probed(q, 5, 2, idx_offset=1 << 40, selector=_bitmap(c["sel_off"]), sel_bit0=13, groups=ql), off)
    _same(ix.search_probed(_dev(q), 5, 2, idx_offset=1 << 40, selector=ram.Selector.from_mask(c["sel_off"]), sel_bit0=13, groups=_dev(ql)), off)
    ids = np.flatnonzero(c["sel"])                                                                                                     # a list of row ids
    _same(ix.search_probed(q, 5, 3, selector=[int(i) for i in ids]), fc.search(*base, 5, 3, dtype, par, sel=c["sel"]))


@pytest.mark.parametrize("dtype", STORAGES)
def test_mixed_batch_none_excluded_all_and_short(dtype):
    c, ix, par = planted(dtype)
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    q, ql = c["q"], c["q_labels"]
    none = ql == NONE
    assert none.any() and not none.all()
    plain = ix.search_probed(q, 5, 2)
    for mode in ("exclude", "only"):
        d, i = ix.search_probed(q, 5, 2, groups=ql, group_mode=mode)
        assert np.array_equal(i[none], plain[1][none]) and np.array_equal(d[none].view(np.uint32), plain[0][none].view(np.uint32))
    _same(ix.search_probed(q, 5, 2, groups=np.full(len(q), NONE, np.int32), group_mode="only"), plain)    # no query filtered at all
    # nothing admitted: padding only
    n = len(c["rows"])
    d, i = ix.search_probed(q, 5, 3, selector=_bitmap(np.zeros(n, bool)))
    assert (i == -1).all() and np.isneginf(d).all()
    d, i = ix.search_probed(_dev(q), 5, 3, groups=_dev(np.full(len(q), 77777, np.int32)), group_mode="only")   # a label no row has
    assert (_np(i) == -1).all() and np.isneginf(_np(d)).all()
    # fewer than k admitted: the admitted rows, padding last
    three = np.zeros(n, bool)
    three[np.flatnonzero(c["assign"] == 1)[[0, 700, 2499]]] = True
    d, i = ix.search_probed(q, 5, 8, selector=_bitmap(three))
    _same((d, i), fc.search(*base, 5, 8, dtype, par, sel=three))
    assert ((i >= 0).sum(axis=1) == 3).all() and (i[:, 3:] == -1).all() and np.isneginf(d[:, 3:]).all()
    # a group that covers a whole list
    five = (c["qlabels"] == 5) & ~none
    d, i = ix.search_probed(q, 29, 1, groups=ql)
    assert five.any() and (i[five] == -1).all()


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("dtype", STORAGES)
def test_ties_under_a_bitmap(dtype):
    c = fc.case_ties()
    ix, par = _plant(c, dtype, assign=c["assign"], labels=c["row_labels"])
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    d, i = ix.search_probed(c["q"], 29, 3, selector=_bitmap(c["sel"]))
    assert np.array_equal(i[0], c["admitted_copies"][:29]) and (d[0] == d[0, 0]).all()                 # the lowest admitted copies, ascending
    _same((d, i), fc.search(*base, 29, 3, dtype, par, sel=c["sel"]))
    for mode in ("exclude", "only"):                                                                  # copies of group 2 out / alone
        ql = np.array([2], np.int32)
        want = fc.search(*base, 29, 3, dtype, par, sel=c["sel"], labels=c["row_labels"], q_labels=ql, mode=mode)
        _same(ix.search_probed(c["q"], 29, 3, selector=_bitmap(c["sel"]), groups=ql, group_mode=mode), want)


# ------------------------------------------------------------------ the compacting queue
@pytest.mark.parametrize("dtype", STORAGES)
def test_queue_case(dtype):
    import torch

    ram = _ram()
    c = fc.case_queue()
    ix, par = _plant(c, dtype, assign=c["assign"], labels=c["row_labels"])
    assert ix.list_sizes()[0] == fc.QUEUE_BIG and (ix.probe(c["q"], 1) == 0).all()
    base = (c["rows"], c["q"], c["assign"], c["centroids"])
    one = (c["rows"], c["q"][:1], c["assign"], c["centroids"])
    qd = _dev(c["q"])
    for name, m in c["bitmaps"].items():
        sel = ram.Selector.from_mask(m)
        _same(ix.search_probed(qd[:1], 5, 1, selector=sel), fc.search(*one, 5, 1, dtype, par, sel=m))          # 32 segments
        _same(ix.search_probed(qd, 5, 1, selector=sel), fc.search(*base, 5, 1, dtype, par, sel=m))            # one segment per workgroup
    m = c["bitmaps"]["c129"]
    ql = np.full(512, NONE, np.int32)
    ql[::2] = c["row_labels"][np.flatnonzero(m)[5]]                                                    # every other query loses one group of 8
    want = fc.search(*base, 29, 1, dtype, par, sel=m, labels=c["row_labels"], q_labels=ql)
    _same(ix.search_probed(qd, 29, 1, selector=ram.Selector.from_mask(m), groups=torch.from_numpy(ql).cuda()), want)
    gone = np.flatnonzero(m)[5]
    assert gone not in want[1][0::2] and (want[1] >= 0).all()


# ------------------------------------------------------------------ the three identities of the definition
@pytest.mark.parametrize("dtype", STORAGES)
def test_identities(dtype):
    ram = _ram()
    case = iv.case_gauss(3000, 64, 9, 16)
    ix = ram.IvfIndex(64, 16, dtype=dtype)
    ix.niter = 2
    ix.train(case["rows"])
    ix.add(case["rows"])
    q = case["q"]
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 40, 3000).astype(np.int32)
    ix.set_labels(labels)
    mask = rng.random(3000) < 0.5
    ql = rng.integers(0, 40, 9).astype(np.int32)
    # (1) no filter: the call IS mips_ivf_search -- identical bits through the C entry points
    lib = ix._lib
    qc = np.ascontiguousarray(q)
    out = [(np.empty((9, 5), np.float32), np.empty((9, 5), np.int64)) for _ in range(3)]
    assert lib.mips_ivf_search(ix._h, qc.ctypes.data, ram.DTYPE_F32, 9, 5, 4, out[0][0].ctypes.data, out[0][1].ctypes.data, 0, 0, None) == 0
    assert lib.mips_ivf_search_grp(ix._h, qc.ctypes.data, ram.DTYPE_F32, 9, 5, 4, out[1][0].ctypes.data, out[1][1].ctypes.data, 0, 0, None, 0, 0, None, 0, None) == 0
    assert lib.mips_ivf_search_sel(ix._h, qc.ctypes.data, ram.DTYPE_F32, 9, 5, 4, out[2][0].ctypes.data, out[2][1].ctypes.data, 0, 0, None, 0, 0, None) == 0
    _same(out[1], out[0])
    _same(out[2], out[0])
    # (3) scoring I on the flat index reproduces D
    for kw in ({"selector": _bitmap(mask)}, {"groups": ql}, {"selector": _bitmap(mask), "groups": ql, "group_mode": "only"}):
        d, i = ix.search_probed(q, 5, 4, **kw)
        assert (i >= 0).any()
        again = ix.flat.compute_distance_subset(q, i)
        assert np.array_equal(again.view(np.uint32), d.view(np.uint32))
    if dtype == "sq8":
        return                                                                                         # (no wide search on SQ8 rows)
    # (2) every list probed: the flat index's wide search under the same filter, cut to k
    for kw in ({"selector": _bitmap(mask)}, {"groups": ql, "group_mode": "exclude"}, {"groups": ql, "group_mode": "only"},
               {"selector": ram.Selector.from_mask(mask), "groups": ql, "group_mode": "only"}):
        for nprobe, k in ((16, 29), (17, 5)):
            wd, wi = ix.flat.search_wide(q, 30, **kw)
            _same(ix.search_probed(q, k, nprobe, **kw), (wd[:, :k], wi[:, :k]))


# ------------------------------------------------------------------ the index as it changes
@pytest.mark.parametrize("dtype", STORAGES)
def test_after_mutation(tmp_path, dtype):
    ram = _ram()
    case = iv.case_gauss(3000, 100, 9, 8, seed=9)
    x, q = case["rows"], case["q"]
    ix = ram.IvfIndex(100, 8, dtype=dtype)
    ix.niter = 2
    ix.train(x)
    c = ix.centroids()
    par = ix.flat.sq8_params() if dtype == "sq8" else None
    assign = iv.nearest(x, c)[:, 0]
    labels = (np.arange(3000) // 8).astype(np.int32)
    ql = labels[np.arange(9) * 300 + 7].copy()
    ql[4] = NONE
    mask = np.arange(3000) % 5 != 1
    ix.add(x[:700])
    ix.set_labels(labels[:700])
    _same(ix.search_probed(q, 5, 3, groups=ql), fc.search(x[:700], q, assign[:700], c, 5, 3, dtype, par, labels=labels[:700], q_labels=ql))
    ix.add(_dev(x[700:]))
    with pytest.raises(ValueError, match="label"):
        ix.search_probed(q, 5, 3, groups=ql)                                                           # the new rows carry no label yet
    qc = np.ascontiguousarray(q)
    od, oi = np.empty((9, 5), np.float32), np.empty((9, 5), np.int64)
    assert ix._lib.mips_ivf_search_grp(ix._h, qc.ctypes.data, ram.DTYPE_F32, 9, 5, 3, od.ctypes.data, oi.ctypes.data, 0, 0, None, 0, 0,
                                       ql.ctypes.data, 0, None) == -1                                  # ... and the library says so too
    _same(ix.search_probed(q, 5, 3, selector=_bitmap(mask)), fc.search(x, q, assign, c, 5, 3, dtype, par, sel=mask))   # a bitmap needs none
    ix.set_labels(labels[700:], row0=700)
    assert np.array_equal(ix.labels(), labels) and np.array_equal(ix.labels_of(np.array([5, 2999])), labels[[5, 2999]])
    _same(ix.search_probed(q, 5, 3, selector=_bitmap(mask), groups=ql, group_mode="only"),
          fc.search(x, q, assign, c, 5, 3, dtype, par, sel=mask, labels=labels, q_labels=ql, mode="only"))
    keep = np.arange(3000) % 3 != 0
    assert ix.remove_ids(~keep) == 1000                                                                # the labels follow their rows
    _same(ix.search_probed(_dev(q), 5, 3, selector=_ram().Selector.from_mask(mask[keep]), groups=_dev(ql)),
          fc.search(x[keep], q, assign[keep], c, 5, 3, dtype, par, sel=mask[keep], labels=labels[keep], q_labels=ql))
    ix.save(str(tmp_path / "ivf"))
    iy = ram.IvfIndex.load(str(tmp_path / "ivf"))
    _same(iy.search_probed(q, 29, 2, groups=ql), fc.search(x[keep], q, assign[keep], c, 29, 2, dtype, par, labels=labels[keep], q_labels=ql))
    ix.reset()
    ix.add(x[1000:1500])
    with pytest.raises(ValueError, match="label"):
        ix.search_probed(q, 5, 2, groups=ql)                                                           # reset cleared the labels
    ix.set_labels(labels[1000:1500])
    _same(ix.search_probed(q, 29, 2, groups=ql, group_mode="only"),
          fc.search(x[1000:1500], q, assign[1000:1500], c, 29, 2, dtype, par, labels=labels[1000:1500], q_labels=ql, mode="only"))


# ------------------------------------------------------------------ refusals of the C ABI, by return code
def test_c_abi_refusals():
    ram = _ram()
    x = iv.case_gauss(300, 64, 3, 4)
    ix = ram.IvfIndex(64, 4, dtype="f32")
    lib = ix._lib
    q = np.ascontiguousarray(x["q"])
    od, oi = np.empty((3, 5), np.float32), np.empty((3, 5), np.int64)
    bits = np.full(40, 255, np.uint8)                                                                  # 320 bits
    ql = np.zeros(3, np.int32)

    def grp(k=5, nprobe=2, nq=3, sel=bits.ctypes.data, nbits=320, bit0=0, lab=ql.ctypes.data, mode=0, dt=ram.DTYPE_F32, outs=(od.ctypes.data, oi.ctypes.data)):
        return lib.mips_ivf_search_grp(ix._h, q.ctypes.data, dt, nq, k, nprobe, outs[0], outs[1], 0, 0, sel, nbits, bit0, lab, mode, None)

    assert grp() == -1 and b"not trained" in lib.mips_last_error()                                     # untrained
    ix.train(x["rows"])
    ix.add(x["rows"])
    assert grp() == -1 and b"label" in lib.mips_last_error()                                           # no labels yet
    assert grp(lab=None) == 0                                                                          # ... which a bitmap alone does not need
    ix.set_labels(np.arange(300, dtype=np.int32) // 8)
    assert grp() == 0
    assert grp(bit0=-1) == -1 and grp(bit0=21) == -1 and grp(nbits=299) == -1                           # the bitmap does not cover the rows
    assert grp(bit0=20) == 0
    assert grp(mode=2) == -1 and grp(mode=-1) == -1 and b"grp_mode" in lib.mips_last_error()
    assert grp(k=0) == -1 and grp(k=30) == -1 and grp(nprobe=0) == -1 and grp(dt=ram.DTYPE_SQ8) == -1   # what mips_ivf_search refuses
    assert grp(outs=(od.ctypes.data, None)) == -1
    assert grp(nq=0, outs=(None, None)) == 0                                                           # nq = 0
    assert lib.mips_ivf_search_sel(ix._h, q.ctypes.data, ram.DTYPE_F32, 3, 5, 2, od.ctypes.data, oi.ctypes.data, 0, 0, bits.ctypes.data, 299, 0, None) == -1
    assert lib.mips_ivf_search_sel(ix._h, q.ctypes.data, ram.DTYPE_F32, 3, 5, 2, od.ctypes.data, oi.ctypes.data, 0, 0, bits.ctypes.data, 300, 0, None) == 0
    with pytest.raises(ValueError, match="group_mode"):
        ix.search_probed(x["q"], 5, 1, groups=ql, group_mode="without")
    for name in ("search", "search_packed", "search_wide", "range_search", "search_fused"):
        with pytest.raises(NotImplementedError, match="search_probed"):
            getattr(ix, name)(x["q"], 5)                                                               # the faiss-shaped forms still raise


# ------------------------------------------------------------------ Gaussian rows
@pytest.mark.parametrize("dtype", STORAGES)
@pytest.mark.parametrize("d", [1, 64, 768, 1024])
def test_gauss(d, dtype):
    import torch

    ram = _ram()
    case = iv.case_gauss(3000, d, 9, 16)
    ix = ram.IvfIndex(d, 16, dtype=dtype)
    ix.niter = 2
    ix.train(case["rows"])
    ix.add(case["rows"])
    c = ix.centroids()
    assign = iv.nearest(case["rows"], c)[:, 0]
    par = ix.flat.sq8_params() if dtype == "sq8" else None
    rng = np.random.default_rng(d)
    labels = rng.integers(0, 25, 3000).astype(np.int32)
    ix.set_labels(_dev(labels))
    mask = rng.random(3000) < 0.25
    ql = rng.integers(0, 25, 9).astype(np.int32)
    ql[3] = NONE
    q = case["q"]
    qb = iv.synth.round_to_bf16(q)
    sel = ram.Selector.from_mask(mask)
    base = (case["rows"], q, assign, c)
    for nprobe in (1, 4, 100):
        want = fc.search(*base, 5, nprobe, dtype, par, sel=mask, labels=labels, q_labels=ql, mode="only")
        _same(ix.search_probed(q, 5, nprobe, selector=_bitmap(mask), groups=ql, group_mode="only"), want)
        _same(ix.search_probed(_dev(q), 5, nprobe, selector=sel, groups=_dev(ql), group_mode="only"), want)
        _same(ix.search_probed(_dev(q).to(torch.bfloat16), 5, nprobe, groups=_dev(ql)),
              fc.search(case["rows"], qb, assign, c, 5, nprobe, dtype, par, labels=labels, q_labels=ql))
