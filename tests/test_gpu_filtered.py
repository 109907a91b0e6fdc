"""Filtered search (mips_search_wide_sel / mips_range_search_sel; selector= on MipsIndex, ShardedMipsIndex, faiss_shim and
KnowledgeBase): a selector restricts a wide top-k or a range search to a row subset.  Wide expectations are the oracle's FULL
ranking (orc.search_exact_bruteforce with k = n) with the unselected ids removed, cut to k and padded; range expectations are the
all-pairs recipe of tests/test_gpu_range.py (orc.canonical_pairs / orc.sumsq_canonical, strict float32 rule; phi over ALL rows)
AND-ed with the mask.  Everything is compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth
from retrieval_augmented_mds_amd.mips import KnowledgeBase

pytestmark = pytest.mark.gpu

MASKED = "mips::masked_scan_kernel"
TILE = 128


# ------------------------------------------------------------------ expectations
def _filter_ranking(full, mask, k, metric, idx_offset=0):
    """full = (scores, ids) [nq, n], the oracle's ranking of ALL rows -> the k best selected rows per query, padded."""
    fs, fi = full
    nq = fs.shape[0]
    s = np.full((nq, k), np.inf if metric else -np.inf, np.float32)
    i = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        keep = np.flatnonzero(mask[fi[j]])[:k]
        s[j, :len(keep)] = fs[j, keep]
        i[j, :len(keep)] = fi[j, keep] + idx_offset
    return s, i


def _same(got, exp, what=""):
    s, i = got
    es, ei = exp
    if isinstance(s, torch.Tensor):
        s, i = s.cpu().numpy(), i.cpu().numpy()
    bad = np.flatnonzero((i != ei).any(axis=1))
    assert np.array_equal(i, ei), f"{what}: indices differ in {len(bad)} queries, first {bad[:5]}"
    assert np.array_equal(s.view(np.int32), es.view(np.int32)), f"{what}: scores differ"


def _unpack(packed):
    s, i = ram.unpack_gathered(packed[None], 1)
    return s.cpu().numpy(), i.cpu().numpy()


def _tile_counts(mask):
    pad = np.zeros(-len(mask) % TILE, bool)
    return np.concatenate([mask, pad]).reshape(-1, TILE).sum(axis=1)


def _random_mask(n, density, seed, sparse_tiles=False):
    """A Bernoulli mask; sparse_tiles: the first seed (counting up) whose mask leaves one 128-row tile empty and one with one row."""
    for s in range(seed, seed + 1000):
        mask = np.random.default_rng(s).random(n) < density
        c = _tile_counts(mask)
        if not sparse_tiles or ((c == 0).any() and (c == 1).any()):
            return mask
    raise AssertionError("no such mask")


_CASES = {}


def _gauss_case(n, nq, d, metric):
    """Gaussian bf16 inputs and the oracle's full ranking: computed once per shape and metric, shared, never modified."""
    key = (n, nq, d, metric)
    if key not in _CASES:
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
        _CASES[key] = (x, q, orc.search_exact_bruteforce(q, x, n, metric=metric))
    return _CASES[key]


def _selectors(n):
    lone = np.zeros(n, bool)
    lone[n - 1] = True
    span = np.zeros(n, bool)
    span[131:min(n, 2900)] = True
    return {"half": _random_mask(n, 0.5, 1), "sparse": _random_mask(n, 1 / 64, 2, sparse_tiles=True), "span": span, "last row": lone,
            "ones": np.ones(n, bool), "zeros": np.zeros(n, bool)}


# ------------------------------------------------------------------ 1. Gaussian bf16, both metrics
@pytest.mark.parametrize("n,nq,d,k", [(4099, 129, 1024, 100), (777, 5, 100, 64), (9001, 70, 256, 5)])
@pytest.mark.parametrize("metric", [0, 1])
def test_gaussian_bf16_matches_filtered_oracle(n, nq, d, k, metric):
    x, q, full = _gauss_case(n, nq, d, metric)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    plain = ix.search_wide(q, k)
    assert ix.last_kernel.startswith("mips::wide_scan_kernel")
    sels = _selectors(n)
    c = _tile_counts(sels["sparse"])
    assert (c == 0).any() and (c == 1).any()                       # both empty and nearly empty tiles are scanned
    for name, mask in sels.items():
        got = ix.search_wide(q, k, selector=ram.Selector.from_mask(mask))
        st = ix.margin_stats()
        print(f"n={n} nq={nq} d={d} k={k} metric={metric} {name} ({int(mask.sum())} rows): {st}")
        assert ix.last_kernel == MASKED
        assert st["unresolved"] == 0 and st["flagged"] == st["rescanned"] >= 0
        _same(got, _filter_ranking(full, mask, k, metric), name)
        if name == "ones":
            _same(got, plain, "all ones against the unfiltered search")
        if name == "zeros":
            assert (got[1] == -1).all()
    ix.search_wide(q, k, selector=None)
    assert ix.last_kernel.startswith("mips::wide_scan_kernel")


# ------------------------------------------------------------------ 2. fewer selected rows than k
@pytest.mark.parametrize("metric", [0, 1])
def test_fewer_selected_rows_than_k_pads(metric):
    n, nq, d, k = 9001, 70, 256, 64
    x, q, full = _gauss_case(n, nq, d, metric)
    mask = np.zeros(n, bool)
    mask[np.random.default_rng(5).choice(n, 50, replace=False)] = True
    exp = _filter_ranking(full, mask, k, metric, idx_offset=1 << 33)
    assert (exp[1][:, 50:] == -1).all() and (exp[1][:, :50] >= 1 << 33).all()
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    sel = ram.Selector.from_mask(mask)
    _same(ix.search_wide(q, k, idx_offset=1 << 33, selector=sel), exp, "padding")
    assert ix.margin_stats()["unresolved"] == 0
    qd = torch.from_numpy(q).cuda()
    _same(_unpack(ix.search_wide_packed(qd, k, idx_offset=1 << 33, selector=sel)), exp, "packed padding")
    if metric == 1:
        _same(ix.search_wide(q, k, force_ip=True, selector=sel), _filter_ranking(_gauss_case(n, nq, d, 0)[2], mask, k, 0), "force_ip")


# ------------------------------------------------------------------ 3. a pool that holds the whole selection is certified
def test_selection_that_fits_in_the_pool_is_certified_outright():
    """120 selected rows: more than k = 100, fewer than the pool's k' = k + 64 = 164.  The pool ends up holding every selected row,
    so nothing outside it can be a result and no query may be flagged -- whatever the scores are (no data-dependent margin)."""
    n, nq, d, k = 9001, 70, 256, 100
    x, q, full = _gauss_case(n, nq, d, 0)
    mask = np.zeros(n, bool)
    mask[np.random.default_rng(6).choice(n, 120, replace=False)] = True
    ix = ram.MipsIndex(d)
    ix.add(x)
    got = ix.search_wide(q, k, selector=mask)
    st = ix.margin_stats()
    print(st)
    assert st == {"flagged": 0, "rescanned": 0, "unresolved": 0}
    _same(got, _filter_ranking(full, mask, k, 0), "120 selected rows")


# ------------------------------------------------------------------ 4. fp32-exact index
@pytest.mark.parametrize("metric", [0, 1])
def test_f32_exact_index(metric):
    rng = np.random.default_rng(31)
    n, nq, d = 6000, 24, 768
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    full = orc.search_exact_bruteforce(q, x, n, metric=metric)
    mask = _random_mask(n, 0.5, 3)
    ix = ram.MipsIndex(d, metric=metric, dtype="f32")
    ix.add(x)
    sel = ram.Selector.from_mask(mask)
    for k in (5, 100):
        got = ix.search_wide(q, k, selector=sel)
        st = ix.margin_stats()
        print(f"f32 k={k} metric={metric}: {st}")
        assert st["unresolved"] == 0 and ix.last_kernel == MASKED
        _same(got, _filter_ranking(full, mask, k, metric), f"f32 k={k}")


# ------------------------------------------------------------------ 5. ties
def test_lattice_ties_lowest_selected_row_wins():
    x = synth.generate(1, 0, 5000, 128, synth.KIND_LATTICE)
    q = synth.generate(2, 0, 19, 128, synth.KIND_LATTICE)
    full = orc.search_exact_bruteforce(q, x, 5000)
    mask = _random_mask(5000, 0.5, 4)
    ix = ram.MipsIndex(128)
    ix.add(x)
    for k in (30, 200):
        exp = _filter_ranking(full, mask, k, 0)
        assert k < 200 or (np.diff(exp[0], axis=1) == 0).sum() > 0    # tied scores inside the results: their order is by row
        _same(ix.search_wide(q, k, selector=mask), exp, f"lattice k={k}")
        assert ix.margin_stats()["unresolved"] == 0


# ------------------------------------------------------------------ 6. the settlement must not bring back excluded rows
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_excluded_near_duplicates_stay_excluded_when_queries_are_settled(dtype):
    """The construction of test_gpu_wide_k.py::test_near_duplicates_across_the_kth_place_are_flagged_and_settled with M = 400 / 600
    copies of the star row, of which the selector clears the 100 highest-scoring ones (the highest rows).  The selected copies are
    then exactly that test's 300 / 500 and its argument carries over: the pool (k' = 164 / 381) cannot hold them all and those it
    leaves out lie within the scan's error bound of the k-th result, so the star queries are flagged and settled by brute force --
    which scores EVERY row, the cleared copies (all better than any result) included, and must not append them."""
    rng = np.random.default_rng(11)
    n, d, nq, k = 20000, 768, 16, 100
    M = 400 if dtype == "bf16" else 600
    x = synth.round_to_bf16(rng.standard_normal((n, d)).astype(np.float32))
    q = synth.round_to_bf16(rng.standard_normal((nq, d)).astype(np.float32))
    v = synth.round_to_bf16(rng.standard_normal(d).astype(np.float32))
    rows = 1003 + 16 * np.arange(M)
    x[rows] = v
    x[rows, 5] = (np.arange(M) % 16).astype(np.float32)
    x[rows, 9] = (np.arange(M) // 16).astype(np.float32)
    star = v.copy()
    star[5] = 2.0 ** -12
    star[9] = 2.0 ** -8
    stars = np.arange(0, nq, 8)
    q[stars] = star
    full = orc.search_exact_bruteforce(q, x, n)
    cleared = rows[M - 100:]
    assert np.array_equal(np.sort(full[1][stars[0], :100]), cleared)                 # (the construction does what it says: the
    mask = np.ones(n, bool)                                                          # cleared copies are the unfiltered top 100,
    mask[cleared] = False                                                            # the filtered one the next 100 copies)
    exp = _filter_ranking(full, mask, k, 0)
    assert np.array_equal(np.sort(exp[1][stars[0]]), rows[M - 200:M - 100])
    ix = ram.MipsIndex(d, dtype=dtype)
    ix.add(x)
    sel = ram.Selector.from_mask(mask)
    for queries in (q, torch.from_numpy(q).cuda()):                                  # host-output and stream-ordered form
        got = ix.search_wide(queries, k, selector=sel)
        st = ix.margin_stats()
        print(dtype, type(queries).__name__, st)
        assert st["flagged"] > 0 and st["rescanned"] == st["flagged"] and st["unresolved"] == 0
        ids = got[1].cpu().numpy() if isinstance(got[1], torch.Tensor) else got[1]
        assert not np.isin(ids, cleared).any(), "a cleared row came back"
        _same(got, exp, "flood")


# ------------------------------------------------------------------ 7. sel_bit0: row shards read a global selector
@pytest.mark.parametrize("metric", [0, 1])
def test_shards_read_the_global_selector_from_their_first_row(metric):
    n, nq, d, k = 9001, 70, 256, 64
    x, q, full = _gauss_case(n, nq, d, metric)
    mask = _random_mask(n, 0.5, 8)
    sel = ram.Selector.from_mask(mask)
    whole = ram.MipsIndex(d, metric=metric)
    whole.add(x)
    exp = _filter_ranking(full, mask, k, metric)
    _same(whole.search_wide(q, k, selector=sel), exp, "unsharded")
    qd = torch.from_numpy(q).cuda()
    bounds = [0, 2999, 6003, n]                                                      # ragged, no bound a multiple of 8
    assert all(b % 8 for b in bounds[1:])
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        shard = ram.MipsIndex(d, metric=metric)
        shard.add(x[lo:hi])
        if metric == 1:
            shard.set_phi(whole.phi())
        parts.append(shard.search_wide_packed(qd, k, lo, selector=sel, sel_bit0=lo))
        assert shard.last_kernel == MASKED and shard.margin_stats()["unresolved"] == 0
    merged = ram.merge_topk_sorted_packed(torch.cat(parts), nq, len(parts), k, metric)
    _same(merged, exp, "three shards merged")


# ------------------------------------------------------------------ 8. more than one query slice
def test_more_queries_than_one_slice():
    n, nq, d, k = 3000, 4100, 64, 40
    x = synth.generate(3, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(4, 0, nq, d, synth.KIND_GAUSS)
    mask = _random_mask(n, 0.5, 9)
    ix = ram.MipsIndex(d)
    ix.add(x)
    got = ix.search_wide(q, k, selector=mask)
    assert ix.margin_stats()["unresolved"] == 0
    # the ranking's first 400 places (a full one costs n^2 per query): they hold k selected rows for every query -- asserted --
    # so removing the unselected ids and cutting to k gives what the full ranking gives
    head = orc.search_exact_bruteforce(q, x, 400)
    assert (mask[head[1]].sum(axis=1) >= k).all()
    _same(got, _filter_ranking(head, mask, k, 0), "4100 queries")


# ------------------------------------------------------------------ 9. range search
def _values(q, x, metric):
    """float32 canonical output value of every (query, row) pair: the inner product, or |q|^2 + phi - 2 q.x (metric 1)."""
    n = x.shape[0]
    dot = orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1)))
    if metric == 1:
        phi = orc.sumsq_canonical(x).max()
        return (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * dot).astype(np.float32)
    return dot.astype(np.float32)


def _boundary_radii(vals, metric):
    """A third of the queries get the exact float32 score of one of their own rows (that row and its ties are out), a third the
    nextafter of such a score towards the permissive side (they are in), the rest run from "nothing" to "every row", +-inf
    included.  `vals` [nq, n] float32."""
    nq, n = vals.shape
    permissive = np.float32(np.inf if metric == 1 else -np.inf)
    r = np.empty(nq, np.float32)
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


def _expected_range(vals, r, metric, mask, idx_offset=0):
    lims, D, I = [0], [], []
    for j in range(vals.shape[0]):
        ids = np.flatnonzero((vals[j] < r[j] if metric == 1 else vals[j] > r[j]) & mask)
        lims.append(lims[-1] + len(ids))
        D.append(vals[j][ids])
        I.append(ids + idx_offset)
    return np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def _same_range(got, exp, what=""):
    lims, D, I = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in got)
    el, eD, eI = exp
    assert lims.shape == el.shape and lims[0] == 0
    for j in range(len(el) - 1):
        a, b = int(lims[j]), int(lims[j + 1])
        ea, eb = int(el[j]), int(el[j + 1])
        assert b - a == eb - ea, f"{what}: query {j} has {b - a} hits, expected {eb - ea}"
        assert np.array_equal(I[a:b], eI[ea:eb]), f"{what}: ids of query {j} differ"
        assert np.array_equal(D[a:b], eD[ea:eb]), f"{what}: scores of query {j} differ"
    assert np.array_equal(lims.astype(np.int64), el) and len(D) == len(I) == el[-1]


@pytest.mark.parametrize("n,nq,d", [(4099, 129, 1024), (777, 5, 100)])
@pytest.mark.parametrize("metric", [0, 1])
def test_range_search_matches_masked_all_pairs(n, nq, d, metric):
    x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
    vals = _values(q, x, metric)
    r = _boundary_radii(vals, metric)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    for name, mask in (("half", _random_mask(n, 0.5, 1)), ("sparse", _random_mask(n, 1 / 64, 2, sparse_tiles=True))):
        sel = ram.Selector.from_mask(mask)
        exp = _expected_range(vals, r, metric, mask)
        got = ix.range_search(q, r, selector=sel)
        print(f"n={n} nq={nq} d={d} metric={metric} {name}: {exp[0][-1]} hits")
        _same_range(got, exp, name)
        assert ix.last_kernel == MASKED
        assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}
        # cap = 0: a counting call; its counts are the true ones
        qd = torch.from_numpy(q).cuda()
        lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        none_s, none_i = torch.empty(0, dtype=torch.float32, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda")
        ix.range_search_into(qd, r, lims, none_s, none_i, selector=sel)
        assert np.array_equal(lims.cpu().numpy(), exp[0])
        # the non-synchronising form with CUDA tensors, ids offset
        D = torch.empty(int(exp[0][-1]) + 3, dtype=torch.float32, device="cuda")
        I = torch.empty(int(exp[0][-1]) + 3, dtype=torch.int64, device="cuda")
        ix.range_search_into(qd, r, lims, D, I, idx_offset=1 << 33, selector=sel)
        total = int(exp[0][-1])
        _same_range((lims, D[:total], I[:total]), _expected_range(vals, r, metric, mask, idx_offset=1 << 33), name + ", into")
    # an all-zeros selector: nothing, whatever the radius
    lims, D, I = ix.range_search(q, r, selector=np.zeros(n, bool))
    assert (lims == 0).all() and len(D) == len(I) == 0
    if metric == 0:                                                # r = -inf: exactly the selected rows, ascending, for every query
        mask = _random_mask(n, 0.5, 1)
        lims, D, I = ix.range_search(q, -np.inf, selector=mask)
        ids = np.flatnonzero(mask)
        assert np.array_equal(lims, len(ids) * np.arange(nq + 1)) and np.array_equal(I, np.tile(ids, nq))
    ix.range_search(q, r)
    assert ix.last_kernel.startswith("mips::wide_scan_kernel")


@pytest.mark.parametrize("metric", [0, 1])
def test_range_search_f32_exact_index(metric):
    rng = np.random.default_rng(32)
    n, nq, d = 6000, 24, 768
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    vals = _values(q, x, metric)
    r = _boundary_radii(vals, metric)
    mask = _random_mask(n, 0.5, 3)
    ix = ram.MipsIndex(d, metric=metric, dtype="f32")
    ix.add(x)
    _same_range(ix.range_search(q, r, selector=mask), _expected_range(vals, r, metric, mask), "f32")
    assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}


# ------------------------------------------------------------------ 10. device and host bitmap, a selector used twice
def test_device_and_host_bitmap_agree_and_a_selector_is_reusable():
    n, nq, d, k = 9001, 70, 256, 64
    x, q, full = _gauss_case(n, nq, d, 0)
    mask = _random_mask(n, 1 / 64, 2, sparse_tiles=True)
    sel = ram.Selector.from_mask(mask)
    assert sel.bits.is_cuda and sel.bits.dtype == torch.uint8 and sel.nbits == n
    host = np.packbits(mask, bitorder="little")
    assert np.array_equal(sel.numpy(), host)
    ix = ram.MipsIndex(d)
    ix.add(x)
    exp = _filter_ranking(full, mask, k, 0)
    first = ix.search_wide(q, k, selector=sel)
    _same(first, exp, "device bitmap")
    _same(ix.search_wide(q, k, selector=host), exp, "host bitmap")
    _same(ix.search_wide(torch.from_numpy(q).cuda(), k, selector=host), exp, "host bitmap, device queries")
    _same(ix.search_wide(q, k, selector=sel), first, "the same selector again")
    _same(ix.search_wide(q, k, selector=torch.from_numpy(mask).cuda()), exp, "bool tensor")
    _same(ix.search_wide(q, k, selector=sel.invert().invert()), exp, "inverted twice")
    a = ix.range_search(q, 40.0, selector=sel)
    b = ix.range_search(q, 40.0, selector=host)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[0][-1] > 0


# ------------------------------------------------------------------ 11. plain C
def test_c_abi_sel_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_sel_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_sel_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


# ------------------------------------------------------------------ 12. drop-in surfaces
def test_faiss_shim_selectors_and_knowledge_base():
    n, nq, d, k = 9001, 70, 256, 5
    x, q, full = _gauss_case(n, nq, d, 0)
    fs = ram.faiss_shim
    fx = fs.IndexFlat(d, fs.METRIC_INNER_PRODUCT, dtype="bf16")
    fx.add(x)
    mask = _random_mask(n, 0.5, 12)
    ids = np.flatnonzero(mask)
    span = (np.arange(n) >= 131) & (np.arange(n) < 2900)
    vals = _values(q, x, 0)
    r = _boundary_radii(vals, 0)
    for name, sel, m in (("range", fs.IDSelectorRange(131, 2900), span), ("batch", fs.IDSelectorBatch(ids), mask),
                         ("array", fs.IDSelectorArray(ids), mask), ("bitmap", fs.IDSelectorBitmap(np.packbits(mask, bitorder="little")), mask),
                         ("not", fs.IDSelectorNot(fs.IDSelectorBatch(ids)), ~mask)):
        params = fs.SearchParameters(sel=sel)
        for kk in (k, 100):
            _same(fx.search(q, kk, params=params), _filter_ranking(full, m, kk, 0), f"faiss_shim search, {name}")
        lims, D, I = fx.range_search(q, r, params=params)
        assert lims.dtype == np.uint64
        _same_range((lims.astype(np.int64), D, I), _expected_range(vals, r, 0, m), f"faiss_shim range_search, {name}")
    _same(fx.search(q, k, params=None), (full[0][:, :k], full[1][:, :k]), "params=None")
    with pytest.raises(TypeError):
        fx.search(q, k, sel=fs.IDSelectorRange(0, 5))
    with pytest.raises(TypeError):
        fx.range_search(q, r, sel=fs.IDSelectorRange(0, 5))
    kb = KnowledgeBase({"emb": x, "row": np.arange(n)})
    kb.add_faiss_index("emb", metric_type=0, dtype="bf16")
    scores, examples = kb.get_nearest_examples_batch("emb", q, k, selector=ram.Selector.from_mask(mask))
    exp = _filter_ranking(full, mask, k, 0)
    for j in range(nq):
        assert np.array_equal(np.asarray(scores[j]), exp[0][j]) and np.array_equal(np.asarray(examples[j]["row"]), exp[1][j])


# ------------------------------------------------------------------ 13. the sharded facade
def _rank_worker(rank, world, port, n, nq, d, k, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        rng = np.random.default_rng(3)
        x = synth.round_to_bf16((synth.generate(151, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
        qn = synth.round_to_bf16(synth.generate(152, 0, nq, d, synth.KIND_GAUSS))
        qd = torch.from_numpy(qn).cuda()
        mask = _random_mask(n, 0.5, 13)
        sel = ram.Selector.from_mask(mask)
        ok = True
        for metric in (0, 1):
            ix = ram.ShardedMipsIndex(d, metric=metric, device=0)
            ix.add_global(x)
            exp = _filter_ranking(orc.search_exact_bruteforce(qn, x, n, metric=metric), mask, k, metric)
            s, i = ix.search_wide(qd, k, selector=sel)                      # device fast path
            ok &= s.is_cuda and bool(np.array_equal(i.cpu().numpy(), exp[1]) and np.array_equal(s.cpu().numpy(), exp[0]))
            ok &= ix.margin_stats()["unresolved"] == 0 and ix.local.last_kernel == MASKED
            s, i = ix.search_wide(qn, k, selector=mask)                     # generic path: NumPy in, NumPy out, a bare mask
            ok &= isinstance(s, np.ndarray) and bool(np.array_equal(i, exp[1]) and np.array_equal(s, exp[0]))
            s, i = ram.index.route_search(ix, qd, 5, selector=sel)          # search() with a selector routes to the wide search
            ok &= bool(np.array_equal(i.cpu().numpy(), exp[1][:, :5]) and np.array_equal(s.cpu().numpy(), exp[0][:, :5]))
            s, i = ix.search(qd, 5, selector=sel)
            ok &= bool(np.array_equal(i.cpu().numpy(), exp[1][:, :5]))
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_sharded_search_wide_with_a_global_selector(tmp_path):
    """Two row shards on processes sharing cuda:0 (the worker of test_gpu_wide_sharded.py): the selector is global and replicated,
    each shard reads it from its first row on; equal to the filtered oracle on the unsharded index, both metrics."""
    import torch.multiprocessing as mp

    world, n, k = 2, 20001, 100
    port = 29300 + (os.getpid() % 2000)
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, n, 50, 256, k, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


# ------------------------------------------------------------------ 14. refusals
def test_refusals():
    d = 64
    x = synth.generate(3, 0, 300, d, synth.KIND_GAUSS)
    q = np.zeros((2, d), np.float32)
    ix = ram.MipsIndex(d)
    ix.add(x)
    sel = ram.Selector.from_mask(np.ones(300, bool))
    with pytest.raises(NotImplementedError):
        ix.search_wide(q, ram.MAX_K_WIDE + 1, selector=sel)
    with pytest.raises(ValueError):                                             # nbits too small
        ix.search_wide(q, 40, selector=ram.Selector.from_mask(np.ones(299, bool)))
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, selector=sel, sel_bit0=1)
    with pytest.raises(ValueError):
        ix.search_wide(q, 40, selector=sel, sel_bit0=-1)
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, selector=np.ones(299, bool))
    for dtype in ("fp8_e4m3", "fp8_e4m3_docs"):
        f8 = ram.MipsIndex(d, dtype=dtype)
        f8.add(x)
        with pytest.raises(NotImplementedError):
            f8.search_wide(q, 40, selector=sel)
        with pytest.raises(NotImplementedError):
            f8.range_search(q, 0.0, selector=sel)
    wide = ram.MipsIndex(1100)
    wide.add(synth.generate(3, 0, 300, 1100, synth.KIND_GAUSS))
    with pytest.raises(NotImplementedError):
        wide.search_wide(np.zeros((2, 1100), np.float32), 40, selector=sel)
    # the C ABI itself: the same refusals, by return code
    import ctypes

    lib = ram._lib.load()
    bits = sel.bits
    out_s = torch.empty((2, 40), dtype=torch.float32, device="cuda")
    out_i = torch.empty((2, 40), dtype=torch.int64, device="cuda")
    qd = torch.from_numpy(q).cuda()
    dev = ram._lib.Q_DEVICE | ram._lib.OUT_DEVICE | ram._lib.SEL_DEVICE

    def wide_rc(index, k, nbits, bit0):
        return lib.mips_search_wide_sel(index._h, qd.data_ptr(), ram._lib.DTYPE_F32, 2, k, out_s.data_ptr(), out_i.data_ptr(), 0, dev,
                                        bits.data_ptr(), nbits, bit0, None)

    assert wide_rc(ix, 40, 300, 0) == 0
    assert wide_rc(ix, 40, 299, 0) == -1 and b"selector" in lib.mips_last_error()          # MIPS_E_INVALID
    assert wide_rc(ix, 40, 300, 1) == -1 and wide_rc(ix, 40, 300, -1) == -1
    assert wide_rc(ix, ram.MAX_K_WIDE + 1, 300, 0) == -3 and wide_rc(f8, 40, 300, 0) == -3 and wide_rc(wide, 40, 300, 0) == -3   # MIPS_E_UNSUPPORTED
    lims = torch.empty(3, dtype=torch.int64, device="cuda")
    radii = np.zeros(2, np.float32)

    def range_rc(flags, nbits, bit0):
        return lib.mips_range_search_sel(ix._h, qd.data_ptr(), ram._lib.DTYPE_F32, 2, radii.ctypes.data, lims.data_ptr(), None, None, 0, 0, flags,
                                         bits.data_ptr(), nbits, bit0, None)

    assert range_rc(dev, 300, 0) == 0
    assert range_rc(dev | ram._lib.OUT_PACKED, 300, 0) == -1                                  # MIPS_OUT_PACKED on the range call
    assert range_rc(dev, 299, 0) == -1 and range_rc(dev, 300, -1) == -1
    torch.cuda.synchronize()
