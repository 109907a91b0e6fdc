"""Exact range search (mips_range_search / MipsIndex.range_search): every expected set is computed here from the oracle's canonical
arithmetic on ALL pairs -- orc.canonical_pairs / orc.sumsq_canonical, the strict float32 rule -- and compared per query, ids
(ascending) and scores, exactly; no query is left out.  Radii are per query and sit on the boundary: a third of the queries get
the exact float32 score of one of their own rows (that row and its ties are out), a third the nextafter of such a score towards
the permissive side (they are in), the rest run from "nothing" through ~50 hits to "every row", +-inf included."""
import os
import subprocess

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth
from retrieval_augmented_mds_amd.mips import KnowledgeBase, augment_xb, augment_xq

pytestmark = pytest.mark.gpu


def _values(q, x, metric):
    """float32 canonical output value of every (query, row) pair: the inner product, or |q|^2 + phi - 2 q.x (metric 1)."""
    n = x.shape[0]
    dot = orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1)))
    if metric == 1:
        phi = orc.sumsq_canonical(x).max()
        return (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * dot).astype(np.float32)
    return dot.astype(np.float32)


def _boundary_radii(vals, metric):
    """See the module docstring.  `vals` [nq, n] float32."""
    nq, n = vals.shape
    permissive = np.float32(np.inf if metric == 1 else -np.inf)    # L2 admits more as the radius grows, inner product as it falls
    r = np.empty(nq, np.float32)
    for j in range(nq):
        best = np.sort(vals[j]) if metric == 1 else np.sort(vals[j])[::-1]     # best first
        own = best[(7 * j) % min(n, 60)]
        if j % 3 == 0:
            r[j] = own
        elif j % 3 == 1:
            r[j] = np.nextafter(own, permissive)
        else:
            r[j] = [best[0], best[min(n - 1, 50)], np.nextafter(best[-1], permissive), -permissive, permissive][(j // 3) % 5]
    return r


def _expected(vals, r, metric, idx_offset=0):
    lims, D, I = [0], [], []
    for j in range(vals.shape[0]):
        ids = np.flatnonzero(vals[j] < r[j] if metric == 1 else vals[j] > r[j])
        lims.append(lims[-1] + len(ids))
        D.append(vals[j][ids])
        I.append(ids + idx_offset)
    return np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def _same(got, exp, what=""):
    lims, D, I = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in got)
    el, eD, eI = exp
    assert lims.shape == el.shape and lims[0] == 0
    for j in range(len(el) - 1):                                   # per query: the first difference names its query
        a, b = int(lims[j]), int(lims[j + 1])
        ea, eb = int(el[j]), int(el[j + 1])
        assert b - a == eb - ea, f"{what}: query {j} has {b - a} hits, expected {eb - ea}"
        assert np.array_equal(I[a:b], eI[ea:eb]), f"{what}: ids of query {j} differ"
        assert np.array_equal(D[a:b], eD[ea:eb]), f"{what}: scores of query {j} differ"
    assert np.array_equal(lims.astype(np.int64), el) and len(D) == len(I) == el[-1]


_CASE1 = {}


def _case1(n, nq, d, metric):
    """Inputs, radii and expectation of a Gaussian bf16 case: computed once, shared (the faiss_shim test reuses one), not modified."""
    key = (n, nq, d, metric)
    if key not in _CASE1:
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
        vals = _values(q, x, metric)
        r = _boundary_radii(vals, metric)
        _CASE1[key] = (x, q, r, _expected(vals, r, metric))
    return _CASE1[key]


# ------------------------------------------------------------------ 1. Gaussian bf16, both metrics
@pytest.mark.parametrize("n,nq,d", [(4099, 129, 1024), (20000, 64, 769), (777, 5, 100), (30011, 70, 256)])
@pytest.mark.parametrize("metric", [0, 1])
def test_gaussian_bf16_matches_oracle(n, nq, d, metric):
    x, q, r, exp = _case1(n, nq, d, metric)
    ix = ram.MipsIndex(d, metric=metric)
    ix.add(x)
    got = ix.range_search(q, r)
    print(f"n={n} nq={nq} d={d} metric={metric}: {exp[0][-1]} hits")
    assert all(isinstance(t, np.ndarray) for t in got) and got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64
    _same(got, exp, "gaussian bf16")
    assert "wide_scan_kernel" in ix.last_kernel
    assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}
    again = ix.range_search(q, r)                                  # a fixed order: two calls agree bit for bit
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------ 2. fp32-exact index
@pytest.mark.parametrize("metric", [0, 1])
def test_f32_exact_index(metric):
    rng = np.random.default_rng(31)
    n, nq, d = 30000, 40, 768
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    vals = _values(q, x, metric)
    r = _boundary_radii(vals, metric)
    ix = ram.MipsIndex(d, metric=metric, dtype="f32")
    ix.add(x)
    _same(ix.range_search(q, r), _expected(vals, r, metric), "f32")
    assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}


# ------------------------------------------------------------------ 3. massive exact ties
@pytest.mark.parametrize("metric", [0, 1])
def test_lattice_ties_on_above_and_below_a_tied_value(metric):
    x = synth.generate(1, 0, 5000, 128, synth.KIND_LATTICE)
    q = synth.generate(2, 0, 19, 128, synth.KIND_LATTICE)
    vals = _values(q, x, metric)
    tied = np.empty(len(q), np.float32)
    for j in range(len(q)):
        u, c = np.unique(vals[j], return_counts=True)
        many = u[c >= max(2, c.max() // 2)]                        # values shared by many rows; take the best of them
        tied[j] = many[0] if metric == 1 else many[-1]
        assert (vals[j] == tied[j]).sum() >= 2
    ix = ram.MipsIndex(128, metric=metric)
    ix.add(x)
    for r in (tied, np.nextafter(tied, np.float32(np.inf)), np.nextafter(tied, np.float32(-np.inf))):
        _same(ix.range_search(q, r), _expected(vals, r, metric), "lattice")


def test_all_ones_rows_return_arange():
    n, d = 3000, 128
    ix = ram.MipsIndex(d)
    ix.add(np.ones((n, d), np.float32))
    lims, D, I = ix.range_search(np.ones((3, d), np.float32), float(d) - 0.5)
    assert np.array_equal(lims, [0, n, 2 * n, 3 * n]) and np.array_equal(I, np.tile(np.arange(n), 3)) and (D == float(d)).all()
    lims, D, I = ix.range_search(np.ones((3, d), np.float32), float(d))         # strict: on the common score nothing passes
    assert np.array_equal(lims, [0, 0, 0, 0]) and len(D) == len(I) == 0


# ------------------------------------------------------------------ 5. more than one slice, many chunks
def test_more_queries_than_one_slice():
    x = synth.generate(3, 0, 3000, 64, synth.KIND_GAUSS)
    q = synth.generate(4, 0, 4100, 64, synth.KIND_GAUSS)
    vals = _values(q, x, 0)
    r = _boundary_radii(vals, 0)
    ix = ram.MipsIndex(64)
    ix.add(x)
    _same(ix.range_search(q, r), _expected(vals, r, 0), "4100 queries")


def test_many_chunks_equal_the_strictly_better_prefix_of_search_wide():
    """4096 device-generated queries over 2^17 synthetic rows (16 chunks): with the radius on each query's 100th search_wide score
    the hits are exactly the strictly better prefix of search_wide(q, 1024) -- the oracle is not used at this size."""
    n, d, nq = 1 << 17, 768, 4096
    ix = ram.MipsIndex(d)
    ix.add_synthetic(n, row0=0, seed=synth.SEED_DOCS, kind=synth.KIND_GAUSS)
    qd = ram.synth_fill(nq, d, 0, synth.SEED_QUERIES, synth.KIND_GAUSS, dtype="bf16")
    s, i = ix.search_wide(qd, 1024)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    r = s[:, 99].copy()
    lims, D, I = ix.range_search(qd, r)
    assert lims.is_cuda and D.is_cuda and I.is_cuda
    lims, D, I = lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
    for j in range(nq):
        m = int((s[j] > r[j]).sum())                               # (scores descend: a prefix)
        assert m <= 99 and lims[j + 1] - lims[j] == m, j
        order = np.argsort(i[j, :m])
        assert np.array_equal(I[lims[j]:lims[j + 1]], i[j, :m][order]), j
        assert np.array_equal(D[lims[j]:lims[j + 1]], s[j, :m][order]), j


# ------------------------------------------------------------------ 6. capacity protocol at the C level
def test_capacity_counts_stay_true_and_the_repeat_is_complete():
    n, nq, d = 20000, 64, 769
    x, q, r, exp = _case1(n, nq, d, 0)
    total = int(exp[0][-1])
    assert total > 1000
    ix = ram.MipsIndex(d)
    ix.add(x)
    lib = ram._lib.load()
    qc = np.ascontiguousarray(q, np.float32)

    def call(cap, lims, D, I):
        return lib.mips_range_search(ix._h, qc.ctypes.data, ram._lib.DTYPE_F32, nq, r.ctypes.data, lims.ctypes.data,
                                     D.ctypes.data if D is not None else None, I.ctypes.data if I is not None else None, cap, 0, 0, None)

    small = total // 3
    lims = np.full(nq + 1, -1, np.int64)
    assert call(small, lims, np.empty(small, np.float32), np.empty(small, np.int64)) == 0
    assert np.array_equal(lims, exp[0])                            # the true counts although nothing fits
    lims0 = np.full(nq + 1, -1, np.int64)
    assert call(0, lims0, None, None) == 0                         # the counting call
    assert np.array_equal(lims0, exp[0])
    D, I = np.empty(total, np.float32), np.empty(total, np.int64)
    assert call(total, lims, D, I) == 0                            # the repeat with the exact size
    _same((lims, D, I), exp, "exact cap")


# ------------------------------------------------------------------ 7. device tensors, offsets, edges
@pytest.mark.parametrize("qdtype", [torch.float32, torch.bfloat16])
def test_range_search_into_cuda_tensors(qdtype):
    n, nq, d = 30011, 70, 256
    x, q, r, exp = _case1(n, nq, d, 0)
    ix = ram.MipsIndex(d)
    ix.add(torch.from_numpy(x).cuda())
    qd = torch.from_numpy(q).cuda().to(qdtype)
    cap = int(exp[0][-1]) + 5
    lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    D = torch.empty(cap, dtype=torch.float32, device="cuda")
    I = torch.empty(cap, dtype=torch.int64, device="cuda")
    assert ix.range_search_into(qd, r, lims, D, I) is None
    total = int(lims[-1])
    _same((lims, D[:total], I[:total]), exp, str(qdtype))
    got = ix.range_search(qd, r)                                   # CUDA tensor in -> CUDA tensors out
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
    _same(got, exp, "range_search, device")


def test_idx_offset_and_force_ip():
    x = synth.generate(3, 0, 6000, 200, synth.KIND_GAUSS)
    q = synth.generate(4, 0, 9, 200, synth.KIND_GAUSS)
    ix = ram.MipsIndex(200, metric=1)
    ix.add(x)
    v1, v0 = _values(q, x, 1), _values(q, x, 0)
    r1, r0 = _boundary_radii(v1, 1), _boundary_radii(v0, 0)
    _same(ix.range_search(q, r1, idx_offset=1 << 33), _expected(v1, r1, 1, idx_offset=1 << 33), "offset")
    _same(ix.range_search(q, r0, force_ip=True), _expected(v0, r0, 0), "force_ip")


def test_scalar_radius_empty_index_and_no_queries():
    ix = ram.MipsIndex(64)
    lims, D, I = ix.range_search(np.zeros((3, 64), np.float32), -1.0)
    assert np.array_equal(lims, [0, 0, 0, 0]) and len(D) == len(I) == 0
    x = synth.generate(3, 0, 100, 64, synth.KIND_GAUSS)
    ix.add(x)
    lims, D, I = ix.range_search(np.zeros((0, 64), np.float32), 0.0)
    assert np.array_equal(lims, [0]) and len(D) == len(I) == 0 and D.dtype == np.float32 and I.dtype == np.int64
    q = synth.generate(4, 0, 7, 64, synth.KIND_GAUSS)
    vals = _values(q, x, 0)
    _same(ix.range_search(q, 0.25), _expected(vals, np.full(7, 0.25, np.float32), 0), "scalar radius")


# ------------------------------------------------------------------ 8. refusals
def test_unsupported_requests_raise():
    for dtype in ("fp8_e4m3", "fp8_e4m3_docs"):
        f8 = ram.MipsIndex(64, dtype=dtype)
        f8.add(synth.generate(3, 0, 100, 64, synth.KIND_GAUSS))
        with pytest.raises(NotImplementedError):
            f8.range_search(np.zeros((1, 64), np.float32), 0.0)
    big = ram.MipsIndex(1100)
    big.add(synth.generate(3, 0, 100, 1100, synth.KIND_GAUSS))
    with pytest.raises(NotImplementedError):
        big.range_search(np.zeros((1, 1100), np.float32), 0.0)
    ix = ram.MipsIndex(64)
    ix.add(synth.generate(3, 0, 100, 64, synth.KIND_GAUSS))
    with pytest.raises((ValueError, RuntimeError)):
        ix.range_search(np.zeros((2, 64), np.float32), np.array([0.0, np.nan], np.float32))
    lib = ram._lib.load()
    q = np.zeros((2, 64), np.float32)
    lims, D, I = np.zeros(3, np.int64), np.zeros(8, np.float32), np.zeros(8, np.int64)

    def call(handle, r, flags):
        return lib.mips_range_search(handle, q.ctypes.data, ram._lib.DTYPE_F32, 2, r.ctypes.data, lims.ctypes.data, D.ctypes.data,
                                     I.ctypes.data, 8, 0, flags, None)

    ok = np.zeros(2, np.float32)
    assert call(ix._h, np.array([0.0, np.nan], np.float32), 0) == -1                     # MIPS_E_INVALID
    assert call(ix._h, ok, ram._lib.OUT_PACKED) == -1
    assert call(ix._h, ok, ram._lib.OUT_PACKED | ram._lib.OUT_DEVICE) == -1
    assert call(big._h, ok, 0) == -3                                                     # MIPS_E_UNSUPPORTED
    assert call(ix._h, np.array([np.inf, -np.inf], np.float32), 0) == 0 and np.array_equal(lims, [0, 0, 100])


# ------------------------------------------------------------------ 9. faiss drop-in
@pytest.mark.parametrize("metric", [0, 1])
def test_faiss_shim_range_search(metric):
    n, nq, d = 4099, 129, 1024
    x, q, r, exp = _case1(n, nq, d, metric)
    fs = ram.faiss_shim
    if metric == 1:
        fx = fs.IndexFlat(d + 1, fs.METRIC_L2, dtype="bf16")
        fx.add(augment_xb(x.astype(np.float64)).astype(np.float32))
        lims, D, I = fx.range_search(augment_xq(q), float(r[5]))
    else:
        fx = fs.IndexFlatIP(d)
        fx.add(x)
        lims, D, I = fx.range_search(q, float(r[5]))
    assert lims.dtype == np.uint64 and lims.shape == (nq + 1,) and D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (int(lims[-1]),)
    # case 1's expectation is per-query radii; faiss takes ONE threshold: the same pairs' values against r[5] (~50 hits in query 5)
    vals = _values(q, x, metric)
    _same((lims, D, I), _expected(vals, np.full(nq, r[5], np.float32), metric), "faiss_shim")
    got = fx.mips_index.range_search(q, r)                         # and the per-query radii through the index behind the shim
    _same(got, exp, "faiss_shim.mips_index")


# ------------------------------------------------------------------ 10. near-duplicate self-join
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_knowledge_base_near_duplicates(dtype):
    rng = np.random.default_rng(5)
    n, d = 3000, 128
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    if dtype == "bf16":
        x = synth.round_to_bf16(x)
    rows = rng.permutation(n)
    a, b = np.sort(rows[:70]), np.sort(rows[70:75])               # 70 copies: past the 64-hit flood threshold of the top-k paths
    x[a] = x[a[0]]
    x[b] = x[b[0]]
    kb = KnowledgeBase({"emb": x})
    kb.add_faiss_index("emb", metric_type=0, dtype=dtype)
    i, j, s = kb.near_duplicates("emb", 0.99, batch_rows=1000)
    exp = sorted([(int(u), int(v)) for c in (a, b) for ui, u in enumerate(c) for v in c[ui + 1:]])
    assert len(exp) == 70 * 69 // 2 + 5 * 4 // 2
    assert list(zip(i.tolist(), j.tolist())) == exp               # exactly the planted pairs, i < j, sorted by (i, j)
    assert i.dtype == np.int64 and j.dtype == np.int64 and s.dtype == np.float32
    self_dot = orc.canonical_pairs(x[i], x, j[:, None])[:, 0].astype(np.float32)
    assert np.array_equal(s, self_dot)


# ------------------------------------------------------------------ 11. plain C
def test_c_abi_range_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_range_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_range_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
