"""Tie floods: queries for which MORE than 64 rows reach the k-th key of the first scan's result (the exact pass keeps a hit
list of RESOLVE_CAP = 64 rows per flagged query, csrc/resolve_kernels.hpp).  Two families, planted into Gaussian backgrounds:

  near-duplicate floods  exact scores distinct, the scan cannot tell the members apart (bf16 / e4m3: copies a few ulp
                         steps apart under a query whose MFMA chains climb far above the final score; fp32-exact index:
                         clusters that bf16 cannot separate), so the first result keeps the wrong members and every member
                         above them reaches its k-th key;
  exact-tie floods       k - 1 clear winners and M identical rows tied for the k-th place: (k - 1) + M hits by
                         construction -- 64 still fits the hit list, 65 does not.

Every fixture runs on every path that reaches the exact pass (host buffers, device outputs, the split tail, packed
outputs with an offset, the one-launch hook with and without an ignore id inside the flood, "margin_check" = 2) and must
return the canonical top-k (ties: lowest index first) with nothing left unresolved."""
import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu

OFF = 777  # idx_offset of the packed searches


# ------------------------------------------------------------------ references
def _brute(q, x, k, metric):
    """Tie-safe canonical top-k by full enumeration.  IP: the oracle's C brute force.  L2: every row's canonical dot, the
    float32 distance |q|^2 + phi - 2 ip, ranked by (distance asc, idx asc) -- the oracle's brute force re-ranks only the
    k + 16 best by inner product, which a flood of equal float32 distances with distinct inner products can outnumber."""
    if metric == 0:
        return orc.search_exact_bruteforce(q, x, k)
    n = len(x)
    ip = orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (len(q), 1)))
    phi = orc.sumsq_canonical(x).max()
    dist = (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * ip).astype(np.float32)
    order = np.stack([np.lexsort((np.arange(n), dist[r]))[:k] for r in range(len(q))])
    return np.take_along_axis(dist, order, axis=1), order.astype(np.int64)


def _keys(q, x, metric):
    """canonical float32 keys (larger = better) of every row for each query"""
    ip = orc.canonical_pairs(q, x, np.tile(np.arange(len(x), dtype=np.int64), (len(q), 1)))
    if metric == 0:
        return ip.astype(np.float32)
    phi = orc.sumsq_canonical(x).max()
    return -(orc.sumsq_canonical(q)[:, None] + phi - 2.0 * ip).astype(np.float32)


def _stored(ix):
    raw = ix.rows_raw()
    if ix.dtype == "bf16":
        return synth.bf16_bits_to_f32(raw)
    return raw if ix.dtype == "f32" else synth.e4m3_bits_to_f32(raw)


def _to_storage(dtype, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype in ("bf16", "fp8_e4m3_docs"):
        return synth.round_to_bf16(a)
    return a if dtype == "f32" else synth.round_to_e4m3(a)


def _rows_to_storage(dtype, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "bf16":
        return synth.round_to_bf16(a)
    return a if dtype == "f32" else synth.round_to_e4m3(a)


# ------------------------------------------------------------------ fixtures
def _near_dup_quantised(dtype, d, n, nq, M, seed):
    """The near-duplicate case of test_gpu_parity.py (_near_duplicate_case) for any d and storage.  Every row carries +A on
    the first h coordinates and -A on the last h; the star queries carry Q there, so every MFMA chain climbs to Q A h before
    the informative middle part (|score| < 600) comes back -- at a granularity far coarser than the steps between the M
    copies of the star row, whose exact scores rise by one step each.  bf16: one coordinate, 1 + t 2^-7, under a query
    weight of 2^-7.  e4m3 (3 mantissa bits): the step count t spread over several coordinates, 1 + a_i / 8 with sum a_i = t,
    under weights of 2^-9.  The copies sit 16 rows apart (one sub-list); the exact top k are the HIGHEST-index copies."""
    rng = np.random.default_rng(seed)
    f8 = dtype != "bf16"
    A, Q = (16.0, 256.0) if f8 else (1.0, 16.0)
    h = (d - 256) // 2 if d >= 768 else d // 4
    x = synth.generate(seed + 1, 0, n, d, synth.KIND_GAUSS)
    x[:, :h] = A
    x[:, d - h:] = -A
    q = synth.generate(seed + 2, 0, nq, d, synth.KIND_GAUSS)
    sign = np.where(rng.random(d - 2 * h) < 0.5, -1.0, 1.0).astype(np.float32)
    star_x = np.full(d, A, np.float32)
    star_x[d - h:] = -A
    star_x[h:d - h] = sign
    star_q = np.full(d, Q, np.float32)
    star_q[d - h:] = Q
    star_q[h:d - h] = sign
    cols = h + 3 + 5 * np.arange(19 if f8 else 1)
    star_q[cols] = 2.0 ** -9 if f8 else 2.0 ** -7
    rows = 1003 + 16 * np.arange(M)
    for t, r in enumerate(rows):
        x[r] = star_x
        if f8:
            a = np.minimum(7, np.maximum(0, t - 7 * np.arange(len(cols))))   # sum a_i = t, each 0 .. 7
            x[r, cols] = 1.0 + a / 8.0
        else:
            x[r, cols[0]] = 1.0 + t * 2.0 ** -7
    stars = np.arange(0, nq, max(1, nq // 8))[:8]
    q[stars] = star_q
    assert np.array_equal(_rows_to_storage(dtype, x[rows]), x[rows]) and np.array_equal(_to_storage(dtype, q[stars]), q[stars])
    return x, q, stars


def _near_dup_f32(d, n, nq, M, seed):
    """fp32 rows bf16 cannot tell apart: clusters of M members, each the centre times (1 + 1e-4 g) plus 1e-4 noise
    (test_f32_exact_two_stage_near_duplicates with clusters of M instead of 40), in a Gaussian background; the flood
    queries lie near the centres."""
    rng = np.random.default_rng(seed)
    nc = 3
    c = rng.standard_normal((nc, d)).astype(np.float32)
    cl = (np.repeat(c, M, axis=0) * (1.0 + 1e-4 * rng.standard_normal((nc * M, 1)))).astype(np.float32)
    cl += (1e-4 * rng.standard_normal(cl.shape)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    at = np.sort(rng.choice(n - nc * M, 1, replace=False))[0]
    x[at:at + nc * M] = cl
    q = rng.standard_normal((nq, d)).astype(np.float32)
    stars = np.arange(0, nq, max(1, nq // 8))[:8]
    q[stars] = c[np.arange(len(stars)) % nc] + 0.01 * rng.standard_normal((len(stars), d)).astype(np.float32)
    return x, q, stars


def _tie_flood(dtype, d, n, nq, k, M, seed):
    """k - 1 rows 2v and M rows v (v exactly representable): the flood queries (v plus a little noise) rank the 2v rows
    first and tie the M copies of v for the k-th place -- (k - 1) + M rows reach the k-th key, and the expected result is
    the winners, then the LOWEST-index copy.  The other queries are pushed away from v (q . v < 0): no copy reaches them."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    v = _rows_to_storage(dtype, rng.standard_normal(d).astype(np.float32))
    ties = np.sort(rng.choice(np.arange(50, n - 200), M, replace=False))
    wins = n - 1 - 7 * np.arange(k - 1)
    x[ties] = v
    x[wins] = 2.0 * v
    q = rng.standard_normal((nq, d)).astype(np.float32) - 0.2 * v
    stars = np.arange(0, nq, max(1, nq // 8))[:8]
    q[stars] = v + 0.05 * rng.standard_normal((len(stars), d)).astype(np.float32)
    return x, q, stars, ties, wins


# ------------------------------------------------------------------ the paths
def _run_paths(ix, x, q, stars, k, metric, kernel=None, fused=True):
    """Every path that reaches the exact pass, against the tie-safe brute force (flood queries) and the oracle (the rest)."""
    dtype = ix.dtype
    xs = _stored(ix)
    qs = _to_storage(dtype, q)
    nq = len(q)
    free = np.setdiff1d(np.arange(nq), stars)
    kb = min(k + 1, ram.MAX_K)
    bs, bi = _brute(qs[stars], xs, kb, metric)                  # (k + 1: the ignore filter below)
    es, ei = orc.search_exact(qs, xs, k, metric=metric)
    es[stars], ei[stars] = bs[:, :k], bi[:, :k]

    def same(s, i, what, off=0):
        s = s.cpu().numpy() if isinstance(s, torch.Tensor) else s
        i = i.cpu().numpy() if isinstance(i, torch.Tensor) else i
        bad = (i != ei + off).any(axis=1) | (s.view(np.uint32) != es.view(np.uint32)).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {nq} rows differ (flood rows {int(bad[stars].sum())}), stats {ix.margin_stats()}"

    def settled(what):
        st = ix.margin_stats()
        assert st["unresolved"] == 0 and st["rescanned"] == st["flagged"], (what, st)
        return st

    qd = torch.from_numpy(q).cuda()
    tail = torch.cuda.Stream()
    for fast in (1, 2):                                          # 2: the optimistic first scans for device outputs as well
        ix.set_param("f32_fast", fast)
        s, i = ix.search(q, k)                                   # host buffers: certified now
        if kernel is not None:
            assert kernel(ix.last_kernel), ix.last_kernel
        same(s, i, f"host f32_fast={fast}")
        settled(f"host f32_fast={fast}")
        s, i = ix.search(qd, k)                                  # device outputs: stream-ordered
        same(s, i, f"device f32_fast={fast}")
        settled(f"device f32_fast={fast}")
        pk = ix.search_packed(qd, k, OFF)                        # packed payload, idx_offset
        same(pk[..., 0].cpu().numpy().astype(np.uint32).view(np.float32), pk[..., 1], f"packed f32_fast={fast}", OFF)
        settled(f"packed f32_fast={fast}")
        ix.set_param("margin_check", 2)                          # certify and synchronise
        s, i = ix.search(qd, k)
        if kernel is not None and fast == 2:
            assert kernel(ix.last_kernel), ix.last_kernel
        same(s, i, f"margin_check=2 f32_fast={fast}")
        settled(f"margin_check=2 f32_fast={fast}")
        ix.set_param("margin_check", 1)
    ix.set_param("f32_fast", 1)
    s, i = ix.search(qd, k, tail_stream=tail)                    # split tail: select, re-score, exact pass on the tail stream
    torch.cuda.synchronize()
    same(s, i, "split tail")
    settled("split tail")
    pk = ix.search_packed(qd, k, OFF, tail_stream=tail)
    torch.cuda.synchronize()
    same(pk[..., 0].cpu().numpy().astype(np.uint32).view(np.float32), pk[..., 1], "packed split tail", OFF)
    if not fused:
        return
    # the hook's call shape: <= 16 flood queries in one call, with and without an ignore id inside the flood
    qf = torch.from_numpy(np.ascontiguousarray(q[stars])).cuda()
    s, i = ix.search_fused(qf, k)
    assert np.array_equal(i.cpu().numpy(), bi[:, :k]) and np.array_equal(s.cpu().numpy(), bs[:, :k]), ("fused", ix.margin_stats())
    settled("fused")
    if k + 1 <= (13 if dtype == "fp8_e4m3" else ram.MAX_K):   # (k + 1 fetched; e4m3 queries: k <= 13)
        ban = bi[:, k - 1].copy()                                # the k-th member: the flood itself
        s, i = ix.search_fused(qf, k, ignore=torch.from_numpy(ban).cuda())
        assert np.array_equal(i.cpu().numpy(), np.delete(bi, k - 1, axis=1)), ("fused + ignore", ix.margin_stats())
        assert np.array_equal(s.cpu().numpy(), np.delete(bs, k - 1, axis=1)), ("fused + ignore", ix.margin_stats())
        settled("fused + ignore")
    ix.check()


def _hits(x, qf, first_i, metric):
    """rows whose canonical key reaches the key of the k-th row of first_i, per query of qf"""
    keys = _keys(qf, x, metric)
    kk = np.take_along_axis(keys, first_i[:, -1:], axis=1)
    return (keys >= kk).sum(axis=1)


def _index(x, dtype, metric):
    ix = ram.MipsIndex(x.shape[1], metric=metric, dtype=dtype)
    ix.add(x)
    return ix


V4 = lambda name: name.startswith("mips::scan_kernel_v4") and name.endswith(", 4>")   # pools of 32 out of sub-lists
K3 = lambda name: name.startswith("mips::scan_kernel_k3<4, 32, 2, 0, 4>")           # pitch 1024, pools of 32
TWO_STAGE = lambda name: not name.startswith("mips::scan_kernel<")                  # fp32-exact: stage 1 on bf16 rows


# ------------------------------------------------------------------ near-duplicate floods
@pytest.mark.parametrize("dtype,d,n,nq,k,M,metric", [
    ("bf16", 768, 40000, 100, 5, 127, 0),
    ("bf16", 768, 40000, 100, 1, 70, 1),
    ("bf16", 768, 40000, 300, 10, 127, 0),       # > 256 queries, k = 10: pools of 32 out of scan_kernel_v4's sub-lists
    ("bf16", 1024, 40000, 300, 10, 70, 1),       # pitch 1024, > 256 queries: pools of 32 out of scan_kernel_k3's sub-lists
    ("bf16", 1024, 30000, 60, 29, 127, 0),
    ("bf16", 300, 30000, 60, 5, 127, 0),
    ("fp8_e4m3", 768, 30000, 60, 5, 127, 0),
    ("fp8_e4m3", 1024, 30000, 60, 13, 70, 1),
    ("fp8_e4m3_docs", 768, 30000, 60, 10, 127, 0),
    ("fp8_e4m3_docs", 1024, 30000, 60, 1, 70, 1),
])
def test_near_duplicate_floods(dtype, d, n, nq, k, M, metric):
    x, q, stars = _near_dup_quantised(dtype, d, n, nq, M, seed=d + k + M)
    ix = _index(x, dtype, metric)
    kernel = V4 if (d == 768 and nq > 256) else K3 if (d == 1024 and nq > 256) else None
    _run_paths(ix, x, q, stars, k, metric, kernel=kernel)
    if d == 300 or (d == 768 and k == 5):                        # the plain exact pass (no MFMA pre-filter) on the same case
        ix.set_param("resolve", 2)
        _run_paths(ix, x, q, stars, k, metric, fused=False)


@pytest.mark.parametrize("d,n,nq,k,M,metric", [
    (768, 30000, 60, 5, 70, 0),
    (768, 30000, 60, 5, 300, 1),
    (1024, 30000, 60, 10, 1000, 0),
    (300, 30000, 60, 1, 300, 0),
    (768, 20000, 60, 29, 300, 0),
])
def test_f32_cluster_floods(d, n, nq, k, M, metric):
    x, q, stars = _near_dup_f32(d, n, nq, M, seed=d + M + k)
    ix = _index(x, "f32", metric)
    _run_paths(ix, x, q, stars, k, metric, kernel=TWO_STAGE if k <= 13 else None)


# ------------------------------------------------------------------ exact-tie floods
@pytest.mark.parametrize("dtype,d,k,metric", [
    ("bf16", 768, 1, 0),
    ("bf16", 1024, 5, 1),
    ("bf16", 768, 29, 0),
    ("f32", 1024, 10, 0),
    ("f32", 768, 5, 1),
    ("fp8_e4m3", 768, 13, 0),
    ("fp8_e4m3_docs", 1024, 5, 0),
    ("bf16", 300, 10, 1),
])
@pytest.mark.parametrize("hits", [64, 65])                       # (k - 1) + M: fits the hit list / one over
def test_exact_tie_floods(dtype, d, k, metric, hits):
    M = hits - (k - 1)
    n, nq = 20000, 40
    x, q, stars, ties, wins = _tie_flood(dtype, d, n, nq, k, M, seed=d + k + hits)
    ix = _index(x, dtype, metric)
    xs = _stored(ix)
    bs, bi = _brute(_to_storage(dtype, q[stars]), xs, k, metric)
    assert np.array_equal(bi, np.tile(np.concatenate([np.sort(wins), ties[:1]]), (len(stars), 1)))   # winners, lowest copy
    assert (_hits(xs, _to_storage(dtype, q[stars]), bi, metric) == hits).all()
    _run_paths(ix, x, q, stars, k, metric)


@pytest.mark.parametrize("dtype,d,k,metric", [("f32", 768, 5, 0), ("bf16", 300, 10, 1)])
def test_exact_tie_flood_of_1000(dtype, d, k, metric):
    x, q, stars, ties, wins = _tie_flood(dtype, d, 30000, 300, k, 1000, seed=1000 + d)
    ix = _index(x, dtype, metric)
    _run_paths(ix, x, q, stars, k, metric)


# ------------------------------------------------------------------ rows wider than 1024: the wide-list re-scan
@pytest.mark.parametrize("dtype,M", [("f32", 300), ("bf16", 127)])
def test_floods_wider_than_1024(dtype, M):
    d, n, nq, k = 1100, 20000, 60, 5
    if dtype == "f32":
        x, q, stars = _near_dup_f32(d, n, nq, M, seed=1100)
    else:
        x, q, stars = _near_dup_quantised(dtype, d, n, nq, M, seed=1100)
    ix = _index(x, dtype, 0)
    xs, qs = _stored(ix), _to_storage(dtype, q)
    es, ei = orc.search_exact(qs, xs, k)
    es[stars], ei[stars] = _brute(qs[stars], xs, k, 0)
    s, i = ix.search(q, k)
    assert np.array_equal(i, ei) and np.array_equal(s, es), ix.margin_stats()
    s, i = ix.search(torch.from_numpy(q).cuda(), k)
    assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es), ix.margin_stats()
