"""Shared pieces of tests/test_range_sharded_host.py and tests/test_gpu_range_sharded.py.  Not a test file; no GPU is needed to
import it.

  _values, _boundary_radii, _expected, _same   restated from tests/test_gpu_range.py (which is neither edited nor imported): the
             canonical float32 value of every (query, row) pair from the oracle, radii ON the boundary -- the exact score of an own
             row, its nextafter, +-inf -- the expected CSR triple, and the per-query bit-for-bit comparison.  Two optional arguments
             are new: _values takes the phi of a LARGER index (an L2 shard measures distances with the global phi), _expected a
             bool mask [n] or [nq, n] of the rows that may answer (selector AND group rule).
  record_words, make_record, split_record      the part record of include/mips_hip_sharded.h in NumPy.
  merge_records                                the NumPy restatement of mips_range_merge_records: the reference of the merge
             kernel on the GPU and the injected merge step of the gloo rehearsal on the CPU.
  synthetic_parts                              per-(part, query) hit lists with about half the counts 0.
"""
import numpy as np
import torch

from oracle import mips_oracle as orc

PAD_ID = -7                       # what make_record leaves in the unused id entries; the unused scores are NaN


def _values(q, x, metric, phi=None):
    """float32 canonical output value of every (query, row) pair: the inner product, or |q|^2 + phi - 2 q.x (metric 1).  phi:
    that of the index the rows belong to (default: of x itself)."""
    n = x.shape[0]
    dot = orc.canonical_pairs(q, x, np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1)))
    if metric == 1:
        if phi is None:
            phi = orc.sumsq_canonical(x).max()
        return (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * dot).astype(np.float32)
    return dot.astype(np.float32)


def _boundary_radii(vals, metric):
    """`vals` [nq, n] float32 -> per-query radii: a third of the queries get the exact float32 score of one of their own rows (that
    row and its ties are out), a third the nextafter of such a score towards the permissive side (they are in), the rest run from
    "nothing" through ~50 hits to "every row", +-inf included."""
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


def _expected(vals, r, metric, idx_offset=0, mask=None):
    lims, D, I = [0], [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    for j in range(vals.shape[0]):
        hit = vals[j] < r[j] if metric == 1 else vals[j] > r[j]
        if mask is not None:
            hit = hit & (mask if mask.ndim == 1 else mask[j])
        ids = np.flatnonzero(hit)
        lims.append(lims[-1] + len(ids))
        D.append(vals[j][ids])
        I.append(ids + idx_offset)
    return np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def _same(got, exp, what=""):
    lims, D, I = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in got)
    el, eD, eI = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in exp)   # (a device result as the expectation)
    assert lims.shape == el.shape and lims[0] == 0
    for j in range(len(el) - 1):                                   # per query: the first difference names its query
        a, b = int(lims[j]), int(lims[j + 1])
        ea, eb = int(el[j]), int(el[j + 1])
        assert b - a == eb - ea, f"{what}: query {j} has {b - a} hits, expected {eb - ea}"
        assert np.array_equal(I[a:b], eI[ea:eb]), f"{what}: ids of query {j} differ"
        assert np.array_equal(D[a:b].view(np.uint32), eD[ea:eb].view(np.uint32)), f"{what}: scores of query {j} differ"
    assert np.array_equal(lims.astype(np.int64), el) and len(D) == len(I) == el[-1]


# ------------------------------------------------------------------ the part record
def record_words(nq, stride):
    """MIPS_RANGE_RECORD_WORDS, written out once more"""
    return nq + 1 + stride + (stride + 1) // 2


def make_record(lims, D, I, stride):
    """(lims int64 [nq + 1], D float32 [m], I int64 [m]) -> int64 [record_words(nq, stride)].  m may differ from lims[-1]: a
    truncated part keeps the true lims and its first `stride` entries.  Unused entries: ids PAD_ID, scores NaN, the half word
    behind an odd number of scores 0."""
    nq = len(lims) - 1
    rec = np.zeros(record_words(nq, stride), np.int64)
    rec[:nq + 1] = lims
    rec[nq + 1:nq + 1 + stride] = PAD_ID
    sc = rec[nq + 1 + stride:].view(np.float32)
    sc[:stride] = np.nan
    m = min(stride, len(I))
    rec[nq + 1:nq + 1 + m] = I[:m]
    sc[:m] = D[:m]
    return rec


def split_record(rec, nq, stride):
    """-> views (lims [nq + 1], D float32 [stride], I [stride]) of one record"""
    rec = np.asarray(rec)
    assert rec.dtype == np.int64 and rec.shape == (record_words(nq, stride),)
    return rec[:nq + 1], rec[nq + 1 + stride:].view(np.float32)[:stride], rec[nq + 1:nq + 1 + stride]


def merge_records(gathered, parts, nq, stride):
    """mips_range_merge_records in NumPy: `gathered` holds `parts` records end to end, in ascending row order of their shards.
    -> (lims, D, I) with lims the column sums of the parts' lims and the hits of query j the parts' segments of j one after
    the other.  With a truncated part (lims_p[nq] > stride) only lims is defined: D and I are returned as None."""
    g = np.ascontiguousarray(np.asarray(gathered, dtype=np.int64).reshape(parts, record_words(nq, stride)))
    views = [split_record(g[p], nq, stride) for p in range(parts)]
    lims = np.sum([v[0] for v in views], axis=0).astype(np.int64)
    if any(v[0][nq] > stride for v in views):
        return lims, None, None
    D = np.empty(int(lims[nq]), np.float32)
    I = np.empty(int(lims[nq]), np.int64)
    pos = 0
    for j in range(nq):
        assert pos == lims[j]
        for pl, pD, pI in views:
            a, b = int(pl[j]), int(pl[j + 1])
            D[pos:pos + b - a] = pD[a:b]
            I[pos:pos + b - a] = pI[a:b]
            pos += b - a
    assert pos == lims[nq]
    return lims, D, I


def synthetic_parts(parts, nq, seed, max_count=40, counts=None):
    """-> a list of `parts` triples (lims, D, I) as row shards would return them.  counts [parts, nq] (default: drawn, about
    half of them 0, the others 1 .. max_count).  Part p owns the ids [p 2^34, (p + 1) 2^34): ascending within a query, beyond
    int32; the scores are random float32 of either sign."""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = rng.integers(1, max_count + 1, (parts, nq)) * (rng.random((parts, nq)) < 0.5)
    counts = np.asarray(counts, np.int64).reshape(parts, nq)
    out = []
    for p in range(parts):
        lims = np.concatenate([[0], np.cumsum(counts[p])]).astype(np.int64)
        total = int(lims[-1])
        I = np.empty(total, np.int64)
        for j in range(nq):
            c = int(counts[p, j])
            I[lims[j]:lims[j + 1]] = (p << 34) + np.cumsum(rng.integers(1, 9, c))       # ascending, with gaps
        D = rng.standard_normal(total).astype(np.float32)
        out.append((lims, D, I))
    return out


def gather(part_results, stride):
    """the records of synthetic_parts (or of any per-part results) end to end: int64 [parts * record_words]"""
    return np.concatenate([make_record(l, D, I, stride) for l, D, I in part_results])
