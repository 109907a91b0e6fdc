"""Inputs for the calls of the IVF index that are cut into more than one piece, and for list tables of more than 1024 lists, on top of
tests/ivf_cases.py, ivf_search_cases.py, ivf_filter_cases.py, ivf_wide_cases.py and ivf_range_cases.py (the restatements).

The host side cuts a call into pieces and re-derives pointers and launch shapes per piece:
    ivf_assign_rows (host_ivf.hpp)          ASSIGN_CHUNK rows: mips_ivf_add, every iteration of mips_ivf_train
    mips_ivf_probe                          PROBE_SLICE queries, host-output and device-output branch
    ivf_search_impl                         slice_queries(p, k) queries: mips_ivf_search / _sel / _grp / _wide / _wide_grp
    mips_ivf_range_search (host_ivf_range)  RANGE_SLICE queries
    IvfIndex.load(chunk_rows=)              chunk_rows rows
The constants are mirrored here and pinned against the sources by tests/test_ivf_pieces_host.py.

PERIODIC INPUTS.  A call of nq queries uses QP = 7 distinct queries (and the radii tied to them) and LP = 5 distinct group labels,
tiled with those periods: query j is q7[j % 7] with label lab5[j % 5].  The periods are coprime to every piece size (4096, 256, 564),
so the queries behind a piece boundary are NOT those at the same place of the piece before, and 35 = 7 * 5 distinct (query, label)
pairs all occur.  The restatement runs on the distinct inputs only and `expand` indexes its result out to nq queries.
"""
import os
import sys
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ivf_cases as iv  # noqa: E402
import ivf_filter_cases as fc  # noqa: E402
import ivf_range_cases as rc  # noqa: E402

F = np.float32
NONE = fc.LABEL_NONE

# ------------------------------------------------------------------ the mirrored constants
ASSIGN_CHUNK = 65536        # kIvfAssignChunk (host_ivf.hpp)
PROBE_SLICE = 4096          # the literal of both loops of mips_ivf_probe (host_ivf.hpp)
SLICE_QUERIES = 4096        # ivf::kSliceQueries (ivf_search_math.hpp)
PARTS_BUDGET = 256 << 20    # ivf::kPartsBudget
RANGE_SLICE = rc.SLICE      # ivf::kRangeSlice (ivf_range_math.hpp)
SCAN_THREADS = 1024         # mips::IVF_SCAN_THREADS (ivf_kernels.hpp): above it a thread of ivf_offsets_kernel owns several lists
MAX_PROBE = 1024            # mips::IVF_MAX_PROBE


def slice_queries(p, k):
    """ivf::slice_queries of csrc/ivf_search_math.hpp"""
    return min(max(PARTS_BUDGET // (p * k * 16), 1), SLICE_QUERIES)


def pieces(n, piece):
    """how many pieces a loop of step `piece` cuts n items into"""
    return -(-int(n) // int(piece))


# ------------------------------------------------------------------ periodic inputs
QP, LP, RP = 7, 5, 7        # periods of the queries, the group labels and the radii (the radii are tied to the queries)


def tile(nq):
    """-> (qi, li, pi): which of the 7 queries (and radii), which of the 5 labels and which of the 35 (query, label) pairs query j
    of a call uses; pair u is (query u // 5, label u % 5)"""
    j = np.arange(int(nq))
    qi, li = j % QP, j % LP
    return qi, li, qi * LP + li


def pairs(q7, lab5):
    """the 35 distinct (query, label) inputs in the order `tile` numbers them"""
    u = np.arange(QP * LP)
    return np.ascontiguousarray(np.asarray(q7)[u // LP]), np.ascontiguousarray(np.asarray(lab5)[u % LP])


def expand(result, index):
    """a restatement's result on the distinct inputs -> that of the tiled call: (D, I) by rows, CSR (lims, D, I) by stretches"""
    index = np.asarray(index)
    if len(result) == 2:
        return result[0][index], result[1][index]
    lims, D, I = result
    cnt = np.diff(lims)[index]
    out = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    if len(index) == 0:
        return out, D[:0], I[:0]
    take = np.concatenate([np.arange(lims[u], lims[u + 1]) for u in index] + [np.zeros(0, np.int64)]).astype(np.int64)
    return out, D[take], I[take]


def rows_differ(res, a, b):
    """bool per pair of queries (a[t], b[t]): do their rows of a (D, I) result, or their stretches of a CSR result, differ"""
    a, b = np.asarray(a), np.asarray(b)
    if len(res) == 2:
        D, I = res
        return (I[a] != I[b]).any(axis=1) | (D[a].view(np.uint32) != D[b].view(np.uint32)).any(axis=1)
    lims, D, I = res
    return np.array([not (np.array_equal(I[lims[x]:lims[x + 1]], I[lims[y]:lims[y + 1]]) and
                          np.array_equal(D[lims[x]:lims[x + 1]].view(np.uint32), D[lims[y]:lims[y + 1]].view(np.uint32))) for x, y in zip(a, b)])


def coprime(period, piece):
    return gcd(int(period), int(piece)) == 1


def radii_for(per, counts):
    """radii that give query j exactly counts[j] hits among its probed rows (per: rc.probed_scores); None in counts: all of them"""
    out = []
    for (_, _, rep, _), c in zip(per, counts):
        r = rc.radius_for_count(rep, len(rep) if c is None else c)
        assert r is not None, c
        out.append(r)
    return np.array(out, F)


def base(c):
    return c["rows"], c["assign"], c["centroids"]


# ------------------------------------------------------------------ case 1: an add of more than one assign chunk
ADD_N, ADD_D, ADD_NLIST = ASSIGN_CHUNK + 4099, 8, 7


def case_add(seed=31):
    """69 635 Gaussian rows of d = 8, seven planted random unit centroids, 9 queries"""
    rng = np.random.default_rng(seed)
    return {"rows": rng.standard_normal((ADD_N, ADD_D)).astype(F), "rows2": rng.standard_normal((ADD_N, ADD_D)).astype(F),
            "q": rng.standard_normal((9, ADD_D)).astype(F), "nlist": ADD_NLIST,
            "centroids": iv.normalise(rng.standard_normal((ADD_NLIST, ADD_D)).astype(F))}


# ------------------------------------------------------------------ case 2: a training set of more than one assign chunk
TRAIN_N, TRAIN_D, TRAIN_NLIST = 70001, 4, 257      # m = 256 * 257 = 65 792 evenly spaced rows train


def case_train(seed=32):
    return np.random.default_rng(seed).standard_normal((TRAIN_N, TRAIN_D)).astype(F)


def train_step(T, c, a):
    """one update of iv.train: the centroids c moved to the normalised means of their members under the assignments a"""
    c = c.copy()
    for l in np.unique(a):
        mem = T[a == l].astype(np.float64)
        c[l] = iv.normalise((np.cumsum(mem, axis=0)[-1] / np.float64(len(mem))).astype(F))[0]
    return c


# ------------------------------------------------------------------ cases 3, 4, 7: the tiny round-robin index, more queries than a slice
ROBIN_NQ = 4096 + 150
ROBIN_K, ROBIN_NPROBE = 5, 2
ROBIN_COUNTS = (3, 0, None, 1, 50, 0, 17)           # hits of the 7 queries of the range search (None: every probed row)
LAB5 = np.array([0, NONE, 1, 7, 2], np.int32)       # a label no row carries (7) and LABEL_NONE among them


def case_robin():
    """rc.case_round_robin(200, 32, 7, 4) -- 200 rows, row i in list i % 4 -- with three groups spread evenly over every list and a
    bitmap that clears a third of the rows"""
    c = rc.case_round_robin(200, 32, QP, 4)
    c["row_labels"] = ((np.arange(200) // 4) % 3).astype(np.int32)
    c["mask"] = (np.arange(200) // 4 + np.arange(200) % 4) % 3 != 1
    return c


# ------------------------------------------------------------------ case 5: the wide search at p k = 65 536, where a slice is 256 queries
WIDE_NLIST, WIDE_N, WIDE_D, WIDE_K = 64, 3000, 16, 1024
WIDE_NQ = 256 + 44


def case_wide(seed=35):
    """3000 Gaussian rows of d = 16, 64 planted random unit centroids, every list probed; three groups"""
    rng = np.random.default_rng(seed)
    c = {"rows": rng.standard_normal((WIDE_N, WIDE_D)).astype(F), "q": rng.standard_normal((QP, WIDE_D)).astype(F), "nlist": WIDE_NLIST,
         "centroids": iv.normalise(rng.standard_normal((WIDE_NLIST, WIDE_D)).astype(F)), "row_labels": (np.arange(WIDE_N) % 3).astype(np.int32)}
    c["assign"] = iv.nearest(c["rows"], c["centroids"])[:, 0]
    return c


# ------------------------------------------------------------------ case 6: more than 1024 lists
LISTS_NLISTS = (1024, 1025, 2500)
LISTS_N, LISTS_D, LISTS_BIG = 6000, 16, 100
LISTS_NQ = 600                                       # at nlist = 1025, nprobe = 1024, k = 29: slices of 564 and 36 queries


def case_lists(nlist, seed=36):
    """6000 Gaussian rows of d = 16 over `nlist` planted random unit centroids: most lists hold a few rows, many one, many none.
    LISTS_BIG of the rows (scattered) are 3 c + noise of the LAST centroid, so the list with the highest number is a long one, and
    query 0 is 2 c + noise of it; the other six queries are Gaussian."""
    rng = np.random.default_rng(seed * 1000 + nlist)
    cen = iv.normalise(rng.standard_normal((nlist, LISTS_D)).astype(F))
    rows = rng.standard_normal((LISTS_N, LISTS_D)).astype(F)
    at = np.sort(rng.choice(LISTS_N, LISTS_BIG, replace=False))
    rows[at] = (3 * cen[-1] + 0.05 * rng.standard_normal((LISTS_BIG, LISTS_D))).astype(F)
    q = rng.standard_normal((QP, LISTS_D)).astype(F)
    q[0] = (2 * cen[-1] + 0.05 * rng.standard_normal(LISTS_D)).astype(F)
    return {"rows": rows, "q": q, "nlist": nlist, "centroids": cen, "planted": at, "assign": iv.nearest(rows, cen)[:, 0]}


def offsets_one_list_per_thread(assign, nlist):
    """the list table's offsets of a scan in which every one of the SCAN_THREADS threads owns ONE list: the lists from SCAN_THREADS on
    are never counted"""
    cnt = np.bincount(np.asarray(assign), minlength=nlist)
    cnt[SCAN_THREADS:] = 0
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(cnt)
    return off


# ------------------------------------------------------------------ case 8: load in chunks
LOAD_N, LOAD_CHUNK = 3000, 1000


def case_load():
    c = rc.case_round_robin(LOAD_N, 32, 9, 8)
    rng = np.random.default_rng(38)
    c["row_labels"] = rng.integers(0, 40, LOAD_N).astype(np.int32)
    c["q_labels"] = rng.integers(0, 40, 9).astype(np.int32)
    c["q_labels"][4] = NONE
    return c
