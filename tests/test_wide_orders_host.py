"""The constructions of tests/wide_cases.py do what they claim, by the oracle alone (no GPU): a failure of
tests/test_gpu_wide_orders.py cannot be blamed on its inputs.

trending: for the ascending queries at least 0.9 of the rows of every full 8192-row block beat the threshold a pool of k' = 164
entries holds when the block begins (measured: 0.941 .. 0.953), for the descending queries no row after the first block does,
and the data are tie-free (search_exact == search_exact_bruteforce).
floods: the reference result of every query is one score repeated on the k lowest rows of one residue class mod R, and under
the L2 metric the float32 distance of a query's best vector differs from that of its second-best vector -- a tie ACROSS vectors
in float32 would be decided by the row number, behind the k + 16 rows search_exact_bruteforce fetches by inner product: an
artefact of the oracle, not of a kernel.  Asserted for every flood shape the GPU tests use."""
import os
import sys

import numpy as np
import pytest

from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import wide_cases
finally:
    sys.path.pop(0)

K = 100
KP = K + 64           # the pool of a bf16 index at k = 100
BLOCK = 8192


def test_trending_floods_every_block_of_the_ascending_queries_and_none_of_the_descending():
    n, d, nq = 100003, 64, 12
    x, q, u = wide_cases.trending(n, d, nq)
    assert np.abs(x).max() < 64                                            # (measured 46: far inside bf16's range)
    sh = wide_cases.flood_shares(x, q, KP, BLOCK)
    nfull = n // BLOCK
    kind = np.arange(nq) % 3
    up, down, gauss = sh[kind == 0], sh[kind == 1], sh[kind == 2]
    print("ascending, full blocks after the first: min %.4f max %.4f" % (up[:, 1:nfull].min(), up[:, 1:nfull].max()))
    print("descending, blocks after the first: max %.6f" % down[:, 1:].max())
    # a Gaussian query keeps a random component along u (q.u / |u|^2 ~ N(0, 1 / |u|^2): a rise or fall of about 125 against noise
    # of about 8), so these lanes lie anywhere between the two extremes -- printed, not asserted
    print("gaussian, per query over the full blocks after the first: " + ", ".join("%.3f..%.3f" % (r[1:nfull].min(), r[1:nfull].max()) for r in gauss))
    assert (sh[:, 0] == 1.0).all()
    assert (up[:, :nfull] >= 0.9).all()
    assert (down[:, 1:] == 0.0).all()
    assert (gauss[:, 1:nfull] < up[:, 1:nfull].min()).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_trending_is_tie_free(metric):
    x, q, _ = wide_cases.trending(6007, 64, 30)
    es, ei = orc.search_exact(q, x, K, metric=metric)
    bs, bi = orc.search_exact_bruteforce(q, x, K, metric=metric)
    assert np.array_equal(ei, bi) and np.array_equal(es, bs)


def test_run_mask_clears_whole_tiles():
    mask = wide_cases.run_mask(100003)
    tiles = np.concatenate([mask, np.zeros(-len(mask) % 128, bool)]).reshape(-1, 128).sum(axis=1)
    assert (tiles == 0).any() and (tiles == 128).any() and ((tiles > 0) & (tiles < 128)).any()
    assert 0.49 < mask.mean() < 0.51


@pytest.mark.parametrize("R,d,nq", [(20, 64, 600), (350, 32, 300), (20, 64, 4100)])
def test_floods_answer_is_the_lowest_copies_of_one_vector(R, d, nq):
    m = 400
    x, q, v = wide_cases.floods(R, m, d, nq)
    assert x.shape == (R * m, d) and np.array_equal(x[R:2 * R], v)
    # the canonical scores of the R distinct vectors decide everything: x holds nothing else
    ids = np.tile(np.arange(R, dtype=np.int64), (nq, 1))
    dot = orc.canonical_pairs(q, v, ids)
    ip = dot.astype(np.float32)
    phi = orc.sumsq_canonical(x).max()
    dist = (orc.sumsq_canonical(q)[:, None] + phi - 2.0 * dot).astype(np.float32)
    for metric, val in ((0, -ip.astype(np.float64)), (1, dist.astype(np.float64))):
        srt = np.sort(val, axis=1)
        assert (srt[:, 0] < srt[:, 1]).all(), f"metric {metric}: best and second-best vector tie in float32"
    g = np.argmax(dot, axis=1)
    assert np.array_equal(g, np.argmin(dist, axis=1))
    want = g[:, None] + R * np.arange(K)[None, :]
    sub = np.arange(0, nq, max(1, nq // 40))                              # the brute force on a sample: the GPU tests run it whole
    for metric in (0, 1):
        es, ei = orc.search_exact_bruteforce(q[sub], x, K, metric=metric)
        assert np.array_equal(ei, want[sub])
        assert (es == es[:, :1]).all()
        assert np.array_equal(es[:, 0], (ip if metric == 0 else dist)[sub, g[sub]])


def test_graded_floods_answer_is_the_highest_copies_which_the_first_pass_cannot_hold():
    R, d, nq, m = 20, 64, 600, 400
    x, q, v = wide_cases.floods_graded(R, m, d, nq)
    plain = wide_cases.floods(R, m, d, nq)[0]
    assert x.dtype == np.float32 and not np.array_equal(x, plain)
    dot = orc.canonical_pairs(q, v, np.tile(np.arange(R, dtype=np.int64), (nq, 1)))
    g = np.argmax(dot, axis=1)
    assert (dot[np.arange(nq), g] > 1.0).all()                             # the score grows with the copy number
    sub = np.arange(0, nq, 15)
    es, ei = orc.search_exact_bruteforce(q[sub], x, K)
    assert np.array_equal(ei, g[sub, None] + R * (m - 1 - np.arange(K))[None, :])   # copies 399, 398, ..., 300
    assert (np.diff(es, axis=1) < 0).all()
    es, ei = orc.search_exact_bruteforce(q[sub], x, K, metric=1)
    # (two neighbouring copies may round to one float32 distance and then rank by row: the set is that of the inner product)
    assert np.array_equal(np.sort(ei, axis=1), g[sub, None] + R * (m - K + np.arange(K))[None, :])
    # a pool of k' = 381 entries filled with the lowest copies (their bf16 images tie) holds only 81 of these 100 rows
    assert (ei // R >= 381).sum(axis=1).min() == m - 381
