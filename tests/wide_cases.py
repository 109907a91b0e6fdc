"""Input builders of tests/test_wide_orders_host.py and tests/test_gpu_wide_orders.py: rows in an ORDER, and in a multiplicity,
that the Gaussian rows of the other wide-search tests never have.  Not a test file; no GPU is needed to import it.  Every builder
is deterministic, NumPy-only, and returns float32 arrays already rounded to bf16 (the oracle and an index of either storage see
the same values).

  trending   rows whose score under one direction u climbs with the row number: for the queries along +u nearly every row of
             every chunk beats the pool's threshold (a flood in every chunk, not only in the first), for the queries along -u
             none does after the first chunk, and the Gaussian queries lie between them (their random component along u makes
             them rise or fall mildly: shares of 0.2 .. 0.55 measured) -- three kinds of lane side by side in every wave.
  floods     R distinct rows, each stored m times (row i is vector i % R).  With m above the pool size the k-th and the k'-th
             pool entry of EVERY query are copies of one vector: every certificate fails and every query is settled exactly.

flood_shares is the CPU measure of what the first construction claims (tests/test_wide_orders_host.py asserts it)."""
import numpy as np

from oracle import synth

TREND_SEED = 20240611
FLOOD_SEED = 20240612
TREND_RISE = 1000.0       # what the score of a row under the query u gains from the first row to the last


def _bf16(a):
    return synth.round_to_bf16(np.ascontiguousarray(a, dtype=np.float32))


def trending(n, d, nq, seed=TREND_SEED):
    """-> (x [n, d], q [nq, d], u [d]).  x_i = g_i + (A i / n) u with g_i standard normal, u one random bf16 direction and
    A = TREND_RISE / |u|^2: u . x_i climbs by TREND_RISE over the index against noise of about |u|.  Query j is
    +u + 0.1 noise (j % 3 == 0: ascending), -u + 0.1 noise (j % 3 == 1: descending) or plain Gaussian (j % 3 == 2)."""
    rng = np.random.default_rng(seed)
    u = _bf16(rng.standard_normal(d))
    amp = TREND_RISE / float(np.dot(u.astype(np.float64), u.astype(np.float64)))
    ramp = (amp * np.arange(n, dtype=np.float64) / n)[:, None]
    x = _bf16(rng.standard_normal((n, d)) + ramp * u.astype(np.float64)[None, :])
    noise = rng.standard_normal((nq, d))
    kind = np.arange(nq) % 3
    sign = np.where(kind == 0, 1.0, np.where(kind == 1, -1.0, 0.0))[:, None]
    scale = np.where(kind == 2, 1.0, 0.1)[:, None]
    q = _bf16(sign * u.astype(np.float64)[None, :] + scale * noise)
    return x, q, u


def floods(R, m, d, nq, seed=FLOOD_SEED):
    """-> (x [R m, d], q [nq, d], v [R, d]).  R distinct Gaussian bf16 rows v, row i of x is v[i % R]: every chunk of every size
    holds copies of every vector, and the m copies of vector g are the rows g, g + R, g + 2 R, ..."""
    rng = np.random.default_rng(seed)
    v = _bf16(rng.standard_normal((R, d)))
    assert len(np.unique(v, axis=0)) == R
    x = np.ascontiguousarray(v[np.arange(R * m) % R])
    q = _bf16(rng.standard_normal((nq, d)))
    return x, q, v


def floods_graded(R, m, d, nq, seed=FLOOD_SEED):
    """floods for the fp32-exact index, the one builder whose rows are NOT bf16 values: copy c of vector g is
    float32(v[g] (1 + c 2^-19)), c < m <= 512.  The factor stays below half a bf16 step, so every copy has the bf16 image v[g] and
    the scan (which reads that image) scores all copies of a vector alike and keeps the LOWEST rows -- while the canonical float32
    score grows with c wherever q . v[g] > 0: the true top k are the HIGHEST copies, most of them outside a pool of k' < m
    entries.  What the first pass returns is therefore wrong for every query, and only the settlement can put it right."""
    assert m <= 512
    x, q, v = floods(R, m, d, nq, seed)
    c = (np.arange(R * m) // R).astype(np.float64)
    xg = (x.astype(np.float64) * (1.0 + c * 2.0 ** -19)[:, None]).astype(np.float32)
    assert np.array_equal(_bf16(xg), x)
    return np.ascontiguousarray(xg), q, v


def flood_shares(x, q, kp, block=8192):
    """-> float64 [nq, number of blocks]: per block of `block` rows, the share of its rows whose score (float64 inner product)
    beats the kp-th best score among ALL EARLIER rows -- the threshold a pool of kp entries holds when the block begins.  The
    first block has no threshold (share 1); a last, shorter block is measured like the others."""
    s = q.astype(np.float64) @ x.astype(np.float64).T
    n = x.shape[0]
    starts = list(range(0, n, block))
    out = np.ones((q.shape[0], len(starts)))
    for b, r0 in enumerate(starts):
        if r0 < kp:
            continue
        tau = -np.partition(-s[:, :r0], kp - 1, axis=1)[:, kp - 1]
        out[:, b] = (s[:, r0:r0 + block] > tau[:, None]).mean(axis=1)
    return out


def run_mask(n, keep=300, drop=300):
    """bool [n]: runs of `keep` selected rows followed by `drop` cleared ones.  Runs of 300 cleared rows cover whole 128-row
    tiles, which the masked scan must step over."""
    return (np.arange(n) % (keep + drop)) < keep
