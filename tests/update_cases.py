"""Inputs, the NumPy restatement and the deliberately wrong restatements of tests/test_update_host.py and tests/test_gpu_update*.py:
rows overwritten in place by id (include/mips_hip_write.h).  Not a test file; NumPy only, no GPU is needed to import it.

The restatement is the definition itself, the sequential loop: for p = 0 .. n - 1, if 0 <= ids[p] - idx_offset < ntotal, row
ids[p] - idx_offset becomes x[p].  `wrong=` names one mistake an implementation could make; tests/test_update_host.py shows that
every one of them changes the outcome of at least one case below, i.e. that the GPU tests -- which compare with a FRESH index of the
restatement's final rows -- can fail:

  first_wins       of several positions that name one row the first writes it (the loop leaves the LAST)
  offset_ignored   idx_offset is not subtracted
  clamp            an id >= ntotal is clamped to the last row instead of skipped
  truncate32       the int64 id is cut to 32 bits: 2^32 + 3 writes row 3
  image_stale      the bf16 image of an fp32-exact index keeps the old row (stage 1 of the two-stage search scans it)
  xmax2_stale      the cached norm bound max |x|^2 keeps its old value (too small: the margin check certifies a wrong top-k)
  phi_stale        phi keeps its old value (every L2 distance moves with phi)

The stale-cache cases stand on the planted rows of tests/lifecycle_cases.py (decoys the scan ranks first, the truth last), imported,
not edited: the final rows of the "norm" case ARE the rows of its step (A, R, B), reached by overwriting placeholder rows."""
import numpy as np

import lifecycle_cases as lc
from oracle import synth

F32 = np.float32
NTOTAL, D, D_WIDE = 3000, 200, 768      # a ragged last 128-row tile, padding columns behind d; one case at the headline width
OFFSET = 1 << 33                        # the non-zero idx_offset of the cases: a shard that starts beyond 2^32
MARK_BLOCK, SCATTER_BLOCK = 256, 4      # positions one workgroup of pass A / pass B covers (UPD_THREADS, UPD_WAVES)
WRONG_LOOP = ("first_wins", "offset_ignored", "clamp", "truncate32")
WRONG_CACHE = ("image_stale", "xmax2_stale", "phi_stale")


# ------------------------------------------------------------------ the restatement
def local_rows(ids, idx_offset, ntotal, wrong=None):
    """int64 [n]: the local row every position names, -1 for "no row"."""
    out = np.full(len(ids), -1, np.int64)
    for p, i in enumerate(np.asarray(ids, np.int64).tolist()):       # Python ints: no overflow whatever the id
        local = i if wrong == "offset_ignored" else i - int(idx_offset)
        if wrong == "truncate32":
            local &= 0xffffffff
        if wrong == "clamp" and local >= ntotal:
            local = ntotal - 1
        if 0 <= local < ntotal:
            out[p] = local
    return out


def apply_update(rows, ids, x, idx_offset=0, wrong=None):
    """-> (the rows afterwards, the number of distinct rows written).  `rows` is not modified."""
    out = np.array(rows, copy=True)
    local = local_rows(ids, idx_offset, len(rows), wrong)
    written = set()
    for p, r in enumerate(local.tolist()):
        if r < 0 or (wrong == "first_wins" and r in written):
            continue
        out[r] = x[p]
        written.add(r)
    return out, len(written)


def winners(ids, idx_offset, ntotal):
    """bool [n]: the positions whose row value stands at the end (the highest position of every named row)."""
    local = local_rows(ids, idx_offset, ntotal)
    win = np.zeros(len(ids), bool)
    seen = set()
    for p in range(len(ids) - 1, -1, -1):
        if local[p] >= 0 and local[p] not in seen:
            win[p] = True
            seen.add(local[p])
    return win


# ------------------------------------------------------------------ id sets
def id_sets(ntotal=NTOTAL, idx_offset=0):
    """{name: int64 ids}: n = 0, 1, 64, 65, 1000; rows 0 and ntotal - 1; -1, ntotal, 2^32 + 3 and a negative id mixed in (as the
    caller writes them: relative to idx_offset where they are meant as rows of another shard); duplicates, up to 5 copies of one
    id, at positions either side of a workgroup border of pass A (255 | 256) and of pass B (3 | 4)."""
    rng = np.random.default_rng([20250311, ntotal])
    off = int(idx_offset)
    junk = [-1, off + ntotal, off + (1 << 32) + 3, off - 5, -(1 << 62)]
    sets = {"n0": np.zeros(0, np.int64), "n1": np.array([off + ntotal - 1], np.int64)}
    a = rng.choice(np.arange(1, ntotal - 1), 62, replace=False)
    sets["n64"] = off + np.concatenate([[0], a, [ntotal - 1]]).astype(np.int64)             # distinct, both ends
    legit = rng.choice(np.setdiff1d(np.arange(ntotal - 1), [3]), 56, replace=False)          # (row 3 and the last row stay free:
    b = np.concatenate([off + legit, junk]).astype(object)                                  #  truncate32 and clamp would write them)
    b = b[rng.permutation(len(b))]
    dup = int(b[[i for i, v in enumerate(b) if 0 <= v - off < ntotal][0]])
    sets["n65"] = np.array(list(b) + [dup] * 4, dtype=np.int64)                             # 61 + 4 copies of one id at the end
    c = (off + rng.integers(4, ntotal - 1, 1000)).astype(np.int64)                          # random: some rows twice by chance
    five = off + 1717
    for p in (SCATTER_BLOCK - 1, SCATTER_BLOCK, MARK_BLOCK - 1, MARK_BLOCK, 999):
        c[p] = five                                                                         # 5 copies across both borders
    c[2 * MARK_BLOCK - 1] = c[2 * MARK_BLOCK] = off + 2                                      # a pair across the next border
    c[0], c[1] = off + ntotal - 1, off + 0                                                  # both ends, early ...
    for p, j in zip((500, 501, 700, 998), junk):
        c[p] = j                                                                            # ... junk later (clamp: the last row)
    sets["n1000"] = c
    return sets


def new_rows(n, d, seed=1):
    """float32 [n, d], Gaussian, every row different: the row a position carries names the position."""
    return synth.generate(77 + seed, 0, max(n, 1), d, synth.KIND_GAUSS)[:n].astype(F32) * F32(0.75)


def base_rows(ntotal=NTOTAL, d=D):
    return lc.cached(("upd-base", ntotal, d), lambda: synth.generate(5, 0, ntotal, d, synth.KIND_GAUSS).astype(F32))


# ------------------------------------------------------------------ the cached scalars: what the index keeps next to the rows
class State:
    """rows (float32, as an fp32-exact index holds them), the bf16 image of the two-stage search, the two row-norm bounds and
    phi.  The right update keeps the bounds as UPPER bounds (the written rows folded in) and phi exact."""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, F32)
        self.image = synth.round_to_bf16(self.rows)
        self.xmax2, self.dres2 = lc.scalars(self.rows)
        self.phi = float(lc.orc.sumsq_canonical(self.rows).max())

    def updated(self, ids, x, idx_offset=0, wrong=None):
        new = State.__new__(State)
        new.rows, _ = apply_update(self.rows, ids, x, idx_offset, wrong if wrong in WRONG_LOOP else None)
        win = winners(ids, idx_offset, len(self.rows))
        rows_written = local_rows(ids, idx_offset, len(self.rows))[win]
        new.image = self.image.copy()
        if wrong != "image_stale":
            new.image[rows_written] = synth.round_to_bf16(new.rows[rows_written])
        wx, wd = lc.scalars(new.rows[rows_written]) if len(rows_written) else (0.0, 0.0)
        new.xmax2 = self.xmax2 if wrong == "xmax2_stale" else max(self.xmax2, wx)
        new.dres2 = max(self.dres2, wd)
        new.phi = self.phi if wrong == "phi_stale" else float(lc.orc.sumsq_canonical(new.rows).max())
        return new


def model_search(state, q, k=lc.K_SEARCH, pool=32):
    """What search() of an fp32-exact inner-product index answers for ONE float32 query, in the model of
    tests/test_lifecycle_cases_host.py: stage 1 ranks by bf16(q) . image, the pool is its best `pool` rows, the margin check
    (lc.search_certified with the bound lc.bound_e of the cached scalars) certifies the pool's exact top-k or sends the query to
    the exact pass, which returns the truth.  -> (ids [k], certified?)"""
    q = np.asarray(q, F32)[None, :]
    exact = lc.all_dots(q, state.rows)[0]
    scan = (synth.round_to_bf16(q).astype(np.float64) @ state.image.astype(np.float64).T)[0]
    by_scan = np.argsort(-scan, kind="stable")
    members = by_scan[:pool]
    order = members[np.lexsort((members, -exact[members].astype(F32)))]
    tk = exact[order[k - 1]]
    e = float(lc.bound_e(state.rows.shape[1], lc.orc.sumsq_canonical(q)[0], state.xmax2, state.dres2, lc.query_err2(q)[0]))
    if lc.search_certified(scan[by_scan[pool]], e, tk):
        return order[:k], True
    truth = np.lexsort((np.arange(len(exact)), -exact.astype(F32)))
    return truth[:k], False


# ------------------------------------------------------------------ the stale-cache cases
PLACEHOLDERS = lc.NPLANT + lc.NDECOY     # rows of a planted block


def norm_case(d=128):
    """(rows before, ids, new rows, planted queries): blocks A and R and 368 plain placeholder rows; the update turns the
    placeholders into block B -- rows of 10^3 times the norm, which the B-planted queries q = bf16(q) + delta meet.  The final
    rows are those of the lifecycle step (A, R, B)."""
    fam = lc.family(d)
    before = np.concatenate([fam.A, fam.R, fam.A2[:PLACEHOLDERS]])
    at = lc.N_A + PLACEHOLDERS
    return before, np.arange(at, at + PLACEHOLDERS, dtype=np.int64), fam.B, [fam.q[j] for j in fam.b_queries]


def image_case(d=128):
    """(rows before, ids, new rows, query): block A; ONE row becomes a beacon, the bf16 image of a Gaussian query scaled to the
    norm of its neighbours -- its own bf16 image decides that it is found: the old image's score is that of a plain row."""
    fam = lc.family(d)
    j = 0                                                                # (0 % 5: a Gaussian float32 query)
    beacon = synth.round_to_bf16(fam.q[j]) * F32(2.0 ** -3 if d <= 128 else 2.0 ** -5)
    return fam.A, np.array([777], np.int64), beacon[None, :].astype(F32), fam.q[j]


def phi_case(d=128):
    """(rows before, ids, new rows): block A and the extra row of maximal norm (phi ~ 4 10^6); the update makes it a plain row,
    so phi must FALL to block A's maximum."""
    fam = lc.family(d)
    return np.concatenate([fam.A, fam.extra]), np.array([lc.N_A], np.int64), fam.A2[:1]
