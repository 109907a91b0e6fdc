"""CPU proof that tests/test_gpu_lifecycle.py can fail: the planted blocks of tests/lifecycle_cases.py separate a STALE cached
scalar (max |x|^2, max |x - bf16 x|^2, phi of the rows before an add) from the FRESH one in NumPy restatements of the very
bounds the kernels compute -- with the fresh scalars every planted row is inside what the scan is guaranteed to keep, with the
stale ones every planted row falls outside, the wrong top-k is CERTIFIED and the range threshold lies above the planted rows' scan
scores.  Also: the inputs hold exactly the intended values, bf16(h + rho) = h under an independent rounding, the reference is
orc.search_exact_bruteforce's, and the sequences cross the tile, growth and cache boundaries their comments claim.  No GPU."""
import os
import sys

import numpy as np
import pytest

from oracle import mips_oracle as orc
from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import hook_cases as hc
    import lifecycle_cases as lc
finally:
    sys.path.pop(0)

F32, F64 = np.float32, np.float64
DIMS = lc.DIMS


def _ref(d, names):
    """Reference of the fp32-exact index that holds the named blocks, whole, in that order."""
    fam = lc.family(d)
    adds = [(b, 0, len(fam.block(b))) for b in names]
    return adds, lc.cached(("host-ref", d, names), lambda: lc.Reference(fam.q, lc.rows_of(fam, adds)))


# ------------------------------------------------------------------ 1. the inputs are what the docstring says
@pytest.mark.parametrize("d", DIMS)
def test_inputs_hold_the_intended_values_exactly(d):
    fam = lc.family(d)
    body, M, N = fam.body, fam.M, fam.N
    assert len(M) == len(N) == fam.half and len(np.intersect1d(M, N)) == 0
    r = fam.g_body * fam.ph
    assert set(np.unique(r)) == {-1.0, 1.0} and r[M].sum() == 0 and r[N].sum() == 0        # the families are orthogonal
    lv = lc.decoy_levels()
    for blk, plant_at, decoy_at, unit in ((fam.R, fam.r_plant_at, fam.r_decoy_at, fam.unit_r), (fam.B, fam.b_plant_at, fam.b_decoy_at, fam.unit_b)):
        assert blk.dtype == F32 and blk.shape == (lc.NPLANT + lc.NDECOY, d)
        x = blk.astype(F64)
        # the level columns, read back from the float32 array, carry the level (x QSMALL of the query = level units)
        assert np.array_equal(x[plant_at][:, body:].sum(1) * lc.QSMALL, np.arange(lc.NPLANT) * unit)
        assert np.array_equal(x[decoy_at][:, body:].sum(1) * lc.QSMALL, lv * unit)
    R, B = fam.R.astype(F64), fam.B.astype(F64)
    assert np.array_equal(R[fam.r_plant_at][:, :body], np.tile(fam.g_body * (1 + lc.RHO), (lc.NPLANT, 1)))       # h + rho survives float32
    assert np.array_equal(R[fam.r_decoy_at][:, :body], np.tile(fam.g_body, (lc.NDECOY, 1)))
    big = np.zeros(body)
    big[M] = fam.S * fam.ph[M]
    dec = np.zeros(body)
    dec[N] = fam.S * fam.ph[N]
    assert np.array_equal(B[fam.b_plant_at][:, :body], np.tile(big, (lc.NPLANT, 1))) and np.array_equal(B[fam.b_decoy_at][:, :body], np.tile(dec, (lc.NDECOY, 1)))
    p = fam.ph.copy()
    p[M] *= 1 + lc.RHO
    assert np.array_equal(fam.p.astype(F64)[:body], p) and np.array_equal(fam.g.astype(F64)[:body], fam.g_body)
    assert (fam.p[body:] == lc.QSMALL).all() and (fam.g[body:] == lc.QSMALL).all()
    for j in fam.r_queries:
        assert np.array_equal(fam.q[j].astype(F64), fam.g.astype(F64) * fam.scale[j])
    for j in fam.b_queries:
        assert np.array_equal(fam.q[j].astype(F64), fam.p.astype(F64) * fam.scale[j])
    assert fam.r_queries[:2] == [1, 6] and fam.b_queries[:2] == [3, 8]          # both kinds among the first NQ_TINY queries
    assert sum(j < lc.NQ_TINY for j in fam.r_queries) == 2 and sum(j < lc.NQ_TINY for j in fam.b_queries) == 1
    norms = np.sqrt((B[fam.b_plant_at] ** 2).sum(1))
    assert (norms > 700).all() and (norms < 1100).all()                          # "about 10^3"
    assert np.sqrt((fam.A.astype(F64) ** 2).sum(1)).max() < 1.6 and np.sqrt((fam.A2.astype(F64) ** 2).sum(1)).max() < 1.6
    assert not np.array_equal(fam.A[:1037], fam.A2[:1037])
    assert float((fam.extra.astype(F64) ** 2).sum()) == 4 * float((big ** 2).sum()) < lc.PHI_OVERRIDE


@pytest.mark.parametrize("d", DIMS)
def test_bf16_of_the_residual_rows_is_h_under_an_independent_rounding(d):
    fam = lc.family(d)
    body = fam.body
    for x in (fam.A, fam.A2, fam.B, fam.R, fam.extra, fam.q, fam.q_arm):
        assert np.array_equal(hc.bf16_round_bits(x), synth.bf16_bits(synth.round_to_bf16(x)))          # the oracle's rounding = hook_cases' own
    hR = hc.to_bf16(fam.R)
    assert np.array_equal(hR[fam.r_plant_at][:, :body].astype(F64), np.tile(fam.g_body, (lc.NPLANT, 1)))     # bf16(h + rho) = h
    assert np.array_equal(hR[fam.r_plant_at][:, body:], fam.R[fam.r_plant_at][:, body:])
    assert np.array_equal(hR[fam.r_decoy_at], fam.R[fam.r_decoy_at])              # decoys, big rows, plain rows: bf16 values
    for x in (fam.A, fam.A2, fam.B, fam.extra, fam.g[None, :]):
        assert np.array_equal(hc.to_bf16(x), x)
    assert np.array_equal(hc.to_bf16(fam.p[None, :])[0, :body].astype(F64), fam.ph)                            # bf16(p) = ph
    dres2 = lc.scalars(fam.R)[1]
    assert dres2 == body * lc.RHO ** 2 and lc.scalars(fam.A)[1] == 0.0 and lc.scalars(fam.B)[1] == 0.0


# ------------------------------------------------------------------ 2. the reference is the oracle's
@pytest.mark.parametrize("metric", [0, 1])
def test_reference_is_search_exact_bruteforce(metric):
    fam = lc.family(64)
    # (L2 without block B: next to phi ~ 10^6 hundreds of float32 distances tie, and the brute force's L2 form re-ranks only the
    # 16 rows behind the k-th inner product -- the all-pairs ranking is the definition, the brute force its check where it holds)
    _, ref = _ref(64, ("A", "R", "B") if metric == 0 else ("A", "R"))
    for k in (lc.K_SEARCH, lc.K_WIDE):
        s, i = ref.topk(k, metric)
        bs, bi = orc.search_exact_bruteforce(fam.q, ref.rows, k, metric=metric)
        assert np.array_equal(i, bi) and np.array_equal(s.view(np.int32), bs.view(np.int32))
    vals = ref.values(metric)
    radii = lc.radii_for(fam, ref, metric, None, True, metric == 0)
    lims, D, I = ref.range(radii, metric)
    for j in range(lc.NQ):                                          # the construction of tests/test_gpu_range.py, spelled out
        ids = np.flatnonzero(vals[j] < radii[j] if metric == 1 else vals[j] > radii[j])
        assert np.array_equal(I[lims[j]:lims[j + 1]], ids) and np.array_equal(D[lims[j]:lims[j + 1]], vals[j][ids])
    assert lims[-1] == len(D) == len(I) and 0 < lims[-1] < lc.NQ * ref.n
    few = lc.Reference(fam.q[:3], ref.rows[:3])
    s, i = few.topk(5, metric)
    assert (i[:, 3:] == -1).all() and np.isinf(s[:, 3:]).all() and (i[:, :3] >= 0).all()      # padding when k > n


# ------------------------------------------------------------------ 3. stale scalars lose the planted rows, fresh ones keep them
def _scalar_cases(d, which):
    """(names of the blocks in the index, planted queries, planted rows, decoy rows, {name: (xmax2, dres2)}) of the step that adds
    family `which`: "fresh" = the scalars of the rows after the add, the others what a missing invalidation would leave."""
    fam = lc.family(d)
    if which == "R":
        names, before = ("A", "R"), fam.A
        adds, ref = _ref(d, names)
        off = lc.block_offset(adds, "R")
        plant, decoy, queries = off + fam.r_plant_at, off + fam.r_decoy_at, fam.r_queries
    else:
        names, before = ("A", "R", "B"), np.concatenate([fam.A, fam.R])
        adds, ref = _ref(d, names)
        off = lc.block_offset(adds, "B")
        plant, decoy, queries = off + fam.b_plant_at, off + fam.b_decoy_at, fam.b_queries
    fresh, old = lc.scalars(ref.rows), lc.scalars(before)
    sc = {"fresh": fresh, "both stale": old}
    if which == "R":
        sc["dres2 stale"] = (fresh[0], old[1])
        assert old[1] == 0.0 < fresh[1]
    else:
        sc["xmax2 stale"] = (old[0], fresh[1])
        assert old[0] * 400 < fresh[0]
    return fam, ref, queries, plant, decoy, sc


@pytest.mark.parametrize("which", ["R", "B"])
@pytest.mark.parametrize("d", DIMS)
def test_planted_rows_are_inside_the_fresh_bound_and_outside_the_stale_one(d, which):
    fam, ref, queries, plant, decoy, sc = _scalar_cases(d, which)
    scan = lc.scan_scores(fam.q, ref.rows)
    qerr2 = lc.query_err2(fam.q)
    unit = fam.unit_r if which == "R" else fam.unit_b
    shift = fam.shift_r if which == "R" else fam.shift_b
    assert len(queries) == 8
    for j in queries:
        s = fam.scale[j]
        exact, a = ref.dot[j], scan[j]
        # the scores are the construction's: scan = base + level, exact = scan (+ shift on the planted rows)
        base = fam.base_r if which == "R" else fam.base_b
        assert np.array_equal(a[plant], s * (base + np.arange(lc.NPLANT) * unit)) and np.array_equal(exact[plant], a[plant] + s * shift)
        assert np.array_equal(a[decoy], s * (base + lc.decoy_levels() * unit)) and np.array_equal(exact[decoy], a[decoy])
        others = np.setdiff1d(np.arange(ref.n), np.concatenate([plant, decoy]))
        assert exact[others].max() < a[plant].min() or which == "B"            # (B: only the extra row, absent here, would beat them)
        assert a[decoy].min() > a[plant].max() and exact[plant].min() > exact[decoy].max() > exact[others].max()
        for name, (xmax2, dres2) in sc.items():
            e = float(lc.bound_e(d, ref.qq[j], xmax2, dres2, qerr2[j]))
            inside = exact[plant] <= a[plant] + e
            assert inside.all() if name == "fresh" else not inside.any(), (name, j, e / (s * unit))
            if name != "fresh":
                assert e < 0.6 * lc.LEVEL_GAP * s * unit, (name, j, e / (s * unit))    # the gap of the level plan outruns the stale bound


@pytest.mark.parametrize("which", ["R", "B"])
@pytest.mark.parametrize("d", DIMS)
def test_stale_scalars_certify_the_wrong_top_k(d, which):
    """search(): the pool is the K' best scan scores (decoys all), tk the exact dot of the 5th best of them; whatever the bound
    on the rows outside the pool is -- at most the 6th best scan score, at least the planted row's own -- the stale e certifies
    and the fresh e cannot.  search_wide(): the same with k' = wide_pool(64) and the pool's worst scan score."""
    fam, ref, queries, plant, decoy, sc = _scalar_cases(d, which)
    scan = lc.scan_scores(fam.q, ref.rows)
    qerr2 = lc.query_err2(fam.q)
    true5 = ref.topk(lc.K_SEARCH, 0)[1]
    kp = lc.wide_pool(lc.K_WIDE, True)
    assert kp == 336 < lc.NDECOY
    for j in queries:
        a, exact = scan[j], ref.dot[j]
        by_scan = np.argsort(-a, kind="stable")
        assert set(true5[j]) <= set(plant)                            # the truth: planted rows only
        for name, (xmax2, dres2) in sc.items():
            e = float(lc.bound_e(d, ref.qq[j], xmax2, dres2, qerr2[j]))
            for pool in lc.POOLS:
                members = by_scan[:pool]
                assert set(members) <= set(decoy)
                tk = np.sort(exact[members])[::-1][lc.K_SEARCH - 1]
                hi_bnd, lo_bnd = a[by_scan[lc.K_SEARCH]], a[plant].max()
                if name == "fresh":
                    assert not lc.search_certified(lo_bnd, e, tk), (name, j, pool)
                else:
                    assert lc.search_certified(hi_bnd, e, tk), (name, j, pool)
            members = by_scan[:kp]
            assert set(members) <= set(decoy)
            for metric in (0, 1):
                vals = ref.values(metric)[j][members]
                outk = (np.sort(vals) if metric == 1 else np.sort(vals)[::-1])[lc.K_WIDE - 1]
                got = lc.wide_certified(a[members].min(), e, outk, ref.qq[j], ref.local_phi, metric == 1)
                wide_truth = set(ref.topk(lc.K_WIDE, metric)[1][j])
                assert set(plant) <= wide_truth
                if name == "fresh":
                    assert not got, (name, j, metric)
                elif metric == 0 or which == "R":                     # (L2 next to phi ~ 10^6: float32 distances tie, no claim)
                    assert got, (name, j, metric)


@pytest.mark.parametrize("which", ["R", "B"])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", DIMS)
def test_stale_scalars_put_the_range_threshold_above_the_planted_rows(d, metric, which):
    fam, ref, queries, plant, decoy, sc = _scalar_cases(d, which)
    scan = lc.scan_scores(fam.q, ref.rows)
    qerr2 = lc.query_err2(fam.q)
    radii = lc.radii_for(fam, ref, metric, None, True, which == "B")
    vals = ref.values(metric)
    lims, D, I = ref.range(radii, metric)
    for j in queries:
        members = set(I[lims[j]:lims[j + 1]])
        assert set(plant) <= members and 10 < len(members & set(decoy)) < 60          # the planted rows ARE members, with some decoys
        assert (vals[j][plant] < radii[j]).all() if metric == 1 else (vals[j][plant] > radii[j]).all()
        for name, (xmax2, dres2) in sc.items():
            e = float(lc.bound_e(d, ref.qq[j], xmax2, dres2, qerr2[j]))
            tau = float(lc.range_tau(radii[j], ref.qq[j], ref.local_phi, metric == 1, e))
            kept = scan[j][plant] > tau                                # the scan appends what beats tau
            assert kept.all() if name == "fresh" else not kept.any(), (name, j, tau)
            assert (scan[j][list(members - set(plant))] > tau).all()   # the decoys that are members pass either way
    # the other queries keep the boundary radii of tests/test_gpu_range.py
    plain = [j for j in range(lc.NQ) if j not in fam.r_queries and j not in fam.b_queries]
    assert np.array_equal(radii[plain], lc.boundary_radii(vals, metric)[plain]) and np.isinf(radii[plain]).sum() >= 2


def test_range_tau_and_the_bound_follow_the_kernels_on_plain_numbers():
    # the two constants of the scan launches of search(): stage 1 has the model's, the three-segment scan its own (and no dres2)
    assert lc.err_c_three_segment(1024) == 3 * 1024 * 2.0 ** -23 + 2.0 ** -16 > 2.9 * lc.err_c(1024, True)
    assert lc.err_c(768, False) == 768 * 2.0 ** -23 and lc.err_c(768, True) == 768 * 2.0 ** -23 * 1.01
    assert lc.bound_e(64, 4.0, 9.0) == 64 * 2.0 ** -23 * 2 * 3
    assert lc.bound_e(64, 4.0, 9.0, 0.25, 0.01) == 1.01 * 64 * 2.0 ** -23 * 6 + 0.5 * 2 + 3.5 * 0.1
    assert lc.range_tau(np.inf, 1.0, 0.0, False, 0.0) == np.inf and lc.range_tau(np.inf, 1.0, 0.0, True, 0.0) == -np.inf
    assert lc.range_tau(-np.inf, 1.0, 0.0, False, 0.0) == -np.inf and lc.range_tau(-np.inf, 1.0, 0.0, True, 0.0) == np.inf
    t = lc.range_tau(1.0, 1.0, 0.0, False, 0.125)
    assert t.dtype == F32 and 0.875 - 3e-7 < float(t) <= 0.875 - 2.0 ** -23                # image - slack - e, rounded down
    t = lc.range_tau(3.0, 2.0, 5.0, True, 0.0)
    assert float(t) < 2.0 and float(t) > 2.0 - 1e-5                                      # (|q|^2 + phi - r) / 2 = 2


def test_equal_float32_distances_next_to_a_large_phi_are_not_certified():
    """Next to phi = 8e6 a float32 distance has steps of 0.5: a dozen rows share the 5th distance and the lowest ROW among them
    is the answer -- a row the pool of 8 best inner products does not hold.  A margin check on the inner products certifies that
    pool (the outside rows' dots are provably lower); on the float32 keys (margin_key_worse) it cannot, and the exact pass
    settles the query.  The override step of test_phi_follows_the_rows_and_an_override_stays[bf16-64] runs this case."""
    fam = lc.family(64)
    at = int(fam.b_plant_at[0])
    rows = lc.stored_rows(np.concatenate([fam.A, fam.R, fam.B[at:at + 1]]), "bf16")
    ref = lc.Reference(lc.stored_queries(fam.q, "bf16"), rows)
    xmax2 = lc.scalars(rows)[0]
    phi, j = lc.PHI_OVERRIDE, 19
    s, i = ref.topk(lc.K_SEARCH, 1, phi)
    by_dot = np.argsort(-ref.dot[j], kind="stable")
    pool = by_dot[:8]
    assert i[j][4] not in pool and (ref.values(1, phi)[j] == s[j][4]).sum() >= 10 and s[j][4] == s[j][3] + 0.5
    tk = np.sort(ref.dot[j][pool])[::-1][lc.K_SEARCH - 1]
    bnd, e = ref.dot[j][by_dot[8]], float(lc.bound_e(64, ref.qq[j], xmax2))
    assert bnd + e < tk                                              # the inner products alone: "certified"
    assert not lc.search_certified(bnd, e, tk, ref.qq[j], phi, True)  # the keys: flagged, the exact pass settles it


# ------------------------------------------------------------------ 4. phi
@pytest.mark.parametrize("d", DIMS)
def test_every_distance_moves_with_phi(d):
    fam = lc.family(d)
    _, before = _ref(d, ("A", "R"))
    rows = np.concatenate([before.rows, fam.B[fam.b_plant_at[:1]]])
    after = lc.Reference(fam.q, rows)
    assert after.local_phi > before.local_phi + 4e5                                      # one big row moves phi by ~10^6
    stale, fresh = after.values(1, before.local_phi), after.values(1)
    assert (stale != fresh).all()                                                        # every query, every row
    assert (after.values(1, lc.PHI_OVERRIDE) != fresh).all() and lc.PHI_OVERRIDE > lc.Reference(fam.q[:1], fam.extra).local_phi
    s0, i0 = after.topk(5, 1, before.local_phi)
    s1, i1 = after.topk(5, 1)
    assert (s0 != s1).all()


# ------------------------------------------------------------------ 5. the sequences cross what they claim to cross
def _grow(capacity, need, exact=False):
    """grow() of csrc/host_state.hpp: capacity after a request for `need` rows."""
    if need <= capacity:
        return capacity
    cap = need if exact else max(need, capacity + capacity // 2)
    return -(-cap // 256) * 256


def test_sequences_cross_tiles_growth_and_the_hi_row_cache():
    n, first = 0, True
    for step in lc.SEQ_PLAIN:
        for b, lo, hi in step:
            n += hi - lo
            if first:
                assert n % 128 == 0                                    # one add ends exactly on a tile boundary
                first = False
        assert n % 128 != 0                                            # no search sees a whole number of tiles
    total = sum(hi - lo for step in lc.SEQ_PLAIN for _, lo, hi in step)
    assert n == total == lc.N_A + 2 * (lc.NPLANT + lc.NDECOY) + 1 and 2000 <= total <= 10000
    # sequence 2: three growths, with 0 = hi_rows < ntotal, 0 < hi_rows < ntotal and hi_rows == ntotal
    cap = _grow(0, lc.SEQ_GROWTH_RESERVE, exact=True)
    assert cap == 1024
    n, hi_rows, seen = 0, 0, []
    for step in lc.SEQ_GROWTH:
        for b, lo, hi in step:
            new = _grow(cap, n + hi - lo)
            if new != cap:
                seen.append("none" if hi_rows == 0 and n > 0 else "some" if hi_rows < n else "all")
                cap = new
            n += hi - lo
        hi_rows = n                                                    # the search converts what is missing
        assert n % 128 != 0
    assert seen == ["none", "some", "all"]
    fam = lc.family(64)
    assert [lc.has_block(sum(lc.SEQ_GROWTH[:t + 1], []), "R") for t in range(3)] == [False, True, True]
    # sequence 4: behind the second life's last row lie big rows of the first life, to the end of the tile
    first_life = lc.rows_of(fam, lc.SEQ_RESET_FIRST)
    second = lc.rows_of(fam, lc.SEQ_RESET_SECOND)
    n2 = len(second)
    assert n2 == 1037 and n2 % 128 != 0 and 2800 < len(first_life) < 3200
    tail = first_life[n2:-(-n2 // 128) * 128].astype(F64)
    assert len(tail) == 115 and (np.sqrt((tail ** 2).sum(1)) > 500 * np.sqrt((second.astype(F64) ** 2).sum(1)).max()).all()
    assert not np.array_equal(lc.stored_rows(first_life[:n2], "bf16"), lc.stored_rows(second, "bf16"))   # stale hi rows would be WRONG rows
    assert lc.has_block(lc.SEQ_RESET_FIRST, "R") and lc.has_block(lc.SEQ_RESET_FIRST, "B") and not lc.has_block(lc.SEQ_RESET_SECOND, "B")


def test_the_arming_queries_cannot_be_certified_with_fresh_scalars():
    """The 80 queries that arm the stage-1 skip before the reset: with block R in the index and FRESH scalars the margin check
    must flag every one of them (their true top-5 are planted rows the pool of 32 cannot hold) -- 80 >= 64 and 80 * 8 > 80."""
    fam = lc.family(128)
    rows = lc.rows_of(fam, lc.SEQ_RESET_FIRST)
    ref = lc.Reference(fam.q_arm, rows)
    scan = lc.scan_scores(fam.q_arm, rows)
    xmax2, dres2 = lc.scalars(rows)
    plant = lc.block_offset(lc.SEQ_RESET_FIRST, "R") + fam.r_plant_at
    assert len(fam.q_arm) == 80 and lc.query_err2(fam.q_arm).max() == 0.0
    for j in range(80):
        by_scan = np.argsort(-scan[j], kind="stable")[:32]
        assert not set(by_scan) & set(plant)
        tk = np.sort(ref.dot[j][by_scan])[::-1][4]
        e = float(lc.bound_e(128, ref.qq[j], xmax2, dres2, 0.0))
        assert not lc.search_certified(scan[j][plant].max(), e, tk)
