"""Searches on an index that changes between the calls: search -> add -> search (with and without growth), phi following the
rows and its override, reset and a smaller second life, add_synthetic in between, and the same with CUDA tensors on streams of
their own.  ONE index object lives through each sequence; after every step each search path -- search() at k = 5 with 8 queries
(the one-launch kernel where the row pitch allows it) and with 40, search_wide() at k = 64, range_search() -- is compared, every
query, indices and scores bit for bit, with (a) the oracle's canonical arithmetic over all pairs applied to the rows the index
should hold at that step (tests/lifecycle_cases.py: Reference) and (b) a fresh index built from those rows in one add.

The rows are the planted blocks of tests/lifecycle_cases.py: a cached max |x|^2, max |x - bf16 x|^2, phi or bf16 image that
survives an add or a reset certifies a WRONG top-k on them or drops range members (tests/test_lifecycle_cases_host.py proves it on
NumPy models of the bounds); Gaussian rows would hide it."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import lifecycle_cases as lc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

PLAIN_PATHS = ("search8", "search40", "wide", "range")
F8_PATHS = ("search8", "search40")                      # e4m3 storage is limited to search()
FILTER_PATHS = ("wide_sel", "range_sel", "wide_grp", "range_grp")
# margin_stats() of the live index is compared with the fresh index's on these paths, wherever both dispatched the same kernel
# (test_margin_stats_repeat_on_fresh_indexes shows that two fresh indexes report the same counts there)
STATS_PATHS = ("search8", "search40", "wide", "range")


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same_topk(got, exp, what):
    s, i = (_np(t) for t in got)
    es, ei = exp
    assert s.dtype == np.float32 and i.dtype == np.int64 and s.shape == es.shape and i.shape == ei.shape, what
    for j in range(len(ei)):                                       # per query: the first difference names its query
        assert np.array_equal(i[j], ei[j]), f"{what}: ids of query {j} differ: {i[j][:8]} / {ei[j][:8]}"
        assert np.array_equal(s[j].view(np.int32), es[j].view(np.int32)), f"{what}: scores of query {j} differ: {s[j][:5]} / {es[j][:5]}"


def _same_range(got, exp, what):
    lims, D, I = (_np(t) for t in got)
    el, eD, eI = exp
    assert lims.shape == el.shape and lims[0] == 0, what
    for j in range(len(el) - 1):
        a, b, ea, eb = int(lims[j]), int(lims[j + 1]), int(el[j]), int(el[j + 1])
        assert b - a == eb - ea, f"{what}: query {j} has {b - a} hits, expected {eb - ea}"
        assert np.array_equal(I[a:b], eI[ea:eb]), f"{what}: ids of query {j} differ"
        assert np.array_equal(D[a:b].view(np.int32), eD[ea:eb].view(np.int32)), f"{what}: scores of query {j} differ"
    assert np.array_equal(lims.astype(np.int64), el) and len(D) == len(I) == el[-1], what


def _equal_arrays(a, b, what):
    for x, y in zip(a, b):
        x, y = _np(x), _np(y)
        assert x.shape == y.shape and np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), what


class Live:
    """One index that lives through a sequence, the rows it should hold, and the checks of a step."""

    def __init__(self, d, storage, metric, reserve=None, filters=False, device=False):
        self.fam, self.d, self.storage, self.metric = lc.family(d), d, storage, metric
        self.filters, self.device = filters, device
        self.ix = ram.MipsIndex(d, metric=metric, dtype=storage)
        self.phi = None                                            # the override in force
        self.pending = None                                        # device mode: a search issued and not yet waited for
        self.pieces, self.rows = [], np.zeros((0, d), np.float32)
        self.paths = (F8_PATHS if storage.startswith("fp8") else PLAIN_PATHS) + (FILTER_PATHS if filters else ())
        if device:
            self.s_add, self.s_search = torch.cuda.Stream(), torch.cuda.Stream()
            self.q_dev = torch.from_numpy(self.fam.q).cuda()
            self.ix.set_param("margin_check", 3)
            torch.cuda.synchronize()
        if reserve is not None:
            self.ix.reserve(reserve)

    # ---- changes
    def add(self, piece, rows=None):
        """piece = (block, lo, hi) of the family, or a name with the rows given."""
        x = self.fam.block(piece[0])[piece[1]:piece[2]] if rows is None else rows
        n0 = len(self.rows)
        if self.device:
            xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            torch.cuda.synchronize()                               # the upload is done; the add itself goes to a stream of its own
            with torch.cuda.stream(self.s_add):
                self.ix.add(xd)
                if self.filters:
                    self.ix.set_labels(torch.from_numpy(lc.row_labels(n0 + len(x))[n0:].astype(np.int32)).cuda(), row0=n0)
            self.keep = xd                                         # (alive until the next call on the index orders the streams)
            self.settle()                                          # the search issued BEFORE this add: it saw the rows of its step
        else:
            self.ix.add(x)
            if self.filters:
                self.ix.set_labels(lc.row_labels(n0 + len(x))[n0:], row0=n0)
        self.pieces.append(tuple(piece))
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def settle(self):
        """Device mode: wait for the search that check() left in flight and compare it with ITS step's expectation."""
        if self.pending is not None:
            out, exp, tag = self.pending
            self.pending = None
            self.s_search.synchronize()
            _same_topk(out, exp, tag)

    def add_synthetic(self, n, row0, seed):
        self.ix.add_synthetic(n, row0=row0, seed=seed, kind=synth.KIND_GAUSS)
        self.pieces.append(("synthetic", row0, n, seed))
        self.rows = np.concatenate([self.rows, synth.generate(seed, row0, n, self.d, synth.KIND_GAUSS)])

    def reset(self):
        self.ix.reset()
        self.phi, self.pieces, self.rows = None, [], np.zeros((0, self.d), np.float32)

    # ---- expectations
    def reference(self):
        key = ("gpu-ref", self.d, self.storage, tuple(self.pieces))
        return lc.cached(key, lambda: lc.Reference(lc.stored_queries(self.fam.q, self.storage), lc.stored_rows(self.rows, self.storage)))

    def expected(self, path, ref):
        n, nq = ref.n, lc.NQ
        admit = None
        if path.endswith("_sel"):
            admit = np.tile(lc.row_mask(n)[None, :], (nq, 1))
        elif path.endswith("_grp"):
            admit = lc.admit_groups(lc.row_labels(n), lc.query_labels(nq), "exclude", ram.LABEL_NONE)
        if path == "search8":
            s, i = ref.topk(lc.K_SEARCH, self.metric, self.phi)
            return s[:lc.NQ_TINY], i[:lc.NQ_TINY]
        if path == "search40":
            return ref.topk(lc.K_SEARCH, self.metric, self.phi)
        if path.startswith("wide"):
            return ref.topk(lc.K_WIDE, self.metric, self.phi, admit)
        return ref.range(self.radii(ref), self.metric, self.phi, admit)

    def radii(self, ref):
        blocks = [p for p in self.pieces if len(p) == 3]
        return lc.radii_for(self.fam, ref, self.metric, self.phi, lc.has_block(blocks, "R"), lc.has_block(blocks, "B"))

    # ---- one search of one path on an index
    def run(self, ix, path, ref):
        q = self.q_dev if self.device else self.fam.q
        n = ref.n
        kw = {}
        if path.endswith("_sel"):
            kw["selector"] = lc.row_mask(n)
        elif path.endswith("_grp"):
            kw["groups"] = lc.query_labels(lc.NQ)
        ctx = torch.cuda.stream(self.s_search) if self.device else contextlib.nullcontext()
        with ctx:
            if path == "search8":
                out = ix.search(q[:lc.NQ_TINY], lc.K_SEARCH)
            elif path == "search40":
                out = ix.search(q, lc.K_SEARCH)
            elif path.startswith("wide"):
                out = ix.search_wide(q, lc.K_WIDE, **kw)
            elif self.device:                                      # range_search_into: device outputs, nothing synchronises
                cap = int(self.expected(path, ref)[0][-1]) + 8
                lims = torch.full((lc.NQ + 1,), -7, dtype=torch.int64, device="cuda")
                D = torch.full((cap,), np.nan, dtype=torch.float32, device="cuda")
                I = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
                assert ix.range_search_into(q, self.radii(ref), lims, D, I, **kw) is None
                out = (lims, D, I)
            else:
                out = ix.range_search(q, self.radii(ref), **kw)
        if self.device:
            self.s_search.synchronize()
            assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in out)
            if path.startswith("range"):
                total = int(out[0][-1])
                out = (out[0], out[1][:total], out[2][:total])
        return tuple(_np(t) for t in out)

    def fresh(self):
        ix = ram.MipsIndex(self.d, metric=self.metric, dtype=self.storage)
        if self.device:
            ix.set_param("margin_check", 3)
        ix.add(self.rows)
        if self.phi is not None:
            ix.set_phi(self.phi)
        if self.filters:
            ix.set_labels(lc.row_labels(len(self.rows)))
        return ix

    def check(self, what):
        """Every path on the live index against the oracle, then against a fresh index of the same rows."""
        ref = self.reference()
        n = ref.n
        assert self.ix.ntotal == n == len(self.rows)
        fresh = self.fresh()
        if self.metric == 1:
            assert self.ix.phi() == fresh.phi(), what
            assert self.ix.phi() == (self.phi if self.phi is not None else ref.local_phi), what
        for path in self.paths:
            tag = f"{what}, {path} ({self.storage}, metric {self.metric}, d {self.d}, {n} rows)"
            exp = self.expected(path, ref)
            got = self.run(self.ix, path, ref)
            kernel, stats = self.ix.last_kernel, self.ix.margin_stats()
            ids = got[2] if path.startswith("range") else got[1]
            assert ids.size == 0 or int(ids.max()) < n, f"{tag}: a row past ntotal was returned"
            (_same_range if path.startswith("range") else _same_topk)(got, exp, tag)
            again = self.run(fresh, path, ref)
            _equal_arrays(got, again, f"{tag}: differs from a fresh index")
            assert stats["unresolved"] == 0, (tag, stats)
            if path in STATS_PATHS and fresh.last_kernel == kernel:
                assert fresh.margin_stats() == stats, (tag, kernel, stats, fresh.margin_stats())
        if self.device:
            # one more search, issued once and NOT waited for: the next add arrives on its own stream while this one may still be
            # in flight (the search -> add direction of the stream ordering); add() and the end of the test settle it
            with torch.cuda.stream(self.s_search):
                out = self.ix.search(self.q_dev, lc.K_SEARCH)
            self.pending = (out, self.expected("search40", ref), f"{what}: the search in flight when the next add was issued")
        return ref


def _pad(d):
    return d % 128 == 0


COMBOS = [(s, m, d) for d in (128, 1024) for s in ("bf16", "f32") for m in (0, 1)] + [("f32", 0, 64), ("bf16", 1, 64)]
F8_COMBOS = [("fp8_e4m3", 0, 128), ("fp8_e4m3_docs", 1, 128), ("fp8_e4m3_docs", 0, 1024)]
FILTERED = ("f32", 0, 128)                                          # the combination that also runs with selector= and groups=
_ID = lambda c: f"{c[0]}-m{c[1]}-d{c[2]}"  # noqa: E731


def _stored_equal(live):
    raw = live.ix.rows_raw()
    want = lc.stored_rows(live.rows, live.storage)
    if live.storage == "bf16":
        raw = synth.bf16_bits_to_f32(raw)
    elif live.storage != "f32":
        raw = synth.e4m3_bits_to_f32(raw)
    assert np.array_equal(raw.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------ 0. what the margin_stats comparison rests on
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_margin_stats_repeat_on_fresh_indexes(storage):
    a, b = Live(128, storage, 0), Live(128, storage, 0)
    for live in (a, b):
        for step in lc.SEQ_PLAIN[:3]:
            for piece in step:
                live.add(piece)
    ref = a.reference()
    for path in STATS_PATHS:
        ra, rb = a.run(a.ix, path, ref), b.run(b.ix, path, ref)
        _equal_arrays(ra, rb, path)
        assert a.ix.last_kernel == b.ix.last_kernel and a.ix.margin_stats() == b.ix.margin_stats(), (path, a.ix.margin_stats(), b.ix.margin_stats())


# ------------------------------------------------------------------ 1. search -> add -> search, no growth
@pytest.mark.parametrize("combo", COMBOS + F8_COMBOS, ids=_ID)
def test_search_add_search_without_growth(combo):
    storage, metric, d = combo
    live = Live(d, storage, metric, reserve=sum(hi - lo for step in lc.SEQ_PLAIN for _, lo, hi in step), filters=combo == FILTERED)
    for t, step in enumerate(lc.SEQ_PLAIN):
        for piece in step:
            live.add(piece)
        live.check(f"plain step {t}")
        if t == 0 and storage in ("bf16", "f32") and _pad(d):
            live.run(live.ix, "search8", live.reference())
            assert live.ix.last_kernel.startswith("mips::tiny_search_kernel"), live.ix.last_kernel
    _stored_equal(live)


# ------------------------------------------------------------------ 2. search -> add with growth -> search
@pytest.mark.parametrize("combo", COMBOS, ids=_ID)
def test_search_add_search_across_growth(combo):
    storage, metric, d = combo
    live = Live(d, storage, metric, reserve=lc.SEQ_GROWTH_RESERVE, filters=combo == FILTERED)
    for t, step in enumerate(lc.SEQ_GROWTH):
        for piece in step:
            live.add(piece)
        live.check(f"growth step {t}")
    fresh = live.fresh()
    assert np.array_equal(live.ix.rows_raw().view(np.uint8), fresh.rows_raw().view(np.uint8))   # bit-identical to one add
    _stored_equal(live)
    if live.filters:
        assert np.array_equal(live.ix.labels(), lc.row_labels(len(live.rows)))


# ------------------------------------------------------------------ 3. phi follows the rows; an override stays
@pytest.mark.parametrize("storage,d", [("bf16", 128), ("f32", 128), ("f32", 1024), ("bf16", 64)])
def test_phi_follows_the_rows_and_an_override_stays(storage, d):
    live = Live(d, storage, 1)
    fam = live.fam
    live.add(("A", 0, lc.N_A))
    live.add(("R", 0, lc.NPLANT + lc.NDECOY))
    small = live.check("before the big row").local_phi
    at = int(fam.b_plant_at[0])
    live.add(("B", at, at + 1))                                    # one row of norm ~10^3
    big = live.check("after the big row").local_phi
    assert big > small + 4e5 and live.ix.phi() == big
    live.ix.set_phi(lc.PHI_OVERRIDE)
    live.phi = lc.PHI_OVERRIDE
    live.check("override")
    live.add(("X", 0, 1))                                          # a larger row still: the override stays
    bigger = live.reference().local_phi
    assert big < bigger < lc.PHI_OVERRIDE
    live.check("override, after a larger row")
    live.ix.clear_phi()
    live.phi = None
    live.check("override cleared")
    assert live.ix.phi() == bigger


# ------------------------------------------------------------------ 4. reset, then a smaller index
@pytest.mark.parametrize("combo", COMBOS + F8_COMBOS, ids=_ID)
def test_reset_then_a_smaller_index(combo):
    storage, metric, d = combo
    live = Live(d, storage, metric, filters=combo == FILTERED)
    fam = live.fam
    for piece in lc.SEQ_RESET_FIRST:
        live.add(piece)
    live.check("first life")
    if storage == "f32":
        # the near-duplicate search that arms the stage-1 skip (tests/test_gpu_parity.py::test_f32_exact_two_stage_near_duplicates):
        # every one of the 80 queries is flagged, so the next searches skip stage 1 -- reset() does not clear that
        arm = lc.cached(("arm-ref", d, tuple(live.pieces)), lambda: lc.Reference(fam.q_arm, live.rows))
        exp = arm.topk(lc.K_SEARCH, metric)
        _same_topk(live.ix.search(fam.q_arm, lc.K_SEARCH), exp, "arming search")
        st = live.ix.margin_stats()
        assert st["flagged"] >= 64 and st["unresolved"] == 0, st
        _same_topk(live.ix.search(fam.q_arm, lc.K_SEARCH), exp, "armed search")
        assert live.ix.last_kernel.startswith("mips::scan_kernel<"), live.ix.last_kernel     # stage 1 skipped
    live.reset()
    assert live.ix.ntotal == 0
    if live.filters:
        try:                                                       # the labels are gone: empty, or refused
            assert len(live.ix.labels()) == 0
        except (ValueError, RuntimeError):
            pass
    for piece in lc.SEQ_RESET_SECOND:
        live.add(piece)
    assert live.ix.ntotal == 1037
    if live.filters:
        assert np.array_equal(live.ix.labels(), lc.row_labels(1037))
    live.check("second life")                                      # whatever path last_kernel names: exact, ids < ntotal, = fresh
    _stored_equal(live)


def test_labels_do_not_survive_a_reset():
    live = Live(128, "bf16", 0)
    for piece in lc.SEQ_RESET_FIRST:
        live.add(piece)
    live.ix.set_labels(lc.row_labels(len(live.rows)))
    live.reset()
    for piece in lc.SEQ_RESET_SECOND:
        live.add(piece)
    with pytest.raises(ValueError):                                # rows without a label: refused, not answered from old labels
        live.ix.search_wide(live.fam.q, lc.K_WIDE, groups=lc.query_labels(lc.NQ))
    with pytest.raises(ValueError):
        live.ix.range_search(live.fam.q, 0.0, groups=lc.query_labels(lc.NQ))
    live.filters, live.paths = True, FILTER_PATHS
    live.ix.set_labels(lc.row_labels(1037)[::-1].copy())           # other labels than the first life's ...
    live.ix.set_labels(lc.row_labels(1037))                        # ... and the ones the expectation uses (a rewrite)
    live.check("labels of the second life")


# ------------------------------------------------------------------ 5. add_synthetic in between
@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("metric", [0, 1])
def test_add_synthetic_in_between(storage, metric):
    live = Live(128, storage, metric)
    live.add(("A", 0, 1037))
    before = live.check("before add_synthetic").local_phi
    live.add_synthetic(lc.SYNTH_ROWS, lc.SYNTH_ROW0, lc.SYNTH_SEED)  # Gaussian rows of norm ~ sqrt(d): the maximum norm rises
    after = live.check("after add_synthetic").local_phi
    assert after > 20 * before
    live.add(("R", 0, lc.NPLANT + lc.NDECOY))
    live.check("after the residual rows")
    _stored_equal(live)


# ------------------------------------------------------------------ 6. device tensors, adds and searches on different streams
@pytest.mark.parametrize("combo", [("f32", 0, 128), ("bf16", 1, 128), ("f32", 1, 1024), ("bf16", 0, 1024)], ids=_ID)
def test_device_calls_on_other_streams_see_whole_updates(combo):
    """Sequence 1 with CUDA tensors in and out under margin_check = 3: the searches (range_search_into included) run on one
    non-default stream, every add (and set_labels) on another, reserve on the null stream.  An add is never followed by a host
    synchronisation before the searches of its step (add -> search), and the last search of a step is left in flight while the
    next add is issued (search -> add); the other searches of a step are waited for before they are compared.  Each call is
    issued once and in order -- the index orders the streams itself."""
    storage, metric, d = combo
    live = Live(d, storage, metric, reserve=sum(hi - lo for step in lc.SEQ_PLAIN for _, lo, hi in step), filters=combo == FILTERED, device=True)
    for t, step in enumerate(lc.SEQ_PLAIN):
        for piece in step:
            live.add(piece)
        live.check(f"device step {t}")
    live.settle()
    torch.cuda.synchronize()
    _stored_equal(live)
