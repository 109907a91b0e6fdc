"""mips_index_update / MipsIndex.update_rows on the GPU.  The contract: after an update the index cannot be told from a FRESH index
of the same type that was given the final rows in order -- every assertion here is bit for bit against such an index, whose rows
are those of the sequential loop (tests/update_cases.py: apply_update).

Part 1, storage: every storage and metric, 3000 rows (a ragged last 128-row tile) of d = 200 (padding columns) and one case at
d = 768; the id sets of update_cases.id_sets (n = 0, 1, 64, 65, 1000, both ends of the index, -1 / ntotal / 2^32 + 3 / negative ids,
up to 5 copies of an id across workgroup borders of the winner pass) in host and device form, with and without idx_offset; after
every call rows_raw() of the whole index (untouched rows and padding with it), reconstruct, labels and the count; then every search
path the storage serves.  Raw inputs (bf16 bits, e4m3 bytes, SQ8 codes), the refusals and the plain-C consumer.

Part 2, the cached scalars: ONE index lives through search -> update -> search on the planted rows of tests/lifecycle_cases.py (the
machinery of tests/test_gpu_lifecycle.py: the all-pairs oracle AND a fresh index after every step).  tests/test_update_host.py shows
on NumPy models that a bf16 image, a norm bound or a phi left stale by the update changes these answers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import lifecycle_cases as lc
    import test_gpu_lifecycle as gl
    import update_cases as uc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

COMBOS = [("bf16", 0), ("bf16", 1), ("f32", 0), ("f32", 1), ("fp8_e4m3", 0), ("fp8_e4m3", 1), ("fp8_e4m3_docs", 0), ("fp8_e4m3_docs", 1),
          ("sq8", 0)]
_ID = lambda c: f"{c[0]}-m{c[1]}"  # noqa: E731


def _make(storage, metric, d, rows=None, like=None):
    """An index of that type; an 'sq8' index gets the range of `like` (or is trained on `rows`): one quantiser for both."""
    ix = ram.MipsIndex(d, metric=metric, dtype=storage)
    if storage == "sq8":
        if like is not None:
            ix.set_sq8_params(*like.sq8_params())
        else:
            ix.train(rows)
    if rows is not None:
        ix.add(rows)
    return ix


def _queries(d, x_new):
    """40 Gaussian queries and 8 of the new rows themselves (an updated row is then a top hit)."""
    q = synth.generate(901, 0, 40, d, synth.KIND_GAUSS).astype(np.float32)
    q[1:17:2] = x_new[:8]
    return np.ascontiguousarray(q)


def _same_searches(ix, fresh, storage, q, what):
    """Every search path the storage serves, live index against fresh index."""
    paths = [("search8", lambda i: i.search(q[:8], 5)), ("search40", lambda i: i.search(q, 5))]
    qd = torch.from_numpy(q).cuda()
    paths.append(("search_fused", lambda i: i.search_fused(qd[:8], 5)))
    paths.append(("search device", lambda i: i.search(qd, 5)))
    if storage in ("bf16", "f32"):
        paths.append(("search_wide", lambda i: i.search_wide(q, 64)))
        radius = fresh.search_wide(q, 64)[0][:, 20].copy()            # the 21st score of every query: 20 hits and ties
        paths.append(("range_search", lambda i: i.range_search(q, radius)))
    for name, run in paths:
        gl._equal_arrays(run(ix), run(fresh), f"{what}: {name} differs from a fresh index")
    D, I = ix.search(q, 5)
    sub = ix.compute_distance_subset(q, I)
    gl._equal_arrays([sub], [fresh.compute_distance_subset(q, I)], f"{what}: compute_distance_subset")
    assert np.array_equal(sub.view(np.int32), D.view(np.int32)), f"{what}: the scores of the rows found are not the search's"


def _same_storage(ix, fresh, labels, what):
    assert ix.ntotal == fresh.ntotal, what
    assert np.array_equal(ix.rows_raw().view(np.uint8), fresh.rows_raw().view(np.uint8)), f"{what}: stored rows differ"
    ids = np.arange(ix.ntotal - 1, -1, -7)
    for raw in (False, True):
        a, b = ix.reconstruct_batch(ids, raw=raw), fresh.reconstruct_batch(ids, raw=raw)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: reconstruct differs"
    assert np.array_equal(ix.labels(), labels), f"{what}: labels changed"


def _forms(ids, x, form):
    if form == "host":
        return ids, x
    if form == "device":
        return torch.from_numpy(ids).cuda(), torch.from_numpy(x).cuda()
    if form == "ids device":
        return torch.from_numpy(ids).cuda(), x
    return ids.tolist() if len(ids) < 100 else ids, torch.from_numpy(x).cuda()      # "rows device"


# ------------------------------------------------------------------ 1. storage
def _run_id_sets(storage, metric, d, set_names, forms):
    base = uc.base_rows(uc.NTOTAL, d)
    ix = _make(storage, metric, d, base)
    labels = (np.arange(uc.NTOTAL) % 7).astype(np.int32)
    ix.set_labels(labels)
    ix.search(base[:9], 5)                                             # the caches are warm: norm bound, phi, the bf16 image
    model = base
    step = 0
    for off in (0, uc.OFFSET):
        sets = uc.id_sets(uc.NTOTAL, off)
        for name in set_names:
            ids = sets[name]
            for form in forms:
                step += 1
                x = uc.new_rows(len(ids), d, seed=step)
                what = f"{storage} m{metric} d{d}, {name}, offset {off}, {form}"
                i_arg, x_arg = _forms(ids, x, form)
                count = ix.update_rows(i_arg, x_arg, idx_offset=off, return_count=True)
                model, want = uc.apply_update(model, ids, x, off)
                assert count == want, f"{what}: {count} rows written, expected {want}"
                fresh = _make(storage, metric, d, model, like=ix)
                _same_storage(ix, fresh, labels, what)
                if name == "n1000" and form == forms[-1]:
                    _same_searches(ix, fresh, storage, _queries(d, x[uc.winners(ids, off, uc.NTOTAL)]), what)
    return ix, model


@pytest.mark.parametrize("combo", COMBOS, ids=_ID)
def test_rows_counts_and_searches_equal_a_fresh_index(combo):
    storage, metric = combo
    _run_id_sets(storage, metric, uc.D, ("n0", "n1", "n64", "n65", "n1000"), ("host", "device"))


@pytest.mark.parametrize("storage", ["bf16", "f32", "sq8"])
def test_the_headline_width_and_mixed_forms(storage):
    _run_id_sets(storage, 0, uc.D_WIDE, ("n65", "n1000"), ("ids device", "rows device"))


def test_update_rows_without_a_count_returns_nothing_and_a_search_behind_it_sees_the_rows():
    d = uc.D
    base = uc.base_rows(uc.NTOTAL, d)
    ix = _make("bf16", 0, d, base)
    ids = uc.id_sets()["n1000"]
    x = uc.new_rows(1000, d, seed=3)
    qd = torch.from_numpy(_queries(d, x[uc.winners(ids, 0, uc.NTOTAL)])).cuda()
    ix.search(qd, 5)
    side = torch.cuda.Stream()                                         # the update on one stream, the search on another
    xd, idd = torch.from_numpy(x).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert ix.update_rows(idd, xd) is None
    got = ix.search(qd, 5)                                             # ordered behind the update by the index
    torch.cuda.synchronize()
    fresh = _make("bf16", 0, d, uc.apply_update(base, ids, x)[0])
    gl._equal_arrays(got, fresh.search(qd, 5), "a search enqueued behind the update")


def test_raw_inputs_are_stored_as_add_stores_them():
    d, n = uc.D, uc.NTOTAL
    ids = uc.id_sets()["n65"]
    win = uc.winners(ids, 0, n)
    bf = synth.bf16_bits(uc.new_rows(65, d, seed=8))
    base = uc.base_rows(n, d)
    for storage in ("bf16", "f32"):                                    # bf16 bit patterns, host (np.uint16) and device (torch.bfloat16)
        want = uc.apply_update(base, ids, synth.bf16_bits_to_f32(bf))[0]
        for form in ("host", "device"):
            ix = _make(storage, 0, d, base)
            ix.search(base[:9], 5)
            xs = bf if form == "host" else torch.from_numpy(bf.view(np.int16)).cuda().view(torch.bfloat16)
            assert ix.update_rows(ids, xs, return_count=True) == int(win.sum())
            _same_storage(ix, _make(storage, 0, d, want), np.zeros(0, np.int32), f"bf16 bits into {storage}, {form}")
    codes = np.random.default_rng(4).integers(0, 255, (65, d), dtype=np.uint8)
    codes[codes == 0x7f] = 0x7e                                        # (no NaN codes: a NaN row has no order)
    for storage in ("fp8_e4m3", "fp8_e4m3_docs", "sq8"):               # raw bytes: e4m3 codes, SQ8 codes
        ix = _make(storage, 0, d, base)
        before = ix.rows_raw()
        assert ix.update_rows(ids, codes, return_count=True) == int(win.sum())
        want = uc.apply_update(before, ids, codes)[0]
        assert np.array_equal(ix.rows_raw(), want), storage
        fresh = _make(storage, 0, d, like=ix)
        fresh.add(want)
        _same_storage(ix, fresh, np.zeros(0, np.int32), f"raw codes into {storage}")
        q = _queries(d, uc.new_rows(8, d))
        gl._equal_arrays(ix.search(q, 5), fresh.search(q, 5), f"raw codes into {storage}: search")


def test_refusals_and_the_empty_calls_leave_the_index_alone():
    d, n = 64, 1000
    x = synth.generate(3, 0, n, d, synth.KIND_GAUSS)
    ix = ram.MipsIndex(d, metric=ram.METRIC_L2, dtype="f32")
    ix.add(x)
    q = x[:9]
    phi, before = ix.phi(), ix.search(q, 5)
    L, h = ix._lib, ix._h
    ids = np.array([1, 2, 3], np.int64)
    rows = np.ascontiguousarray(x[:3])
    cnt = ctypes.c_int64(-7)
    F32, E4M3, SQ8 = ram._lib.DTYPE_F32, ram._lib.DTYPE_FP8_E4M3, ram._lib.DTYPE_SQ8
    assert L.mips_index_update(None, ids.ctypes.data, 3, 0, rows.ctypes.data, F32, 0, None, None) == -1           # MIPS_E_INVALID
    assert L.mips_index_update(h, ids.ctypes.data, -1, 0, rows.ctypes.data, F32, 0, None, None) == -1
    assert L.mips_index_update(h, None, 3, 0, rows.ctypes.data, F32, 0, None, None) == -1
    assert L.mips_index_update(h, ids.ctypes.data, 3, 0, None, F32, 0, None, None) == -1
    for bad in (E4M3, SQ8, 17):                                                                                   # what add refuses here
        assert L.mips_index_update(h, ids.ctypes.data, 3, 0, rows.ctypes.data, bad, 0, None, None) == -1
    assert L.mips_index_update(h, ids.ctypes.data, 1 << 31, 0, rows.ctypes.data, F32, 0, None, None) == -3        # MIPS_E_UNSUPPORTED
    assert L.mips_index_update(h, None, 0, 0, None, F32, 0, ctypes.byref(cnt), None) == 0 and cnt.value == 0       # n == 0
    dev_cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    flags = ram._lib.OUT_DEVICE
    assert L.mips_index_update(h, None, 0, 0, None, F32, flags, ctypes.c_void_p(dev_cnt.data_ptr()), None) == 0 and int(dev_cnt) == 0
    assert ix.phi() == phi
    gl._equal_arrays(ix.search(q, 5), before, "after the refused and the empty calls")
    # a device count, and ids that all name no row: nothing is written
    idd = torch.tensor([-1, n, n + 5], dtype=torch.int64, device="cuda")
    xd = torch.from_numpy(rows).cuda()
    flags = ram._lib.IDS_DEVICE | ram._lib.Q_DEVICE | ram._lib.OUT_DEVICE
    dev_cnt.fill_(-7)
    assert L.mips_index_update(h, ctypes.c_void_p(idd.data_ptr()), 3, 0, ctypes.c_void_p(xd.data_ptr()), F32, flags,
                               ctypes.c_void_p(dev_cnt.data_ptr()), None) == 0
    assert int(dev_cnt) == 0 and np.array_equal(ix.rows_raw(), x)
    idd = torch.tensor([5, 5, n - 1], dtype=torch.int64, device="cuda")
    assert L.mips_index_update(h, ctypes.c_void_p(idd.data_ptr()), 3, 0, ctypes.c_void_p(xd.data_ptr()), F32, flags,
                               ctypes.c_void_p(dev_cnt.data_ptr()), None) == 0
    assert int(dev_cnt) == 2 and np.array_equal(ix.rows_raw()[[5, n - 1]], rows[[1, 2]])
    empty = ram.MipsIndex(d)
    assert empty.update_rows(ids, rows, return_count=True) == 0 and empty.ntotal == 0
    sq = ram.MipsIndex(d, dtype="sq8")
    with pytest.raises(RuntimeError, match="not trained"):
        sq.update_rows(ids, rows)
    with pytest.raises(ValueError):
        ix.update_rows(ids[:2], rows)                                  # 2 ids for 3 rows
    with pytest.raises(ValueError):
        ix.update_rows(ids.astype(np.float32), rows)
    with pytest.raises(ValueError):
        ix.update_rows(ids, rows[:, :10])


def test_an_override_of_phi_stays_and_clearing_it_gives_the_new_maximum():
    d, n = 64, 600
    x = synth.generate(3, 0, n, d, synth.KIND_GAUSS)
    ix = ram.MipsIndex(d, metric=ram.METRIC_L2, dtype="bf16")
    ix.add(x)
    ix.set_phi(123.0)
    big = (x[:1] * np.float32(40.0)).astype(np.float32)
    ix.update_rows([17], big)
    assert ix.phi() == 123.0                                           # as after add and remove_ids
    ix.clear_phi()
    want = uc.apply_update(x, [17], big)[0]
    assert ix.phi() == float(lc.orc.sumsq_canonical(synth.round_to_bf16(want)).max())


def test_c_abi_update_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_update_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_update_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


# ------------------------------------------------------------------ 2. search -> update -> search on the planted rows
class LiveU(gl.Live):
    """gl.Live with updates: `pieces` names the rows the index holds afterwards (the key of the cached reference)."""

    def update(self, ids, x, pieces, device=False):
        ids, x = np.asarray(ids, np.int64), np.ascontiguousarray(x, np.float32)
        if device:
            self.ix.update_rows(torch.from_numpy(ids).cuda(), torch.from_numpy(x).cuda())
        else:
            assert self.ix.update_rows(ids, x, return_count=True) == len(np.unique(ids))
        self.rows = uc.apply_update(self.rows, ids, x)[0]
        self.pieces = list(pieces)

    def check(self, what):
        """gl.Live.check without the comparison of margin_stats(): after an update the row-norm bounds are UPPER bounds, so the live
        index may flag more queries than a fresh one -- and must settle every one of them exactly, which is what stays asserted."""
        ref = self.reference()
        n = ref.n
        assert self.ix.ntotal == n == len(self.rows)
        fresh = self.fresh()
        if self.metric == 1:
            assert self.ix.phi() == fresh.phi() == ref.local_phi, what
        for path in self.paths:
            tag = f"{what}, {path} ({self.storage}, metric {self.metric}, d {self.d}, {n} rows)"
            got = self.run(self.ix, path, ref)
            stats = self.ix.margin_stats()
            (gl._same_range if path.startswith("range") else gl._same_topk)(got, self.expected(path, ref), tag)
            gl._equal_arrays(got, self.run(fresh, path, ref), f"{tag}: differs from a fresh index")
            assert stats["unresolved"] == 0, (tag, stats)
        return ref


A_PIECE, BLOCK = ("A", 0, lc.N_A), uc.PLACEHOLDERS


def test_the_bf16_image_and_the_residual_bound_follow_an_update():
    """fp32-exact index: placeholders -> block R (rows x = h + rho whose bf16 image is h: the decoys lead the scan, the truth has
    the planted rows first; max |x - bf16 x|^2 rises from 0), then ONE row -> a beacon whose own bf16 image decides it is found."""
    live = LiveU(128, "f32", 0)
    live.add(A_PIECE)
    live.add(("A2", 0, BLOCK))
    live.check("before the update")                                    # warm: image up to ntotal, both bounds, the margin statistics
    live.update(np.arange(lc.N_A, lc.N_A + BLOCK), live.fam.R, [A_PIECE, ("R", 0, BLOCK)])
    ref = live.check("placeholders became block R")
    off = lc.N_A
    for j in live.fam.r_queries:                                       # the truth: planted rows only
        assert set(ref.topk(lc.K_SEARCH, 0)[1][j]) <= set((off + live.fam.r_plant_at).tolist())
    _, ids, x, _ = uc.image_case(128)
    live.update(ids, x, [A_PIECE, ("R", 0, BLOCK), ("beacon", int(ids[0]), 0, 0)], device=True)
    ref = live.check("one row became the beacon")
    assert ref.topk(1, 0)[1][0, 0] == ids[0]


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_the_norm_bound_rises_then_an_add_and_another_update(storage):
    """Placeholders -> block B: rows of 10^3 times the norm, met by queries q = bf16(q) + delta; a bound left at ~1 certifies the
    decoys.  Then a further add (the extra row: a new maximum) and another update that takes it down again."""
    live = LiveU(128, storage, 0)
    for piece in (A_PIECE, ("R", 0, BLOCK), ("A2", 0, BLOCK)):
        live.add(piece)
    live.check("before the update")
    at = lc.N_A + BLOCK
    live.update(np.arange(at, at + BLOCK), live.fam.B, [A_PIECE, ("R", 0, BLOCK), ("B", 0, BLOCK)], device=storage == "f32")
    ref = live.check("placeholders became block B")
    if storage == "f32":
        for j in live.fam.b_queries:
            assert set(ref.topk(lc.K_SEARCH, 0)[1][j]) <= set((at + live.fam.b_plant_at).tolist())
    live.add(("X", 0, 1))
    live.check("a further add")
    last = at + BLOCK
    live.update([last, 0, last], np.concatenate([live.fam.A2[:2], live.fam.A2[7:8]]),
                [A_PIECE, ("R", 0, BLOCK), ("B", 0, BLOCK), ("X", 0, 1), ("upd", last, 0, 7)])
    live.check("another update")


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_phi_falls_when_the_longest_row_shrinks(storage):
    live = LiveU(128, storage, 1)
    live.add(A_PIECE)
    live.add(("X", 0, 1))
    big = live.check("before the update").local_phi
    _, ids, x = uc.phi_case(128)
    live.update(ids, x, [A_PIECE, ("A2", 0, 1)])
    small = live.check("the longest row became a plain row").local_phi      # (asserts phi() == the fresh index's == the oracle's)
    assert small < big / 1000
