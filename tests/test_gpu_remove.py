"""mips_index_remove / MipsIndex.remove_ids on the GPU.

Part 1, data movement: after a removal rows_raw(), labels() and ntotal are the NumPy model of tests/remove_cases.py, bit for bit
-- every storage and row pitch, index sizes around the window borders, every pattern, with "remove_window_rows" = 128 and 384 and
the default, bitmaps that start at bit 0 / 3 / 13 in host and device memory, id arrays with duplicates, a partial labelled prefix,
the refusals, and the same from plain C.

Part 2, searches after a removal: ONE index lives through add -> remove -> remove -> add with growth -> remove -> reset -> a
smaller second life -> remove on the planted blocks of tests/lifecycle_cases.py; after every step each search path is compared,
every query, indices and scores bit for bit, with the all-pairs reference on the rows the index should hold and with a fresh
index built from those rows in one add (the machinery of tests/test_gpu_lifecycle.py).  tests/test_remove_host.py shows on NumPy
models that a phi or a bf16 image left stale by the removal changes these answers.

Part 3: KnowledgeBase.remove_rows / drop_near_duplicates and faiss_shim.IndexFlat.remove_ids."""
import hashlib
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
    import remove_cases as rm
    import test_gpu_lifecycle as gl
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

STORAGES = [("bf16", 64), ("bf16", 100), ("bf16", 1024), ("bf16", 1100), ("fp8_e4m3", 64), ("fp8_e4m3_docs", 64), ("f32", 64), ("f32", 72)]


def _as_f32(raw, storage):
    if storage == "bf16":
        return synth.bf16_bits_to_f32(raw)
    return raw if storage == "f32" else synth.e4m3_bits_to_f32(raw)


def _check_index(ix, storage, x, labels, nlabelled, mask, what):
    rows, lab, nlab = rm.expected(x, labels, nlabelled, mask)
    assert ix.ntotal == len(rows), what
    got = _as_f32(ix.rows_raw(), storage) if len(rows) else np.zeros((0, x.shape[1]), np.float32)
    assert got.shape == rows.shape and np.array_equal(got.view(np.int32), rows.view(np.int32)), f"{what}: rows differ"
    assert ix._nlabelled == nlab and np.array_equal(ix.labels(), lab.astype(np.int32)), f"{what}: labels differ"


# ------------------------------------------------------------------ 1. data movement
@pytest.mark.parametrize("storage,d", STORAGES, ids=lambda v: str(v))
def test_rows_and_labels_after_a_removal(storage, d):
    ix = ram.MipsIndex(d, dtype=storage)
    for window in rm.WINDOWS:
        ix.set_param("remove_window_rows", window)
        W = window or rm.W_MODEL
        for n in rm.sizes(W):
            x = rm.rows_for(n, d, storage, seed=n)
            labels = (np.arange(n) * 5 % 13).astype(np.int32)
            for name, mask in rm.patterns(n, W).items():
                ix.reset()
                ix.add(x)
                ix.set_labels(labels)
                removed = ix.remove_ids(mask)
                what = f"{storage} d {d}, window {window}, {n} rows, {name}"
                assert removed == int(mask.sum()), what
                _check_index(ix, storage, x, labels, n, mask, what)
    # the pad columns behind d stay zero: a row added after the removals scores as it does on a fresh index
    q = rm.rows_for(3, d, storage, seed=5)
    ix.add(q)
    fresh = ram.MipsIndex(d, dtype=storage)
    fresh.add(_as_f32(ix.rows_raw(), storage))
    a, b = ix.search(q, 3), fresh.search(q, 3)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


@pytest.mark.parametrize("storage,d", [("bf16", 100), ("f32", 72), ("fp8_e4m3", 64)], ids=lambda v: str(v))
def test_bitmaps_ids_and_a_partial_labelled_prefix(storage, d):
    W = 128
    n = 5 * W + 37
    x = rm.rows_for(n, d, storage)
    labels = (np.arange(n) % 11).astype(np.int32)
    ix = ram.MipsIndex(d, dtype=storage)
    ix.set_param("remove_window_rows", W)
    pats = rm.patterns(n, W)

    def rebuilt(nlab):
        ix.reset()
        ix.add(x)
        if nlab:
            ix.set_labels(labels[:nlab])
        return ix

    for nlab in (0, 1, W, W + 1, 300, n):                          # no labels, a prefix inside / on / behind a window border, all
        for name in ("random_50pct", "run_3w5", "first", "all"):
            mask = pats[name]
            for bit0 in (0, 3, 13):
                host = rm.bitmap(mask, bit0, pad_bits=5)
                what = f"{name}, {nlab} labelled, bit0 {bit0}"
                assert rebuilt(nlab).remove_ids(host, sel_bit0=bit0) == mask.sum(), what                       # host bitmap
                _check_index(ix, storage, x, labels, nlab, mask, what + " (host)")
                assert rebuilt(nlab).remove_ids(torch.from_numpy(host).cuda(), sel_bit0=bit0) == mask.sum()   # device bitmap
                _check_index(ix, storage, x, labels, nlab, mask, what + " (device)")
                sel = ram.Selector.from_bitmap(host, bit0 + n + 5)
                assert rebuilt(nlab).remove_ids(sel, sel_bit0=bit0) == mask.sum()
                _check_index(ix, storage, x, labels, nlab, mask, what + " (Selector)")
    mask = pats["random_1pct"] | pats["last"]
    ids = np.flatnonzero(mask)
    dup = np.concatenate([ids, ids[::-1], ids[:3]])                # duplicates, unordered
    for form in (dup, dup.astype(np.int32), torch.from_numpy(dup), torch.from_numpy(dup).cuda(), dup.tolist()):
        assert rebuilt(n).remove_ids(form) == len(ids)
        _check_index(ix, storage, x, labels, n, mask, "ids")
    assert rebuilt(n).remove_ids(mask) == len(ids) and rebuilt(n).remove_ids(torch.from_numpy(mask).cuda()) == len(ids)   # bool masks
    _check_index(ix, storage, x, labels, n, mask, "bool tensor")
    with pytest.raises(ValueError):
        ix.remove_ids(np.array([ix.ntotal]))                       # an id the index does not hold


def test_nothing_removed_keeps_the_cached_scalars_and_refusals_leave_the_index_alone():
    d, n = 64, 1000
    x = synth.generate(3, 0, n, d, synth.KIND_GAUSS)
    ix = ram.MipsIndex(d, metric=ram.METRIC_L2, dtype="f32")
    ix.add(x)
    q = x[:9]
    phi, before = ix.phi(), ix.search(q, 5)
    assert ix.remove_ids(np.zeros(n, bool)) == 0 and ix.ntotal == n and ix.phi() == phi
    again = ix.search(q, 5)
    assert np.array_equal(again[1], before[1]) and np.array_equal(again[0].view(np.int32), before[0].view(np.int32))
    ix.set_phi(123.0)                                              # a value no row has
    # an override stays across a real removal, as it stays across an add
    assert ix.remove_ids(np.arange(n) < 10) == 10 and ix.phi() == 123.0
    ix.clear_phi()
    assert ix.phi() == float(lc.orc.sumsq_canonical(x[10:]).max())
    # refusals
    m = ix.ntotal
    for bad in (lambda: ix.remove_ids(np.zeros(m - 1, bool)),                          # too few bits
                lambda: ix.remove_ids(np.zeros(m, bool), sel_bit0=1),                  # bit0 + ntotal > nbits
                lambda: ix.remove_ids(np.zeros(m + 8, bool), sel_bit0=-1),
                lambda: ix.set_param("remove_window_rows", 100),
                lambda: ix.set_param("remove_window_rows", -128)):
        with pytest.raises((ValueError, RuntimeError)):
            bad()
    import ctypes

    counts = (ctypes.c_int64 * 2)()
    host = np.zeros((m + 20) // 8 + 1, np.uint8)
    L = ix._lib
    assert L.mips_index_remove(ix._h, host.ctypes.data, 8 * len(host), -1, 0, counts, None) == -1         # MIPS_E_INVALID
    assert L.mips_index_remove(ix._h, host.ctypes.data, m + 2, 3, 0, counts, None) == -1
    assert L.mips_index_remove(ix._h, None, 8 * len(host), 0, 0, counts, None) == -1
    assert L.mips_index_remove(ix._h, host.ctypes.data, 8 * len(host), 0, 0, None, None) == -1
    assert L.mips_index_remove(ix._h, host.ctypes.data, 8 * len(host), 3, 0, counts, None) == 0 and list(counts) == [0, 0]
    assert ix.ntotal == m
    empty = ram.MipsIndex(d)
    assert L.mips_index_remove(empty._h, None, 0, 0, 0, counts, None) == 0 and empty.remove_ids(np.zeros(0, bool)) == 0


def test_add_appends_at_the_new_end_with_and_without_growth():
    d = 100
    ix = ram.MipsIndex(d, dtype="bf16")
    ix.set_param("remove_window_rows", 128)
    x = rm.rows_for(1000, d, "bf16")
    ix.reserve(1024)
    ix.add(x)
    ix.set_labels(np.arange(1000))
    mask = rm.patterns(1000, 128)["every_other"]
    assert ix.remove_ids(mask) == 500
    y = rm.rows_for(700, d, "bf16", seed=9)
    ix.add(y[:100])                                                # 600 rows: inside the 1024 reserved
    ix.set_labels(np.arange(1000, 1100), row0=500)
    ix.add(y[100:])                                                # 1200 rows: growth
    want = np.concatenate([x[~mask], y])
    assert ix.ntotal == 1200 and np.array_equal(synth.bf16_bits_to_f32(ix.rows_raw()), want)
    assert np.array_equal(ix.labels(), np.concatenate([np.arange(1000)[~mask], np.arange(1000, 1100)]))
    assert ix.remove_ids(np.arange(1200) >= 550) == 650            # cuts the labelled prefix at 550
    assert ix._nlabelled == 550 and np.array_equal(synth.bf16_bits_to_f32(ix.rows_raw()), want[:550])


def test_c_abi_remove_from_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_remove_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(root, "tests", "c_abi_remove_smoke.c"), "-I", os.path.join(root, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


# ------------------------------------------------------------------ 2. searches after a removal
class LiveR(gl.Live):
    """gl.Live with removals: the labels travel with their rows, so they are tracked instead of derived from the row number."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.labels = np.zeros(0, np.int64)

    def add(self, piece, rows=None):
        n0 = len(self.rows)
        super().add(piece, rows)
        self.labels = np.concatenate([self.labels, lc.row_labels(len(self.rows))[n0:]])

    def reset(self):
        super().reset()
        self.labels = np.zeros(0, np.int64)

    def remove(self, mask, window):
        self.ix.set_param("remove_window_rows", window)
        if self.device:                                            # the removal on a stream of its own, behind a search in flight
            md = torch.from_numpy(mask).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(self.s_add):
                removed = self.ix.remove_ids(md)
            self.settle()                                          # the search issued BEFORE the removal answered on the old rows
        else:
            removed = self.ix.remove_ids(mask)
        assert removed == int(mask.sum())
        self.rows, self.labels = self.rows[~mask], self.labels[~mask]
        self.pieces.append(("removed", hashlib.sha1(mask.tobytes()).hexdigest()[:16]))
        if self.filters:
            assert np.array_equal(self.ix.labels(), self.labels.astype(np.int32))

    def expected(self, path, ref):
        if not path.endswith("_grp"):
            return super().expected(path, ref)
        admit = lc.admit_groups(self.labels, lc.query_labels(lc.NQ), "exclude", ram.LABEL_NONE)
        if path.startswith("wide"):
            return ref.topk(lc.K_WIDE, self.metric, self.phi, admit)
        return ref.range(self.radii(ref), self.metric, self.phi, admit)

    def fresh(self):
        ix = super().fresh()
        if self.filters:
            ix.set_labels(self.labels)
        return ix


def _block_mask(live, name, at=None):
    """Rows of block `name` (all of them, or those at the block positions `at`) in an index that holds A, R, B in that order."""
    n = len(live.rows)
    off = {"A": 0, "R": lc.N_A, "B": lc.N_A + lc.NPLANT + lc.NDECOY}[name]
    size = lc.N_A if name == "A" else lc.NPLANT + lc.NDECOY
    m = np.zeros(n, bool)
    m[off + (np.arange(size) if at is None else np.asarray(at))] = True
    return m


def _life(live):
    """The sequence of the module docstring; every removal under another window."""
    fam = live.fam
    for piece in (("A", 0, lc.N_A), ("R", 0, lc.NPLANT + lc.NDECOY), ("B", 0, lc.NPLANT + lc.NDECOY)):
        live.add(piece)                                            # capacities 2304, 3456: the third add fits
    first = live.check("1: A, R, B").local_phi
    live.remove(_block_mask(live, "B", fam.b_plant_at), 128)       # the truth of the B-planted queries changes: the decoys win
    live.check("2: B's planted rows gone")
    decoys = np.zeros(len(live.rows), bool)
    decoys[lc.N_A + lc.NPLANT + lc.NDECOY:] = True                 # what is left of B, as long as the planted rows were
    live.remove(decoys, 384)
    small = live.check("2b: no big row left").local_phi
    if not live.storage.startswith("fp8"):
        assert first > 400 * small                                 # phi and the maximal norm had to fall (~S^2 / 2, tests/test_remove_host.py)
    live.remove(_block_mask(live, "R", fam.r_plant_at), 0)         # rows move inside the bf16 image of an fp32-exact index
    live.check("3: R's planted rows gone")
    assert live.ix.ntotal == lc.N_A + lc.NDECOY
    live.add(("A2", 0, lc.N_A))                                    # 4530 rows > 3456: growth
    live.check("4: added with growth")
    n = len(live.rows)
    live.remove((np.arange(n) % 3 == 1) | ((np.arange(n) >= 700) & (np.arange(n) < 1300)), 384)
    live.check("5: a third and a run gone")
    live.reset()
    for piece in lc.SEQ_RESET_SECOND:
        live.add(piece)
    live.check("7: second life")
    mask = rm.patterns(len(live.rows), 128)["random_1pct"]
    mask[0] = True
    live.remove(mask, 128)
    live.check("8: second life, rows removed")
    gl._stored_equal(live)


@pytest.mark.parametrize("combo", gl.COMBOS + gl.F8_COMBOS, ids=gl._ID)
def test_searches_after_removals(combo):
    storage, metric, d = combo
    _life(LiveR(d, storage, metric, filters=combo == gl.FILTERED))


@pytest.mark.parametrize("combo", [("f32", 1, 128), ("bf16", 0, 1024)], ids=gl._ID)
def test_device_removal_on_another_stream(combo):
    """CUDA tensors under margin_check = 3: searches on stream A, adds and removals on stream B.  check() leaves a search in
    flight on A; the removal is issued on B without waiting for it; remove() then waits and compares that search with the OLD
    rows' expectation, and the searches of the next check(), on A again, answer on the new rows."""
    storage, metric, d = combo
    live = LiveR(d, storage, metric, device=True)
    _life(live)
    live.settle()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the facades
def test_faiss_shim_remove_ids():
    fs = ram.faiss_shim
    d, n = 64, 2000
    x = synth.generate(4, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(5, 0, 20, d, synth.KIND_GAUSS)
    mask = rm.patterns(n, 128)["random_50pct"]
    for dtype in ("f32", "bf16"):
        a, b = fs.IndexFlat(d, fs.METRIC_INNER_PRODUCT, dtype=dtype), fs.IndexFlat(d, fs.METRIC_INNER_PRODUCT, dtype=dtype)
        a.add(x)
        b.add(x[~mask])
        assert a.remove_ids(fs.IDSelectorBitmap(np.packbits(mask, bitorder="little"))) == mask.sum() and a.ntotal == b.ntotal
        assert a.remove_ids(np.array([10 ** 6], np.int64)) == 0   # an id the index does not hold: nothing, as in faiss
        for got, exp in zip(a.search(q, 5), b.search(q, 5)):
            assert np.array_equal(got.view(np.int32) if got.dtype == np.float32 else got, exp.view(np.int32) if exp.dtype == np.float32 else exp)
    # L2 on phi-augmented rows: phi follows the stored rows, the result is a shim index built from the survivors
    xa = ram.augment_xb(x[:500] * np.linspace(0.5, 2.0, 500, dtype=np.float32)[:, None])
    xa = np.ascontiguousarray(xa, np.float32)
    a = fs.IndexFlat(d + 1, fs.METRIC_L2)
    a.add(xa)
    longest = int(np.argmax(np.square(xa[:, :-1]).sum(1)))
    assert a.remove_ids(np.array([longest, 3, 3], np.int64)) == 2
    keep = np.ones(500, bool)
    keep[[longest, 3]] = False
    assert a.ntotal == 498 and a.mips_index.phi() == float(lc.orc.sumsq_canonical(xa[keep][:, :-1]).max())
    assert a.remove_ids(fs.IDSelectorRange(0, 10 ** 9)) == 498 and a.ntotal == 0


def test_knowledge_base_remove_rows_and_drop_near_duplicates():
    rng = np.random.default_rng(4)
    n, d = 300, 64
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    clusters = ([5, 17, 200, 299], [40, 41], [100, 150, 250])
    for c in clusters:
        x[c] = x[c[0]]
    aid = np.arange(n) // 10
    kb = ram.KnowledgeBase({"emb": x.copy(), "aid": aid.copy(), "text": [f"t{i}" for i in range(n)]})
    kb.add_faiss_index("emb", index_name="ix", metric_type=0)
    kb.set_groups("ix", "aid")
    index = kb.get_index("ix").faiss_index
    # remove_rows: columns, index and groups stay aligned
    assert kb.remove_rows([7, 7, 260]) == 2
    keep = np.ones(n, bool)
    keep[[7, 260]] = False
    assert len(kb) == n - 2 == index.ntotal and kb["text"][7] == "t8" and np.array_equal(kb["emb"], x[keep])
    assert np.array_equal(index.rows_raw(), x[keep]) and np.array_equal(kb.group_codes("ix", kb["aid"], "only"), index.labels())
    s, ex = kb.get_nearest_examples_batch("ix", x[keep][:6], k=3, groups=kb["aid"][:6], group_mode="only")
    for j in range(6):
        assert set(ex[j]["aid"]) == {kb["aid"][j]} and ex[j]["text"][0] == kb["text"][j]     # its own group only, itself first
    with pytest.raises(ValueError):
        kb.remove_rows([len(kb)])
    # drop_near_duplicates: one row per cluster stays
    before = {c: list(v) for c, v in kb.columns.items()}
    i, j, _ = kb.near_duplicates("ix", 0.99)
    gone = kb.drop_near_duplicates("ix", 0.99)
    assert np.array_equal(gone, np.unique(j)) and len(gone) == sum(len(c) - 1 for c in clusters)
    assert len(kb) == n - 2 - len(gone) == index.ntotal
    left = [t for k, t in enumerate(before["text"]) if k not in set(gone.tolist())]
    assert kb["text"] == left and {"t5", "t40", "t100"} <= set(left) and not {"t17", "t41", "t150", "t299"} & set(left)
    assert all(len(a) == 0 for a in kb.near_duplicates("ix", 0.99))
    assert np.array_equal(kb.group_codes("ix", kb["aid"], "only"), index.labels())
