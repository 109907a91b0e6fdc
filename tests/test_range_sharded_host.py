"""Range search on the row-sharded index, the parts that need no GPU: the second header and its export, the part record, the NumPy
restatement of the merge against a literal per-query concatenation, the partition + record + all-reduce + all-gather + merge
plumbing of ShardedMipsIndex.range_search on the ranks of a gloo group (the oracle stands in for the local search, the NumPy
restatement for the merge), and KnowledgeBase.near_duplicates over a duck-typed sharded index.  Every comparison is bit for bit,
per query."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import synth
from retrieval_augmented_mds_amd.mips import KnowledgeBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import range_cases as rc  # noqa: E402


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return text, set(re.findall(r"\b(mips_[a-z0-9_]+)\s*\(", text))


# ------------------------------------------------------------------ 1. ABI pins
def test_second_header_declares_and_library_exports_the_record_merge():
    text, declared = _declared(os.path.join(ROOT, "include", "mips_hip_sharded.h"))
    assert re.search(r"\bint\s+mips_range_merge_records\s*\(", text)
    assert '#include "mips_hip.h"' in text
    assert set(ram._lib.EXPORTS_SHARDED) == declared == {"mips_range_merge_records"}
    main_text, main_declared = _declared(os.path.join(ROOT, "include", "mips_hip.h"))
    assert set(ram._lib.EXPORTS) == main_declared and len(ram._lib.EXPORTS) == 41      # the first header is as it was
    assert not main_declared & declared
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", main_text).group(1)) == ram._lib.ABI_VERSION == 1
    assert "MIPS_ABI_VERSION" not in text                         # one version for the library, defined in the first header
    lib = ram._lib.load()                                          # builds, loads and binds: AttributeError if the symbol is missing
    assert len(lib.mips_range_merge_records.argtypes) == 11
    assert ram._lib.HEADER_SHARDED in ram._lib._sources()          # a change of the header rebuilds the library
    assert callable(ram.range_merge_records) and "range_merge_records" in ram.__all__


def test_record_words_macro_agrees_with_the_python_helper():
    text, _ = _declared(os.path.join(ROOT, "include", "mips_hip_sharded.h"))
    m = re.search(r"#define MIPS_RANGE_RECORD_WORDS\(nq, stride\) (.*)", text)
    assert m, "MIPS_RANGE_RECORD_WORDS(nq, stride) is not defined"
    expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
    for nq in (0, 1, 5, 4099):
        for stride in (0, 1, 2, 7):
            w = eval(expr, {"nq": nq, "stride": stride})
            assert w == ram._lib.range_record_words(nq, stride) == rc.record_words(nq, stride) == nq + 1 + stride + (stride + 1) // 2
            rec = torch.zeros(w, dtype=torch.int64)
            lims, D, I = ram.sharded.range_record_views(rec, nq, stride)
            assert lims.shape == (nq + 1,) and D.shape == I.shape == (stride,) and D.dtype == torch.float32 and I.dtype == torch.int64
            assert all(t.is_contiguous() for t in (lims, D, I))
            D.fill_(1.5)
            I.fill_(-3)
            lims.fill_(9)                                          # the three views tile the record: the NumPy reading agrees
            nl, nD, nI = rc.split_record(rec.numpy(), nq, stride)
            assert (nl == 9).all() and (nD == 1.5).all() and (nI == -3).all()


def test_sharded_index_has_the_range_surface():
    assert hasattr(ram.ShardedMipsIndex, "range_search") and hasattr(ram.ShardedMipsIndex, "range_search_into")
    for fn in (ram.MipsIndex.range_search_into, ram.MipsIndex.range_search):
        assert inspect.signature(fn).parameters["sel_bit0"].default == 0
    p = inspect.signature(ram.ShardedMipsIndex.range_search).parameters
    assert list(p)[1:] == ["q", "radius", "idx_offset", "force_ip", "selector", "groups", "group_mode"]
    assert "part_cap" in inspect.signature(ram.ShardedMipsIndex.range_search_into).parameters
    p = inspect.signature(ram.ShardedMipsIndex.__init__).parameters
    assert p["local_range_search"].default is None and p["range_merge"].default is None


# ------------------------------------------------------------------ 2. the NumPy restatement of the merge
def test_numpy_merge_equals_a_literal_concatenation():
    # hits[p][j]: (score, id) of part p, query j; part 1 is empty, query 2 is empty everywhere, query 3 lives in the last part only
    hits = [
        [[(0.5, 3), (1.5, 9)], [(2.0, 4)], [], []],
        [[], [], [], []],
        [[(-1.0, 100)], [(3.0, 101), (4.0, 102), (5.0, 190)], [], [(7.0, 150)]],
    ]
    nq, stride = 4, 5
    parts = []
    for part in hits:
        lims = np.cumsum([0] + [len(h) for h in part]).astype(np.int64)
        flat = [e for h in part for e in h]
        parts.append((lims, np.array([e[0] for e in flat], np.float32), np.array([e[1] for e in flat], np.int64)))
    g = rc.gather(parts, stride)
    assert g.shape == (3 * rc.record_words(nq, stride),)
    lims, D, I = rc.merge_records(g, 3, nq, stride)
    want = [[e for part in hits for e in part[j]] for j in range(nq)]
    assert lims.tolist() == [0, 3, 7, 7, 8]
    for j in range(nq):
        assert list(zip(D[lims[j]:lims[j + 1]].tolist(), I[lims[j]:lims[j + 1]].tolist())) == want[j]
    assert not np.isnan(D).any() and (I != rc.PAD_ID).all()
    # drawn parts, an odd stride above every total
    parts = rc.synthetic_parts(3, 33, seed=1)
    stride = max(int(p[0][-1]) for p in parts) | 1
    lims, D, I = rc.merge_records(rc.gather(parts, stride + 2), 3, 33, stride + 2)
    for j in range(33):
        seg = [p[2][p[0][j]:p[0][j + 1]] for p in parts]
        assert np.array_equal(I[lims[j]:lims[j + 1]], np.concatenate(seg))
        assert (np.diff(I[lims[j]:lims[j + 1]]) > 0).all()        # ascending parts of ascending ids: ascending
    # a truncated part: the counts stay true, the restatement defines nothing else
    big = (np.array([0, 4, 9], np.int64), np.arange(9, dtype=np.float32), np.arange(9, dtype=np.int64))
    lims, D, I = rc.merge_records(rc.gather([big, big], 4), 2, 2, 4)
    assert lims.tolist() == [0, 8, 18] and D is None and I is None


# ------------------------------------------------------------------ 3. gloo ranks, injected steps
def _gloo_worker(rank, world, port, n, nq, d, metric, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = synth.generate(9, 0, n, d, synth.KIND_LATTICE)        # lattice data: ties across the shard borders
        q = synth.generate(10, 0, nq, d, synth.KIND_LATTICE)
        lo, hi = ram.shard_bounds(n, world, rank)
        phi = rc.orc.sumsq_canonical(x).max()
        calls = []

        def local_range_search(qq, radius, off, force_ip=False):  # the oracle stands in for the device search of this shard
            assert off == lo and isinstance(qq, np.ndarray)
            calls.append(bool(force_ip))
            m = 0 if force_ip else metric
            rr = ram.MipsIndex._radii(radius, len(qq))
            if hi == lo:
                return np.zeros(len(qq) + 1, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)
            return rc._expected(rc._values(qq, x[lo:hi], m, phi=phi), rr, m, idx_offset=lo)   # L2: the phi of the WHOLE index

        merges = []

        def range_merge(gathered, parts, nq_, stride):
            assert parts == world and isinstance(gathered, np.ndarray) and gathered.shape == (parts * rc.record_words(nq_, stride),)
            merges.append(stride)
            return rc.merge_records(gathered, parts, nq_, stride)

        ix = ram.ShardedMipsIndex(d, metric=metric, local_range_search=local_range_search, range_merge=range_merge)
        assert (ix.rank, ix.world) == (rank, world) and ix.local is None
        ix.set_global_size(n)
        vals = rc._values(q, x, metric)
        r = rc._boundary_radii(vals, metric)
        exp = rc._expected(vals, r, metric)
        got = ix.range_search(q, r)
        assert all(isinstance(t, np.ndarray) for t in got) and got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64
        rc._same(got, exp, f"rank {rank}")
        assert calls == [False]                                    # the default guess holds these results: no repeat
        shard_totals = [int(((exp[2] >= a) & (exp[2] < b)).sum()) for a, b in (ram.shard_bounds(n, world, t) for t in range(world))]
        assert merges == [max(shard_totals)]                       # the records travel at the size of the largest shard result
        if metric == 1:                                            # force_ip reaches the local step
            v0 = rc._values(q, x, 0)
            r0 = rc._boundary_radii(v0, 0)
            rc._same(ix.range_search(q, r0, force_ip=True), rc._expected(v0, r0, 0), "force_ip")
            assert calls[-1] is True
        with pytest.raises(ValueError):
            ix.range_search(q, r, idx_offset=5)
        # a first stride too small on some ranks only: every row answers every query, so a shard of m rows finds nq * m hits
        everything = np.float32(np.inf if metric == 1 else -np.inf)
        sizes = [b - a for a, b in (ram.shard_bounds(n, world, t) for t in range(world))]
        guess = nq * (n // world)
        assert min(sizes) * nq <= guess < max(sizes) * nq
        ix._range_stride_guess = lambda nq_: guess
        del calls[:], merges[:]
        got = ix.range_search(q, everything)
        rc._same(got, rc._expected(vals, np.full(nq, everything), metric), "after the repeat")
        assert len(calls) == (2 if (hi - lo) * nq > guess else 1), (rank, calls)      # exactly one repeat, only where it was needed
        assert merges == [max(sizes) * nq]
        ret[rank] = len(calls)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,metric", [(2, 1003, 0), (3, 1003, 0), (3, 2, 0), (2, 1003, 1), (3, 1003, 1), (3, 2, 1)])
def test_sharded_range_search_gloo(world, n, metric):
    """n = 2 at world 3 leaves the last shard empty (and the first stride of the repeat case at 0)."""
    import torch.multiprocessing as mp

    port = 28100 + (os.getpid() % 2000) + 3 * world + n % 7 + metric
    ret = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, port, n, 5, 64, metric, ret), nprocs=world, join=True)
    repeats = dict(ret)
    assert sorted(repeats) == list(range(world))
    sizes = [b - a for a, b in (ram.shard_bounds(n, world, t) for t in range(world))]
    assert [repeats[t] for t in range(world)] == [2 if s > n // world else 1 for s in sizes] and 1 in repeats.values() and 2 in repeats.values()


# ------------------------------------------------------------------ 4. the self-join over a sharded index
class FakeShardedRangeIndex:
    """What KnowledgeBase.near_duplicates needs of a sharded index -- range_search, metric_type, d -- over row shards searched
    with NumPy (float64 scores rounded to float32), packed into records and merged by the NumPy restatement."""

    def __init__(self, x, bounds):
        self.x = np.asarray(x, dtype=np.float32)
        self.d, self.ntotal, self.metric_type = self.x.shape[1], self.x.shape[0], 0
        self.bounds = bounds

    def range_search(self, q, radius):
        q = np.asarray(q, dtype=np.float32)
        r = ram.MipsIndex._radii(radius, q.shape[0])
        local = []
        for lo, hi in self.bounds:
            val = (q.astype(np.float64) @ self.x[lo:hi].astype(np.float64).T).astype(np.float32)
            local.append(rc._expected(val, r, 0, idx_offset=lo))
        stride = max(int(p[0][-1]) for p in local)
        words = ram._lib.range_record_words(q.shape[0], stride)
        g = rc.gather(local, stride)
        assert g.shape == (len(local) * words,)
        return rc.merge_records(g, len(local), q.shape[0], stride)


def test_near_duplicates_over_a_duck_typed_sharded_index():
    rng = np.random.default_rng(4)                                 # the planted case of tests/test_range_host.py
    x = rng.standard_normal((300, 24)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[[5, 17, 200, 299]] = x[5]
    x[[40, 41]] = x[40]
    kb = KnowledgeBase({"emb": x})
    kb.add_faiss_index("emb", custom_index=FakeShardedRangeIndex(x, [(0, 41), (41, 41), (41, 200), (200, 300)]))   # 40 | 41 apart
    i, j, s = kb.near_duplicates("emb", 0.99, batch_rows=64)
    assert list(zip(i.tolist(), j.tolist())) == [(5, 17), (5, 200), (5, 299), (17, 200), (17, 299), (40, 41), (200, 299)]
    assert i.dtype == np.int64 and j.dtype == np.int64 and s.dtype == np.float32 and np.allclose(s, 1.0, atol=1e-5)
