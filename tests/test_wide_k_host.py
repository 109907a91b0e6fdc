"""Wide top-k, the parts that need no GPU: the C ABI declares and exports mips_search_wide, the limits agree between the header
and the package, and the Python callers route k > MAX_K to an index's search_wide (and only then, and only if it has one)."""
import os
import re

import numpy as np

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_wide_search():
    header = open(os.path.join(ROOT, "include", "mips_hip.h")).read()
    assert re.search(r"\bint\s+mips_search_wide\s*\(", header)
    assert int(re.search(r"#define MIPS_MAX_K_WIDE (\d+)", header).group(1)) == ram.MAX_K_WIDE == ram._lib.MAX_K_WIDE == 1024
    assert int(re.search(r"#define MIPS_MAX_K (\d+)", header).group(1)) == ram.MAX_K == 29
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", header).group(1)) == 1
    assert "mips_search_wide" in ram._lib.EXPORTS
    lib = ram._lib.load()
    assert hasattr(lib, "mips_search_wide")
    assert lib.mips_search_wide.argtypes == lib.mips_search.argtypes


class _Recording:
    """Stands in for the device index: exact search on bf16-rounded data, every call recorded."""

    def __init__(self, x, metric=0):
        self.x = synth.round_to_bf16(np.asarray(x, dtype=np.float32))
        self.d = self.x.shape[1]
        self.metric = self.metric_type = metric
        self.calls = []

    @property
    def ntotal(self):
        return len(self.x)

    def _go(self, name, q, k, **kw):
        self.calls.append((name, np.asarray(q).shape, int(k), dict(kw)))
        q = synth.round_to_bf16(np.asarray(q, dtype=np.float32))
        return orc.search_exact_bruteforce(q, self.x, k, metric=0 if kw.get("force_ip") else self.metric)

    def search(self, q, k, idx_offset=0, force_ip=False):
        return self._go("search", q, k, force_ip=force_ip)


class _RecordingWide(_Recording):
    def search_wide(self, q, k, idx_offset=0, force_ip=False):
        return self._go("search_wide", q, k, force_ip=force_ip)


def _names(ix):
    return [(c[0], c[2]) for c in ix.calls]


def test_faiss_shim_routes_by_k():
    x = synth.generate(3, 0, 400, 24, synth.KIND_GAUSS)
    q = synth.generate(4, 0, 3, 24, synth.KIND_GAUSS)
    fx = ram.faiss_shim.IndexFlatIP(24)
    fx._inner = _RecordingWide(x)
    s, i = fx.search(q, 100)
    assert s.shape == (3, 100) and np.array_equal(i, orc.search_exact_bruteforce(synth.round_to_bf16(q), fx._inner.x, 100)[1])
    fx.search(q, 10)
    fx.search(q, ram.MAX_K)
    assert _names(fx._inner) == [("search_wide", 100), ("search", 10), ("search", ram.MAX_K)]
    plain = ram.faiss_shim.IndexFlatIP(24)
    plain._inner = _Recording(x)                       # no search_wide: still served, through search
    s, i = plain.search(q, 100)
    assert s.shape == (3, 100) and _names(plain._inner) == [("search", 100)]


def test_knowledge_base_routes_by_k():
    x = synth.generate(3, 0, 400, 24, synth.KIND_GAUSS)
    q = synth.generate(4, 0, 2, 24, synth.KIND_GAUSS)
    cols = {"mips_column": [str(i) for i in range(400)], "aid": [[i] for i in range(400)]}
    wide = _RecordingWide(x)
    kb = ram.KnowledgeBase(dict(cols), wide, "mips_cls")
    scores, examples = kb.get_nearest_examples_batch("mips_cls", q, k=100)
    assert [len(s) for s in scores] == [100, 100] and len(examples[0]["mips_column"]) == 100
    kb.get_nearest_examples_batch("mips_cls", q, k=10)
    assert _names(wide) == [("search_wide", 100), ("search", 10)]
    plain = _Recording(x)
    kb = ram.KnowledgeBase(dict(cols), plain, "mips_cls")
    scores, _ = kb.get_nearest_examples_batch("mips_cls", q, k=100)
    assert [len(s) for s in scores] == [100, 100] and _names(plain) == [("search", 100)]


def test_mips_facade_routes_by_k():
    x = synth.generate(3, 0, 300, 32, synth.KIND_GAUSS)
    data = {"mips_column": [f"doc {i}" for i in range(300)], "aid": [f"a{i}" for i in range(300)]}
    m = ram.Mips(ram.MipsArgs(mips_metric_type=0, mips_normalize=False), data=data)
    wide = _RecordingWide(x)
    m.embeddings = ram.KnowledgeBase(dict(data), wide, m.index_name)
    q = synth.generate(5, 0, 4, 32, synth.KIND_GAUSS)
    m.search(q, k=ram.MAX_K, ignore_indexes=[0, 1, 2, 3])     # fetches k + 1 = 30: wide
    m.search(q, k=ram.MAX_K)
    m.np_search(q, k=64)
    m.np_search(q, k=2)
    assert _names(wide) == [("search_wide", 30), ("search", 29), ("search_wide", 64), ("search", 2)]
    assert wide.calls[2][3]["force_ip"] is True
