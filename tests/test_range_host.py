"""CPU tests of the range-search surface: the C ABI declares and the binding binds mips_range_search; faiss_shim.IndexFlat.range_search
and KnowledgeBase.near_duplicates run over a fake index object that implements range_search with NumPy (radius broadcasting, the
uint64 lims, the i < j pair logic, L2 column stripping)."""
import os
import re

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram
from retrieval_augmented_mds_amd.mips import KnowledgeBase, augment_xb, augment_xq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeRangeIndex:
    """range_search of MipsIndex in NumPy (float64 scores rounded to float32; hits in ascending row order)."""

    def __init__(self, x, metric=0):
        self.x = np.asarray(x, dtype=np.float32)
        self.d = self.x.shape[1]
        self.ntotal = self.x.shape[0]
        self.metric_type = metric
        self.seen = []

    def range_search(self, q, radius, idx_offset=0, force_ip=False):
        q = np.asarray(q, dtype=np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, q.shape
        self.seen.append(q.shape)
        r = ram.MipsIndex._radii(radius, q.shape[0])
        x64, q64 = self.x.astype(np.float64), q.astype(np.float64)
        val = q64 @ x64.T
        if self.metric_type == 1 and not force_ip:
            val = np.square(q64).sum(axis=1)[:, None] + np.square(x64).sum(axis=1).max() - 2.0 * val
        val = val.astype(np.float32)
        hit = val < r[:, None] if (self.metric_type == 1 and not force_ip) else val > r[:, None]
        lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
        qi, ri = np.nonzero(hit)
        return lims, val[qi, ri], ri.astype(np.int64) + idx_offset


def test_header_declares_and_binding_binds_range_search():
    header = open(os.path.join(ROOT, "include", "mips_hip.h")).read()
    m = re.search(r"int mips_range_search\(([^;]*)\);", header)
    assert m, "mips_range_search is not declared in mips_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 12 and params[4].startswith("const float* radii") and "out_lims" in params[5] and "cap" in params[8]
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", header).group(1)) == ram._lib.ABI_VERSION == 1
    assert "mips_range_search" in ram._lib.EXPORTS
    lib = ram._lib.load()                                          # builds, loads and binds: AttributeError if the symbol is missing
    assert len(lib.mips_range_search.argtypes) == 12


def test_radius_broadcasting():
    radii = ram.MipsIndex._radii
    assert np.array_equal(radii(0.5, 3), np.full(3, 0.5, np.float32)) and radii(0.5, 3).dtype == np.float32
    assert np.array_equal(radii([1, 2, 3], 3), np.array([1, 2, 3], np.float32))
    assert np.array_equal(radii(np.float64(np.inf), 2), np.array([np.inf, np.inf], np.float32))
    assert radii(1.0, 0).shape == (0,)
    with pytest.raises(ValueError):
        radii([1.0, 2.0], 3)
    with pytest.raises(ValueError, match="NaN"):
        radii([1.0, np.nan, 0.0], 3)


def test_faiss_shim_range_search_over_a_fake_index():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 16)).astype(np.float32)
    q = rng.standard_normal((7, 16)).astype(np.float32)
    fs = ram.faiss_shim
    fx = fs.IndexFlatIP(16)
    fx._inner = FakeRangeIndex(x)
    lims, D, I = fx.range_search(q.astype(np.float64), 4.0)        # faiss casts to float32 as well
    assert lims.dtype == np.uint64 and lims.shape == (8,) and lims[0] == 0
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (int(lims[-1]),) and lims[-1] > 0
    for j in range(7):
        ids = I[int(lims[j]):int(lims[j + 1])]
        assert np.array_equal(ids, np.flatnonzero((q[j].astype(np.float64) @ x.T.astype(np.float64)).astype(np.float32) > 4.0))
    # L2: the reference's augmented vectors; the index behind the shim sees the stripped columns
    fl = fs.IndexFlat(17, fs.METRIC_L2)
    fake = fl._inner = FakeRangeIndex(x, metric=1)
    phi = np.square(x.astype(np.float64)).sum(axis=1).max()
    lims, D, I = fl.range_search(augment_xq(q), float(phi))
    assert fake.seen == [(7, 16)] and lims.dtype == np.uint64 and lims[-1] > 0
    xa, qa = augment_xb(x.astype(np.float64)), augment_xq(q).astype(np.float64)
    dist = np.square(qa[:, None, :] - xa[None, :, :]).sum(axis=2)  # plain squared L2 on the augmented vectors: what faiss computes
    assert np.allclose(D, dist[np.repeat(np.arange(7), np.diff(lims.astype(np.int64))), I], rtol=1e-5)
    bad = augment_xq(q)
    bad[0, -1] = 1.0
    with pytest.raises(ValueError, match="augmentation"):
        fl.range_search(bad, 1.0)


def test_near_duplicates_pairs_over_a_fake_index():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((300, 24)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[[5, 17, 200, 299]] = x[5]
    x[[40, 41]] = x[40]
    kb = KnowledgeBase({"emb": x})
    fake = FakeRangeIndex(x)
    kb.add_faiss_index("emb", custom_index=fake)
    i, j, s = kb.near_duplicates("emb", 0.99, batch_rows=64)
    assert list(zip(i.tolist(), j.tolist())) == [(5, 17), (5, 200), (5, 299), (17, 200), (17, 299), (40, 41), (200, 299)]
    assert i.dtype == np.int64 and j.dtype == np.int64 and s.dtype == np.float32 and np.allclose(s, 1.0, atol=1e-5)
    assert fake.seen == [(64, 24)] * 4 + [(44, 24)]                # the column in batches of batch_rows
    i, j, s = kb.near_duplicates("emb", 2.0)                       # nothing that close: empty arrays of the same types
    assert len(i) == len(j) == len(s) == 0 and i.dtype == np.int64 and s.dtype == np.float32
    # L2: the indexed column is the augmented one; the index stores -- and is queried with -- the stripped rows
    xa = augment_xb(x.astype(np.float64)).astype(np.float32)
    kl = KnowledgeBase({"aug": xa})
    fake_l2 = FakeRangeIndex(x, metric=1)
    kl.add_faiss_index("aug", index_name="l2", custom_index=fake_l2)
    i, j, s = kl.near_duplicates("l2", 0.02, batch_rows=128)       # distance 2 - 2 cos < 0.02
    assert list(zip(i.tolist(), j.tolist())) == [(5, 17), (5, 200), (5, 299), (17, 200), (17, 299), (40, 41), (200, 299)]
    assert fake_l2.seen == [(128, 24), (128, 24), (44, 24)]
    with pytest.raises(ValueError, match="add_faiss_index"):
        KnowledgeBase({"emb": x}, index=object(), index_name="foreign").near_duplicates("foreign", 0.5)
