"""The layers above the index: Mips.refresh_embeddings equals rebuilding from the refreshed matrix -- flat f32 (both metrics), SQ8
storage and an IVF index with every list probed (the trained range / lists come from the first mips_train_size rows, which the
refresh leaves alone, so the rebuild trains the same) --, KnowledgeBase.update_rows keeps the indexed column in step with its index
(the stripped L2 column of add_faiss_index included), and faiss_shim's update_vectors on its index classes."""
import os
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import update_cases as uc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

N, D, TRAIN = 2000, 64, 512


def _eq(a, b, what):
    a, b = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in a], [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in b]
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what


def _case():
    rng = np.random.default_rng(31)
    x = (rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    ids = rng.integers(TRAIN, N, 300).astype(np.int64)
    ids[[5, 6, 299]] = N - 1                                         # a row refreshed three times: the last value stays
    y = (rng.standard_normal((300, D)) * rng.uniform(0.5, 3.0, (300, 1))).astype(np.float32)   # some longer than any row before
    q = np.concatenate([rng.standard_normal((8, D)).astype(np.float32), y[[299, 0, 17, 100]]])
    return x, ids, y, uc.apply_update(x, ids, y)[0], q


CONFIGS = {"flat f32": dict(mips_index_dtype="f32"),
           "flat f32 L2": dict(mips_index_dtype="f32", mips_metric_type=1),
           "flat bf16 raw": dict(mips_index_dtype="bf16", mips_normalize=False),
           "SQ8": dict(mips_string_factory="SQ8", mips_train_size=TRAIN),
           "IVF f32": dict(mips_index_dtype="f32", mips_nlist=8, mips_nprobe=8, mips_train_size=TRAIN),
           "IVF SQ8": dict(mips_string_factory="SQ8", mips_nlist=8, mips_nprobe=8, mips_train_size=TRAIN)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_refresh_embeddings_equals_a_rebuild(name, tmp_path):
    import torch

    x, ids, y, final, q = _case()
    data = {"mips_column": [f"text {i}" for i in range(N)], "aid": list(range(N))}
    live = ram.Mips(ram.MipsArgs(mips_tmp_folder=str(tmp_path / "a"), **CONFIGS[name]), data=data)
    live.build_index(x)
    qp = live._prepare_query(q.copy())
    live.search(qp, k=5)                                             # warm
    y_dev = torch.from_numpy(y).cuda()
    keep = y_dev.clone()
    live.refresh_embeddings(ids, y_dev)
    assert torch.equal(y_dev, keep)                                  # the caller's tensor is not normalised in place
    rebuilt = ram.Mips(ram.MipsArgs(mips_tmp_folder=str(tmp_path / "b"), **CONFIGS[name]), data=data)
    rebuilt.build_index(final)
    a, b = live._index(), rebuilt._index()
    assert a.ntotal == b.ntotal == N
    flat_a, flat_b = (a.flat, b.flat) if isinstance(a, ram.IvfIndex) else (a, b)
    assert np.array_equal(flat_a.rows_raw().view(np.uint8), flat_b.rows_raw().view(np.uint8)), name
    if isinstance(a, ram.IvfIndex):
        assert np.array_equal(a.assignments(), b.assignments())
    if "L2" in name:
        assert live.phi == rebuilt.phi == a.phi()
    assert live.max_norm >= rebuilt.max_norm                         # (grows with the refreshed rows, never shrinks)
    _eq(live.search(qp, k=5), rebuilt.search(qp, k=5), name)
    qd = torch.from_numpy(q).cuda()
    _eq(live.search_device(qd, k=5), rebuilt.search_device(qd, k=5), name + ": search_device")
    live.refresh_embeddings(np.zeros(0, np.int64), np.zeros((0, D), np.float32))   # nothing to refresh
    _eq(live.search(qp, k=5), rebuilt.search(qp, k=5), name + ": after an empty refresh")
    with pytest.raises(ValueError):
        live.refresh_embeddings([N], y[:1])                          # a row the base does not hold


def test_existing_refusals_stay():
    with pytest.raises(NotImplementedError):
        ram.Mips(ram.MipsArgs(mips_string_factory="IVF256,SQ8")).build_index(np.zeros((4, 8), np.float32))
    with pytest.raises(NotImplementedError):
        ram.Mips(ram.MipsArgs(mips_shard=True, mips_nlist=4))._nlist()
    with pytest.raises(RuntimeError, match="no index"):
        ram.Mips(ram.MipsArgs()).refresh_embeddings([0], np.zeros((1, 8), np.float32))


@pytest.mark.parametrize("metric", [0, 1])
def test_knowledge_base_keeps_the_column_in_step_with_the_index(metric):
    x, ids, y, final, q = _case()
    if metric == 1:                                                  # the reference indexes phi-augmented rows: constant norm
        phi = max(ram.get_phi(x), ram.get_phi(final))
        col, new, want = ram.augment_xb(x, phi=phi), ram.augment_xb(final, phi=phi)[ids], ram.augment_xb(final, phi=phi)
        queries = ram.augment_xq(q)
    else:
        col, new, want, queries = x.copy(), y, final, q
    kb = ram.KnowledgeBase({"cls": col.copy(), "text": [f"t{i}" for i in range(N)]})
    kb.add_faiss_index("cls", "mips_cls", metric_type=metric)
    kb.get_nearest_examples_batch("mips_cls", queries, k=5)
    kb.update_rows("mips_cls", ids, new)
    assert np.array_equal(kb["cls"], want) and kb["text"][N - 1] == f"t{N - 1}"
    fresh = ram.KnowledgeBase({"cls": want.copy(), "text": [f"t{i}" for i in range(N)]})
    fresh.add_faiss_index("cls", "mips_cls", metric_type=metric)
    a, b = kb.get_index("mips_cls").faiss_index, fresh.get_index("mips_cls").faiss_index
    assert np.array_equal(a.rows_raw(), b.rows_raw()) and a.d == D
    sa, ea = kb.get_nearest_examples_batch("mips_cls", queries, k=5)
    sb, eb = fresh.get_nearest_examples_batch("mips_cls", queries, k=5)
    for u, v, eu, ev in zip(sa, sb, ea, eb):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)) and eu["text"] == ev["text"]
    with pytest.raises(ValueError):
        kb.update_rows("mips_cls", [N], new[:1])
    with pytest.raises(ValueError):
        kb.update_rows("mips_cls", ids[:3], new[:2])


def test_the_shim_updates_vectors_on_its_index_classes():
    from retrieval_augmented_mds_amd import faiss_shim as faiss

    x, ids, y, final, q = _case()
    for make in (lambda: faiss.IndexFlatIP(D), lambda: faiss.IndexScalarQuantizer(D, faiss.ScalarQuantizer.QT_8bit, faiss.METRIC_INNER_PRODUCT)):
        a, b = make(), make()
        for ix, rows in ((a, x), (b, final)):
            ix.train(x[:TRAIN])
            ix.add(rows)
        a.search(q, 5)
        assert a.update_vectors(ids, y) == len(np.unique(ids)) and a.ntotal == N
        _eq(a.search(q, 5), b.search(q, 5), type(a).__name__)
        assert a.update_vectors(np.zeros(0, np.int64), np.zeros((0, D), np.float32)) == 0
    phi = max(ram.get_phi(x), ram.get_phi(final))
    a, b = faiss.IndexFlatL2(D + 1), faiss.IndexFlatL2(D + 1)
    a.add(ram.augment_xb(x, phi=phi))
    b.add(ram.augment_xb(final, phi=phi))
    assert a.update_vectors(ids, ram.augment_xb(final, phi=phi)[ids]) == len(np.unique(ids))
    _eq(a.search(ram.augment_xq(q), 5), b.search(ram.augment_xq(q), 5), "IndexFlatL2")
    with pytest.raises(NotImplementedError):
        a.update_vectors(ids[:2], np.ones((2, D + 1), np.float32))   # not phi-augmented
