"""`Mips` over an IVF index (MipsArgs.mips_nlist > 0): leak-free retrieval end to end.  search(ignore_groups=aid) never returns a row of
the query's own article and equals the NumPy restatement of tests/ivf_filter_cases.py on the rows, centroids and assignments the
index holds; with every list probed (mips_nprobe = mips_nlist) every route -- search, search_device with ignore_indexes and with
return_rows, forward(ignore_own_group=True), np_search -- equals the same Mips over the flat index bit for bit; save / load keep the
results; what an IVF index does not serve is refused by name."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_filter_cases as fc  # noqa: E402

N, D, NQ = 2000, 64, 12


def _ram():
    import retrieval_augmented_mds_amd as ram

    return ram


def _data():
    rng = np.random.default_rng(21)
    sizes = []
    while sum(sizes) < N:
        sizes.append(int(rng.integers(1, 41)))                                   # articles of 1 .. 40 rows
    aid = np.repeat(np.arange(len(sizes)) + 1000, sizes)[:N]
    x = rng.standard_normal((N, D)).astype(np.float32)
    qrow = rng.choice(N, NQ, replace=False)                                      # every query sits next to a row of its own article
    q = (x[qrow] + 0.05 * rng.standard_normal((NQ, D))).astype(np.float32)
    data = {"mips_column": [f"text {i}" for i in range(N)], "aid": [int(a) for a in aid]}
    return x, data, aid, q, qrow


_made = {}


def _mips(tmp, nlist, nprobe):
    ram = _ram()
    key = (nlist, nprobe)
    if key not in _made:
        x, data, aid, q, qrow = _data()
        m = ram.Mips(ram.MipsArgs(mips_nlist=nlist, mips_index_dtype="f32", mips_nprobe=nprobe, mips_tmp_folder=str(tmp / f"m{nlist}_{nprobe}")), data=data)
        m.build_index(x)
        _made[key] = m
    return _made[key]


def _eq(a, b):
    a, b = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in a], [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in b]
    assert np.array_equal(a[1], b[1]), (a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("nprobe", [None, 2, 8])
def test_search_never_returns_the_own_group_and_equals_the_restatement(tmp_path_factory, nprobe):
    ram = _ram()
    tmp = tmp_path_factory.getbasetemp()
    x, data, aid, q, qrow = _data()
    m = _mips(tmp, 8, nprobe)
    index = m._index()
    assert isinstance(index, ram.IvfIndex) and index.nlist == 8 and index.nprobe == (nprobe or 1) and index.ntotal == N
    qp = m._prepare_query(q.copy())
    own = aid[qrow]
    s, i = m.search(qp, k=5, ignore_groups=own)
    assert (i >= 0).any() and not (aid[np.where(i >= 0, i, 0)] == own[:, None])[i >= 0].any()          # no row of the own article
    rows = index.reconstruct_n(0, N)                                                                   # what the index holds
    uniq, codes = np.unique(aid, return_inverse=True)
    want = fc.search(rows, qp, index.assignments(), index.centroids(), 5, nprobe or 1, "f32", labels=codes.astype(np.int32),
                     q_labels=np.searchsorted(uniq, own).astype(np.int32))
    _eq((s, i), want)
    assert float(m.retrieved_group_hits(i, own).sum()) == 0.0
    if nprobe == 8:                                                                                    # every list: unfiltered, the own row comes first
        plain = m.search(qp, k=5)
        assert (aid[plain[1][:, 0]] == own).all() and float(m.retrieved_group_hits(plain[1], own)[:, 0].sum()) == NQ


def test_every_list_probed_equals_the_flat_facade(tmp_path_factory):
    import torch

    tmp = tmp_path_factory.getbasetemp()
    x, data, aid, q, qrow = _data()
    ivf, flat = _mips(tmp, 8, 8), _mips(tmp, 0, None)
    own = aid[qrow]
    qp = ivf._prepare_query(q.copy())
    _eq(ivf.search(qp, k=5), flat.search(qp, k=5))
    _eq(ivf.search(qp, k=5, ignore_groups=own), flat.search(qp, k=5, ignore_groups=own))
    a, b = ivf.search(qp, ignore_indexes=list(qrow), k=5), flat.search(qp, ignore_indexes=list(qrow), k=5)
    assert [list(map(int, r)) for r in a[1]] == [list(map(int, r)) for r in b[1]]
    assert [[np.float32(v).view(np.uint32) for v in r] for r in a[0]] == [[np.float32(v).view(np.uint32) for v in r] for r in b[0]]
    assert all(int(r) not in row for r, row in zip(qrow, a[1]))
    qd = torch.from_numpy(q).cuda()
    ign = torch.from_numpy(qrow.astype(np.int64)).cuda()
    _eq(ivf.search_device(qd, k=5), flat.search_device(qd, k=5))
    _eq(ivf.search_device(qd, ignore_indexes=ign, k=5), flat.search_device(qd, ignore_indexes=ign, k=5))
    _eq(ivf.search_device(qd, ignore_indexes=ign, k=5, ignore_groups=own), flat.search_device(qd, ignore_indexes=ign, k=5, ignore_groups=own))
    ra, rb = ivf.search_device(qd, k=3, return_rows=True, ignore_groups=own), flat.search_device(qd, k=3, return_rows=True, ignore_groups=own)
    _eq(ra[:2], rb[:2])
    assert ra[2].is_cuda and ra[2].shape == (NQ, 3, D) and torch.equal(ra[2], rb[2])
    fa = ivf.forward(q.copy(), aid=list(own), k=4, ignore_own_group=True)
    fb = flat.forward(q.copy(), aid=list(own), k=4, ignore_own_group=True)
    _eq((fa.scores, fa.indices), (fb.scores, fb.indices))
    assert fa.flat_texts == fb.flat_texts and len(fa.flat_texts) == NQ * 4
    _eq(ivf.np_search(q, k=5), flat.np_search(q, k=5))                                                 # exhaustive: the inner flat index
    one = _mips(tmp, 8, None)
    _eq(one.np_search(q, k=5), flat.np_search(q, k=5))                                                 # ... whatever nprobe is
    kb = ivf.embeddings
    sa, ea = kb.get_nearest_examples_batch(ivf.index_name, qp, k=4, groups=own)
    sb, eb = flat.embeddings.get_nearest_examples_batch(flat.index_name, qp, k=4, groups=own)
    assert all(np.array_equal(u, v) for u, v in zip(sa, sb)) and [e["mips_column"] for e in ea] == [e["mips_column"] for e in eb]


def test_save_load_round_trip(tmp_path):
    ram = _ram()
    x, data, aid, q, qrow = _data()
    args = ram.MipsArgs(mips_nlist=8, mips_index_dtype="f32", mips_nprobe=3, mips_tmp_folder=str(tmp_path / "m"))
    m = ram.Mips(args, data=data)
    m.build_index(x)
    own = aid[qrow]
    qp = m._prepare_query(q.copy())
    before = m.search(qp, k=5, ignore_groups=own)
    plain = m.search(qp, k=5)
    m.save()
    assert m.embeddings is None
    m2 = ram.Mips(args)
    m2.load()
    index = m2._index()
    assert isinstance(index, ram.IvfIndex) and index.nprobe == 3 and index.ntotal == N
    _eq(m2.search(qp, k=5), plain)
    _eq(m2.search(qp, k=5, ignore_groups=own), before)


def test_refusals(tmp_path):
    ram = _ram()
    x, data, aid, q, qrow = _data()
    with pytest.raises(NotImplementedError, match="IVF"):
        ram.Mips(ram.MipsArgs(mips_nlist=8, mips_string_factory="IVF8,Flat", mips_tmp_folder=str(tmp_path)), data=data).build_index(x)   # never a factory string
    with pytest.raises(NotImplementedError, match="L2"):
        ram.Mips(ram.MipsArgs(mips_nlist=8, mips_metric_type=1, mips_tmp_folder=str(tmp_path)), data=data).build_index(x)
    with pytest.raises(NotImplementedError, match="mips_shard"):
        ram.Mips(ram.MipsArgs(mips_nlist=8, mips_shard=True, mips_tmp_folder=str(tmp_path)), data=data).build_index(x)
    with pytest.raises(NotImplementedError, match="streaming"):
        ram.Mips(ram.MipsArgs(mips_nlist=8, mips_tmp_folder=str(tmp_path)), data=data).begin_index_build(D)
    m = _mips(tmp_path, 8, 2)
    qp = m._prepare_query(q.copy())
    assert m.search(qp, k=29)[1].shape == (NQ, 29)
    with pytest.raises(NotImplementedError, match="k"):
        m.search(qp, k=30)
    with pytest.raises(NotImplementedError, match="k"):
        m.search(qp, ignore_indexes=list(qrow), k=29)                                                  # k + 1 = 30
    kb = m.embeddings
    with pytest.raises(NotImplementedError, match="IVF"):
        kb.near_duplicates(m.index_name, 0.9)
    with pytest.raises(NotImplementedError, match="IVF"):
        kb.drop_near_duplicates(m.index_name, 0.9)
    with pytest.raises(NotImplementedError, match="IVF"):
        kb.remove_rows([1, 2])
    assert len(kb) == N and m._index().ntotal == N
