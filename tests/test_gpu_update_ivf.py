"""mips_ivf_update / IvfIndex.update_rows on the GPU: nlist = 8, the three storages.  After an update the index equals a FRESH IvfIndex
with the same centroids (set_centroids; an 'sq8' index the same range) that was given the final rows of the sequential loop
(tests/update_cases.py): assignments, list sizes, the stored rows, and search_probed, search_probed_wide and range_search_probed,
bit for bit -- after an update that moves rows between lists (duplicates, ids that name no row, host and device forms) and after
one that empties a list.  flat.update_rows alone changes the row and leaves it in its old list."""
import os
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import test_gpu_lifecycle as gl
    import update_cases as uc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

N, D, NLIST, NPROBE = uc.NTOTAL, 64, 8, 3


def _fresh(live, rows):
    ix = ram.IvfIndex(D, NLIST, dtype=live.dtype)
    ix.set_centroids(live.centroids())
    if live.dtype == "sq8":
        ix.set_sq8_params(*live.flat.sq8_params())
    ix.add(rows)
    return ix


def _same_index(live, rows, what):
    fresh = _fresh(live, rows)
    assert live.ntotal == fresh.ntotal == len(rows), what
    assert np.array_equal(live.assignments(), fresh.assignments()), f"{what}: assignments differ"
    assert np.array_equal(live.list_sizes(), fresh.list_sizes()), f"{what}: list sizes differ"
    assert np.array_equal(live.flat.rows_raw().view(np.uint8), fresh.flat.rows_raw().view(np.uint8)), f"{what}: stored rows differ"
    q = synth.generate(902, 0, 24, D, synth.KIND_GAUSS).astype(np.float32)
    q[:6] = rows[[0, 5, 1717, N - 1, 2, 40]]                       # rows of the index as queries: updated ones among them
    qd = torch.from_numpy(q).cuda()
    for name, run in (("search_probed", lambda i: i.search_probed(q, 5, NPROBE)),
                      ("search_probed (device)", lambda i: i.search_probed(qd, 5, NPROBE)),
                      ("search_probed, every list", lambda i: i.search_probed(q, 5, NLIST)),
                      ("search_probed_wide", lambda i: i.search_probed_wide(q, 64, NPROBE))):
        gl._equal_arrays(run(live), run(fresh), f"{what}: {name} differs from a fresh index")
    radius = fresh.search_probed_wide(q, 64, NPROBE)[0][:, 20].copy()
    gl._equal_arrays(live.range_search_probed(q, radius, NPROBE), fresh.range_search_probed(q, radius, NPROBE), f"{what}: range_search_probed")
    gl._equal_arrays(live.flat.search(q, 5), fresh.flat.search(q, 5), f"{what}: the flat search")
    return fresh


@pytest.mark.parametrize("storage", ["bf16", "f32", "sq8"])
def test_rows_move_between_lists_and_a_list_is_emptied(storage):
    base = uc.base_rows(N, D)
    ix = ram.IvfIndex(D, NLIST, dtype=storage)
    ix.niter = 2
    ix.train(base)
    ix.add(base)
    ix.search_probed(base[:9], 5, NPROBE)                          # warm
    model, step = base, 0
    for off in (0, uc.OFFSET):
        sets = uc.id_sets(N, off)
        for name, form in (("n0", "host"), ("n65", "device"), ("n1000", "host"), ("n1000", "device")):
            step += 1
            ids, x = sets[name], uc.new_rows(len(sets[name]), D, seed=10 + step)
            before = ix.assignments()
            i_arg, x_arg = (ids, x) if form == "host" else (torch.from_numpy(ids).cuda(), torch.from_numpy(x).cuda())
            count = ix.update_rows(i_arg, x_arg, idx_offset=off, return_count=True)
            model, want = uc.apply_update(model, ids, x, off)
            assert count == want
            what = f"{storage}, {name}, offset {off}, {form}"
            _same_index(ix, model, what)
            if name == "n1000":
                written = np.unique(uc.local_rows(ids, off, N)[uc.local_rows(ids, off, N) >= 0])
                moved = ix.assignments() != before
                assert moved[written].sum() > len(written) // 2 and not moved[np.setdiff1d(np.arange(N), written)].any(), what
    # one list loses all its rows: they become copies of another list's centroid
    sizes, assign = ix.list_sizes(), ix.assignments()
    gone = int(np.argmin(np.where(sizes > 0, sizes, N)))
    other = (gone + 3) % NLIST
    ids = np.flatnonzero(assign == gone).astype(np.int64)
    x = np.tile(ix.centroids()[other], (len(ids), 1)) * (1.0 + np.arange(len(ids), dtype=np.float32)[:, None] / 64)
    assert ix.update_rows(ids, x.astype(np.float32), return_count=True) == len(ids) == sizes[gone]
    model, _ = uc.apply_update(model, ids, x.astype(np.float32))
    _same_index(ix, model, f"{storage}: list {gone} emptied")
    assert ix.list_sizes()[gone] == 0 and (ix.assignments()[ids] != gone).all()
    # an add and an update behind it
    ix.add(base[:300])
    model = np.concatenate([model, base[:300]])
    tail = np.array([N + 299, N, 7, N + 299], np.int64)
    y = uc.new_rows(4, D, seed=99)
    assert ix.update_rows(tail, y, return_count=True) == 3
    _same_index(ix, uc.apply_update(model, tail, y)[0], f"{storage}: after an add")


def test_flat_update_rows_alone_leaves_the_assignments_and_refusals():
    base = uc.base_rows(N, D)
    ix = ram.IvfIndex(D, NLIST, dtype="f32")
    ix.niter = 2
    with pytest.raises(RuntimeError, match="not trained"):
        ix.update_rows([0], base[:1])
    ix.train(base)
    ix.add(base)
    before = ix.assignments()
    ids = uc.id_sets(N)["n64"]
    x = -base[ids]                                                 # the opposite vector: its nearest list is another one
    assert ix.flat.update_rows(ids, x, return_count=True) == 64
    assert np.array_equal(ix.assignments(), before)                # the rows changed, their lists did not
    assert np.array_equal(ix.flat.rows_raw(), uc.apply_update(base, ids, x)[0])
    D5, I5 = ix.search_probed(x[:8], 5, NLIST)                      # every list probed: exact on what it reads
    gl._equal_arrays((D5, I5), ix.flat.search(x[:8], 5), "flat update, every list probed")
    assert ix.update_rows(ids, x, return_count=True) == 64          # the IVF call moves them
    assert (ix.assignments()[ids] != before[ids]).sum() > 32
    with pytest.raises(NotImplementedError):
        ix.update_rows(ids, np.zeros((64, D), np.uint8))           # raw codes cannot be assigned to a list
    with pytest.raises(ValueError):
        ix.update_rows(ids[:3], x)
