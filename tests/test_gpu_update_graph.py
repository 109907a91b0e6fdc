"""update_rows + search under HIP graph capture.  With device ids and rows mips_index_update never synchronises on an inner-product
index, and no grid, pointer, size or loop bound depends on the VALUES of the ids; this is the test of that: warm up, capture the
update and a search behind it once, replay twice with other ids (ids that name no row and duplicates among them) and other rows
in the same buffers, and compare every time with a fresh index of the rows the sequential loop leaves -- the captured search's
output, the stored rows, and a host search (on the fp32-exact index: the two-stage search over the bf16 image the replays wrote).

One `python -c` child under a time limit, in the way of tests/test_gpu_ivf_search_graph.py: a fault ends the child and nothing else."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
import retrieval_augmented_mds_amd as ram
import update_cases as uc
from oracle import synth
N, D = uc.NTOTAL, uc.D
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).view(np.uint32)   # float32 scores, bit for bit
base = uc.base_rows(N, D)
sets = [uc.id_sets(N, 0)["n1000"].copy() for _ in range(3)]
sets[1] = np.roll(sets[1], 333)                                  # the duplicates and the junk at other positions
sets[2] = np.where(np.arange(1000) % 3 == 0, -1, sets[2][::-1])  # a third of the positions name no row
rows = [uc.new_rows(1000, D, seed=40 + t) for t in range(3)]
q = synth.generate(903, 0, 12, D, synth.KIND_GAUSS).astype(np.float32)
for storage in ("bf16", "f32"):
    ix = ram.MipsIndex(D, dtype=storage)
    ix.add(base)
    ix.search(q, 5)                                              # host search: the caches are warm (f32: the bf16 image exists)
    idbuf, xbuf, qd = dev(sets[0]).clone(), dev(rows[0]).clone(), dev(q)
    q[3], q[7] = rows[1][999], rows[2][0]                        # (rows the replays write are among the queries)
    qd.copy_(dev(q))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                # warm-up off the default stream: the owner array is allocated
        ix.update_rows(idbuf, xbuf)
        ix.search(qd, 5)
    torch.cuda.synchronize()
    model = uc.apply_update(base, sets[0], rows[0])[0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ix.update_rows(idbuf, xbuf)
        Dg, Ig = ix.search(qd, 5)
    for t in (1, 2, 0):                                          # two other sets, then the captured one again
        idbuf.copy_(dev(sets[t])); xbuf.copy_(dev(rows[t]))
        g.replay()
        torch.cuda.synchronize()
        model = uc.apply_update(model, sets[t], rows[t])[0]
        fresh = ram.MipsIndex(D, dtype=storage)
        fresh.add(model)
        assert np.array_equal(ix.rows_raw().view(np.uint8), fresh.rows_raw().view(np.uint8)), (storage, t, "rows")
        Df, If = fresh.search(qd, 5)
        assert np.array_equal(Ig.cpu().numpy(), If.cpu().numpy()) and np.array_equal(bits(Dg), bits(Df)), (storage, t, "captured search")
        Dh, Ih = ix.search(q, 5)
        Dw, Iw = fresh.search(q, 5)
        assert np.array_equal(Ih, Iw) and np.array_equal(bits(Dh), bits(Dw)), (storage, t, "host search")
    print(storage, "replays ok")
print("update replays ok")
"""


def test_update_and_search_replay_with_other_ids_and_rows():
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert out.returncode == 0 and "update replays ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
