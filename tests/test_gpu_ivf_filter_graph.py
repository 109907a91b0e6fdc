"""The filtered IVF search under HIP graph capture (the extended capture contract): no grid, pointer, size or loop bound
of mips_ivf_search_grp depends on the VALUES of the queries, the query labels or the bitmap, so a graph captured once replays with
other queries, other q_labels contents and a bitmap rewritten in place, and each replay equals the eager call bit for bit.

One fresh `python -c` child under a time limit, started once: a fault ends that child and nothing else, and is met once."""
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
import ivf_cases as iv
case = iv.case_gauss(3000, 64, 12, 16)
ix = ram.IvfIndex(64, 16, dtype="f32")
ix.niter = 2
ix.train(case["rows"])
ix.add(case["rows"])
rng = np.random.default_rng(5)
labels = rng.integers(0, 30, 3000).astype(np.int32)
ix.set_labels(labels)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
sets = []
for n in range(4):
    q = case["q"] if n == 0 else rng.standard_normal((12, 64)).astype(np.float32)
    ql = rng.integers(0, 30, 12).astype(np.int32)
    ql[n] = ram.LABEL_NONE
    mask = rng.random(3000) < (0.9, 0.5, 0.1, 0.02)[n]
    sets.append((q, ql, np.packbits(mask, bitorder="little")))
want = [ix.search_probed(q, 5, 4, selector=bits, groups=ql, group_mode="exclude") for q, ql, bits in sets]   # eager, host inputs
assert len(set(w[1].tobytes() for w in want)) == 4
qbuf, lbuf = dev(sets[0][0]).clone(), dev(sets[0][1]).clone()
sel = ram.Selector.from_bitmap(dev(sets[0][2]).clone(), 3000)
side = torch.cuda.Stream()
with torch.cuda.stream(side):                               # warm-up off the default stream: the scratch takes its size
    ix.search_probed(qbuf, 5, 4, selector=sel, groups=lbuf, group_mode="exclude")
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    D, I = ix.search_probed(qbuf, 5, 4, selector=sel, groups=lbuf, group_mode="exclude")
for n in (1, 2, 3):                                         # three sets that are not the captured one
    qbuf.copy_(dev(sets[n][0]))
    lbuf.copy_(dev(sets[n][1]))
    sel.bits.copy_(dev(sets[n][2]))                         # the bitmap rewritten in place
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy(), want[n][1]), n
    assert np.array_equal(D.cpu().numpy().view(np.uint32), want[n][0].view(np.uint32)), n
print("filtered search replays ok")
"""


def test_filtered_search_replays_with_other_queries_labels_and_bitmap():
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                         timeout=240, env=dict(os.environ))
    assert out.returncode == 0 and "filtered search replays ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
