"""The wide IVF search under HIP graph capture (the capture contract of mips_ivf_search_grp holds unchanged for
mips_ivf_search_wide_grp): no grid, pointer, size or loop bound depends on the VALUES of the queries or the query labels, so a graph
captured once replays with other queries and other label contents, and each replay equals the eager call bit for bit.

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
    sets.append((q, ql))
want = [ix.search_probed_wide(q, 64, 4, groups=ql, group_mode="exclude") for q, ql in sets]        # eager, host inputs
assert len(set(w[1].tobytes() for w in want)) == 4
for (q, ql), w in zip(sets, want):                                                                  # hard negatives: no row of the query's own group
    own = labels[np.where(w[1] >= 0, w[1], 0)] == ql[:, None]
    assert not (own & (w[1] >= 0)).any() and (w[1][:, :30] >= 0).all()
qbuf, lbuf = dev(sets[0][0]).clone(), dev(sets[0][1]).clone()
side = torch.cuda.Stream()
with torch.cuda.stream(side):                               # warm-up off the default stream: the scratch takes its size
    ix.search_probed_wide(qbuf, 64, 4, groups=lbuf, group_mode="exclude")
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    D, I = ix.search_probed_wide(qbuf, 64, 4, groups=lbuf, group_mode="exclude")
for n in (1, 2, 3):                                         # three sets that are not the captured one
    qbuf.copy_(dev(sets[n][0]))
    lbuf.copy_(dev(sets[n][1]))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy(), want[n][1]), n
    assert np.array_equal(D.cpu().numpy().view(np.uint32), want[n][0].view(np.uint32)), n
print("wide search replays ok")
"""


def test_wide_search_replays_with_other_queries_and_labels():
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                         timeout=240, env=dict(os.environ))
    assert out.returncode == 0 and "wide search replays ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
