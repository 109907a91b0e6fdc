"""The range search over the probed lists under HIP graph capture (the capture contract of mips_ivf_search_grp, extended in
the same words to mips_ivf_range_search_grp): no grid, pointer, size or loop bound depends on the VALUES of the queries, the radii or
the query labels -- how many hits there are, where they land and how long a stretch is exist on the device only -- so a graph captured
once replays with other queries, other radii and other label contents, and each replay equals the eager call bit for bit.

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
CAP = 12 * 3000
sets = []
for n in range(4):
    q = case["q"] if n == 0 else rng.standard_normal((12, 64)).astype(np.float32)
    ql = rng.integers(0, 30, 12).astype(np.int32)
    ql[n] = ram.LABEL_NONE
    r = rng.uniform(-4.0, 12.0, 12).astype(np.float32)         # from most of the probed rows down to a handful
    r[(n + 5) % 12] = np.inf                                    # an empty query, elsewhere in every set
    r[(n + 7) % 12] = -np.inf                                   # every probed admitted row
    sets.append((q, ql, r))
want = [ix.range_search_probed(q, r, 4, groups=ql, group_mode="exclude") for q, ql, r in sets]      # eager, host inputs
assert len(set(w[0].tobytes() for w in want)) == 4 and all(0 < w[0][-1] < CAP for w in want)
for (q, ql, r), (lims, D, I) in zip(sets, want):                                                     # no row of the query's own group, all above the radius
    for j in range(12):
        assert not (labels[I[lims[j]:lims[j + 1]]] == ql[j]).any() and (D[lims[j]:lims[j + 1]] > r[j]).all()
        assert (np.diff(I[lims[j]:lims[j + 1]]) > 0).all()
qbuf, lbuf, rbuf = dev(sets[0][0]).clone(), dev(sets[0][1]).clone(), dev(sets[0][2]).clone()
lims = torch.empty(13, dtype=torch.int64, device="cuda")
D = torch.empty(CAP, dtype=torch.float32, device="cuda")
I = torch.empty(CAP, dtype=torch.int64, device="cuda")
side = torch.cuda.Stream()
with torch.cuda.stream(side):                               # warm-up off the default stream: the scratch takes its size
    ix.range_search_probed_into(qbuf, rbuf, lims, D, I, nprobe=4, groups=lbuf, group_mode="exclude")
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    ix.range_search_probed_into(qbuf, rbuf, lims, D, I, nprobe=4, groups=lbuf, group_mode="exclude")
for n in (1, 2, 3):                                         # three sets that are not the captured one
    qbuf.copy_(dev(sets[n][0]))
    lbuf.copy_(dev(sets[n][1]))
    rbuf.copy_(dev(sets[n][2]))
    g.replay()
    torch.cuda.synchronize()
    wl, wd, wi = want[n]
    total = int(wl[-1])
    assert np.array_equal(lims.cpu().numpy(), wl), n
    assert np.array_equal(I[:total].cpu().numpy(), wi), n
    assert np.array_equal(D[:total].cpu().numpy().view(np.uint32), wd.view(np.uint32)), n
print("range search replays ok")
"""


def test_range_search_replays_with_other_queries_radii_and_labels():
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                         timeout=240, env=dict(os.environ))
    assert out.returncode == 0 and "range search replays ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
