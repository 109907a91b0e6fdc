"""The IVFPQ search under HIP graph capture (include/mips_hip_ivfpq.h: the capture contract of mips_ivfpq_search).  No launch of the
search depends on query values -- grid, block, LDS size, pointers and loop bounds come from (ns, k, M, d, p, nlist, ntotal, the compute
units); the probed lists, their sizes and their rows are read on the device -- and this is the test of that: one device-in /
device-out search is captured, replayed twice with other queries (which probe other lists), and every replay equals the eager call
bit for bit -- once on the 4-wave scan (d = 32, M = 4) and once on the 16-wave one (d = 80, M = 40), whose launch sets its dynamic
LDS attribute on every call, under capture too.  The capture runs in a fresh `python -c` child under a time limit, so a fault
ends that child and nothing else, and is met once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SEARCH = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
import retrieval_augmented_mds_amd as ram
import ivfpq_cases as vc
case = vc.case_planted({d}, {M}, 8, 1000, 4)
ix = ram.IvfPqIndex({d}, 8, {M})
ix.set_centroids(case["centroids"])
ix.set_codebook(case["codebook"])
ix.add_codes(case["codes"], case["assign"])
ix.nprobe = 3
rng = np.random.default_rng(5)
sets = [case["q"]] + [rng.standard_normal((4, {d})).astype(np.float32) for _ in range(2)]
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
want = [ix.search(q, 5) for q in sets]                      # eager
probed = [vc.probe(q, case["centroids"], 3)[0] for q in sets]
assert not np.array_equal(probed[0], probed[1]) and not np.array_equal(probed[0], probed[2])   # other queries, other lists
for w, q in zip(want, sets):
    ref = vc.search(q, case["centroids"], case["codebook"], case["codes"], case["assign"], 5, 3)
    assert np.array_equal(w[1], ref[1]) and np.array_equal(w[0].view(np.uint32), ref[0].view(np.uint32))
buf = dev(sets[0]).clone()
side = torch.cuda.Stream()
with torch.cuda.stream(side):                               # warm-up off the default stream: the scratch takes its size
    ix.search(buf, 5)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    D, I = ix.search(buf, 5)
for n in (1, 2):                                            # two sets that are not the captured one
    buf.copy_(dev(sets[n]))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy(), want[n][1]), n
    assert np.array_equal(D.cpu().numpy().view(np.uint32), want[n][0].view(np.uint32)), n
print("search replays ok")
"""


@pytest.mark.parametrize("d,M", [(32, 4), (80, 40)])
def test_search_replays_with_other_queries(d, M):
    out = subprocess.run([sys.executable, "-c", _SEARCH.format(root=ROOT, tests=os.path.join(ROOT, "tests"), d=d, M=M)], capture_output=True, text=True,
                         timeout=240, env=dict(os.environ))
    assert out.returncode == 0 and "search replays ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
