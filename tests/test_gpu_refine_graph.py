"""The two-stage search under HIP graph capture (include/mips_hip_refine.h: the capture contract).  No launch of search_candidates or
rerank depends on query values -- grid, block, LDS size, pointers and loop bounds come from (ns, k, kc, M, d, p, nlist, ntotal, the
compute units); probed lists, rows and candidate ids are read and range-checked on the device -- and this is the test of that: at
nq = 4, 1000 rows and k = 64 one device-in / device-out search_candidates followed by rerank is captured in one stream after a warm-up
call, replayed twice with other queries in the same buffers, and every replay equals the eager call bit for bit -- once at d = 32,
M = 4 (four pools) and once at d = 80, M = 40 (sixteen).  The capture runs in a fresh `python -c` child under a time limit, so a
fault ends that child and nothing else, and is met once."""
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
x = (vc.reconstruct(case["codes"], case["assign"], case["centroids"], case["codebook"]) + 0.3 * rng.standard_normal((1000, {d}))).astype(np.float32)
store = ram.MipsIndex({d})
store.add(x)
sets = [case["q"]] + [rng.standard_normal((4, {d})).astype(np.float32) for _ in range(2)]
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
def two_stage(q):
    _, C = ix.search_candidates(q, 64)
    return store.rerank(q, C, 10)
want = [two_stage(q) for q in sets]                         # eager, host in and out
assert not np.array_equal(want[0][1], want[1][1]) and not np.array_equal(want[0][1], want[2][1])
buf = dev(sets[0]).clone()
side = torch.cuda.Stream()
with torch.cuda.stream(side):                               # warm-up off the default stream: the scratch takes its size
    two_stage(buf)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    D, I = two_stage(buf)
for n in (1, 2):                                            # two sets that are not the captured one
    buf.copy_(dev(sets[n]))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy(), want[n][1]), n
    assert np.array_equal(D.cpu().numpy().view(np.uint32), want[n][0].view(np.uint32)), n
print("two-stage replays ok")
"""


@pytest.mark.parametrize("d,M", [(32, 4), (80, 40)])
def test_two_stage_search_replays_with_other_queries(d, M):
    out = subprocess.run([sys.executable, "-c", _SEARCH.format(root=ROOT, tests=os.path.join(ROOT, "tests"), d=d, M=M)], capture_output=True, text=True,
                         timeout=240, env=dict(os.environ))
    assert out.returncode == 0 and "two-stage replays ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
