"""The report of the last search (MipsIndex.margin_stats) across entry points: one fixed sequence of calls on an index of
near-duplicate rows (the generator of tools/dispatch_record.py: queries get flagged), the statistics read after every step.

The expected values were recorded on the commit before the report became one value per call (SearchReport); that commit and
this one agree on every step but the one marked below."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, D, NQ = 3001, 768, 64
UNKNOWN = (-1, 0, 0)

STEPS = ("host search", "device search", "device search, resolve_budget=1", "wide search k=30, device", "range search, counting call",
         "device search, margin_check=0", "margin_check back to 1, no search", "host search on the emptied index",
         "split-tail search", "remove 100 rows, device search")

# (flagged, rescanned, unresolved) after each step, as recorded on the parent commit
RECORDED = {
    "bf16": [(58, 58, 0), (58, 58, 0), (58, 58, 9), (0, 0, 0), (0, 0, 0), (-1, 0, 0), (0, 0, 0), (0, 0, 0), (64, 64, 0), (56, 56, 0)],
    "f32": [(64, 64, 0), (64, 64, 0), (64, 0, 64), (0, 0, 0), (0, 0, 0), (-1, 0, 0), (0, 0, 0), (0, 0, 0), (64, 64, 0), (64, 64, 0)],
}
# Step 7 is the one deliberate difference.  The search of step 6 ran without the margin check, so it counted nothing and its
# report names no device word; setting the knob back does not make an older call's word (the parent read the wide search's of
# step 4 there) the count of the last search: it stays "unknown" until the next search.
# (Step 8: a search of an empty index certifies trivially and reports (0, 0, 0); on the parent it wrote nothing and the same
# figures were the ones step 7 had cached.)
EXPECTED = {dt: [UNKNOWN if i == 6 else s for i, s in enumerate(steps)] for dt, steps in RECORDED.items()}


def _dups():
    spec = importlib.util.spec_from_file_location("dispatch_record", os.path.join(ROOT, "tools", "dispatch_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._dups(D, ROWS, NQ, seed=D + 7)


def run_sequence(dtype):
    import torch

    import retrieval_augmented_mds_amd as ram

    x, q_host = _dups()
    q_dev = torch.from_numpy(q_host).cuda()
    ix = ram.MipsIndex(D, dtype=dtype)
    ix.add(x)
    got = []

    def note(synchronize=True):
        s = ix.margin_stats(synchronize=synchronize)
        got.append((s["flagged"], s["rescanned"], s["unresolved"]))

    ix.search(q_host, 10)                                   # 1
    note()
    ix.search(q_dev, 10)                                    # 2
    note()
    ix.set_param("resolve_budget", 1)                       # 3
    ix.search(q_dev, 10)
    note()
    ix.set_param("resolve_budget", 0)
    ix.search_wide(q_dev, 30)                               # 4
    note()
    lims = torch.empty(NQ + 1, dtype=torch.int64, device="cuda")
    ix.range_search_into(q_dev, 0.0, lims, torch.empty(0, dtype=torch.float32, device="cuda"),
                         torch.empty(0, dtype=torch.int64, device="cuda"))  # 5
    note()
    ix.set_param("margin_check", 0)                         # 6
    ix.search(q_dev, 10)
    note()
    ix.set_param("margin_check", 1)                         # 7
    note()
    ix.reset()                                              # 8
    ix.search(q_host, 10)
    note()
    ix.add(x)
    tail = torch.cuda.Stream()                              # 9
    ix.search(q_dev, 10, tail_stream=tail)
    note(synchronize=True)
    tail.synchronize()
    assert ix.remove_ids(np.arange(100, dtype=np.int64) * 30) == 100  # 10
    ix.search(q_dev, 10)
    note()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_report_sequence(dtype):
    got = run_sequence(dtype)
    for name, g, e in zip(STEPS, got, EXPECTED[dtype]):
        print(f"{dtype} {name}: {g} (expected {e})")
    assert got == EXPECTED[dtype]
