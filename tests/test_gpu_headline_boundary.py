"""The headline scan instance, mips::scan_kernel_v4<6, 24, 2, 0, false, 1>, at the block counts where its block boundary changes
what it does: the ring prologue with fewer blocks than stages, the blocks that fetch the shared insert bounds and the ones that
fetch nothing, and the counted wait before the block barrier, which differs between the two (tests/boundary_cases.py lists
the block counts and why).  d = 768, 8 splits, rows = 256 nb and 256 nb - 31 (one row in the last block), 257 queries (seven
idle waves and one wave with a single live query in the second tile) and 512 (no idle wave), k = 5 and k = 1.

Every case is compared bit for bit with orc.search_exact and asserts that exactly this instance answered, that no query stayed
unresolved and that the index reports no scan error.  The rows are Gaussian with late winners planted: five multiples of every
third query (of the first 32 such queries) in the last block of a split and in blocks 8 and 9 -- a bound that a changed
refresh path read too high would refuse them.  tests/test_boundary_cases_host.py shows on the oracle alone that they are the
exact top 5."""
import os
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import boundary_cases as bc
    import headline_cases as hc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

CASES = [(nb, n) for nb in bc.BLOCKS_PER_SPLIT for n in bc.row_counts(nb)]


def _search(x, q, k):
    ix = ram.MipsIndex(bc.D, dtype="bf16")
    ix.add(x)
    ix.set_param("nsplit", bc.NSPLIT)
    s, i = ix.search(q, k)
    st = ix.margin_stats()
    assert ix.last_kernel == hc.KERNEL, f"dispatched to {ix.last_kernel}"
    assert st["unresolved"] == 0, st
    ix.check()
    return s, i, st


@pytest.mark.parametrize("nb,n", CASES)
def test_late_winners_match_the_oracle(nb, n):
    x, q, plants = bc.late_winners(nb, n)
    es, ei = orc.search_exact(q, x, 5)                    # once per data set: the first 257 queries and k = 1 are slices of it
    for query, rows in plants.items():
        assert sorted(ei[query]) == sorted(rows)
    for nq in bc.QUERY_COUNTS:
        for k in bc.KS:
            s, i, st = _search(x, q[:nq], k)
            what = f"nb {nb} rows {n} nq {nq} k {k}"
            print(f"{what}: flagged {st['flagged']}")
            bad = np.flatnonzero((i != ei[:nq, :k]).any(axis=1))
            assert np.array_equal(i, ei[:nq, :k]), f"{what}: indices differ in queries {bad[:8]} ({len(bad)} of {nq})"
            assert np.array_equal(s, es[:nq, :k]), f"{what}: scores differ"
