"""What tests/headline_cases.py claims about its inputs, shown on the CPU oracle alone (no GPU, no library): the planted rows
are the top k of their query, they share one running list of scan_kernel_v4's mapping, and the duplicate case has the answer
its docstring says.  tests/test_gpu_headline_scan.py runs the same inputs through the kernel."""
import os
import sys

import numpy as np
import pytest

from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import headline_cases as hc
finally:
    sys.path.pop(0)


def test_planted_rows_share_one_sub_list_of_the_kernels_mapping():
    """row % 32 places a row in its block, / 16 gives the half, % 16 / 4 the lane group; with 8 splits of 20011 rows a split
    is 79 blocks.  The five planted rows: one split, one half, one lane group, five blocks -- one list of 4 entries."""
    rows = hc.plant_rows()
    tps = hc.tiles_per_split(hc.N_ROWS)
    assert tps == 79 and len(rows) == 5 and max(rows) < hc.N_ROWS
    cs = [hc.coords(r, tps) for r in rows]
    for r, (split, block, half, group) in zip(rows, cs):
        in_block = r % 32
        assert (in_block // 16, (in_block % 16) // 4) == (half, group) == (hc.PLANT_HALF, hc.PLANT_GROUP)
        assert split == 0 and block == r // 32
    assert len({c[1] for c in cs}) == 5
    assert len({(c[0], c[3]) for c in cs}) == 1          # what a running list is keyed by
    assert hc.coords(33, 1) == (1, 1, 0, 0) and hc.coords(31, 1) == (0, 0, 1, 3) and hc.coords(20010, 79)[0] == 7


@pytest.mark.parametrize("d", hc.DIMS)
def test_planted_rows_are_the_top_five_of_their_query(d):
    x, q, rows = hc.planted(d)
    es, ei = orc.search_exact(q[hc.PLANT_QUERY:hc.PLANT_QUERY + 1], x, 6)
    order = [rows[i] for i in np.argsort(-np.asarray(hc.PLANT_SCALES), kind="stable")]
    assert list(ei[0, :5]) == order                      # by scale, descending
    qq = float(np.dot(q[hc.PLANT_QUERY].astype(np.float64), q[hc.PLANT_QUERY].astype(np.float64)))
    assert np.allclose(es[0, :5], np.sort(np.asarray(hc.PLANT_SCALES))[::-1] * qq, rtol=2.0 ** -8)   # (rows rounded to bf16)
    assert es[0, 5] < 0.5 * es[0, 4]                     # nothing else comes near: the fifth place is a planted row's for sure
    # the other queries do not see the planted rows at the top: their answers are those of the plain Gaussian rows +- a row
    x0, _ = hc.gauss(d)
    assert np.array_equal(np.flatnonzero((x != x0).any(axis=1)), np.sort(rows))


def test_duplicate_rows_rank_by_row_number():
    d = hc.DIMS[1]
    x, q, rows = hc.duplicates(d)
    assert len(rows) == hc.DUP_COPIES and len({hc.coords(r, 16)[2:] for r in rows}) == 8   # both halves x four lane groups
    assert len({hc.coords(r, 16)[0] for r in rows}) >= 2
    es, ei = orc.search_exact(q[hc.DUP_QUERY:hc.DUP_QUERY + 1], x, 5, slack=hc.DUP_COPIES + 16)
    assert list(ei[0]) == rows[:5] and len(set(es[0])) == 1


def test_trending_rows_keep_the_insert_path_busy():
    """For an ascending query most blocks of 32 rows hold a row above the 8th best score of all rows before the block -- the
    most an insert bound can be (8 class words vouch for 8 rows), so the kernel's insert path runs in at least those blocks.
    The score climbs by 1000 / 125 = 8 per block against noise of |u| ~ 28 per row: the best of a block's 32 rows (~ +2 sigma)
    has to beat the 8th best of ALL earlier rows, which lies about one block-rise per rank behind the front."""
    d = hc.DIMS[1]
    x, q = hc.trending(d)
    s = x.astype(np.float64) @ q[0].astype(np.float64)   # query 0: along +u
    nblk = len(s) // 32
    hits = 0
    for b in range(1, nblk):
        bound = np.partition(s[:32 * b], -8)[-8]
        hits += bool(s[32 * b:32 * b + 32].max() > bound)
    print(f"{hits} of {nblk - 1} blocks insert")
    assert hits > (nblk - 1) // 2, (hits, nblk)
