"""The headline scan instance, mips::scan_kernel_v4<6, 24, 2, 0, false, 1> (row pitch 768, several query tiles, k <= 5), at
the edges of its one-pass block epilogue and of its 4-deep running lists.  Every case is compared bit for bit with
orc.search_exact and asserts that exactly this instance answered.  Inputs: tests/headline_cases.py (whose claims
tests/test_headline_cases_host.py shows on the oracle alone).

Row counts: 33 (the second block holds one row: the ragged mask of both halves), 97 (four blocks, the last with one row) and
20011 with the automatic split count and with 8 splits (79 blocks per split: the 3-stage ring wraps many times; a row count
of 97 cannot wrap it, since the launch never makes fewer than 8 splits and then gives every split one block)."""
import os
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import headline_cases as hc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

_GAUSS, _ORACLE = {}, {}


def _gauss(d):
    if d not in _GAUSS:
        x, q = hc.gauss(d)
        x.setflags(write=False)
        q.setflags(write=False)
        _GAUSS[d] = (x, q)
    return _GAUSS[d]


def _oracle(d, n):
    """exact top 5 of the first n Gaussian rows, computed once (the top 1 is its first column: same order)"""
    if (d, n) not in _ORACLE:
        x, q = _gauss(d)
        es, ei = orc.search_exact(q, x[:n], 5)
        es.setflags(write=False)
        ei.setflags(write=False)
        _ORACLE[(d, n)] = (es, ei)
    return _ORACLE[(d, n)]


def _search(x, q, k, nsplit, d):
    ix = ram.MipsIndex(d, dtype="bf16")
    ix.add(x)
    ix.set_param("nsplit", nsplit)
    s, i = ix.search(q, k)
    st = ix.margin_stats()
    assert ix.last_kernel == hc.KERNEL, f"dispatched to {ix.last_kernel}"
    assert st["unresolved"] == 0, st
    ix.check()
    return s, i, st


def _same(s, i, es, ei, what):
    bad = np.flatnonzero((i != ei).any(axis=1))
    assert np.array_equal(i, ei), f"{what}: indices differ in queries {bad[:8]} ({len(bad)} of {len(ei)})"
    assert np.array_equal(s, es), f"{what}: scores differ"


@pytest.mark.parametrize("k", (5, 1))
@pytest.mark.parametrize("n,nsplit", [(33, 0), (97, 0), (hc.N_ROWS, 0), (hc.N_ROWS, hc.FORCED_NSPLIT)])
@pytest.mark.parametrize("d", hc.DIMS)
def test_gaussian_rows_match_the_oracle(d, n, nsplit, k):
    x, q = _gauss(d)
    es, ei = _oracle(d, n)
    s, i, st = _search(x[:n], q, k, nsplit, d)
    print(f"d {d} n {n} nsplit {nsplit or 'auto'} k {k}: flagged {st['flagged']} of {hc.NQ}")
    _same(s, i, es[:, :k], ei[:, :k], f"d {d} n {n} nsplit {nsplit} k {k}")


@pytest.mark.parametrize("d", hc.DIMS)
def test_five_winners_in_one_sub_list_are_settled_exactly(d):
    """The top 5 of one query all belong to ONE running list (same split, half and lane group; five blocks), which keeps 4: the
    list drops a true top-5 member, its 4th score -- itself a top-5 score -- becomes the bound on what it dropped, the margin
    check has to flag the query and the exact pass has to bring the fifth row back.  k = 1 needs no such help and is exact too."""
    x, q, rows = hc.planted(d)
    es, ei = orc.search_exact(q, x, 5)
    assert sorted(ei[hc.PLANT_QUERY]) == sorted(rows)
    s, i, st = _search(x, q, 5, hc.FORCED_NSPLIT, d)
    print(f"d {d}: flagged {st['flagged']}, rescanned {st['rescanned']}")
    _same(s, i, es, ei, f"planted, d {d}")
    assert st["flagged"] >= 1, st
    s, i, st = _search(x, q, 1, hc.FORCED_NSPLIT, d)
    _same(s, i, es[:, :1], ei[:, :1], f"planted, k 1, d {d}")


@pytest.mark.parametrize("nsplit", (0, hc.FORCED_NSPLIT))
def test_trending_rows_insert_in_every_block(nsplit):
    d = hc.DIMS[1]
    x, q = hc.trending(d)
    es, ei = orc.search_exact(q, x, 5)
    s, i, st = _search(x, q, 5, nsplit, d)
    print(f"trending nsplit {nsplit or 'auto'}: flagged {st['flagged']} of {hc.NQ}")
    _same(s, i, es, ei, f"trending, nsplit {nsplit}")


@pytest.mark.parametrize("k", (5, 1))
def test_seventy_copies_of_the_winner_return_the_lowest_rows(k):
    d = hc.DIMS[0]
    x, q, rows = hc.duplicates(d)
    es, ei = orc.search_exact(q, x, k, slack=hc.DUP_COPIES + 16)      # (candidates: every copy, so that the row number decides)
    assert list(ei[hc.DUP_QUERY]) == rows[:k]
    s, i, st = _search(x, q, k, hc.FORCED_NSPLIT, d)
    print(f"duplicates k {k}: flagged {st['flagged']}")
    _same(s, i, es, ei, f"duplicates, k {k}")
