"""What tests/boundary_cases.py claims about its inputs, shown on the CPU oracle alone (no GPU, no library): the planted rows
are the exact top 5 of their queries at every block count and row count, and they lie where the docstrings say -- in the last
block of a split and in blocks 8 and 9.  tests/test_gpu_headline_boundary.py runs the same inputs through the kernel."""
import os
import sys

import numpy as np
import pytest

from oracle import mips_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import boundary_cases as bc
    import headline_cases as hc
finally:
    sys.path.pop(0)

CASES = [(nb, n) for nb in bc.BLOCKS_PER_SPLIT for n in bc.row_counts(nb)]


def test_the_row_counts_give_every_split_nb_blocks_and_the_second_one_a_one_row_last_block():
    for nb, n in CASES:
        assert hc.tiles_per_split(n, bc.NSPLIT) == nb
        assert -(-n // 32) == bc.NSPLIT * nb            # no split is short of a block
        assert n % 32 in (0, 1)
    assert [bc.target_blocks(nb) for nb in (1, 8, 9, 10, 17)] == [[0], [7], [8], [9, 8], [16, 8, 9]]


@pytest.mark.parametrize("nb,n", CASES)
def test_planted_rows_are_the_top_five_of_their_queries(nb, n):
    x, q, plants = bc.late_winners(nb, n)
    assert len(plants) >= bc.NSPLIT * bc.PLANT_SLOTS - bc.PLANT_SLOTS and all(qq % bc.PLANT_EVERY == 0 for qq in plants)
    assert max(plants) < min(bc.QUERY_COUNTS)            # the same planted queries whichever query count runs
    all_rows = [r for rows in plants.values() for r in rows]
    assert len(set(all_rows)) == len(all_rows) and max(all_rows) < n
    queries = sorted(plants)
    es, ei = orc.search_exact(q[queries], x, 6)
    by_scale = np.argsort(-np.asarray(hc.PLANT_SCALES), kind="stable")
    for row, query in enumerate(queries):
        assert list(ei[row, :5]) == [plants[query][i] for i in by_scale], (nb, n, query)
        assert es[row, 5] < 0.5 * es[row, 4]             # nothing else comes near the fifth place
    # where they lie: every planted row is in a target block of its split, but for the few that the ragged end moved back
    targets = set(bc.target_blocks(nb))
    moved = 0
    for j, query in enumerate(queries):
        cs = [hc.coords(r, nb) for r in plants[query]]
        assert len({(half, group) for _, _, half, group in cs}) == 5      # five different (half, lane group) places
        moved += sum((blk - split * nb) not in targets for split, blk, _, _ in cs)
        own = query // bc.PLANT_EVERY % bc.NSPLIT
        assert all(split == own or (n % 32 == 1 and own == bc.NSPLIT - 1 and split < own) for split, _, _, _ in cs)
    assert moved <= (0 if n % 32 == 0 else 5 * bc.PLANT_SLOTS), moved   # (at most: every row of the 4 queries of split 7)
    if n % 32 == 1:                                      # the one row of the ragged last block is a planted winner
        assert n - 1 in all_rows
    if nb >= 10:
        blocks = {hc.coords(r, nb)[1] % nb for r in all_rows}
        assert {8, 9, nb - 1} <= blocks


def test_no_block_is_planted_all_over():
    for nb, n in CASES:
        _, _, plants = bc.late_winners(nb, n)
        per_block = np.bincount([r // 32 for rows in plants.values() for r in rows], minlength=-(-n // 32))
        assert per_block.max() <= (20 if n % 32 == 0 else 28), (nb, n, per_block.max())   # (+ 8 places for moved rows)
