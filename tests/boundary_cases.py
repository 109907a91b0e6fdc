"""Input builders of tests/test_boundary_cases_host.py and tests/test_gpu_headline_boundary.py: searches of the pitch-768
shared-block instance of scan_kernel_v4 (tests/headline_cases.py: KERNEL) at the block counts where its ring prologue, its
bound-refresh schedule and the counted wait of its block barrier change what they do.  Not a test file; no GPU is needed to
import it.  Every builder is deterministic and returns float32 arrays already rounded to bf16.

The kernel (csrc/scan_kernel_v4.hpp) scans a split of `nb` consecutive 32-row blocks through a 3-stage ring: the prologue
issues two stages, every block issues the stage two blocks ahead.  Blocks 0 .. 7 of a split and every 8th block after them
fetch the shared insert bounds; the other blocks fetch nothing, and the wait before a wave arrives at the block barrier
counts the operations the wave issued in that block -- one more in a block that fetched.  With 8 splits and 256 nb rows
every split has nb blocks:
    nb = 1, 2       fewer blocks than ring stages            nb = 3        one block beyond the prologue
    nb = 7, 8       only blocks that fetch                    nb = 9, 10    the first block that fetches nothing (8), and one after
    nb = 16         seven such blocks in a row (9 .. 15)      nb = 17       the fetch at block 16 behind them
Rows = 256 nb - 31 leaves ONE row in the last block of the index (the kernel's ragged path)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import headline_cases as hc
finally:
    sys.path.pop(0)

D = 768
NSPLIT = hc.FORCED_NSPLIT                      # 8
BLOCKS_PER_SPLIT = (1, 2, 3, 7, 8, 9, 10, 16, 17)
QUERY_COUNTS = (257, 512)                      # 257: the second query tile has 7 idle waves and one wave with a single live query
KS = (5, 1)
MAX_ROWS = 256 * max(BLOCKS_PER_SPLIT)
PLANT_EVERY = 3                                # late winners: every third query ...
PLANT_SLOTS = 4                                # ... 4 queries per split, 32 in all (what one target block per split holds: below)


def row_counts(nb):
    """the two row counts of a block count: full blocks, and one row in the last block of the index"""
    return (256 * nb, 256 * nb - 31)


def target_blocks(nb):
    """blocks of a split (numbered inside the split) that receive late winners: the LAST one, and blocks 8 and 9 -- the first
    block that fetches no bounds and its successor -- where the split has them.  The last block comes first: the first row of
    the first planted query of a split is row 0 of it, the one row the last block of the index has when it is ragged"""
    return [nb - 1] + [b for b in (8, 9) if b < nb - 1]


def plant_rows(nb, n):
    """-> {query: [five rows]} for queries 0, 3, 6, .. (PLANT_SLOTS per split).  Planted query j belongs to split j % 8; its five
    rows go round the target blocks of that split, each into another (half, lane group) of its block: in-block position number
    x -> half (x // 4) % 2, group x % 4, row x // 8 of the group, and the five rows of a query take five consecutive x.  A row
    past the end of the index (only in the one-row last block) moves back block by block, to row 3 of the same half and lane
    group, until the place is free."""
    tps = hc.tiles_per_split(n)
    assert tps == nb, (tps, nb)
    targets = target_blocks(nb)
    used, out = set(), {}
    for j in range(NSPLIT * PLANT_SLOTS):
        split, slot = j % NSPLIT, j // NSPLIT
        rows = []
        for m, _ in enumerate(hc.PLANT_SCALES):
            x = 5 * slot + m
            blk = split * nb + targets[(m + slot) % len(targets)]
            row = 32 * blk + 16 * ((x // 4) % 2) + 4 * (x % 4) + x // 8
            while row >= 0 and (row >= n or row in used):
                row = (row - 32) | 3                 # (row 3 of a lane group is nobody's first choice)
            if row < 0:
                break
            used.add(row)
            rows.append(row)
        if len(rows) == len(hc.PLANT_SCALES):
            out[PLANT_EVERY * j] = rows
    return out


_GAUSS = []


def gauss():
    """the Gaussian rows and queries of tests/headline_cases.py, MAX_ROWS x 768 and 512 x 768, made once"""
    if not _GAUSS:
        x, q = hc.gauss(D, n=MAX_ROWS, nq=max(QUERY_COUNTS))
        x.setflags(write=False)
        q.setflags(write=False)
        _GAUSS.append((x, q))
    return _GAUSS[0]


def late_winners(nb, n):
    """-> (x [n, 768], q [512, 768], plants): the first n Gaussian rows, in which plants[query][i] = PLANT_SCALES[i] * q[query]
    (built as headline_cases.planted builds its rows).  A planted row scores about scale * |q|^2 ~ scale * 768 for its query
    against ~ 28 for a Gaussian row, so the five are the top 5 of their query, and they arrive late: in the last block of
    their split, and in blocks 8 and 9, after the bounds have risen.  A bound read too high there would refuse them.  The
    same data serves 257 queries (its first 257) and 512: every planted query is below 96."""
    x0, q = gauss()
    x = x0[:n].copy()
    plants = plant_rows(nb, n)
    for query, rows in plants.items():
        for r, s in zip(rows, hc.PLANT_SCALES):
            x[r] = hc.bf16(np.float32(s) * q[query])
    return x, q, plants
