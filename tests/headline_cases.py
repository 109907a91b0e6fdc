"""Input builders of tests/test_headline_cases_host.py and tests/test_gpu_headline_scan.py: searches that the pitch-768
shared-block instance of scan_kernel_v4 answers (row pitch 768, more than one query tile, k <= 5), at the places where its
one-pass block epilogue and its 4-deep running lists can go wrong.  Not a test file; no GPU is needed to import it.  Every
builder is deterministic and returns float32 arrays already rounded to bf16, so the oracle and the index see the same values.

The kernel's mapping (csrc/scan_kernel_v4.hpp): a document block is 32 rows, a split is `tps` consecutive blocks, lane (c, g)
of a wave sees rows 4 g .. 4 g + 3 of either 16-row half of a block, and keeps ONE running list per query for them.  The
coordinates of a row are therefore
    block = row // 32, split = block // tps, half = (row % 32) // 16, group = (row % 16) // 4,
and two rows of one (split, group) compete for the same list; `half` only says which of the two accumulator sets of the block
pass carries the row."""
import os
import sys

import numpy as np

from oracle import synth

KERNEL = "mips::scan_kernel_v4<6, 24, 2, 0, false, 1>"
NQ = 257                  # two query tiles of 256: the instance that shares document blocks between tiles
DIMS = (700, 768)         # both pad to row pitch 768; 700 leaves 68 zero columns in every row and query
N_ROWS = 20011
ROW_COUNTS = (33, 97, N_ROWS)   # a ragged second block / four blocks with one row in the last / many blocks per split
FORCED_NSPLIT = 8
DOC_BLOCK = 32

# the planted sub-list: split 0 of the 8-split geometry, second half, lane group 2 -- five different blocks
PLANT_QUERY = 131
PLANT_BLOCKS = (3, 10, 17, 40, 70)
PLANT_HALF, PLANT_GROUP = 1, 2
PLANT_SCALES = (2.0, 2.25, 1.75, 2.5, 1.5)     # neither ascending nor descending in the row number

DUP_QUERY = 200
DUP_COPIES = 70
SMALL_ROWS = 4001         # trending and duplicate cases: 126 blocks, 16 per split with 8 splits


def bf16(a):
    return synth.round_to_bf16(np.ascontiguousarray(a, dtype=np.float32))


def tiles_per_split(n, nsplit=FORCED_NSPLIT):
    ntiles = -(-n // DOC_BLOCK)
    return -(-ntiles // nsplit)


def coords(row, tps):
    """-> (split, block, half, group) of a row: see the module docstring"""
    block = row // DOC_BLOCK
    return block // tps, block, (row % DOC_BLOCK) // 16, (row % 16) // 4


def gauss(d, n=N_ROWS, nq=NQ):
    """-> (x [n, d], q [nq, d]): the Gaussian rows and queries of the other scan tests, as bf16 values"""
    x = bf16(synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS))
    q = bf16(synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS))
    return x, q


def plant_rows():
    """five rows of ONE sub-list (same split with 8 splits, same half, same lane group) in five different blocks"""
    return [DOC_BLOCK * b + 16 * PLANT_HALF + 4 * PLANT_GROUP + (b % 4) for b in PLANT_BLOCKS]


def planted(d):
    """-> (x, q, rows): Gaussian data in which rows[i] = PLANT_SCALES[i] * q[PLANT_QUERY].  The five rows are the top 5 of that
    query (a Gaussian row scores about |q| ~ 27 against |q|^2 ~ 700), and all five belong to one running list of the kernel,
    which keeps 4: the list must drop a member of the true top 5, and only the certificate can bring it back."""
    x, q = gauss(d)
    x = x.copy()
    rows = plant_rows()
    for r, s in zip(rows, PLANT_SCALES):
        x[r] = bf16(np.float32(s) * q[PLANT_QUERY])      # (rounded to bf16: within 2^-9 of the scale)
    return x, q, rows


def trending(d):
    """rows whose score climbs with the row number for every third query (tests/wide_cases.py): for those queries nearly every
    block holds a row above the insert bound, so the insert path runs in every block and the lists turn over all the time"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import wide_cases
    finally:
        sys.path.pop(0)
    x, q, _ = wide_cases.trending(SMALL_ROWS, d, NQ)
    return x, q


def duplicates(d):
    """-> (x, q, rows): DUP_COPIES copies of 2 * q[DUP_QUERY], 53 rows apart from row 101 on (every lane group, both halves,
    several splits).  All score the same: the top k are the k LOWEST row numbers among them."""
    x, q = gauss(d, n=SMALL_ROWS)
    x = x.copy()
    rows = [101 + 53 * i for i in range(DUP_COPIES)]
    assert rows[-1] < SMALL_ROWS
    x[rows] = bf16(np.float32(2.0) * q[DUP_QUERY])
    return x, q, rows
