"""Inputs and the NumPy model of the row-removal tests (tests/test_remove_host.py, tests/test_gpu_remove.py and
tests/test_gpu_remove_sharded.py).  Not a test file; NumPy only, no GPU is needed to import it.

A removal is data movement: what the index holds afterwards -- rows, labels, the labelled prefix -- is `expected()` of what it
held before, bit for bit.  The patterns are written against the window W of the native plan (csrc/remove_plan.hpp): a window
that keeps everything, one that keeps nothing, runs that end on a window border, a long run in the middle (the direct path
behind the bounce path), and random removals at three densities."""
import numpy as np

WINDOWS = (128, 384, 0)              # "remove_window_rows": two test windows and the default (0 = automatic)
W_MODEL = 384                        # the window the sizes and patterns are written against, whatever window the index uses


def sizes(W=W_MODEL):
    return (1, 127, 128, 129, W - 1, W, W + 1, 5 * W + 37)


def expected(x, labels, nlabelled, mask):
    """The index after remove_ids(mask): (rows, labels of the new labelled prefix, new nlabelled).  x [n, d] any dtype; labels
    [>= nlabelled] ints (rows [0, nlabelled) carry one); mask bool [n], True = the row leaves."""
    mask = np.asarray(mask, dtype=np.bool_)
    assert mask.shape == (x.shape[0],) and 0 <= nlabelled <= x.shape[0]
    keep = ~mask
    return x[keep], np.asarray(labels)[:nlabelled][keep[:nlabelled]], int(keep[:nlabelled].sum())


def patterns(n, W=W_MODEL, seed=0):
    """name -> bool [n] removal mask.  Patterns that need more rows than n has are left out."""
    rng = np.random.default_rng([seed, n, W])
    r = np.arange(n)
    out = {
        "none": np.zeros(n, bool),
        "all": np.ones(n, bool),
        "first": r == 0,
        "last": r == n - 1,
        "first_of_every_window": r % W == 0,
        "last_of_every_window": (r % W == W - 1) | (r == n - 1),
        "every_other": r % 2 == 1,
        "random_1pct": rng.random(n) < 0.01,
        "random_50pct": rng.random(n) < 0.5,
        "random_99pct": rng.random(n) < 0.99,
    }
    if n >= 2 * W:
        out["one_window"] = (r >= W) & (r < 2 * W)
    if n >= 4 * W + 37:
        out["run_3w5"] = (r >= W + 11) & (r < W + 11 + 3 * W + 5)   # bounce (the window it starts in), nothing, nothing, then direct
    return out


def window_counts(mask, W):
    """Surviving rows per window of W rows: the input of the native plan."""
    n = len(mask)
    return [int((~mask[s:s + W]).sum()) for s in range(0, n, W)]


def bitmap(mask, bit0=0, pad_bits=0, fill=True):
    """uint8 bitmap in which bit bit0 + i is mask[i]; the bits before bit0 and `pad_bits` behind the mask are SET when fill is
    True (they speak about rows the index does not hold: a removal must not look at them)."""
    full = np.concatenate([np.full(bit0, fill, bool), np.asarray(mask, bool), np.full(pad_bits, fill, bool)])
    return np.packbits(full, bitorder="little")


def rows_for(n, d, storage, seed=1):
    """Distinct, exactly representable rows: column c holds digit c % 3 of the row number (base m) shifted by c, so a row that
    lands in the wrong place or a column that moved is visible.  float32 [n, d], d >= 3, n <= m^3; every storage type keeps the
    values exactly (m = 16: integers of |v| <= 8 for e4m3; m = 256: |v| <= 128 for bf16 and f32)."""
    m = 16 if storage.startswith("fp8") else 256
    assert d >= 3 and n <= m ** 3
    r = np.arange(n, dtype=np.int64)[:, None]
    c = np.arange(d, dtype=np.int64)[None, :]
    return ((r // m ** (c % 3) + c + seed) % m - m // 2).astype(np.float32)
