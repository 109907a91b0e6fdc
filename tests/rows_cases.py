"""Inputs and NumPy models of the rows-by-id tests (tests/test_rows_host.py, tests/test_gpu_rows.py and
tests/test_gpu_rows_sharded.py).  Not a test file; NumPy and the CPU oracle only, no GPU is needed to import it.

Reconstruction is data movement: the float32 a row comes back as is the exact value of what the storage holds, bit for bit, and
"no row" is a NaN (or zero) row.  Subset scoring is the canonical score of DESIGN.md section 2 for the pairs the caller names.
The id patterns are written against what a gather kernel gets wrong: ids cut to 32 bits, the wrong row pitch, the storage's
padding columns, arithmetic on the way (which loses -0.0), and the order of the fp64 sum."""
import os
import sys

import numpy as np

from oracle import mips_oracle as orc
from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import lifecycle_cases as lc
finally:
    sys.path.pop(0)

INT64_MIN = -(1 << 63)
NAN_BITS, NAN_BF16, NAN_E4M3 = 0x7FC00000, 0x7FC0, 0x7F
SENTINEL = 0xDEADBEEF                      # what an output buffer holds where nothing may be written

STORAGES = lc.STORAGES                     # "bf16", "f32", "fp8_e4m3", "fp8_e4m3_docs"
DIMS = (1, 7, 8, 100, 768, 800, 1024, 1536)
NTOTALS = (1, 127, 129, 5000)
SIZES = (0, 1, 63, 64, 65, 4097)           # n of a call: below, at and above a wave, more than one workgroup


def dims_of(storage):
    return tuple(d for d in DIMS if d <= 1024 or not storage.startswith("fp8"))


def pitch_of(storage, d):
    """Row pitch in elements of the array the rows are read from (csrc/mips_hip.hip, mips_index_create; "f32": the plane of the
    fp32 originals)."""
    up = lambda v, m: (v + m - 1) // m * m
    if storage.startswith("fp8"):
        return up(d, 256)
    if storage == "f32" or d > 1024:
        return up(d, 64)
    return 1024 if d > 768 else up(d, 128)


def rows_data(storage, d, n, seed=0):
    """float32 [n, d] to add, and what the storage makes of it (the values a reconstruction returns)."""
    rng = np.random.default_rng([seed, d, n])
    x = (rng.standard_normal((n, d)) * rng.uniform(0.25, 4.0, (n, 1))).astype(np.float32)
    return x, lc.stored_rows(x, storage)


def planted_f32(n=129, d=100):
    """Rows for an "f32" index with what only a bit copy keeps: -0.0, denormals, NaNs with a payload."""
    x, _ = rows_data("f32", d, n, seed=9)
    b = x.view(np.uint32)
    b[3, 0], b[3, d - 1] = 0x80000000, 0x80000000              # -0.0
    b[5, 1], b[5, 2] = 0x00000001, 0x807FFFFF                  # the smallest and the largest denormal
    b[7, d // 2], b[7, 0] = 0x7FC12345, 0xFFC54321             # quiet NaNs with payloads
    b[n - 1, :] = 0x80000000
    return x


def raw_bits(stored, storage):
    """The storage's own bits of stored values: np.uint16 (bf16), np.uint8 (e4m3) or float32."""
    if storage == "f32":
        return stored
    return synth.bf16_bits(stored) if storage == "bf16" else synth.e4m3_bits(stored)


def id_patterns(ntotal, seed=0):
    """name -> int64 ids [n] in LOCAL numbering.  Names that start with "bad_" hold an id >= ntotal, which a call with host ids
    rejects; a call with device ids answers it with "no row"."""
    rng = np.random.default_rng([seed, ntotal])
    r = np.arange(ntotal, dtype=np.int64)
    out = {
        "identity": r,
        "reversed": r[::-1].copy(),
        "one_row": np.full(65, ntotal // 2, np.int64),
        "duplicates": rng.integers(0, max(ntotal // 4, 1), 4097),
        "ends": np.array([0, ntotal - 1, ntotal - 1, 0], np.int64),
        "int64_min": np.array([INT64_MIN, 0, INT64_MIN + 1], np.int64),
        "bad_ntotal": np.array([0, ntotal, ntotal - 1], np.int64),
        "bad_two32_plus_3": np.array([min(3, ntotal - 1), (1 << 32) + 3, (1 << 32), (1 << 40) + 3], np.int64),
    }
    scattered = rng.integers(0, ntotal, 4097)
    scattered[rng.random(4097) < 0.3] = -1
    out["minus_one"] = scattered
    for n in SIZES:
        out[f"n{n}"] = rng.integers(0, ntotal, n)
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in out.items()}


def _local(ids, idx_offset, ntotal):
    """(local rows with -1 for "no row", valid mask); the comparison is made on Python integers: nothing wraps."""
    flat = [int(v) - int(idx_offset) for v in np.asarray(ids).reshape(-1)]
    valid = np.array([0 <= v < ntotal for v in flat], dtype=bool).reshape(np.shape(ids))
    local = np.array([v if 0 <= v < ntotal else -1 for v in flat], dtype=np.int64).reshape(np.shape(ids))
    return local, valid


def model_reconstruct(stored, ids, idx_offset=0, zero_missing=False):
    """float32 [..., d]: stored[ids - idx_offset] bit for bit, a NaN (zero_missing: zero) row where the id names no row."""
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    local, valid = _local(ids, idx_offset, stored.shape[0])
    out = np.full(local.shape + (stored.shape[1],), 0 if zero_missing else NAN_BITS, dtype=np.uint32)
    out[valid] = stored.view(np.uint32)[local[valid]]
    return out.view(np.float32)


def model_reconstruct_raw(stored, storage, ids, idx_offset=0, zero_missing=False):
    if storage == "f32":
        return model_reconstruct(stored, ids, idx_offset, zero_missing)
    bits = raw_bits(stored, storage)
    local, valid = _local(ids, idx_offset, stored.shape[0])
    out = np.full(local.shape + (stored.shape[1],), 0 if zero_missing else (NAN_BF16 if storage == "bf16" else NAN_E4M3), dtype=bits.dtype)
    out[valid] = bits[local[valid]]
    return out


def model_scores(q, stored, ids, metric=0, phi=0.0, idx_offset=0):
    """float32 [nq, k]: the canonical score of (q[j], stored[ids[j, t] - idx_offset]); q as the index stages it
    (lc.stored_queries).  Inner product: float32 of the sequential fp64 sum; L2: float32(|q|^2 + phi - 2 dot); "no row": -inf /
    +inf."""
    local, _ = _local(ids, idx_offset, stored.shape[0])
    x = stored if stored.shape[0] else np.zeros((1, stored.shape[1]), np.float32)
    canon = orc.canonical_pairs(q, x, local)               # -inf where local < 0
    with np.errstate(over="ignore"):                       # (a distance past float32 is +inf, as on the device)
        if metric == 1:
            return (orc.sumsq_canonical(q)[:, None] + float(phi) - 2.0 * canon).astype(np.float32)
        return canon.astype(np.float32)


# ------------------------------------------------------------------ NumPy forms of the kernels, right and wrong
def storage_image(stored, ld):
    """The array a gather reads: uint32 bits of the decoded values, [n][ld], zero padding columns."""
    img = np.zeros((stored.shape[0], ld), np.uint32)
    img[:, :stored.shape[1]] = np.ascontiguousarray(stored, dtype=np.float32).view(np.uint32)
    return img


def kernel_reconstruct(img, d, ids, idx_offset, out, zero_missing=False, mutant=None):
    """Writes uint32 out[i, :d] (out [n][out_ld >= d], prefilled by the caller) the way the gather kernel does -- or the way a
    wrong one would: "ids_int32", "pitch_d", "leak_padding", "float_add"."""
    ntotal, ld = img.shape
    ids = np.asarray(ids, dtype=np.int64)
    if mutant == "ids_int32":
        ids = ids.astype(np.int32).astype(np.int64)
        idx_offset = int(np.int64(idx_offset).astype(np.int32))
    local, valid = _local(ids, idx_offset, ntotal)
    flat = img.reshape(-1)
    for i in range(len(ids)):
        if not valid[i]:
            out[i, :d] = 0 if zero_missing else NAN_BITS
        elif mutant == "pitch_d":
            out[i, :d] = flat[local[i] * d:local[i] * d + d]
        elif mutant == "leak_padding":
            w = min(ld, out.shape[1])
            out[i, :w] = img[local[i], :w]
        elif mutant == "float_add":
            with np.errstate(all="ignore"):
                out[i, :d] = (np.zeros(d, np.float32) + img[local[i], :d].view(np.float32)).view(np.uint32)
        else:
            out[i, :d] = img[local[i], :d]
    return out


def _tree_sum(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else 0.0


def kernel_scores(q, stored, ids, metric=0, phi=0.0, mutant=None):
    """model_scores, or what a wrong kernel would give: "pairwise" (a tree instead of the sequential fp64 sum), "l2_as_ip"."""
    if mutant is None:
        return model_scores(q, stored, ids, metric, phi)
    if mutant == "l2_as_ip":
        return model_scores(q, stored, ids, 0, phi)
    assert mutant == "pairwise"
    local, valid = _local(ids, 0, stored.shape[0])
    q64, x64 = q.astype(np.float64), stored.astype(np.float64)
    out = np.full(local.shape, np.inf if metric == 1 else -np.inf, np.float32)
    with np.errstate(all="ignore"):
        for j in range(local.shape[0]):
            qq = _tree_sum(q64[j] * q64[j])
            for t in range(local.shape[1]):
                if valid[j, t]:
                    dot = _tree_sum(q64[j] * x64[local[j, t]])
                    out[j, t] = np.float32(qq + phi - 2.0 * dot) if metric == 1 else np.float32(dot)
    return out


def spread_data(n=64, d=24, nq=6, seed=4):
    """Rows and queries (float32 powers of two) whose dot products depend on the ORDER of the fp64 sum, visibly in float32: the
    products of every four columns are +B, s, -B, s' with B = 2^60 .. 2^79 and |s|, |s'| <= 8.  Summed sequentially B swallows s
    and s' survives; summed in pairs both small terms are swallowed.  For an "f32" index (nothing is rounded)."""
    assert d % 4 == 0
    rng = np.random.default_rng(seed)
    small = rng.choice([-1.0, 1.0], (n, d)) * np.exp2(rng.integers(-3, 4, (n, d)))
    prod = small.copy()
    big = np.exp2(60 + np.arange(n) % 20)[:, None]
    prod[:, 0::4] = big
    prod[:, 2::4] = -big
    qpat = rng.choice([-1.0, 1.0], d) * np.exp2(rng.integers(-2, 3, d))   # the same magnitudes in every query: products stay powers of two
    q = (qpat[None, :] * rng.choice([1.0, 2.0, 4.0], (nq, 1))).astype(np.float32)
    x = (prod / qpat[None, :]).astype(np.float32)
    return x, q


def score_ids(ntotal, nq, k, seed=0):
    """int64 [nq, k]: rows in no order, duplicates, -1 slots."""
    rng = np.random.default_rng([seed, ntotal, nq, k])
    ids = rng.integers(0, ntotal, (nq, k))
    ids[rng.random((nq, k)) < 0.1] = -1
    return np.ascontiguousarray(ids, dtype=np.int64)


def l2_column(rows, phi):
    """The augmentation column faiss_shim re-attaches: float32(sqrt(max(phi - sum x^2, 0))), the sum sequential in fp64."""
    sq = orc.sumsq_canonical(np.ascontiguousarray(rows, dtype=np.float32))
    return np.sqrt(np.maximum(float(phi) - sq, 0.0)).astype(np.float32)
