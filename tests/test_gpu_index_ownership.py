"""Nothing is lost on destroy: an index that has used every family of device storage -- rows, the fp32 originals and the
bf16 image of an fp32-exact index, labels, both scratch sets, the wide / range / selector / rows-by-id / removal scratch -- is
created and dropped 16 times; the free device memory after the 16th cycle may lie below that after the 2nd (by then torch's
own caching allocator has reached its steady state) by no more than a bound.

The bound is the drift of the same file on the commit before the index's members owned their resources, plus 8 MiB: every
storage family of a cycle is at least 1 MiB, so a single one lost per cycle costs at least 14 MiB over the 14 cycles, while
allocator granularity does not.  Measured there: 16 MiB (bf16), 14 MiB (f32), 0 (fp8_e4m3), the three run in this order in one
process -- the bf16 and f32 cycles lose about 1 MiB each for a while on that commit as on this one (the figure levels off and
depends on what the process did before; the fp8 cycles, which make no wide / range / by-id / removal call, lose nothing)."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, HALF, NQ, K = 1 << 18, 1 << 17, 65, 5
CYCLES = 16
MIB = 1 << 20
PARENT_DRIFT = {"bf16": 16777216, "f32": 14680064, "fp8_e4m3": 0}  # bytes, free after cycle 2 minus free after cycle 16, on the parent commit


def _cycle(dtype):
    """One index from creation to destruction -> every result it returned, as NumPy arrays."""
    import torch

    import retrieval_augmented_mds_amd as ram

    d = 256 if dtype == "fp8_e4m3" else 64
    out = {}
    ix = ram.MipsIndex(d, dtype=dtype)
    labels = (np.arange(ROWS) % 7).astype(np.int32)
    ix.add_synthetic(HALF, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
    ix.set_labels(labels[:HALF])
    ix.add_synthetic(HALF, HALF, ram.SEED_DOCS, ram.SYNTH_GAUSS)  # grow() copies the first half
    ix.set_labels(labels[HALF:], row0=HALF)                       # the labels grow and keep the first half
    q_dev = ram.synth_fill(NQ, d, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS).float()
    q_host = q_dev.cpu().numpy()
    out["host_D"], out["host_I"] = ix.search(q_host, K)
    out["dev_D"], out["dev_I"] = ix.search(q_dev, K)
    out["packed"] = ix.search_packed(q_dev, K)
    tail = torch.cuda.Stream()
    out["split_D"], out["split_I"] = ix.search(q_dev, K, tail_stream=tail)
    tail.synchronize()
    if dtype != "fp8_e4m3":
        mask = np.arange(ROWS) % 2 == 0
        groups = (np.arange(NQ) % 7).astype(np.int32)
        out["wide_sel_D"], out["wide_sel_I"] = ix.search_wide(q_dev, 30, selector=mask)
        out["wide_grp_D"], out["wide_grp_I"] = ix.search_wide(q_dev, 30, groups=groups)
        lims = torch.empty(NQ + 1, dtype=torch.int64, device="cuda")
        D = torch.empty(ROWS, dtype=torch.float32, device="cuda")
        I = torch.empty(ROWS, dtype=torch.int64, device="cuda")
        ix.range_search_into(q_dev, 24.0, lims, D, I)  # (3 sigma of the scores: a few hundred hits per query)
        total = int(lims[-1].item())
        assert 0 < total <= ROWS
        out["range_lims"], out["range_D"], out["range_I"] = lims, D[:total], I[:total]
        ids = (np.arange(8192, dtype=np.int64) * 31) % ROWS
        out["rows"] = ix.reconstruct_batch(ids)
        out["subset"] = ix.compute_distance_subset(q_host, out["host_I"])
        if dtype == "f32":
            out["fused_D"], out["fused_I"] = ix.search_fused(q_dev, K, normalize=True)
        out["removed"] = np.array([ix.remove_ids(np.arange(ROWS) % 3 == 0)])
        out["ntotal"] = np.array([ix.ntotal])
    out = {n: (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)) for n, a in out.items()}
    del ix, tail
    gc.collect()
    torch.cuda.synchronize()
    return out


def measure(dtype):
    """-> (drift in bytes, the results of the first cycle, those of the last)"""
    import torch

    first = last = None
    free = {}
    for c in range(1, CYCLES + 1):
        last = _cycle(dtype)
        if first is None:
            first = last
        if c in (2, CYCLES):
            free[c] = torch.cuda.mem_get_info()[0]
    return free[2] - free[CYCLES], first, last


@pytest.mark.parametrize("dtype", ["bf16", "f32", "fp8_e4m3"])
def test_nothing_is_lost_on_destroy(dtype):
    drift, first, last = measure(dtype)
    print(f"{dtype}: free after cycle 2 minus free after cycle {CYCLES} = {drift} bytes ({drift / MIB:.2f} MiB)")
    assert drift <= PARENT_DRIFT[dtype] + 8 * MIB, (dtype, drift)
    assert sorted(first) == sorted(last)
    for name in first:
        assert np.array_equal(first[name], last[name], equal_nan=name == "rows"), name
