"""Row-removal rate on the GPU box: MipsIndex.remove_ids against two yardsticks on the same GPU in the same process.

Index 2^20 x 768 (synthetic Gaussian), bf16 and fp32-exact storage; four removal patterns -- the first row, 1 % at random, 50 %
at random, the last row only (nothing moves) -- and three windows, 16 / 64 / 256 MiB of rows per gather launch
("remove_window_rows" = bytes / row pitch, a multiple of 128).  Per point:
  remove    remove_ids(selector) on a freshly filled index, the selector already on the device     (host clock, ends in a sync)
  copy      (a) one device-to-device copy of exactly the bytes the removal moves (every array)      (HIP events)
            floor = copy x (direct bytes + 2 x bounce bytes) / moved bytes: a row that goes through the bounce buffer crosses twice
  rebuild   (b) rows_raw -> filter on the host -> reset -> add: the only way before remove_ids       (host clock, once per pattern)
remove and copy alternate.  Which rows go direct and which through the bounce buffer is the plan of csrc/remove_plan.hpp,
restated here from the per-window counts.  Three surviving rows are read back and compared with what they held before.
    python tools/remove_rate.py [--rows 1048576 --dim 768 --reps 5 --out profiles/remove/remove_rate.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--storages", nargs="*", default=["bf16", "f32"])
ap.add_argument("--windows-mib", type=int, nargs="*", default=[16, 64, 256])
ap.add_argument("--no-rebuild", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("remove_rate.py measures on the GPU; none is visible")

n = a.rows
rng = np.random.default_rng(1)
PATTERNS = {"first_row": np.arange(n) == 0, "random_1pct": rng.random(n) < 0.01, "random_50pct": rng.random(n) < 0.5, "last_row": np.arange(n) == n - 1}


def plan_rows(mask, W):
    """(moved, direct, bounce, launches) rows of the plan of csrc/remove_plan.hpp for this mask and window."""
    kept = [int((~mask[s:s + W]).sum()) for s in range(0, len(mask), W)]
    rows = [min(W, len(mask) - s) for s in range(0, len(mask), W)]
    w = 0
    while w < len(kept) and kept[w] == rows[w]:
        w += 1
    base, direct, bounce, launches = sum(kept[:w]), 0, 0, 0
    for v in range(w, len(kept)):
        if kept[v] > 0:
            launches += 1
            if base + kept[v] <= v * W:
                direct += kept[v]
            else:
                bounce += kept[v]
        base += kept[v]
    return direct + bounce, direct, bounce, launches


def median(v):
    return sorted(v)[len(v) // 2]


lines = []
for storage in a.storages:
    ix = ram.MipsIndex(a.dim, dtype=storage)
    ix.reserve(n)
    pitch = (a.dim + 127) // 128 * 128 * 2 if storage == "bf16" else (a.dim + 63) // 64 * 64 * 4   # bytes per row of one array
    arrays = 1 if storage == "bf16" else 2                                                          # f32: [hi | lo] planes + fp32 rows
    scratch = torch.empty(2 * n * pitch * arrays, dtype=torch.uint8, device="cuda")   # source and destination of the copy

    def fill():
        ix.reset()
        ix.add_synthetic(n, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)

    for name, mask in PATTERNS.items():
        sel = ram.Selector.from_mask(mask)
        new_at = np.cumsum(~mask) - 1
        probes = [int(p) for p in np.flatnonzero(~mask)[[0, (~mask).sum() // 2, -1]]]
        rebuild_ms = None
        if not a.no_rebuild:                                       # (b), once: it does not depend on the window
            fill()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = ix.rows_raw()
            rows = rows[~mask]
            ix.reset()
            ix.add(rows)
            torch.cuda.synchronize()
            rebuild_ms = (time.perf_counter() - t0) * 1e3
            assert ix.ntotal == int((~mask).sum())
            del rows
        for mib in a.windows_mib:
            W = max(128, (mib << 20) // pitch // 128 * 128)
            ix.set_param("remove_window_rows", W)
            moved, direct, bounce, launches = plan_rows(mask, W)
            nbytes = moved * pitch * arrays
            src, dst = scratch[:nbytes], scratch[scratch.numel() // 2:scratch.numel() // 2 + nbytes]
            t_rm, t_cp, ok = [], [], True
            for rep in range(a.reps + 1):                          # rep 0 warms both sides up
                fill()
                before = [ix.rows_raw(p, 1) for p in probes]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                removed = ix.remove_ids(sel)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if nbytes:
                    dst.copy_(src)
                e1.record()
                e1.synchronize()
                ok &= removed == int(mask.sum()) and ix.ntotal == n - removed
                ok &= all(np.array_equal(ix.rows_raw(int(new_at[p]), 1), b) for p, b in zip(probes, before))
                if rep:
                    t_rm.append((t1 - t0) * 1e3)
                    t_cp.append(e0.elapsed_time(e1))
            rm_ms, cp_ms = median(t_rm), median(t_cp)
            floor_ms = cp_ms * (direct + 2 * bounce) / moved if moved else 0.0
            lines.append({"what": "remove_ids", "storage": storage, "rows": n, "dim": a.dim, "pattern": name, "removed": int(mask.sum()),
                          "window_mib": mib, "window_rows": W, "launches": launches * arrays, "moved_rows": moved, "direct_rows": direct,
                          "bounce_rows": bounce, "moved_bytes": nbytes, "remove_ms": rm_ms, "copy_ms": cp_ms, "floor_ms": floor_ms,
                          "remove_over_copy": rm_ms / cp_ms if moved else None, "remove_over_floor": rm_ms / floor_ms if moved else None,
                          "rebuild_ms": rebuild_ms, "remove_ms_all": t_rm, "copy_ms_all": t_cp, "rows_checked_equal": bool(ok)})
            print(json.dumps(lines[-1]), flush=True)
    del ix, scratch
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
