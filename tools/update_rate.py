"""Rate of MipsIndex.update_rows on the GPU box (include/mips_hip_write.h), with the protocol of tools/remove_rate.py /
ivf_rate.py: HIP events, alternating blocks, median and spread, everything in one process on one GPU.

Index `--rows` x `--dim` (synthetic Gaussian) on bf16, fp32-exact and SQ8 storage.  For n = 32, 1024, 65536 device rows with device
ids (random rows of the index, so some twice):
  update          update_rows(ids, x)                                     -- three launches over the n positions
  update+search   the same followed by one search of 8 device queries      -- what a training step with a rolling refresh issues
  search          that search alone
the three alternate, `--reps` times after one warm-up round; and once per storage
  rebuild         reset + add of the whole matrix (what the reference does every mips_rebuild_every steps), rows already on the device.
Reported: the medians with (min, max), the bytes the update writes (n x the stored bytes of a row: bf16 2 ld; fp32-exact the two
bf16 planes + the fp32 original + the bf16 image; SQ8 ld) per second of the update's median against the HBM figure of
profiles/SUMMARY.md (8 TB/s), and (update+search) - search: the claim is that at n = 32 it does not grow with the rows of the index.
    python tools/update_rate.py [--rows 1048576 --dim 768 --reps 9 --out profiles/update/update_rate.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import retrieval_augmented_mds_amd as ram

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--storages", nargs="*", default=["bf16", "f32", "sq8"])
ap.add_argument("--counts", type=int, nargs="*", default=[32, 1024, 65536])
ap.add_argument("--no-rebuild", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("update_rate.py measures on the GPU; none is visible")
HBM_BYTES_PER_S = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}


def row_bytes(storage, d):
    if storage == "bf16":
        return 2 * (1024 if d > 768 else (d + 127) // 128 * 128) if d <= 1024 else 2 * ((d + 63) // 64 * 64)
    if storage == "sq8":
        return (d + 255) // 256 * 256
    plane = (d + 63) // 64 * 64
    hp = 0 if d > 1024 else 256 if d <= 256 else (d + 127) // 128 * 128 if d <= 768 else 1024
    return 2 * plane * 2 + plane * 4 + hp * 2


n, d = a.rows, a.dim
gen = torch.Generator(device="cuda").manual_seed(7)
x = ram.synth_fill(n, d, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS, dtype="f32")
q = ram.synth_fill(8, d, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="f32")
lines = []
for storage in a.storages:
    ix = ram.MipsIndex(d, dtype=storage)
    if storage == "sq8":
        ix.train(x[:1 << 16])
    ix.reserve(n)
    ix.add(x)
    ix.search(q, 5)
    torch.cuda.synchronize()
    rebuild = None
    if not a.no_rebuild:
        t = []
        for rep in range(4):

            def again():
                ix.reset()
                ix.add(x)

            ms = timed(again)
            if rep:
                t.append(ms)
        ix.search(q, 5)
        rebuild = stats(t)
    for m in a.counts:
        ids = torch.randint(0, n, (m,), generator=gen, device="cuda", dtype=torch.int64)
        y = torch.randn((m, d), generator=gen, device="cuda", dtype=torch.float32) * 0.036   # about the norm of the synthetic rows
        blocks = {"update": lambda: ix.update_rows(ids, y),
                  "update+search": lambda: (ix.update_rows(ids, y), ix.search(q, 5)),
                  "search": lambda: ix.search(q, 5)}
        t = {k: [] for k in blocks}
        for rep in range(a.reps + 1):                              # rep 0 warms every block up (the owner array, the scratch)
            for k, fn in blocks.items():
                ms = timed(fn)
                if rep:
                    t[k].append(ms)
        got = ix.reconstruct_batch(ids[-1:])                       # the last position always wins its row
        want = y[-1:] if storage == "f32" else None
        ok = want is None or bool(torch.equal(got, want))
        line = {"what": "update_rows", "storage": storage, "rows": n, "dim": d, "n": m, "row_bytes": row_bytes(storage, d),
                "bytes_written": m * row_bytes(storage, d), "rebuild": rebuild, "last_row_checked": ok}
        for k in blocks:
            line[k] = stats(t[k])
            line[k + "_all_ms"] = t[k]
        upd = line["update"]["median_ms"] * 1e-3
        line["update_bytes_per_s"] = line["bytes_written"] / upd
        line["update_fraction_of_hbm"] = line["update_bytes_per_s"] / HBM_BYTES_PER_S
        line["update+search_minus_search_ms"] = line["update+search"]["median_ms"] - line["search"]["median_ms"]
        lines.append(line)
        print(json.dumps(line), flush=True)
    del ix
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
