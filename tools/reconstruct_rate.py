"""Rows-by-id rates on the GPU box: MipsIndex.reconstruct_batch and compute_distance_subset against yardsticks on the same GPU in
the same process.

Index 2^20 x 768 bf16 (synthetic Gaussian); the ids are what real searches return: search (Q = 4096, k = 5) and search_wide
(k = 100).  Per case one JSON line:
  reconstruct   reconstruct_batch(I) -> float32 [Q, k, d], CUDA ids, device time between HIP events
  torch         (a) torch.index_select + .float() on a device copy of the same rows                    (HIP events)
  old_route     (b) rows_raw of the WHOLE index to the host, then NumPy indexing: the only way before   (host clock, once)
  subset        compute_distance_subset(q, I) against torch.einsum in float64 on rows gathered by torch (HIP events)
reconstruct and torch alternate, so both see the same neighbours on the box; each is reported as median, minimum, maximum and
spread = (max - min) / median over the repeats, and as bytes moved per second (2 bytes read and 4 written per element).
    python tools/reconstruct_rate.py [--rows 1048576 --dim 768 --queries 4096 --reps 20 --out profiles/reconstruct/reconstruct_rate.jsonl]"""
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
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ks", type=int, nargs="*", default=[5, 100])
ap.add_argument("--no-old-route", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("reconstruct_rate.py measures on the GPU; none is visible")

n, d, nq = a.rows, a.dim, a.queries
SEED_DOCS, SEED_QUERIES = 0xD0C5, 0x0E21
KIND_GAUSS = 1


def stats(ms, nbytes=None):
    s = sorted(ms)
    med = s[len(s) // 2]
    out = {"median_ms": med, "min_ms": s[0], "max_ms": s[-1], "spread": (s[-1] - s[0]) / med}
    if nbytes is not None:
        out["gbytes_per_s"] = nbytes / (med * 1e-3) / 1e9
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


ix = ram.MipsIndex(d, dtype="bf16")
ix.reserve(n)
ix.add_synthetic(n, 0, SEED_DOCS, KIND_GAUSS)
copy = ram.synth_fill(n, d, 0, SEED_DOCS, KIND_GAUSS, "bf16")          # the yardstick's device copy of the same rows
q = ram.synth_fill(nq, d, 0, SEED_QUERIES, KIND_GAUSS, "f32")
lines = []
old_route = None
for k in a.ks:
    D, I = ix.search(q, k) if k <= ram.MAX_K else ix.search_wide(q, k)
    flat = I.reshape(-1)
    nbytes = flat.numel() * d * (2 + 4)
    ours = lambda: ix.reconstruct_batch(I)
    theirs = lambda: torch.index_select(copy, 0, flat).float().view(nq, k, d)
    same = bool(torch.equal(ours(), theirs()))
    t_ours, t_torch = [], []
    for rep in range(a.reps + 3):                                   # three warm-up rounds
        t0, _ = timed(ours)
        t1, _ = timed(theirs)
        if rep >= 3:
            t_ours.append(t0)
            t_torch.append(t1)
    so, st = stats(t_ours, nbytes), stats(t_torch, nbytes)
    line = {"what": "reconstruct_batch", "rows": n, "dim": d, "queries": nq, "k": k, "ids": int(flat.numel()), "bytes_moved": nbytes,
            "reconstruct": so, "torch_index_select_float": st, "ratio_median": so["median_ms"] / st["median_ms"],
            "within_spread": so["median_ms"] <= st["median_ms"] * (1.0 + max(so["spread"], st["spread"])), "equal_to_torch": same,
            "reconstruct_ms_all": t_ours, "torch_ms_all": t_torch}
    if not a.no_old_route:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = ix.rows_raw()                                       # the whole index crosses to the host
        t_read = time.perf_counter() - t0
        ids = I.cpu().numpy()
        t0 = time.perf_counter()
        got = (host[ids].astype(np.uint32) << np.uint32(16)).view(np.float32)
        t_index = time.perf_counter() - t0
        line["old_route"] = {"rows_raw_ms": t_read * 1e3, "numpy_index_ms": t_index * 1e3, "total_ms": (t_read + t_index) * 1e3,
                             "equal": bool(np.array_equal(got.view(np.uint32), ours().cpu().numpy().view(np.uint32)))}
        del host, got
    lines.append(line)
    print(json.dumps(line), flush=True)

    # subset scores against float64 einsum on rows gathered by torch
    sub = lambda: ix.compute_distance_subset(q, I)
    ein = lambda: torch.einsum("qd,qkd->qk", q.double(), torch.index_select(copy, 0, flat).view(nq, k, d).double()).float()
    close = float((sub() - ein()).abs().max())
    t_sub, t_ein = [], []
    for rep in range(a.reps + 3):
        t0, _ = timed(sub)
        t1, _ = timed(ein)
        if rep >= 3:
            t_sub.append(t0)
            t_ein.append(t1)
    line = {"what": "compute_distance_subset", "rows": n, "dim": d, "queries": nq, "k": k, "pairs": int(flat.numel()),
            "subset": stats(t_sub), "torch_einsum_f64": stats(t_ein), "ratio_median": stats(t_sub)["median_ms"] / stats(t_ein)["median_ms"],
            "equal_to_search": bool(torch.equal(sub(), D)), "max_abs_diff_to_einsum": close, "subset_ms_all": t_sub, "einsum_ms_all": t_ein}
    lines.append(line)
    print(json.dumps(line), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
