"""Range-search rate on the GPU box: MipsIndex.range_search against a torch yardstick on the same GPU in the same run.

Index 2^20 x 768 bf16 (synthetic Gaussian), device tensors, nq in {64, 4096}; per nq three sets of per-query radii giving about
10, 100 and 1000 hits per query (each query's 11th / 101st / 1001st search_wide score: the rows strictly above it).  Per point:
  into      range_search_into(q, r, lims, D, I) with tensors of the exact size: only enqueues        (HIP events, alternating)
  range     range_search(q, r): the same plus the capacity guess, the read of lims[-1] and the copy    (host clock, ends in a sync)
  torch     (q @ x[c0:c1].T > r[:, None]).nonzero() over row blocks, bf16 GEMM: the yardstick         (HIP events, alternating)
The yardstick's scores are bf16-rounded GEMM outputs, not canonical ones: its hit count is printed next to the exact one, it
is a measure of time only.  Then the self-join: KnowledgeBase.near_duplicates over a 2^17-row index with one row planted 70
times (host clock; it includes the host round trip of every batch).  No target is fixed for any of this.
    python tools/range_rate.py [--rows 1048576 --dim 768 --reps 5 --out profiles/range/range_rate.jsonl]"""
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
ap.add_argument("--queries", type=int, nargs="*", default=[64, 4096])
ap.add_argument("--hits", type=int, nargs="*", default=[10, 100, 1000])
ap.add_argument("--block", type=int, default=1 << 17, help="rows of the index per torch GEMM")
ap.add_argument("--join-rows", type=int, default=1 << 17, help="rows of the self-join index (0 = skip)")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("range_rate.py measures on the GPU; none is visible")

ix = ram.MipsIndex(a.dim)
ix.add_synthetic(a.rows, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
x = torch.from_numpy(ix.rows_bf16().view("int16")).cuda().view(torch.bfloat16)  # the stored rows, as torch sees them


def torch_range(q, r):
    rt = r[:, None].to(torch.bfloat16)
    parts = []
    for c0 in range(0, a.rows, a.block):
        nz = (q @ x[c0:c0 + a.block].T > rt).nonzero()
        nz[:, 1] += c0
        parts.append(nz)
    return torch.cat(parts, 0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(v):
    return sorted(v)[len(v) // 2]


lines = []
for nq in a.queries:
    q = ram.synth_fill(nq, a.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="bf16")
    top_s, _ = ix.search_wide(q, min(1024, max(a.hits) + 1))
    for h in a.hits:
        r_dev = top_s[:, min(h, top_s.shape[1] - 1)].contiguous()
        r = r_dev.cpu().numpy()
        lims, D, I = ix.range_search(q, r)                      # warm-up of both sides; the exact size
        total = int(lims[-1])
        nz = torch_range(q, r_dev)
        torch.cuda.synchronize()
        lims2 = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        D2 = torch.empty(total, dtype=torch.float32, device="cuda")
        I2 = torch.empty(total, dtype=torch.int64, device="cuda")
        ti, tt, tr = [], [], []
        for _ in range(a.reps):                                  # alternating, so that drift hits all three
            ti.append(timed(lambda: ix.range_search_into(q, r, lims2, D2, I2)))
            tt.append(timed(lambda: torch_range(q, r_dev)))
            t0 = time.perf_counter()
            ix.range_search(q, r)
            torch.cuda.synchronize()
            tr.append((time.perf_counter() - t0) * 1e3)
        same = bool(torch.equal(lims2, lims) and torch.equal(I2, I) and torch.equal(D2.view(torch.int32), D.view(torch.int32)))
        lines.append({"what": "range vs torch", "nq": nq, "hits_per_query": total / nq, "into_ms": median(ti), "range_search_ms": median(tr),
                      "torch_ms": median(tt), "into_over_torch": median(ti) / median(tt), "into_ms_all": ti, "range_search_ms_all": tr,
                      "torch_ms_all": tt, "hits_exact": total, "hits_torch_bf16_scores": int(nz.shape[0]), "repeat_equal": same,
                      "kernel": ix.last_kernel})
        print(json.dumps(lines[-1]), flush=True)
del x

if a.join_rows > 0:
    jx = ram.MipsIndex(a.dim)
    jx.add_synthetic(a.join_rows, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
    jx.add(np.repeat(jx.rows_raw(0, 1), 69, axis=0))             # row 0 now exists 70 times
    kb = ram.KnowledgeBase({}, index=jx, index_name="kb")
    thr = 0.9 * a.dim                                            # unit-variance rows: |x|^2 ~ d, distinct rows score ~ N(0, d)
    i, j, s = kb.near_duplicates("kb", thr)                      # warm-up
    tj = []
    for _ in range(max(1, a.reps // 2)):
        t0 = time.perf_counter()
        i, j, s = kb.near_duplicates("kb", thr)
        torch.cuda.synchronize()
        tj.append((time.perf_counter() - t0) * 1e3)
    lines.append({"what": "near_duplicates self-join", "rows": jx.ntotal, "dim": a.dim, "batch_rows": 4096, "threshold": thr, "pairs": int(len(i)),
                  "expected_pairs": 70 * 69 // 2, "ms": median(tj), "ms_all": tj})
    print(json.dumps(lines[-1]), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
