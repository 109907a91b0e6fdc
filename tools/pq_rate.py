"""What a search costs on the product-quantised index next to the "sq8" and "bf16" indexes over the SAME rows, what it finds, and
what building it costs, on the GPU box.  The protocol of tools/sq8_rate.py: one process; device-resident queries; every (index, Q)
variant is timed with HIP events around blocks of back-to-back searches (stream-ordered, nothing synchronises inside a block) after
a warm-up of every shape; the variants ALTERNATE block by block; the figure per variant is the median of its blocks with their
minimum and maximum.
    python tools/pq_rate.py rate   [--rows 1048576 16777216] [--dim 768] [--m 96] [--queries 1 8 16 64] [--k 5] [--rounds 9] [--calls 10]
    python tools/pq_rate.py recall [--rows 1048576] [--dim 768] [--m 96] [--queries 1024]
Rows: the Gaussian generator of the synthetic workloads, produced on the device in chunks; the PQ and SQ8 indexes are trained on the
first chunk (2^18 rows).  `rate` prints, per (rows, Q): ms per call and bytes per row of the three indexes; for the PQ scan the table
reads per second against the ds_read_b32 rate of the compute units (32 lanes per clock per CU: 256 CUs x 2.4 GHz x 32), the code
bytes per second -- as requested (nq x ntotal x M: every query's workgroups read the codes) and as HBM delivers them at least
(ntotal x M per call) against its 8 TB/s -- and which of the two fractions is the larger; and once per `rows` the training and add
rates in rows per second.  `recall` prints recall@5 and recall@29 against the fp32-exact index on the data sets of tools/recall.py
(Gaussian, clustered, clustered and normalised).  One JSON line each."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

HBM_BYTES_PER_S = 8.0e12
LDS_READS_PER_S = 256 * 2.4e9 * 32   # ds_read_b32, conflict-free: 128 B per clock per compute unit


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def rate(a):
    chunk = 1 << 18
    for rows in a.rows:
        idx = {"pq": ram.PqIndex(a.dim, a.m), "sq8": ram.MipsIndex(a.dim, dtype="sq8"), "bf16": ram.MipsIndex(a.dim, dtype="bf16")}
        idx["sq8"].reserve(rows)
        idx["bf16"].reserve(rows)
        build = {"rows": rows, "dim": a.dim, "M": a.m, "pq_add_s": 0.0}
        for r0 in range(0, rows, chunk):
            x = ram.synth_fill(min(chunk, rows - r0), a.dim, r0, ram.SEED_DOCS, ram.SYNTH_GAUSS, dtype="f32")
            if r0 == 0:
                idx["sq8"].train(x)
                build["train_rows_given"], build["pq_niter"] = int(x.shape[0]), idx["pq"].niter
                build["pq_train_s"] = wall(lambda: idx["pq"].train(x))
            build["pq_add_s"] += wall(lambda: idx["pq"].add(x))
            idx["sq8"].add(x)
            idx["bf16"].add(x)
            del x
        build["pq_train_rows_per_s"] = min(build["train_rows_given"], 65536) / build["pq_train_s"]
        build["pq_add_rows_per_s"] = rows / build["pq_add_s"]
        print(json.dumps(build), flush=True)
        bytes_per_row = {"pq": idx["pq"].bytes_per_row, "sq8": -(-a.dim // 256) * 256, "bf16": 2 * -(-a.dim // 64) * 64}
        for nq in a.queries:
            q = ram.synth_fill(nq, a.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="f32")
            variants = {name: (lambda ix=ix: ix.search(q, a.k)) for name, ix in idx.items()}
            for fn in variants.values():  # warm-up: code objects, scratch, first-use allocations
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
            t = {name: [] for name in variants}
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    t[name].append(block_ms(fn, a.calls))
            med = {name: float(np.median(v)) for name, v in t.items()}
            rec = {"rows": rows, "dim": a.dim, "M": a.m, "queries": nq, "k": a.k, "rounds": a.rounds, "calls_per_block": a.calls,
                   "bytes_per_row": bytes_per_row,
                   "ms_per_call": {name: {"median": med[name], "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}}
            sec = med["pq"] * 1e-3
            rec["pq_table_reads_per_s"] = nq * rows * a.m / sec
            rec["pq_lds_fraction"] = rec["pq_table_reads_per_s"] / LDS_READS_PER_S
            # code bytes as the workgroups REQUEST them (every query's workgroups read the codes; L2 and the memory-side cache serve
            # most of the repeats) and as HBM must deliver them at least (once per call)
            rec["pq_code_bytes_requested_per_s"] = nq * rows * a.m / sec
            rec["pq_code_bytes_once_per_s"] = rows * a.m / sec
            rec["pq_hbm_fraction"] = rec["pq_code_bytes_once_per_s"] / HBM_BYTES_PER_S
            rec["pq_binds"] = "table reads (LDS)" if rec["pq_lds_fraction"] >= rec["pq_hbm_fraction"] else "code bytes (memory)"
            rec["hbm_fraction"] = {name: rows * bytes_per_row[name] / (med[name] * 1e-3) / HBM_BYTES_PER_S for name in ("sq8", "bf16")}
            rec["pq_over_sq8"], rec["pq_over_bf16"] = med["pq"] / med["sq8"], med["pq"] / med["bf16"]
            print(json.dumps(rec), flush=True)
        del idx
        torch.cuda.empty_cache()


def recall(a):
    g = torch.Generator(device="cuda").manual_seed(1234)
    for kind, normalize in (("gauss", False), ("clustered", False), ("clustered", True)):
        if kind == "gauss":
            x = torch.randn(a.rows, a.dim, device="cuda", generator=g)
            q = torch.randn(a.queries, a.dim, device="cuda", generator=g)
        else:
            c = torch.randn(a.rows // 64, a.dim, device="cuda", generator=g)
            x = c.repeat_interleave(64, 0) + 0.05 * torch.randn(a.rows, a.dim, device="cuda", generator=g)
            pick = torch.randint(0, a.rows // 64, (a.queries,), device="cuda", generator=g)
            q = c[pick] + 0.05 * torch.randn(a.queries, a.dim, device="cuda", generator=g)
        if normalize:
            x = x / x.norm(dim=1, keepdim=True)
            q = q / q.norm(dim=1, keepdim=True)
        ref = ram.MipsIndex(a.dim, dtype="f32")
        ref.add(x)
        truth = {k: ref.search(q, k)[1].cpu().numpy() for k in (5, 29)}
        ref.check()
        del ref
        for name in ("pq", "sq8", "bf16"):
            ix = ram.PqIndex(a.dim, a.m) if name == "pq" else ram.MipsIndex(a.dim, dtype=name)
            ix.train(x)
            ix.add(x)
            rec = {"data": kind, "normalized": normalize, "rows": a.rows, "dim": a.dim, "queries": a.queries, "index": name,
                   "bytes_per_row": a.m if name == "pq" else None}
            for k in (5, 29):
                got = ix.search(q, k)[1].cpu().numpy()
                rec[f"recall_at_{k}"] = float(np.mean([len(set(truth[k][r]) & set(got[r])) / k for r in range(a.queries)]))
                if k == 5:
                    rec["top1_agree"] = float(np.mean(truth[k][:, 0] == got[:, 0]))
            del ix
            print(json.dumps(rec), flush=True)
        del x, q


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "recall"))
    ap.add_argument("--rows", type=int, nargs="+", default=None)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--queries", type=int, nargs="+", default=None)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    if a.mode == "rate":
        a.rows = a.rows or [1 << 20, 1 << 24]
        a.queries = a.queries or [1, 8, 16, 64]
        rate(a)
    else:
        a.rows = (a.rows or [1 << 20])[0]
        a.queries = (a.queries or [1024])[0]
        recall(a)
