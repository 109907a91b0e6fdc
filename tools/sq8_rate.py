"""What a search costs on the 8-bit scalar-quantised index ("sq8") next to the e4m3-documents index ("fp8_e4m3_docs": the same
bytes, another conversion step) and the bf16 index (twice the bytes), on the GPU box.
One process holds the three indexes over the SAME rows; every (index, Q) variant is timed with HIP events around blocks of
back-to-back device-resident searches (stream-ordered, nothing synchronises inside a block), the variants ALTERNATE block by block,
and the figure per variant is the median of its blocks with their minimum and maximum.
    python tools/sq8_rate.py [--rows 1048576 16777216] [--dim 768] [--queries 8 32 64] [--k 5] [--rounds 15] [--calls 20]
Rows: the Gaussian generator of the synthetic workloads, produced on the device in chunks; the SQ8 index is trained on the first
chunk (2^18 rows).  hbm_fraction = stored bytes of the index / time / 8 TB/s.  One JSON line per (rows, Q)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

HBM_BYTES_PER_S = 8.0e12
DTYPES = ("sq8", "fp8_e4m3_docs", "bf16")
BYTES = {"sq8": 1, "fp8_e4m3_docs": 1, "bf16": 2}


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    chunk = 1 << 18
    for rows in a.rows:
        idx = {dt: ram.MipsIndex(a.dim, dtype=dt) for dt in DTYPES}
        for ix in idx.values():
            ix.reserve(rows)
        for r0 in range(0, rows, chunk):
            x = ram.synth_fill(min(chunk, rows - r0), a.dim, r0, ram.SEED_DOCS, ram.SYNTH_GAUSS, dtype="f32")
            if r0 == 0:
                idx["sq8"].train(x)
            for ix in idx.values():
                ix.add(x)
            del x
        pitch = -(-a.dim // 256) * 256
        for nq in a.queries:
            q = ram.synth_fill(nq, a.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="f32")
            variants = {dt: (lambda ix=idx[dt]: ix.search(q, a.k)) for dt in DTYPES}
            rec = {"rows": rows, "dim": a.dim, "queries": nq, "k": a.k, "rounds": a.rounds, "calls_per_block": a.calls, "kernel": {}, "margin": {}}
            for name, fn in variants.items():  # warm-up: code objects, scratch, first-use allocations
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                rec["kernel"][name] = idx[name].last_kernel
                rec["margin"][name] = idx[name].margin_stats()
            t = {name: [] for name in variants}
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    t[name].append(block_ms(fn, a.calls))
            med = {name: float(np.median(v)) for name, v in t.items()}
            rec["ms_per_call"] = {name: {"median": med[name], "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}
            rec["hbm_fraction"] = {name: rows * (pitch if BYTES[name] == 1 else idx[name].d) * BYTES[name] / (med[name] * 1e-3) / HBM_BYTES_PER_S
                                   for name in variants}
            rec["sq8_over_e4m3_docs"] = med["sq8"] / med["fp8_e4m3_docs"]
            rec["sq8_over_bf16"] = med["sq8"] / med["bf16"]
            print(json.dumps(rec), flush=True)
        del idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
