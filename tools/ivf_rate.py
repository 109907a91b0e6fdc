"""What the search over the probed lists of an IVF index costs next to the flat search of the SAME rows, on the GPU box.
One process holds an "sq8" and a "bf16" IvfIndex (nlist = 256) over the same clustered synthetic rows; for every storage and query
count the variants -- flat.search and search_probed at each nprobe -- are timed with HIP events around blocks of back-to-back
device-resident calls (stream-ordered, nothing synchronises inside a block), the variants ALTERNATE block by block, and the figure
per variant is the median of its blocks with their minimum and maximum.  The yardstick is flat.search in the same run.
    python tools/ivf_rate.py [--rows 1048576] [--dim 768] [--nlist 256] [--queries 8 16] [--k 2] [--nprobe 1 8 32 256]
                             [--large 1024] [--noise 0.1] [--rounds 9] [--calls 20] [--out profiles/ivf/rate.jsonl]
Rows: 256 Gaussian clusters (centres of norm 4, noise of --noise per component), cluster labels drawn at random so that every prefix
is representative; the index trains on the first 65536 rows with 4 k-means iterations.  Queries: rows of the same distribution.
recall_at_k_vs_flat: the share of flat.search's rows that search_probed returns (1.0 by definition once every list is probed).
Per line: ms per call; ivf_over_flat; scanned_bytes = the stored bytes of the rows of the probed lists, summed over the queries
(every query reads its own lists); scan_bytes_per_s = scanned_bytes / time of the WHOLE call (probe, staging, scan, merge), so it
understates the scan; fma_per_s = one fp64 FMA per scanned element."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

HBM_BYTES_PER_S = 8.0e12
BYTES = {"sq8": 1, "bf16": 2}


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def clustered(gen, centres, n, noise):
    lab = torch.randint(0, centres.shape[0], (n,), generator=gen, device="cuda")
    return centres[lab] + noise * torch.randn((n, centres.shape[1]), generator=gen, device="cuda")


def timed(variants, rounds, calls):
    for fn in variants.values():  # warm-up: code objects, scratch, first-use allocations
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t[name].append(block_ms(fn, calls))
    return {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--large", type=int, default=1024, help="one large batch (0: none), at the second nprobe")
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "ivf", "rate.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_rate: no GPU visible; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    centres = torch.randn((256, a.dim), generator=gen, device="cuda")
    centres = 4 * centres / centres.norm(dim=1, keepdim=True)
    idx = {dt: ram.IvfIndex(a.dim, a.nlist, dtype=dt) for dt in BYTES}
    chunk = 1 << 18
    for r0 in range(0, a.rows, chunk):
        x = clustered(gen, centres, min(chunk, a.rows - r0), a.noise)
        if r0 == 0:
            for ix in idx.values():
                ix.niter = 4
                ix.train(x[:65536])
        for ix in idx.values():
            ix.add(x)
        del x
    pitch = {"sq8": -(-a.dim // 256) * 256, "bf16": 1024 if a.dim > 768 else -(-a.dim // 128) * 128}
    sizes = {dt: idx[dt].list_sizes() for dt in BYTES}
    with open(a.out, "w") as out:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        emit({"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "nlist": a.nlist, "noise": a.noise, "k": a.k, "rounds": a.rounds,
              "calls_per_block": a.calls, "list_rows_min_median_max": {dt: [int(s.min()), int(np.median(s)), int(s.max())] for dt, s in sizes.items()}})
        shapes = [(nq, a.nprobe) for nq in a.queries] + ([(a.large, a.nprobe[1:2])] if a.large else [])
        for nq, nprobes in shapes:
            q = clustered(gen, centres, nq, a.noise)
            for dt, ix in idx.items():
                variants = {"flat": (lambda ix=ix: ix.flat.search(q, a.k))}
                for p in nprobes:
                    variants[f"nprobe{p}"] = (lambda ix=ix, p=p: ix.search_probed(q, a.k, p))
                ms = timed(variants, a.rounds, a.calls if nq <= 64 else max(2, a.calls // 5))
                for p in nprobes:
                    P = ix.probe(q, p)
                    rows_scanned = int(sizes[dt][P].sum())
                    t = ms[f"nprobe{p}"]["median"] * 1e-3
                    nbytes = rows_scanned * pitch[dt] * BYTES[dt]
                    emit({"dtype": dt, "queries": nq, "nprobe": p, "ms_per_call": ms[f"nprobe{p}"], "flat_ms_per_call": ms["flat"],
                          "ivf_over_flat": ms[f"nprobe{p}"]["median"] / ms["flat"]["median"], "rows_scanned": rows_scanned, "scanned_bytes": nbytes,
                          "scan_bytes_per_s": nbytes / t, "hbm_fraction": nbytes / t / HBM_BYTES_PER_S, "fma_per_s": rows_scanned * pitch[dt] / t,
                          "flat_kernel": ix.flat.last_kernel})
                fd, fi = ix.flat.search(q, a.k)            # what the probes lose: the share of the flat result's rows they return
                for p in nprobes:
                    _, i = ix.search_probed(q, a.k, p)
                    hit = np.mean([len(set(r.tolist()) & set(f.tolist())) / a.k for r, f in zip(i.cpu().numpy(), fi.cpu().numpy())])
                    emit({"dtype": dt, "queries": nq, "nprobe": p, "recall_at_k_vs_flat": float(hit)})


if __name__ == "__main__":
    main()
