"""What the WIDE search over the probed lists of an IVF index (IvfIndex.search_probed_wide, 30 <= k <= 1024) costs, on the GPU box,
next to its two yardsticks: search_probed(k = 29) -- the narrow search of the same lists, unchanged code -- and, on bf16 rows,
flat.search_wide(k) over ALL rows.  The protocol is that of tools/ivf_rate.py: one process holds an "sq8" and a "bf16" IvfIndex
(nlist = 256) over the same synthetic rows; for every storage, query count and nprobe the variants are timed with HIP events around
blocks of back-to-back device-resident calls (stream-ordered, nothing synchronises inside a block), the variants ALTERNATE block by
block, and the figure per variant is the median of its blocks with their minimum and maximum.  Whole calls: probe, staging, list
scan, merge, finish.
    python tools/ivf_wide_rate.py [--rows 1048576] [--dim 768] [--nlist 256] [--queries 8 16] [--nprobe 1 8 32]
                                  [--k 29 32 64 128 256 1024] [--noise 1.0] [--rounds 9] [--calls 20] [--out profiles/ivf_wide/rate.jsonl]
--noise 1.0 gives evenly filled lists, --noise 0.1 clustered rows and uneven lists (profiles/ivf/README.md).
Per line: ms per call of search_probed_wide(k), of search_probed(29) and (bf16) of flat.search_wide(k) in the same alternation, and
the two ratios.  A k for which min(nprobe, nlist) * k exceeds 65536 is refused by the library and skipped."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

DTYPES = ("sq8", "bf16")


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
        for _ in range(3):
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
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--k", type=int, nargs="+", default=[29, 32, 64, 128, 256, 1024])
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "ivf_wide", "rate.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_wide_rate: no GPU visible; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    centres = torch.randn((256, a.dim), generator=gen, device="cuda")
    centres = 4 * centres / centres.norm(dim=1, keepdim=True)
    idx = {dt: ram.IvfIndex(a.dim, a.nlist, dtype=dt) for dt in DTYPES}
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
    sizes = {dt: idx[dt].list_sizes() for dt in DTYPES}
    with open(a.out, "w") as out:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        emit({"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "nlist": a.nlist, "noise": a.noise, "rounds": a.rounds,
              "calls_per_block": a.calls, "list_rows_min_median_max": {dt: [int(s.min()), int(np.median(s)), int(s.max())] for dt, s in sizes.items()}})
        for nq in a.queries:
            q = clustered(gen, centres, nq, a.noise)
            for dt, ix in idx.items():
                for p in a.nprobe:
                    ks = [k for k in a.k if min(p, a.nlist) * k <= 65536]
                    variants = {"probed29": (lambda ix=ix, p=p: ix.search_probed(q, 29, p))}
                    for k in ks:
                        variants[f"wide{k}"] = (lambda ix=ix, p=p, k=k: ix.search_probed_wide(q, k, p))
                        if dt == "bf16" and k >= 30:
                            variants[f"flat_wide{k}"] = (lambda ix=ix, k=k: ix.flat.search_wide(q, k))
                    ms = timed(variants, a.rounds, a.calls)
                    rows_scanned = int(sizes[dt][ix.probe(q, p)].sum())
                    for k in ks:
                        rec = {"dtype": dt, "queries": nq, "nprobe": p, "k": k, "rows_scanned": rows_scanned, "wide_ms_per_call": ms[f"wide{k}"],
                               "probed29_ms_per_call": ms["probed29"], "wide_over_probed29": ms[f"wide{k}"]["median"] / ms["probed29"]["median"]}
                        if f"flat_wide{k}" in ms:
                            rec["flat_wide_ms_per_call"] = ms[f"flat_wide{k}"]
                            rec["wide_over_flat_wide"] = ms[f"wide{k}"]["median"] / ms[f"flat_wide{k}"]["median"]
                        emit(rec)


if __name__ == "__main__":
    main()
