"""What the group rule and the bitmap cost -- or save -- in the search over the probed lists of an IVF index, on the GPU box.
The protocol of tools/ivf_rate.py: one process holds an "sq8" and a "bf16" IvfIndex (nlist = 256) over the same synthetic rows; for
every storage, query count and nprobe the variants are timed with HIP events around blocks of back-to-back device-resident calls
(stream-ordered, nothing synchronises inside a block), the variants ALTERNATE block by block, and the figure per variant is the
median of its blocks with their minimum and maximum.  The yardstick is the UNFILTERED search_probed in the same run.
    python tools/ivf_filter_rate.py [--rows 1048576] [--dim 768] [--nlist 256] [--queries 8 16] [--k 2] [--nprobe 1 8 32]
                                    [--noise 1.0] [--rounds 9] [--calls 20] [--out profiles/ivf_filter/rate.jsonl]
Variants:
    unfiltered       search_probed(q, k, nprobe)
    exclude8         groups of 8 consecutive rows (label = row // 8), every query excludes the group of a random row: the
                     reference's "not of my own article"
    only_<m>         labels drawn uniformly from [0, m), every query keeps label 0: one row in m is admitted
    bitmap_<m>       a random bitmap that admits one row in m
for m = 2, 16 and 256.  A variant's labels are written (a device-to-device copy, stream-ordered) before its block's first event, so
re-labelling is not timed.  Per line: ms per call of every variant and its ratio to the unfiltered search; `spread` is
(max - min) / median of a variant's blocks."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

DENSITIES = (2, 16, 256)


def block_ms(prep, fn, calls):
    prep()
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
    for prep, fn in variants.values():  # warm-up: code objects, scratch, first-use allocations
        prep()
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (prep, fn) in variants.items():
            t[name].append(block_ms(prep, fn, calls))
    return {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                   "spread": float((np.max(v) - np.min(v)) / np.median(v))} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--dtypes", nargs="+", default=["sq8", "bf16"])
    ap.add_argument("--out", default=os.path.join("profiles", "ivf_filter", "rate.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_filter_rate: no GPU visible; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    centres = torch.randn((256, a.dim), generator=gen, device="cuda")
    centres = 4 * centres / centres.norm(dim=1, keepdim=True)
    idx = {dt: ram.IvfIndex(a.dim, a.nlist, dtype=dt) for dt in a.dtypes}
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
    n = a.rows
    labels = {"exclude8": (torch.arange(n, device="cuda") // 8).to(torch.int32)}
    masks = {}
    for m in DENSITIES:
        labels[f"only_{m}"] = torch.randint(0, m, (n,), generator=gen, device="cuda").to(torch.int32)
        masks[f"bitmap_{m}"] = ram.Selector.from_mask(torch.randint(0, m, (n,), generator=gen, device="cuda") == 0)
    with open(a.out, "w") as out:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        sizes = {dt: ix.list_sizes() for dt, ix in idx.items()}
        emit({"device": torch.cuda.get_device_name(0), "rows": n, "dim": a.dim, "nlist": a.nlist, "noise": a.noise, "k": a.k, "rounds": a.rounds,
              "calls_per_block": a.calls, "list_rows_min_median_max": {dt: [int(s.min()), int(np.median(s)), int(s.max())] for dt, s in sizes.items()},
              "admitted_share": {name: float(s.count()) / n for name, s in masks.items()}})
        for nq in a.queries:
            q = clustered(gen, centres, nq, a.noise)
            own = labels["exclude8"][torch.randint(0, n, (nq,), generator=gen, device="cuda")].contiguous()
            zero = torch.zeros(nq, dtype=torch.int32, device="cuda")
            for dt, ix in idx.items():
                for p in a.nprobe:
                    nothing = lambda: None
                    variants = {"unfiltered": (nothing, lambda ix=ix, p=p: ix.search_probed(q, a.k, p)),
                                "exclude8": (lambda ix=ix: ix.set_labels(labels["exclude8"]),
                                             lambda ix=ix, p=p: ix.search_probed(q, a.k, p, groups=own, group_mode="exclude"))}
                    for m in DENSITIES:
                        variants[f"only_{m}"] = (lambda ix=ix, m=m: ix.set_labels(labels[f"only_{m}"]),
                                                 lambda ix=ix, p=p: ix.search_probed(q, a.k, p, groups=zero, group_mode="only"))
                        variants[f"bitmap_{m}"] = (nothing, lambda ix=ix, p=p, m=m: ix.search_probed(q, a.k, p, selector=masks[f"bitmap_{m}"]))
                    ms = timed(variants, a.rounds, a.calls)
                    base = ms["unfiltered"]["median"]
                    emit({"dtype": dt, "queries": nq, "nprobe": p, "rows_scanned": int(sizes[dt][ix.probe(q, p)].sum()), "ms_per_call": ms,
                          "over_unfiltered": {name: v["median"] / base for name, v in ms.items()}})


if __name__ == "__main__":
    main()
