"""What the RANGE search over the probed lists of an IVF index (IvfIndex.range_search_probed_into) costs, on the GPU box, next to its two
yardsticks: search_probed(k = 29) -- the fixed-k search of the same lists, unchanged code -- and, on bf16 rows, flat.range_search_into
with the same radii over ALL rows.  The protocol is that of tools/ivf_rate.py: one process holds an "sq8" and a "bf16" IvfIndex
(nlist = 256) over the same synthetic rows; for every storage, query count, nprobe and radius the variants are timed with HIP events
around blocks of back-to-back device-resident calls (stream-ordered, nothing synchronises inside a block: caller-allocated outputs,
device radii), the variants ALTERNATE block by block, and the figure per variant is the median of its blocks with their minimum and
maximum.  Whole calls: probe, staging, range scan, lims, place, order.
    python tools/ivf_range_rate.py [--rows 1048576] [--dim 768] [--nlist 256] [--queries 8 16] [--nprobe 1 8 32] [--noise 1.0]
                                   [--rounds 9] [--calls 20] [--out profiles/ivf_range/rate.jsonl]
--noise 1.0 gives evenly filled lists, --noise 0.1 clustered rows and uneven lists (profiles/ivf/README.md).
The radii of a cell are chosen per query, once, from one range call at -inf (every probed row's score): the score below which about
0, about 10 and about 1000 of the query's probed rows lie above, and the one that admits a tenth of them ("tenth").
Per line: the hits per query the radii really give, ms per call of the range search, of search_probed(29) and (bf16) of the flat range
search in the same alternation, and the two ratios."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

DTYPES = ("sq8", "bf16")
TARGETS = ("0", "10", "1000", "tenth")


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


def radii_for(ix, q, p):
    """-> {target: float32 [nq]} and the probed rows per query, from the scores of every probed row"""
    lims, D, _ = ix.range_search_probed(q, float("-inf"), p)
    lims, D = lims.cpu().numpy(), D.cpu().numpy()
    out = {t: [] for t in TARGETS}
    for j in range(len(lims) - 1):
        s = np.sort(D[lims[j]:lims[j + 1]])[::-1]
        for t in TARGETS:
            c = len(s) // 10 if t == "tenth" else int(t)
            out[t].append(np.float32(np.inf) if len(s) == 0 or c == 0 else s[min(c, len(s) - 1)])
    return {t: np.array(v, np.float32) for t, v in out.items()}, np.diff(lims)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "ivf_range", "rate.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_range_rate: no GPU visible; nothing is measured without one")
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
            lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
            flims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
            for dt, ix in idx.items():
                for p in a.nprobe:
                    radii, probed = radii_for(ix, q, p)
                    cap = int(probed.sum())                  # every probed row fits: no call of the grid overflows
                    D = torch.empty(cap, dtype=torch.float32, device="cuda")
                    I = torch.empty(cap, dtype=torch.int64, device="cuda")
                    fcap = max(cap, 1 << 22)                 # the flat search meets the same radii on ALL rows: room for more hits
                    FD = torch.empty(fcap, dtype=torch.float32, device="cuda")
                    FI = torch.empty(fcap, dtype=torch.int64, device="cuda")
                    variants = {"probed29": (lambda ix=ix, p=p: ix.search_probed(q, 29, p))}
                    host_r = {}
                    for t in TARGETS:
                        r = torch.from_numpy(radii[t]).cuda()
                        variants[f"range_{t}"] = (lambda ix=ix, p=p, r=r: ix.range_search_probed_into(q, r, lims, D, I, nprobe=p))
                        if dt == "bf16":                     # the flat range search takes its radii from the host
                            host_r[t] = radii[t]
                            variants[f"flat_{t}"] = (lambda ix=ix, t=t: ix.flat.range_search_into(q, host_r[t], flims, FD, FI))
                    ms = timed(variants, a.rounds, a.calls)
                    flat_total = {}
                    for t in host_r:
                        ix.flat.range_search_into(q, host_r[t], flims, FD, FI)
                        flat_total[t] = flims[-1].item()
                    for t in TARGETS:
                        ix.range_search_probed_into(q, torch.from_numpy(radii[t]).cuda(), lims, D, I, nprobe=p)
                        hits = np.diff(lims.cpu().numpy())
                        rec = {"dtype": dt, "queries": nq, "nprobe": p, "target": t, "rows_scanned": int(probed.sum()),
                               "hits_per_query_min_median_max": [int(hits.min()), float(np.median(hits)), int(hits.max())],
                               "range_ms_per_call": ms[f"range_{t}"], "probed29_ms_per_call": ms["probed29"],
                               "range_over_probed29": ms[f"range_{t}"]["median"] / ms["probed29"]["median"]}
                        if f"flat_{t}" in ms:
                            rec["flat_hits_total"] = int(flat_total[t])
                            rec["flat_range_ms_per_call"] = ms[f"flat_{t}"]
                            rec["range_over_flat_range"] = ms[f"range_{t}"]["median"] / ms[f"flat_{t}"]["median"]
                        emit(rec)


if __name__ == "__main__":
    main()
