"""What cutting the IVF search at its merge costs, on the GPU box: the part search + the merge of the parts over P row parts held by
ONE process on one GPU, against the unsharded search_probed / search_probed_wide of the same build on the same rows.
    python tools/ivf_sharded_rate.py [--rows 1048576] [--dim 768] [--nlist 256] [--parts 1 2 4 8] [--queries 8 16] [--nprobe 1 8 32]
                                     [--ks 5 100] [--dtypes sq8 bf16] [--rounds 7] [--calls 10] [--out profiles/ivf_sharded/rate.jsonl]
Rows and queries: tools/ivf_rate.py's clustered distribution (256 Gaussian clusters, centres of norm 4); the unsharded index trains on
the first 65536 rows (4 k-means iterations), and every part gets ITS centroids (and SQ8 range) and the rows of its range,
shard_bounds(rows, P, r).  Per (storage, queries, nprobe, k) the variants are timed with HIP events around blocks of back-to-back
device-resident calls, the variants ALTERNATE block by block, and the figure per variant is the median of its blocks with their
minimum and maximum:
    unsharded        search_probed (k <= 29) or search_probed_wide of the whole index
    P<p>_all         the p part searches one after the other + ivf_merge_parts: everything a p-way search computes, on one GPU
    P<p>_rank        ONE part search (part 0, the largest) + ivf_merge_parts over the p payloads: what one rank of p runs between
                     the query and the result, without the all-gather (which this single process cannot measure)
The merged result is compared with the unsharded one before anything is timed; a difference ends the run."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


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


def clustered(gen, centres, n, noise):
    lab = torch.randint(0, centres.shape[0], (n,), generator=gen, device="cuda")
    return centres[lab] + noise * torch.randn((n, centres.shape[1]), generator=gen, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--parts", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--queries", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--ks", type=int, nargs="+", default=[5, 100])
    ap.add_argument("--dtypes", nargs="+", default=["sq8", "bf16"])
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "ivf_sharded", "rate.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_sharded_rate: no GPU visible; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    centres = torch.randn((256, a.dim), generator=gen, device="cuda")
    centres = 4 * centres / centres.norm(dim=1, keepdim=True)
    x = torch.cat([clustered(gen, centres, min(1 << 18, a.rows - r0), a.noise) for r0 in range(0, a.rows, 1 << 18)])
    qs = {nq: clustered(gen, centres, nq, a.noise) for nq in a.queries}
    chunk = 1 << 18
    with open(a.out, "w") as out:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        emit({"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "nlist": a.nlist, "noise": a.noise, "parts": a.parts,
              "rounds": a.rounds, "calls_per_block": a.calls})
        for dt in a.dtypes:
            full = ram.IvfIndex(a.dim, a.nlist, dtype=dt)
            full.niter = 4
            full.train(x[:65536])
            for r0 in range(0, a.rows, chunk):
                full.add(x[r0:r0 + chunk])
            cen = full.centroids()
            sets = {}
            for P in a.parts:
                sets[P] = []
                for r in range(P):
                    lo, hi = ram.shard_bounds(a.rows, P, r)
                    part = ram.IvfIndex(a.dim, a.nlist, dtype=dt)
                    part.set_centroids(cen)
                    if dt == "sq8":
                        part.set_sq8_params(*full.flat.sq8_params())
                    for r0 in range(lo, hi, chunk):
                        part.add(x[r0:min(hi, r0 + chunk)])
                    sets[P].append((lo, part))
            for nq in a.queries:
                q = qs[nq]
                for nprobe in a.nprobe:
                    for k in a.ks:
                        unsharded = (lambda: full.search_probed(q, k, nprobe)) if k <= ram.MAX_K else (lambda: full.search_probed_wide(q, k, nprobe))

                        def sharded(P, only_first):
                            payloads, bias = [], None
                            for lo, part in sets[P][:1 if only_first else P]:
                                pk, bias = part.search_part(q, k, nprobe, idx_offset=lo)
                                payloads.append(pk)
                            if only_first:      # the other ranks' payloads as they would arrive: this call's stand in for them
                                payloads += [ready[P][r] for r in range(1, P)]
                            return ram.ivf_merge_parts(torch.cat(payloads), P, nq, k, bias)

                        ready = {P: [part.search_part(q, k, nprobe, idx_offset=lo)[0] for lo, part in sets[P]] for P in a.parts}
                        want = unsharded()
                        for P in a.parts:
                            for only_first in (False, True):
                                got = sharded(P, only_first)
                                if not (torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))):
                                    raise SystemExit(f"{dt} nq {nq} nprobe {nprobe} k {k}: {P} parts differ from the unsharded search")
                        variants = {"unsharded": unsharded}
                        for P in a.parts:
                            variants[f"P{P}_all"] = (lambda P=P: sharded(P, False))
                            variants[f"P{P}_rank"] = (lambda P=P: sharded(P, True))
                        ms = timed(variants, a.rounds, a.calls)
                        emit({"dtype": dt, "queries": nq, "nprobe": nprobe, "k": k, "ms_per_call": ms, "payload_bytes_per_rank": nq * k * 16,
                              "rank_over_unsharded": {f"P{P}": ms[f"P{P}_rank"]["median"] / ms["unsharded"]["median"] for P in a.parts},
                              "all_over_unsharded": {f"P{P}": ms[f"P{P}_all"]["median"] / ms["unsharded"]["median"] for P in a.parts},
                              "equal_to_unsharded": True})
            del full, sets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
