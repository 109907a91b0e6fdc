"""What a search costs on the IVF index over PQ codes next to the flat PqIndex and the IvfIndex "sq8" over the SAME rows, where a
call's time goes, and what it finds, on the GPU box.  The protocol of tools/pq_rate.py: one process; device-resident queries; every
variant is timed with HIP events around blocks of back-to-back whole calls (stream-ordered, nothing synchronises inside a block)
after a warm-up of every shape; the variants ALTERNATE block by block; the figure per variant is the median of its blocks with
their minimum and maximum.
    python tools/ivfpq_rate.py rate   [--rows 1048576] [--data gauss clustered] [--nlist 1024 4096] [--nprobe 1 8 32 128]
                                      [--queries 1 8 16 64] [--dim 768] [--m 96] [--k 5] [--rounds 7] [--calls 10] [--niter 10]
    python tools/ivfpq_rate.py recall [--rows 1048576] [--data gauss clustered] [--nlist 1024] [--nprobe 1 8 32 128] [--queries 256]
Rows: "gauss" is the Gaussian generator of the synthetic workloads; "clustered" is rows // 64 Gaussian centres with 64 rows each at
noise 0.05 (the clustered set of tools/pq_rate.py), row i around centre i mod (rows // 64) so that every chunk sees every region.
Both are produced on the device in chunks of 2^18 rows; every index is trained on the first chunk.
`rate` prints per (data, rows, nlist, nprobe, Q): ms per call of IvfPqIndex.search, PqIndex.search and IvfIndex("sq8").search_probed;
the share of the IVFPQ call by difference -- `probe` is IvfPqIndex.probe alone (the coarse search and two small copies), `fixed` is
the call on an EMPTY twin index (same centroids and codebook, no rows: probe, tables, a scan that finds nothing, merge, finish) and
`scan_rows` is the rest, the part that grows with the probed rows --; the same call with the scan's S forced to what
pq::choose_segments gives for ntotal rows (`ivfpq_s_from_ntotal`; the library takes it for the ntotal * p / nlist rows a query is
expected to score: both S are in `segments`); the mean probed share of the rows, N_j / ntotal; and the ratio
of `scan_rows` to the flat PQ call, to hold against nprobe / nlist.  Per-kernel shares need a kernel trace: `calls` runs one
configuration a fixed number of times for that.
`recall` prints recall@5 / @29 against the fp32-exact flat index per nprobe for by_residual True and False, and PqIndex's on the same
rows.  One JSON line each."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

CHUNK = 1 << 18


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


def pq_segments(ns, k, M, ntotal, cus):
    """pq::choose_segments of csrc/pq_math.hpp: the S the flat PQ scan takes for an index of ntotal rows"""
    waves = 16 if M > 32 else 4
    lds = M * 256 * 4 + waves * 32 * 8 + waves * 4
    per_cu = max(1, min((160 << 10) // lds, 32 // waves))
    S = min(-(-2 * cus * per_cu // ns), -(-ntotal // (64 * waves)))
    if S * k > 65536:
        S = 65536 // k
    return max(S, 1)


def chunk_of(kind, rows, r0, dim, centres):
    n = min(CHUNK, rows - r0)
    if kind == "gauss":
        return ram.synth_fill(n, dim, r0, ram.SEED_DOCS, ram.SYNTH_GAUSS, dtype="f32")
    g = torch.Generator(device="cuda").manual_seed(977 + r0)
    # row i belongs to centre i mod (rows // 64): every chunk, the training chunk too, sees every region of the data
    lab = torch.arange(r0, r0 + n, device="cuda") % centres.shape[0]
    return centres[lab] + 0.05 * torch.randn(n, dim, device="cuda", generator=g)


def queries_of(kind, nq, dim, centres):
    if kind == "gauss":
        return ram.synth_fill(nq, dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="f32")
    g = torch.Generator(device="cuda").manual_seed(4242)
    pick = torch.randint(0, centres.shape[0], (nq,), device="cuda", generator=g)
    return centres[pick] + 0.05 * torch.randn(nq, dim, device="cuda", generator=g)


def centres_of(kind, rows, dim):
    if kind == "gauss":
        return None
    return torch.randn(rows // 64, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1234))


def build(a, kind, rows, nlists, with_sq8=True, residual=(True,)):
    """-> (centres, pq, {nlist: {"ivfpq"[, "ivfpq_raw"], "empty", "ivf_sq8"}}, build record)"""
    centres = centres_of(kind, rows, a.dim)
    pq = ram.PqIndex(a.dim, a.m)
    per = {}
    rec = {"what": "build", "data": kind, "rows": rows, "dim": a.dim, "M": a.m, "niter": a.niter, "train_rows_given": min(CHUNK, rows)}
    for nlist in nlists:
        per[nlist] = {}
        for br in residual:
            ix = ram.IvfPqIndex(a.dim, nlist, a.m, by_residual=br)
            ix.niter = a.niter
            per[nlist]["ivfpq" if br else "ivfpq_raw"] = ix
        if with_sq8:
            per[nlist]["ivf_sq8"] = ram.IvfIndex(a.dim, nlist, "sq8")
            per[nlist]["ivf_sq8"].niter = a.niter
    for r0 in range(0, rows, CHUNK):
        x = chunk_of(kind, rows, r0, a.dim, centres)
        if r0 == 0:
            pq.train(x)
            for nlist, d in per.items():
                for name, ix in d.items():
                    rec[f"{name}_{nlist}_train_s"] = wall(lambda: ix.train(x))
        pq.add(x)
        for nlist, d in per.items():
            for name, ix in d.items():
                rec[f"{name}_{nlist}_add_s"] = rec.get(f"{name}_{nlist}_add_s", 0.0) + wall(lambda: ix.add(x))
        del x
    for nlist, d in per.items():
        full = d["ivfpq"] if "ivfpq" in d else d["ivfpq_raw"]
        empty = ram.IvfPqIndex(a.dim, nlist, a.m)
        empty.set_centroids(full.centroids())
        empty.set_codebook(full.codebook())
        d["empty"] = empty
        sizes = full.list_sizes()
        rec[f"lists_{nlist}"] = {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
    print(json.dumps(rec), flush=True)
    return centres, pq, per


def rate(a):
    for kind in a.data:
        for rows in a.rows:
            centres, pq, per = build(a, kind, rows, a.nlist)
            for nlist in a.nlist:
                ix, empty, sq8 = per[nlist]["ivfpq"], per[nlist]["empty"], per[nlist]["ivf_sq8"]
                sizes = torch.from_numpy(ix.list_sizes()).cuda()
                cus = torch.cuda.get_device_properties(0).multi_processor_count
                for nq in a.queries:
                    q = queries_of(kind, nq, a.dim, centres)
                    for nprobe in a.nprobe:
                        s_all = pq_segments(nq, a.k, a.m, rows, cus)   # S as the flat scan would take it, from ntotal

                        def with_segments(S):
                            ix.scan_segments = S
                            return ix.search(q, a.k, nprobe=nprobe)

                        variants = {"ivfpq": lambda: with_segments(0), "ivfpq_s_from_ntotal": lambda: with_segments(s_all), "pq": lambda: pq.search(q, a.k),
                                    "ivf_sq8": lambda: sq8.search_probed(q, a.k, nprobe=nprobe), "probe": lambda: ix.probe(q, nprobe, return_scores=True),
                                    "fixed": lambda: empty.search(q, a.k, nprobe=nprobe)}
                        for fn in variants.values():  # warm-up: code objects, scratch, first-use allocations
                            for _ in range(3):
                                fn()
                            torch.cuda.synchronize()
                        t = {name: [] for name in variants}
                        for _ in range(a.rounds):
                            for name, fn in variants.items():
                                t[name].append(block_ms(fn, a.calls))
                        med = {name: float(np.median(v)) for name, v in t.items()}
                        probed = sizes[ix.probe(q, nprobe).long()].sum(dim=1).float().mean().item() / rows
                        scan_rows = med["ivfpq"] - med["fixed"]
                        rec = {"what": "rate", "data": kind, "rows": rows, "dim": a.dim, "M": a.m, "nlist": nlist, "nprobe": nprobe, "queries": nq, "k": a.k,
                               "rounds": a.rounds, "calls_per_block": a.calls,
                               "ms_per_call": {name: {"median": med[name], "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()},
                               "share": {"probe": med["probe"] / med["ivfpq"], "tables_merge_finish": (med["fixed"] - med["probe"]) / med["ivfpq"],
                                         "scan_rows": scan_rows / med["ivfpq"]},
                               "probed_share_of_rows": probed, "nprobe_over_nlist": min(nprobe, nlist) / nlist,
                               "scan_rows_over_pq_call": scan_rows / med["pq"], "ivfpq_over_pq": med["ivfpq"] / med["pq"],
                               "segments": {"chosen": pq_segments(nq, a.k, a.m, -(-rows * min(nprobe, nlist) // nlist), cus), "from_ntotal": s_all},
                               "s_from_ntotal_over_chosen": med["ivfpq_s_from_ntotal"] / med["ivfpq"],
                               "ivfpq_over_ivf_sq8": med["ivfpq"] / med["ivf_sq8"]}
                        print(json.dumps(rec), flush=True)
                ix.scan_segments = 0
            del pq, per
            torch.cuda.empty_cache()


def recall(a):
    for kind in a.data:
        rows = a.rows[0]
        centres, pq, per = build(a, kind, rows, a.nlist, with_sq8=False, residual=(True, False))
        q = queries_of(kind, a.queries[0], a.dim, centres)
        ref = ram.MipsIndex(a.dim, dtype="f32")
        for r0 in range(0, rows, CHUNK):
            ref.add(chunk_of(kind, rows, r0, a.dim, centres))
        truth = {k: ref.search(q, k)[1].cpu().numpy() for k in (5, 29)}
        ref.check()
        del ref

        def score(search):
            out = {}
            for k in (5, 29):
                got = search(k).cpu().numpy()
                out[f"recall_at_{k}"] = float(np.mean([len(set(truth[k][r]) & set(got[r])) / k for r in range(len(got))]))
            return out

        print(json.dumps({"what": "recall", "data": kind, "rows": rows, "dim": a.dim, "M": a.m, "queries": a.queries[0], "index": "pq",
                          **score(lambda k: pq.search(q, k)[1])}), flush=True)
        for nlist in a.nlist:
            for name in ("ivfpq", "ivfpq_raw"):
                for nprobe in a.nprobe + [nlist]:
                    if nprobe > 1024:
                        continue
                    print(json.dumps({"what": "recall", "data": kind, "rows": rows, "dim": a.dim, "M": a.m, "queries": a.queries[0], "index": name,
                                      "by_residual": name == "ivfpq", "nlist": nlist, "nprobe": nprobe,
                                      **score(lambda k: per[nlist][name].search(q, k, nprobe=nprobe)[1])}), flush=True)
        del pq, per
        torch.cuda.empty_cache()


def calls(a):
    """one configuration, a.calls * a.rounds whole calls: what a kernel trace is taken of"""
    kind, rows, nlist = a.data[0], a.rows[0], a.nlist[0]
    centres, pq, per = build(a, kind, rows, [nlist], with_sq8=False)
    q = queries_of(kind, a.queries[0], a.dim, centres)
    for _ in range(a.calls * a.rounds):
        per[nlist]["ivfpq"].search(q, a.k, nprobe=a.nprobe[0])
    torch.cuda.synchronize()
    print(json.dumps({"what": "calls", "data": kind, "rows": rows, "nlist": nlist, "nprobe": a.nprobe[0], "queries": a.queries[0],
                      "calls": a.calls * a.rounds}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "recall", "calls"))
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20])
    ap.add_argument("--data", nargs="+", default=["gauss", "clustered"], choices=("gauss", "clustered"))
    ap.add_argument("--nlist", type=int, nargs="+", default=None)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--queries", type=int, nargs="+", default=None)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--niter", type=int, default=10)
    a = ap.parse_args()
    if a.mode == "rate":
        a.nlist = a.nlist or [1024, 4096]
        a.queries = a.queries or [1, 8, 16, 64]
        rate(a)
    elif a.mode == "recall":
        a.nlist = a.nlist or [1024]
        a.queries = a.queries or [256]
        recall(a)
    else:
        a.nlist = a.nlist or [1024]
        a.queries = a.queries or [8]
        calls(a)
