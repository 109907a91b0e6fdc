"""What the two-stage search on PQ codes costs and what it finds, on the GPU box (profiles/refine/README.md).  The
protocol of tools/ivfpq_rate.py, whose generators and timing blocks are imported: one process; device-resident queries; every variant
is timed with HIP events around blocks of back-to-back whole calls (stream-ordered, nothing synchronises inside a block) after a
warm-up of every shape; the variants ALTERNATE block by block; the figure per variant is the median of its blocks with their minimum
and maximum.
    python tools/refine_rate.py rate   [--rows 1048576] [--data gauss clustered] [--nlist 1024] [--nprobe 32] [--queries 1 16 64]
                                       [--dim 768] [--m 96] [--rounds 7] [--calls 10] [--niter 10]
    python tools/refine_rate.py recall [--rows 1048576] [--data gauss clustered] [--nlist 1024] [--nprobe 32 1024] [--queries 256]
    python tools/refine_rate.py order  [--rows 1048576] [--queries 16]
`rate` prints per (data, Q): ms per call of search at k = 29 and of search_candidates at k = 30 / 64 / 256 / 1024 from the same build,
on the PqIndex and on the IvfPqIndex; and ms per call of MipsIndex.rerank to k = 29 for kc = 64 / 256 / 1024 candidate ids (those the
PqIndex returned) against a "bf16" and an "sq8" store of the same rows.
`recall` prints recall@5 / @29 against the fp32-exact flat index of the two calls of RefinedIndex.search -- search_candidates at kc =
64 / 256 / 1024 on either base, rerank against a "bf16" store -- next to the unrefined base (kc = 0).
`order` times search_candidates on a PqIndex whose rows score in strictly ascending, descending and shuffled order for every query
(one decisive code column): ascending makes every row an insertion at the front of its pool.
One JSON line each."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram
from ivfpq_rate import CHUNK, block_ms, centres_of, chunk_of, queries_of

KCS = (64, 256, 1024)


def build(a, kind, rows, stores):
    """-> (centres, pq, ivfpq, {storage: MipsIndex})"""
    centres = centres_of(kind, rows, a.dim)
    pq = ram.PqIndex(a.dim, a.m)
    ivfpq = ram.IvfPqIndex(a.dim, a.nlist, a.m)
    ivfpq.niter = a.niter
    flat = {s: ram.MipsIndex(a.dim, dtype=s) for s in stores}
    for r0 in range(0, rows, CHUNK):
        x = chunk_of(kind, rows, r0, a.dim, centres)
        if r0 == 0:
            pq.train(x)
            ivfpq.train(x)
            if "sq8" in flat:
                flat["sq8"].train(x)
        pq.add(x)
        ivfpq.add(x)
        for ix in flat.values():
            ix.add(x)
        del x
    return centres, pq, ivfpq, flat


def timed(variants, a):
    for fn in variants.values():  # warm-up: code objects, scratch, first-use allocations
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    t = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            t[name].append(block_ms(fn, a.calls))
    return {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}


def rate(a):
    for kind in a.data:
        rows = a.rows
        centres, pq, ivfpq, flat = build(a, kind, rows, ("bf16", "sq8"))
        nprobe = a.nprobe[0]
        for nq in a.queries:
            q = queries_of(kind, nq, a.dim, centres)
            variants = {"pq_search_29": lambda: pq.search(q, 29), "ivfpq_search_29": lambda: ivfpq.search(q, 29, nprobe=nprobe)}
            for k in (30,) + KCS:
                variants[f"pq_candidates_{k}"] = lambda k=k: pq.search_candidates(q, k)
                variants[f"ivfpq_candidates_{k}"] = lambda k=k: ivfpq.search_candidates(q, k, nprobe=nprobe)
            for kc in KCS:
                ids = pq.search_candidates(q, kc)[1]
                for s, ix in flat.items():
                    variants[f"rerank_{s}_{kc}"] = lambda ix=ix, ids=ids: ix.rerank(q, ids, 29)
            print(json.dumps({"what": "rate", "data": kind, "rows": rows, "dim": a.dim, "M": a.m, "nlist": a.nlist, "nprobe": nprobe, "queries": nq,
                              "rounds": a.rounds, "calls_per_block": a.calls, "ms_per_call": timed(variants, a)}), flush=True)
        del pq, ivfpq, flat
        torch.cuda.empty_cache()


def recall(a):
    for kind in a.data:
        rows = a.rows
        centres, pq, ivfpq, flat = build(a, kind, rows, ("bf16",))
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

        bases = [("pq", pq, {})] + [("ivfpq", ivfpq, {"nprobe": p}) for p in a.nprobe if min(p, a.nlist) <= 1024]
        for name, base, kw in bases:
            head = {"what": "recall", "data": kind, "rows": rows, "dim": a.dim, "M": a.m, "queries": a.queries[0], "base": name, **kw}
            if name == "ivfpq":
                head["nlist"] = a.nlist
            print(json.dumps({**head, "kc": 0, "store": None, **score(lambda k: base.search(q, k, **kw)[1])}), flush=True)
            for kc in KCS:  # RefinedIndex.search at exactly kc candidates: its two calls
                print(json.dumps({**head, "kc": kc, "store": "bf16",
                                  **score(lambda k: flat["bf16"].rerank(q, base.search_candidates(q, kc, **kw)[1], k)[1])}), flush=True)
        del pq, ivfpq, flat
        torch.cuda.empty_cache()


def order(a):
    """rows whose score is decided by code column 0 alone, rising (falling, shuffled) with the row number"""
    rows, nq = a.rows, a.queries[0]
    g = torch.Generator(device="cuda").manual_seed(7)
    cb = np.zeros((a.m, 256, a.dim // a.m), np.float32)
    cb[0, :, 0] = np.arange(256, dtype=np.float32)
    q = torch.randn(nq, a.dim, device="cuda", generator=g)
    q[:, 0] = q[:, 0].abs() + 1
    ramp = (torch.arange(rows, device="cuda") * 256 // rows).to(torch.uint8)
    for name, col in (("ascending", ramp), ("descending", 255 - ramp), ("shuffled", ramp[torch.randperm(rows, device="cuda", generator=g)])):
        ix = ram.PqIndex(a.dim, a.m)
        ix.set_codebook(cb)
        codes = torch.zeros(rows, a.m, dtype=torch.uint8, device="cuda")
        codes[:, 0] = col
        ix.add_codes(codes)
        variants = {"search_29": lambda: ix.search(q, 29)}
        for k in (30,) + KCS:
            variants[f"candidates_{k}"] = lambda k=k: ix.search_candidates(q, k)
        print(json.dumps({"what": "order", "rows_in": name, "rows": rows, "dim": a.dim, "M": a.m, "queries": nq, "rounds": a.rounds,
                          "calls_per_block": a.calls, "ms_per_call": timed(variants, a)}), flush=True)
        del ix, codes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "recall", "order"))
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--data", nargs="+", default=["gauss", "clustered"], choices=("gauss", "clustered"))
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=None)
    ap.add_argument("--queries", type=int, nargs="+", default=None)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--niter", type=int, default=10)
    a = ap.parse_args()
    if a.mode == "rate":
        a.nprobe = a.nprobe or [32]
        a.queries = a.queries or [1, 16, 64]
        rate(a)
    elif a.mode == "recall":
        a.nprobe = a.nprobe or [32, 1024]
        a.queries = a.queries or [256]
        recall(a)
    else:
        a.queries = a.queries or [16]
        order(a)
