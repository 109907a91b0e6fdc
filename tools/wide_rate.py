"""Wide top-k rate on the GPU box: MipsIndex.search_wide against a torch yardstick on the same GPU in the same run.

Index 2^20 x 768 bf16 (synthetic Gaussian), device tensors, nq in {64, 4096}, k in {32, 100, 1000}.  Per point:
  wide      search_wide(q, k)                                                       (HIP events, warm-up, alternating)
  torch     torch.topk over bf16 q @ x.T computed in column chunks, the partial top-k merged by one more topk
            (same GEMM FLOPs; it also writes, re-reads and sorts a score matrix)
and once per nq the second yardstick, recorded without a threshold: search(q, 29), the K' = 32 list scan.
Also printed: flagged queries and the whole search's GEMM FLOP/s as a share of the bf16 MFMA peak (an end-to-end figure; the
scan kernel's own share comes from its time in a rocprofv3 --kernel-trace --stats run of this script).
    python tools/wide_rate.py [--rows 1048576 --dim 768 --reps 5 --out profiles/wide_k/wide_rate.jsonl]

--parts P measures the exchange step of the row-sharded wide search instead: the index is cut into P row shards (shard_bounds),
all on this GPU; per (nq, k) every shard runs search_wide_packed, the payloads are concatenated as the all-gather would deliver
them, and the merge for sorted lists (merge_topk_sorted_packed) is timed against the counting merge (merge_topk_packed) on that
same payload, alternating, with the same HIP-event median; the two outputs must be equal.
    python tools/wide_rate.py --parts 8 --queries 4096 --ks 30 100 [--out profiles/wide_k/merge_rate.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import retrieval_augmented_mds_amd as ram

BF16_DENSE_PEAK = 2.5e15  # MI355X bf16 MFMA, FLOP/s (dense)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--queries", type=int, nargs="*", default=[64, 4096])
ap.add_argument("--ks", type=int, nargs="*", default=[32, 100, 1000])
ap.add_argument("--chunk", type=int, default=1 << 17, help="columns of the score matrix per torch.topk")
ap.add_argument("--parts", type=int, default=0, help="P > 0: time the sharded exchange step's merge kernels on P row shards")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("wide_rate.py measures on the GPU; none is visible")

if a.parts <= 0:
    ix = ram.MipsIndex(a.dim)
    ix.add_synthetic(a.rows, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
    x = torch.from_numpy(ix.rows_bf16().view("int16")).cuda().view(torch.bfloat16)  # the stored rows, as torch sees them


def torch_topk(q, k):
    best_s = best_i = None
    for c0 in range(0, a.rows, a.chunk):
        s = q @ x[c0:c0 + a.chunk].T
        ps, pi = torch.topk(s, min(k, s.shape[1]), dim=1)
        pi = pi + c0
        if best_s is None:
            best_s, best_i = ps, pi
        else:
            cs, ci = torch.cat([best_s, ps], 1), torch.cat([best_i, pi], 1)
            best_s, sel = torch.topk(cs, k, dim=1)
            best_i = torch.gather(ci, 1, sel)
    return best_s, best_i


def timed(fn, reps):
    """median of `reps` HIP-event times, ms"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return sorted(out)[len(out) // 2], out


def merge_rates():
    """--parts: per (nq, k) the shards' search_wide_packed times and the two merges on the concatenated payload"""
    shards = []
    for r in range(a.parts):
        lo, hi = ram.shard_bounds(a.rows, a.parts, r)
        sh = ram.MipsIndex(a.dim)
        sh.add_synthetic(hi - lo, lo, ram.SEED_DOCS, ram.SYNTH_GAUSS)
        shards.append((lo, sh))
    out = []
    for nq in a.queries:
        q = ram.synth_fill(nq, a.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="bf16")
        for k in a.ks:
            payload, shard_ms, flagged = [], [], 0
            for lo, sh in shards:
                payload.append(sh.search_wide_packed(q, k, idx_offset=lo))   # (warm-up; the payload is this call's)
                torch.cuda.synchronize()
                flagged += sh.margin_stats()["flagged"]
                shard_ms.append(timed(lambda: sh.search_wide_packed(q, k, idx_offset=lo), a.reps)[0])
            gathered = torch.cat(payload, 0)
            del payload
            new = ram.merge_topk_sorted_packed(gathered, nq, a.parts, k)
            old = ram.merge_topk_packed(gathered, nq, a.parts, k)
            torch.cuda.synchronize()
            equal = bool(torch.equal(new[1], old[1]) and torch.equal(new[0].view(torch.int32), old[0].view(torch.int32)))
            tn, to = [], []
            for _ in range(a.reps):              # alternating, so that drift hits both
                tn.append(timed(lambda: ram.merge_topk_sorted_packed(gathered, nq, a.parts, k), 1)[0])
                to.append(timed(lambda: ram.merge_topk_packed(gathered, nq, a.parts, k), 1)[0])
            mn, mo = sorted(tn)[len(tn) // 2], sorted(to)[len(to) // 2]
            out.append({"what": "sorted merge vs counting merge", "parts": a.parts, "nq": nq, "k": k, "sorted_merge_ms": mn,
                        "counting_merge_ms": mo, "sorted_over_counting": mn / mo, "outputs_equal": equal, "sorted_ms_all": tn,
                        "counting_ms_all": to, "shard_search_wide_packed_ms": shard_ms, "flagged_over_shards": flagged,
                        "payload_bytes_per_rank": nq * k * 16})
            print(json.dumps(out[-1]), flush=True)
            if not equal:
                raise SystemExit("the two merges disagree")
    return out


lines = merge_rates() if a.parts > 0 else []
for nq in a.queries if a.parts <= 0 else []:
    q = ram.synth_fill(nq, a.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="bf16")
    ix.search(q, 29)
    torch.cuda.synchronize()
    t29, _ = timed(lambda: ix.search(q, 29), a.reps)
    lines.append({"what": "search k=29 (K'=32 lists)", "nq": nq, "ms": t29, "kernel": ix.last_kernel})
    print(json.dumps(lines[-1]), flush=True)
    for k in a.ks:
        ws, wi = ix.search_wide(q, k)       # warm-up of both sides, and the agreement of their index sets
        ts, ti = torch_topk(q, k)
        torch.cuda.synchronize()
        st = ix.margin_stats()
        agree = float((torch.sort(wi, 1).values == torch.sort(ti, 1).values).float().mean())
        tw, tt = [], []
        for _ in range(a.reps):              # alternating, so that drift hits both
            tw.append(timed(lambda: ix.search_wide(q, k), 1)[0])
            tt.append(timed(lambda: torch_topk(q, k), 1)[0])
        mw, mt = sorted(tw)[len(tw) // 2], sorted(tt)[len(tt) // 2]
        flop = 2.0 * nq * a.rows * a.dim
        lines.append({"what": "wide vs torch", "nq": nq, "k": k, "wide_ms": mw, "torch_ms": mt, "wide_over_torch": mw / mt,
                      "meets_bar": bool(mw <= mt), "wide_ms_all": tw, "torch_ms_all": tt, "flagged": st["flagged"],
                      "unresolved": st["unresolved"], "index_set_agreement_with_torch": agree,
                      "whole_search_share_of_bf16_peak": flop / (mw * 1e-3) / BF16_DENSE_PEAK, "kernel": ix.last_kernel})
        print(json.dumps(lines[-1]), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
