"""What the group filter costs in the one-launch hook search (GPU box), at BASELINE config 1's shape: N = 10 000 rows, d = 768,
B = 8 queries, k = 5, on a bf16 and an f32 index, row labels row // 4 (an `aid` column of four rows per article), exclude mode.
One process; every variant is timed with HIP events around blocks of back-to-back calls, the variants ALTERNATE block by block,
and the figure per variant is the median of its blocks with their minimum and maximum:
    ungrouped   MipsIndex.search_fused(q, 5)                          the call as it was
    grouped     MipsIndex.search_fused(q, 5, groups=labels)           one launch under the rule
    wide        MipsIndex.search_wide(q, 5, groups=labels)[:, :5]     device-resident, the route the grouped call replaces
    host        Mips.search(q_numpy, k=5, ignore_groups=aids)         NumPy in, lists out (it synchronises)
usage: python tools/hook_group_rate.py [--rounds 31] [--calls 100] [--ungrouped-only]
--ungrouped-only times the first variant alone, with nothing this tool needs beyond search_fused(q, k): run on another build of
the library it gives the yardstick for "the ungrouped call is unchanged".  One JSON line per index."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import retrieval_augmented_mds_amd as ram

N, D, B, K = 10000, 768, 8, 5


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
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--ungrouped-only", action="store_true")
    args = ap.parse_args()
    for dtype in ("bf16", "f32"):
        rng = np.random.default_rng(0xD0C5)
        x = rng.standard_normal((N, D)).astype(np.float32)
        q = rng.standard_normal((B, D)).astype(np.float32)
        if dtype == "bf16":  # (bf16 values, as the synthetic workloads; the f32 index keeps rows that are not)
            x = torch.from_numpy(x).bfloat16().float().numpy()
            q = torch.from_numpy(q).bfloat16().float().numpy()
        qd = torch.from_numpy(q).cuda()
        rec = {"workload": f"{N}x{D} {dtype} index, B={B}, k={K}, labels row // 4, exclude mode", "rounds": args.rounds, "calls_per_block": args.calls}
        if args.ungrouped_only:
            ix = ram.MipsIndex(D, dtype=dtype)
            ix.add(x)
            variants = {"ungrouped": lambda: ix.search_fused(qd, K)}
            kernels = {}
        else:
            aid = [f"a{r // 4:05d}" for r in range(N)]
            q_aid = [aid[(977 * j) % N] for j in range(B)]
            m = ram.Mips(ram.MipsArgs(mips_topk=K, mips_metric_type=0, mips_normalize=False, mips_index_dtype=dtype),
                         data={"mips_column": [""] * N, "aid": aid})
            m.build_index(x)
            ix = m._index()
            m.search(q, k=K, ignore_groups=q_aid)  # sets the groups (labels row // 4) on first use
            labels = torch.from_numpy(m.embeddings.group_codes(m.index_name, q_aid, "exclude")).cuda()
            assert np.array_equal(ix.labels(), np.arange(N) // 4)
            variants = {
                "ungrouped": lambda: ix.search_fused(qd, K),
                "grouped": lambda: ix.search_fused(qd, K, groups=labels),
                "wide": lambda: tuple(t[:, :K] for t in ix.search_wide(qd, K, groups=labels)),
                "host": lambda: m.search(q, k=K, ignore_groups=q_aid),
            }
            kernels = {}
            a = variants["grouped"]()
            b = variants["wide"]()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), "the two grouped routes differ"
        for name, fn in variants.items():  # warm-up: code objects, scratch, first-use allocations
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            kernels[name] = ix.last_kernel
            rec.setdefault("margin", {})[name] = ix.margin_stats()
        t = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t[name].append(block_ms(fn, args.calls if name != "host" else max(1, args.calls // 10)))
        rec["kernel"] = kernels
        rec["ms_per_call"] = {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}
        if not args.ungrouped_only:
            med = {name: rec["ms_per_call"][name]["median"] for name in variants}
            rec["ratio_grouped_over_ungrouped"] = med["grouped"] / med["ungrouped"]
            rec["ratio_wide_over_grouped"] = med["wide"] / med["grouped"]
            rec["ratio_host_over_grouped"] = med["host"] / med["grouped"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
