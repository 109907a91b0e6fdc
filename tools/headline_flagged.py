"""Flagged queries per step of the headline workload (bench.py's defaults: 2^20 x 768 bf16 rows, Q = 4096, k = 5, device
outputs): bench.py reads mips_index_margin_stats once, after its last step; this reads it after EVERY step (which
synchronises, so nothing here is a timing).  One JSON line: the counts, their mean, the kernel.
    python tools/headline_flagged.py [--steps 20 --warmup 3 --rows N --queries Q --dim D --k K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=5)
    args = ap.parse_args()

    import torch

    import retrieval_augmented_mds_amd as ram

    index = ram.ShardedMipsIndex(args.dim, metric=ram.METRIC_IP, dtype="bf16", device=0)
    index.add_synthetic_global(args.rows, ram.SEED_DOCS, ram.SYNTH_GAUSS)
    q = ram.synth_fill(args.queries, args.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="bf16", device=0)
    for _ in range(max(1, args.warmup)):
        index.search(q, args.k)
    torch.cuda.synchronize()
    flagged, unresolved = [], 0
    for _ in range(args.steps):
        index.search(q, args.k)
        st = index.margin_stats(synchronize=True)
        flagged.append(int(st["flagged"]))
        unresolved += int(st["unresolved"])
    index.check()
    print(json.dumps({"workload": f"{args.rows}x{args.dim} bf16, Q={args.queries}, k={args.k}", "kernel": index.local.last_kernel,
                      "steps": args.steps, "flagged_per_step": flagged, "flagged_mean": sum(flagged) / len(flagged),
                      "unresolved_total": unresolved}), flush=True)


if __name__ == "__main__":
    main()
