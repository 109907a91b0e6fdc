"""Grouped wide top-k rate on the GPU box: MipsIndex.search_wide(q, k, groups=...) against the unfiltered search_wide and the
all-ones masked search of the same index IN THE SAME RUN (the two yardsticks: the code path of a call without any filter, and the
masked instance the grouped one is built on).

Index 2^20 x 768 bf16 (synthetic Gaussian), device tensors, nq in {64, 4096}, k = 100; row labels row // 4 (groups of 4 rows), every
query a member of one group.  Per nq, alternating so that drift hits every variant, the median of --reps HIP-event times of
  unfiltered        search_wide(q, k)
  ones              selector with every row set           (masked_scan_kernel when it cannot skip anything)
  exclude           groups=, exclude mode                 (4 rows per query are left out: the steady state of the append-site test)
  only              groups=, only mode                    (4 rows per query are admitted: tau stays -inf, every block passes)
  exclude + half    exclude mode on top of a Bernoulli(1/2) bitmap
and the ratios to both yardsticks; also the flagged counts, and a check that all-NONE query labels return the unfiltered result.
    python tools/grouped_rate.py [--rows 1048576 --dim 768 --reps 7 --md profiles/grouped/times.md]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import retrieval_augmented_mds_amd as ram

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--group", type=int, default=4, help="rows per group")
ap.add_argument("--queries", type=int, nargs="*", default=[64, 4096])
ap.add_argument("--md", default="", help="write the table as Markdown to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("grouped_rate.py measures on the GPU; none is visible")

n = a.rows
ix = ram.MipsIndex(a.dim)
ix.add_synthetic(n, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
ix.set_labels(torch.arange(n, device="cuda", dtype=torch.int32) // a.group)
ngroups = (n + a.group - 1) // a.group
gen = torch.Generator(device="cuda").manual_seed(1)
ones = ram.Selector.from_range(0, n, n)
half = ram.Selector.from_mask(torch.rand(n, device="cuda", generator=gen) < 0.5)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


lines = []
for nq in a.queries:
    q = ram.synth_fill(nq, a.dim, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="bf16")
    ql = (torch.arange(nq, device="cuda", dtype=torch.int64) * 7919 % ngroups).to(torch.int32)   # every query a member of one group
    none = torch.full((nq,), ram.LABEL_NONE, device="cuda", dtype=torch.int32)
    variants = {
        "unfiltered": {},
        "ones": {"selector": ones},
        "exclude": {"groups": ql, "group_mode": "exclude"},
        "only": {"groups": ql, "group_mode": "only"},
        "exclude + half": {"groups": ql, "group_mode": "exclude", "selector": half},
    }
    warm, flagged, kernel = {}, {}, {}
    for name, kw in variants.items():     # warm-up (scratch allocation) and the statistics of each variant
        warm[name] = ix.search_wide(q, a.k, **kw)
        torch.cuda.synchronize()
        flagged[name] = ix.margin_stats()
        kernel[name] = ix.last_kernel
    free = ix.search_wide(q, a.k, groups=none)
    same = bool(torch.equal(free[1], warm["unfiltered"][1]) and torch.equal(free[0].view(torch.int32), warm["unfiltered"][0].view(torch.int32)))
    times = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, kw in variants.items():
            times[name].append(timed(lambda: ix.search_wide(q, a.k, **kw)))
    med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    for name in variants:
        lines.append({"nq": nq, "k": a.k, "rows": n, "dim": a.dim, "group_rows": a.group, "variant": name, "kernel": kernel[name],
                      "ms": med[name], "over_unfiltered": med[name] / med["unfiltered"], "over_ones": med[name] / med["ones"],
                      "ms_min": min(times[name]), "ms_max": max(times[name]), "ms_all": times[name],
                      "flagged": flagged[name]["flagged"], "unresolved": flagged[name]["unresolved"], "none_equals_unfiltered": same})
        print(json.dumps(lines[-1]), flush=True)
    if not same:
        raise SystemExit("all-NONE query labels and the unfiltered search disagree")

if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write(f"Index {n} x {a.dim} bf16 (synthetic Gaussian), k = {a.k}, groups of {a.group} rows, device tensors, median of {a.reps} "
                "HIP-event times per variant, the variants alternating within a repetition.\n\n")
        f.write("| queries | variant | ms | min .. max | ratio to unfiltered | ratio to ones | flagged |\n|---|---|---|---|---|---|---|\n")
        for ln in lines:
            f.write(f"| {ln['nq']} | {ln['variant']} | {ln['ms']:.3f} | {ln['ms_min']:.3f} .. {ln['ms_max']:.3f} | {ln['over_unfiltered']:.3f} | "
                    f"{ln['over_ones']:.3f} | {ln['flagged']} |\n")
