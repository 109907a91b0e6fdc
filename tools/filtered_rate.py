"""Filtered wide top-k rate on the GPU box: MipsIndex.search_wide(q, k, selector=...) against the unfiltered search_wide of the
same index in the same run (the yardstick: the code path of a call without a selector).

Index 2^20 x 768 bf16 (synthetic Gaussian), device tensors, nq in {64, 4096}, k = 100.  Per nq, alternating so that drift hits
every variant, the median of --reps HIP-event times of
  unfiltered   search_wide(q, k)
  ones         every row selected                      (what the masked instance costs when it cannot skip anything)
  half         Bernoulli(1/2) rows                     (no tile is empty: the cost of masking the epilogue)
  1/64         Bernoulli(1/64) rows                    (about one tile in eight is empty)
  range 1/8    rows [3/8 n, 1/2 n)                     (seven tiles in eight are empty: what tile skipping saves)
and the ratio to the unfiltered time; also the flagged counts, and a check that "ones" returns the unfiltered result bit for bit.
    python tools/filtered_rate.py [--rows 1048576 --dim 768 --reps 7 --md profiles/filtered/README.md]"""
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
ap.add_argument("--queries", type=int, nargs="*", default=[64, 4096])
ap.add_argument("--md", default="", help="write the table as Markdown to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("filtered_rate.py measures on the GPU; none is visible")

n = a.rows
ix = ram.MipsIndex(a.dim)
ix.add_synthetic(n, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
gen = torch.Generator(device="cuda").manual_seed(1)
u = torch.rand(n, device="cuda", generator=gen)
selectors = {
    "unfiltered": None,
    "ones": ram.Selector.from_range(0, n, n),
    "half": ram.Selector.from_mask(u < 0.5),
    "1/64": ram.Selector.from_mask(u < 1.0 / 64),
    "range 1/8": ram.Selector.from_range(3 * n // 8, n // 2, n),
}


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
    warm, flagged = {}, {}
    for name, sel in selectors.items():     # warm-up (scratch allocation) and the statistics of each variant
        warm[name] = ix.search_wide(q, a.k, selector=sel)
        torch.cuda.synchronize()
        flagged[name] = ix.margin_stats()
    same = bool(torch.equal(warm["ones"][1], warm["unfiltered"][1]) and
                torch.equal(warm["ones"][0].view(torch.int32), warm["unfiltered"][0].view(torch.int32)))
    times = {name: [] for name in selectors}
    for _ in range(a.reps):
        for name, sel in selectors.items():
            times[name].append(timed(lambda: ix.search_wide(q, a.k, selector=sel)))
    med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    for name, sel in selectors.items():
        lines.append({"nq": nq, "k": a.k, "rows": n, "dim": a.dim, "selector": name, "selected_rows": n if sel is None else sel.count(),
                      "ms": med[name], "over_unfiltered": med[name] / med["unfiltered"], "ms_all": times[name],
                      "flagged": flagged[name]["flagged"], "unresolved": flagged[name]["unresolved"],
                      "ones_equals_unfiltered": same})
        print(json.dumps(lines[-1]), flush=True)
    if not same:
        raise SystemExit("the all-ones selector and the unfiltered search disagree")

if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("# Filtered wide top-k: times against the unfiltered search\n\n")
        f.write(f"`python tools/filtered_rate.py --md {a.md}` on one MI355X: index {n} x {a.dim} bf16 (synthetic Gaussian), k = {a.k}, "
                f"device tensors, median of {a.reps} HIP-event times per variant, the variants alternating within a repetition.  "
                "The unfiltered `search_wide` of the same run is the yardstick (a call without a selector takes the code path it "
                "took before selectors existed).\n\n")
        f.write("| queries | selector | selected rows | ms | ratio to unfiltered | flagged | all times (ms) |\n|---|---|---|---|---|---|---|\n")
        for ln in lines:
            f.write(f"| {ln['nq']} | {ln['selector']} | {ln['selected_rows']} | {ln['ms']:.3f} | {ln['over_unfiltered']:.3f} | {ln['flagged']} | "
                    f"{', '.join(f'{t:.3f}' for t in ln['ms_all'])} |\n")
        f.write("\nThe all-ones selector returned the unfiltered result bit for bit in every row of the table "
                "(the script stops otherwise); `unresolved` was 0 throughout.\n")
