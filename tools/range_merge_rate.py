"""Rate of the range-search merge of row shards on the GPU box, and the sharded range search end to end.

Merge: synthetic records of `--parts` shards and `--queries` queries holding about `--hits` hits in total, spread evenly over the
queries ("uniform") or all in ONE query ("one-hot": the load a source-major copy must balance).  Per point, alternating in one run:
  merge     mips_range_merge_records into tensors of the exact size: the lims kernel and the copy kernel      (HIP events)
  copy      the yardstick: device-to-device copy_ of the same 12 bytes per hit (float32 scores + int64 ids)  (HIP events)
The merge reads 12 B and writes 12 B per hit like the copy, plus parts * (nq + 1) lims and parts * nq workspace words.
End to end (--e2e): ShardedMipsIndex.range_search on 2 gloo ranks sharing cuda:0 against MipsIndex.range_search on the unsharded
index of the same run, 2^17 x 768 rows, 4096 queries, ~100 hits per query; host clock ending in a synchronise.  Under gloo the
records are staged through the host, which an RCCL group does not do: that run belongs to a multi-GPU machine.
No target is fixed for any of this.
    python tools/range_merge_rate.py [--parts 8 --queries 4096 --hits 1000000 10000000 --reps 9 --e2e --out profiles/range_sharded/range_merge_rate.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import retrieval_augmented_mds_amd as ram


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def records(parts, nq, total, one_hot):
    """-> (gathered CUDA int64, stride, exact total): per-(part, query) counts total / (parts * nq) each, or total / parts in
    query nq / 2 alone; ids ascending per part, random scores."""
    counts = torch.zeros((parts, nq), dtype=torch.int64)
    if one_hot:
        counts[:, nq // 2] = total // parts
    else:
        counts[:] = total // (parts * nq)
        counts[:, : (total // parts) % nq] += 1
    stride = int(counts.sum(1).max())
    words = ram._lib.range_record_words(nq, stride)
    g = torch.empty(parts * words, dtype=torch.int64, device="cuda")
    for p in range(parts):
        lims, D, I = ram.sharded.range_record_views(g[p * words:(p + 1) * words], nq, stride)
        lims.copy_(torch.cat((torch.zeros(1, dtype=torch.int64), counts[p].cumsum(0))))
        D.normal_()
        I.copy_(torch.arange(stride, device="cuda") + (p << 34))
    return g, stride, int(counts.sum())


def merge_rates(a):
    lines = []
    for total in a.hits:
        for one_hot in (False, True):
            g, stride, n = records(a.parts, a.queries, total, one_hot)
            lims = torch.empty(a.queries + 1, dtype=torch.int64, device="cuda")
            D, I = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
            D2, I2 = torch.empty_like(D), torch.empty_like(I)

            def merge():
                ram.range_merge_records(g, a.parts, a.queries, stride, out=(lims, D, I))

            def copy():
                D2.copy_(D)
                I2.copy_(I)

            for _ in range(3):                                   # warm-up of both sides
                merge()
                copy()
            torch.cuda.synchronize()
            assert int(lims[-1]) == n and bool((I[1:] != I[:-1]).all())
            tm, tc = [], []
            for _ in range(a.reps):                              # alternating, so that drift hits both
                tm.append(timed(merge))
                tc.append(timed(copy))
            lines.append({"what": "merge vs copy_", "parts": a.parts, "nq": a.queries, "hits": n, "distribution": "one-hot" if one_hot else "uniform",
                          "merge_ms": median(tm), "copy_ms": median(tc), "merge_over_copy": median(tm) / median(tc),
                          "merge_GBps_read_plus_write": 24e-6 * n / median(tm), "merge_ms_all": tm, "copy_ms_all": tc})
            print(json.dumps(lines[-1]), flush=True)
            del g, D, I, D2, I2
    return lines


def _e2e_rank(rank, world, port, a, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        n, d, nq = a.e2e_rows, a.dim, a.queries
        sh = ram.ShardedMipsIndex(d, device=0)
        sh.add_synthetic_global(n, ram.SEED_DOCS, ram.SYNTH_GAUSS)
        full = ram.MipsIndex(d, device=0)                        # every rank builds it: the radii must be the same everywhere
        full.add_synthetic(n, 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
        q = ram.synth_fill(nq, d, 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS, dtype="bf16")
        r = full.search_wide(q, 101)[0][:, 100].contiguous().cpu().numpy()     # ~100 hits per query
        ref = full.range_search(q, r)
        got = sh.range_search(q, r)                              # warm-up of both sides
        same = all(bool(torch.equal(u, v)) for u, v in zip(ref, got))
        ts, tf = [], []
        for _ in range(a.reps):
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sh.range_search(q, r)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            dist.barrier()
            if rank == 0:                                        # alone on the GPU, like the sharded call's ranks are not
                t0 = time.perf_counter()
                full.range_search(q, r)
                torch.cuda.synchronize()
                tf.append((time.perf_counter() - t0) * 1e3)
        ret[rank] = {"what": "sharded range_search end to end (gloo, ranks share one GPU)", "world": world, "rank": rank, "rows": n, "dim": d,
                     "nq": nq, "hits": int(ref[0][-1]), "equal_to_unsharded": same, "sharded_ms": median(ts), "sharded_ms_all": ts,
                     "unsharded_ms": median(tf) if tf else None, "unsharded_ms_all": tf}
    finally:
        dist.destroy_process_group()


def end_to_end(a):
    import torch.multiprocessing as mp

    ret = mp.Manager().dict()
    mp.spawn(_e2e_rank, args=(2, 29400 + os.getpid() % 500, a, ret), nprocs=2, join=True)
    lines = [ret[r] for r in sorted(ret.keys())]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--hits", type=int, nargs="*", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--e2e", action="store_true", help="also time ShardedMipsIndex.range_search on 2 gloo ranks")
    ap.add_argument("--e2e-rows", type=int, default=1 << 17)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("range_merge_rate.py measures on the GPU; none is visible")
    lines = merge_rates(a)
    if a.e2e:
        torch.cuda.empty_cache()
        lines += end_to_end(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
