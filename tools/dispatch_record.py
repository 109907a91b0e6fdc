"""Dispatch record (GPU box): which kernel answers which mips_search call, what the margin check counted, and a hash of the result.

Walks a fixed list of calls over small indexes (3001 rows: ragged against the 32-, 64- and 128-row blocks) that covers the
thresholds the host dispatch branches on -- storage, row pitch, k, query count, output form, "margin_check", "f32_fast",
"variant", "resolve", "resolve_budget", the fast_skip countdown and the pool of 16 at pitch 1024 on a large index -- and prints
one JSON line per call: {"call", "kernel", "stats", "sha256"}.  Only the public Python API is used, so the same file runs on
any revision: a host-side refactor must reproduce the output line for line.  tests/dispatch_record.json holds the "kernel" and
"stats" columns (tests/test_gpu_dispatch_record.py replays the list against it); a dispatch change edits that file on purpose:
usage: python tools/dispatch_record.py [--write tests/dispatch_record.json] [--only small|large]"""
import argparse, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import retrieval_augmented_mds_amd as ram

ROWS = 3001
DEFAULTS = {"margin_check": 1, "f32_fast": 1, "variant": 0, "resolve": 1, "resolve_budget": 0, "tiny": 1}
FP8_D = (256, 512, 768, 1024)
DS = (64, 320, 256, 512, 768, 1024)
KS = (1, 5, 7, 8, 13, 14, 29)
NQS = (8, 16, 17, 64, 65, 256, 257)


def call(storage, d, k, nq, out="host", data="gauss", metric=0, rows=ROWS, fused=None, keep_state=False, **params):
    return {"storage": storage, "d": d, "k": k, "nq": nq, "out": out, "data": data, "metric": metric, "rows": rows, "fused": fused,
            "keep_state": keep_state, "params": params}


def label(c):
    s = f"{c['storage']} d={c['d']} {c['data']} rows={c['rows']} k={c['k']} nq={c['nq']} {c['out']}"
    if c["metric"]:
        s += " L2"
    if c["fused"]:
        s += f" fused:{c['fused']}"
    if c["keep_state"]:
        s += " (sequence)"
    return s + "".join(f" {n}={v}" for n, v in sorted(c["params"].items()))


def small_calls():
    L = []
    # storage x row pitch
    for st in ("bf16", "f32", "fp8_e4m3", "fp8_e4m3_docs"):
        for d in (DS if st in ("bf16", "f32") else FP8_D):
            L.append(call(st, d, 5, 64))
    # k: the pools of 8 / 10 / 16 / 32, optimistic or not
    for st, d in (("bf16", 768), ("f32", 768)):
        L += [call(st, d, k, 64) for k in KS]
    L += [call("fp8_e4m3_docs", 512, k, 64) for k in (1, 8, 14, 29)]
    L += [call("fp8_e4m3", 512, k, 64) for k in (1, 7, 8, 13)]
    # query count: the one-launch kernel, one query tile / several, 256 < nq at pitch 1024
    for st, d, k in (("bf16", 768, 5), ("bf16", 1024, 5), ("bf16", 1024, 10), ("f32", 1024, 5), ("fp8_e4m3_docs", 768, 5)):
        L += [call(st, d, k, nq, "device") for nq in NQS]
    L += [call("bf16", 1024, 10, nq) for nq in (256, 257)]
    # output forms
    for st, d, k in (("bf16", 768, 5), ("bf16", 768, 10), ("f32", 768, 5)):
        L += [call(st, d, k, 65, out) for out in ("device", "packed", "split")]
    # L2 metric
    L += [call("bf16", 768, 5, 64, out, metric=1) for out in ("host", "device")]
    L += [call("f32", 768, 5, 64, out, metric=1) for out in ("host", "device")]
    # the knobs, on rows whose near-duplicates get queries flagged
    for st, k in (("bf16", 10), ("f32", 5)):
        for out in ("host", "device"):
            L += [call(st, 768, k, 64, out, "dups", margin_check=m) for m in (0, 1, 2, 4)]
            L += [call(st, 768, k, 64, out, "dups", f32_fast=f) for f in (0, 1, 2)]
            L += [call(st, 768, k, 64, out, "dups", resolve=r) for r in (0, 1)]
            L.append(call(st, 768, k, 64, out, "dups", resolve_budget=1))
    L += [call("bf16", 768, 5, 64, out, "dups", resolve_budget=1) for out in ("host", "device", "split")]
    L.append(call("bf16", 768, 10, 64, "device", "dups", resolve=0, margin_check=2))
    # forced kernels
    L += [call("bf16", 768, 5, 130, "device", variant=v) for v in (0, 1, 3, 4, 7)]
    L += [call("bf16", 1024, 5, 64, "device", variant=v) for v in (0, 1, 3, 4, 7)]
    L += [call("bf16", 768, 10, 64, "host", "dups", variant=v) for v in (0, 1, 3, 4, 7)]
    L += [call("fp8_e4m3", 512, 5, 64, "host", variant=v) for v in (0, 3)]
    L += [call("f32", 768, 5, 64, "host", variant=v) for v in (1, 3)]
    # the one-launch kernel switched off, and the fused hook call in both its forms
    L += [call(st, 768, 5, 8, "device", tiny=0) for st in ("bf16", "f32")]
    L += [call("bf16", 768, 5, 8, "device", fused="ignore"), call("bf16", 768, 5, 64, "device", fused="ignore"),
          call("f32", 768, 5, 8, "device", fused="normalize")]
    # the fast_skip countdown: a synchronising call that flags >= 64 queries and more than an eighth arms it, the next 8 skip the
    # optimistic scan, the 9th takes it again
    for st, k in (("bf16", 10), ("f32", 5)):
        L.append(call(st, 768, k, 256, "host", "dups"))
        L += [call(st, 768, k, 256, "host", "dups", keep_state=True) for _ in range(10)]
    return L


def large_calls():
    # bf16 rows at pitch 1024, k <= 5, nq > 256, >= 2^21 rows, a call that certifies: the pool of 16
    return [call("bf16", 1024, 5, 257, "host", rows=1 << 21)]


_indexes = {}


def _dups(d, rows, nq, seed):
    """clusters of 40 near-duplicates (within a bf16 ulp or two of each other) and queries near the centres"""
    rng = np.random.default_rng(seed)
    nc = (rows + 39) // 40
    c = rng.standard_normal((nc, d)).astype(np.float32)
    x = np.repeat(c, 40, axis=0)[:rows]
    x = (x * (1.0 + 5e-4 * rng.standard_normal(x.shape))).astype(np.float32)
    q = (c[rng.integers(0, nc, nq)] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    return x, q


def get_index(c):
    key = (c["storage"], c["d"], c["data"], c["metric"], c["rows"])
    if key not in _indexes:
        if c["rows"] != ROWS:
            _indexes.clear()  # (a large index: the small ones go first)
        ix = ram.MipsIndex(c["d"], metric=c["metric"], dtype=c["storage"])
        if c["data"] == "dups":
            x, q = _dups(c["d"], c["rows"], 257, seed=c["d"] + 7)
            ix.add(x)
        elif c["storage"] == "f32":  # rows and queries that are NOT bf16 values (the synthetic generator emits bf16 values)
            rng = np.random.default_rng(c["d"] + 11)
            ix.add(rng.standard_normal((c["rows"], c["d"])).astype(np.float32))
            q = rng.standard_normal((257, c["d"])).astype(np.float32)
        else:
            ix.add_synthetic(c["rows"], 0, ram.SEED_DOCS, ram.SYNTH_GAUSS)
            q = ram.synth_fill(257, c["d"], 0, ram.SEED_QUERIES, ram.SYNTH_GAUSS).float().cpu().numpy()
        _indexes[key] = (ix, q, torch.from_numpy(q).cuda())
    return _indexes[key]


def run(c):
    ix, q_host, q_dev = get_index(c)
    nq, k, out = c["nq"], c["k"], c["out"]
    if not c["keep_state"]:  # every knob at its default (setting "f32_fast" clears the fast_skip countdown), then the call's own
        for name, value in {**DEFAULTS, **c["params"]}.items():
            ix.set_param(name, value)
    if c["fused"] == "ignore":
        res = ix.search_fused(q_dev[:nq], k, ignore=torch.arange(nq, device="cuda"))
    elif c["fused"] == "normalize":
        res = ix.search_fused(q_dev[:nq], k, normalize=True)
    elif out == "host":
        res = ix.search(q_host[:nq], k)
    elif out == "device":
        res = ix.search(q_dev[:nq], k)
    elif out == "packed":
        res = (ix.search_packed(q_dev[:nq], k),)
    else:  # split tail: select + exact re-score on a stream of their own
        tail = torch.cuda.Stream()
        res = ix.search(q_dev[:nq], k, tail_stream=tail)
        tail.synchronize()
    torch.cuda.synchronize()
    kernel, stats = ix.last_kernel, ix.margin_stats()
    h = hashlib.sha256()
    for a in res:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return {"call": label(c), "kernel": kernel, "stats": stats, "sha256": h.hexdigest()}


def record(which=("small", "large")):
    calls = (small_calls() if "small" in which else []) + (large_calls() if "large" in which else [])
    out = [run(c) for c in calls]
    _indexes.clear()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", help="also write the kernel and margin-stats columns to this JSON file")
    ap.add_argument("--only", choices=("small", "large"))
    a = ap.parse_args()
    recs = record((a.only,) if a.only else ("small", "large"))
    for r in recs:
        print(json.dumps(r, sort_keys=True))
    if a.write:
        with open(a.write, "w") as f:
            json.dump([{n: r[n] for n in ("call", "kernel", "stats")} for r in recs], f, indent=1, sort_keys=True)
            f.write("\n")
