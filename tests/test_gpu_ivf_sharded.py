"""The row-sharded IVF index on the GPU: (a) mips_ivf_search_part + mips_ivf_merge_parts over 1, 2 and 3 parts in ONE process against
the unsharded IvfIndex and the NumPy restatement of the unsharded definition -- three storages, k in {1, 5, 29, 30, 100}, nprobe in
{1, 3, >= nlist}, plain / selector / groups (exclude, only) / both --, (b) the range form through part records, (c) ShardedIvfIndex
on ranks that share one GPU over gloo (world 2 and 3, every rank a child process under its own time limit), (d) the refusals and
the one-rank result, (e) the plain-C consumer of the new header.  Expectations come from tests/ivf_sharded_cases.py, which applies
the restatements of tests/ivf_*_cases.py to the UNSHARDED rows; every comparison is bit for bit."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_range_cases as rg  # noqa: E402
import ivf_sharded_cases as shc  # noqa: E402

pytestmark = pytest.mark.gpu

_BUILT = {}


def _index(c, dtype, lo, hi):
    """an IvfIndex over the rows [lo, hi) of the case with the case's centroids, GLOBAL SQ8 range and labels"""
    ix = ram.IvfIndex(c["rows"].shape[1], c["nlist"], dtype=dtype, device=0)
    ix.set_centroids(c["centroids"])
    if dtype == "sq8":
        ix.set_sq8_params(*c["sq8_params"])
    if hi > lo:
        ix.add(c["rows"][lo:hi])
        ix.set_labels(c["row_labels"][lo:hi])
    return ix


def _built(name, dtype):
    """-> (case, the unsharded index, {P: [(lo, hi, part index)]}, device queries, device selector): built once, shared, not modified"""
    key = (name, dtype)
    if key not in _BUILT:
        c = shc.case(name)
        n = len(c["rows"])
        full = _index(c, dtype, 0, n)
        assert np.array_equal(full.assignments(), c["assign"])
        parts = {P: [(lo, hi, _index(c, dtype, lo, hi)) for lo, hi in shc.bounds(n, P)] for P in (1, 2, 3)}
        _BUILT[key] = (c, full, parts, torch.from_numpy(c["q"]).cuda(), ram.Selector.from_mask(c["sel"], device=0))
    return _BUILT[key]


def _kw(c, sel, flt):
    kw = {}
    if flt in ("selector", "both"):
        kw["selector"] = sel
    if flt in ("exclude", "only", "both"):
        kw.update(groups=c["q_labels"], group_mode="only" if flt == "only" else "exclude")
    return kw


def _np(pair):
    return tuple(t.cpu().numpy() for t in pair)


# ------------------------------------------------------------------ (a) part search + merge in one process
@pytest.mark.parametrize("flt", shc.FILTERS)
@pytest.mark.parametrize("dtype", shc.STORAGES)
def test_part_search_and_merge_equal_the_unsharded_index(dtype, flt):
    c, full, parts, qd, sel = _built("planted", dtype)
    nq, nlist = len(c["q"]), c["nlist"]
    kw = _kw(c, sel, flt)
    for k in shc.KS:
        for nprobe in (1, 3, nlist + 2):
            want = shc.expected(c, dtype, k, nprobe, flt)
            ref = _np(full.search_probed_wide(qd, k, nprobe, **kw))
            assert shc.same(ref, want), (k, nprobe, "unsharded index against the restatement")
            if nprobe >= nlist and dtype != "sq8":                          # every list probed: the flat index's exact wide search
                flat = _np(full.flat.search_wide(qd, max(k, 30), **kw))
                assert shc.same((flat[0][:, :k], flat[1][:, :k]), want), (k, "flat.search_wide")
            for P in (1, 2, 3):
                payloads, bias = [], None
                for lo, hi, ix in parts[P]:
                    pk, b = ix.search_part(qd, k, nprobe, idx_offset=lo, sel_bit0=lo if "selector" in kw else 0, **kw)
                    assert pk.shape == (nq, k, 2) and pk.dtype == torch.int64 and (b is None) == (dtype != "sq8")
                    assert bool((pk[..., 0] >> 32 == 0).all())               # the score bits zero-extended
                    if b is not None:
                        assert bias is None or torch.equal(b, bias)          # B_q is the same on every part
                        bias = b
                    payloads.append(pk)
                got = _np(ram.ivf_merge_parts(torch.cat(payloads).contiguous(), P, nq, k, bias))
                assert shc.same(got, want), (k, nprobe, P)
    # the definition's cases in the result: padding that survives the merge, and the ties across the shard borders
    if flt == "plain":
        d, i = shc.expected(c, dtype, 5, 1)
        assert (i[0, 3:] == -1).all() and i[2].tolist() == list(shc.BORDER_COPIES[:5])


@pytest.mark.parametrize("dtype", shc.STORAGES)
@pytest.mark.parametrize("name,P", [("tiny", 3), ("trained", 3), ("768", 2)])
def test_part_search_on_an_empty_part_on_trained_lists_and_at_768_columns(name, P, dtype):
    c, full, parts, qd, sel = _built(name, dtype)
    nq = len(c["q"])
    if name == "tiny":
        assert [ix.ntotal for _, _, ix in parts[3]] == [2, 2, 0]
    for k, nprobe, flt in ((1, 1, "plain"), (5, 2, "both"), (30, c["nlist"], "selector"), (100, 3, "exclude")):
        kw = _kw(c, sel, flt)
        want = shc.expected(c, dtype, k, nprobe, flt)
        assert shc.same(_np(full.search_probed_wide(qd, k, nprobe, **kw)), want)
        payloads, bias = [], None
        for lo, hi, ix in parts[P]:
            pk, bias = ix.search_part(qd, k, nprobe, idx_offset=lo, sel_bit0=lo if "selector" in kw else 0, **kw)
            payloads.append(pk)
        assert shc.same(_np(ram.ivf_merge_parts(torch.cat(payloads).contiguous(), P, nq, k, bias)), want), (name, k, nprobe, flt)
    # the host form of the part search gives the device form's words
    lo, hi, ix = parts[P][0]
    hp, hb = ix.search_part(c["q"], 5, 2, idx_offset=lo)
    dp, db = ix.search_part(qd, 5, 2, idx_offset=lo)
    assert isinstance(hp, np.ndarray) and np.array_equal(hp, dp.cpu().numpy()) and (hb is None or np.array_equal(hb, db.cpu().numpy()))


@pytest.mark.parametrize("P", [2, 3])
def test_sq8_is_merged_on_S_across_parts(P):
    """Rows 1213 and 24 of the tie case have equal D and different S, the higher S at the higher row, and lie in different parts of 3
    (in one part of 2): the merged result keeps the order of S, as the unsharded index does.  A merge on D would put row 24 first."""
    c, full, parts, qd, sel = _built("sq8_tie", "sq8")
    tie, nq, nlist = c["tie"], len(c["q"]), c["nlist"]
    k, j, r = tie["k"], tie["query"], tie["rank"]
    want = shc.expected(c, "sq8", k, nlist)
    assert want[1][j, r:r + 2].tolist() == list(tie["rows"]) and want[0][j, r] == want[0][j, r + 1]
    assert shc.same(_np(full.search_probed_wide(qd, k, nlist)), want)
    payloads, bias = [], None
    for lo, hi, ix in parts[P]:
        pk, bias = ix.search_part(qd, k, nlist, idx_offset=lo)
        payloads.append(pk)
    gathered = torch.cat(payloads).contiguous()
    got = _np(ram.ivf_merge_parts(gathered, P, nq, k, bias))
    assert shc.same(got, want) and got[1][j, r:r + 2].tolist() == list(tie["rows"])
    # the payload carries S: the two entries differ in their score words, and the restatement of the merge agrees
    g = gathered.cpu().numpy().reshape(P, nq, k, 2)
    words = {int(g[p, j, t, 1]): int(g[p, j, t, 0]) for p in range(P) for t in range(k) if int(g[p, j, t, 1]) in tie["rows"]}
    assert len(words) == 2 and words[tie["rows"][0]] != words[tie["rows"][1]]
    assert shc.same(shc.merge_parts(g, P, nq, k, bias.cpu().numpy()), want)


# ------------------------------------------------------------------ (b) the range form through records
@pytest.mark.parametrize("dtype", shc.STORAGES)
def test_part_records_merge_to_the_unsharded_range_result(dtype):
    c, full, parts, qd, sel = _built("planted", dtype)
    nq = len(c["q"])
    for nprobe, flt in ((1, "plain"), (3, "both"), (c["nlist"], "only")):
        kw = _kw(c, sel, flt)
        radii = shc.radii_for(c, dtype, nprobe, flt)
        want = shc.expected_range(c, dtype, radii, nprobe, flt)
        assert rg.same(_np(full.range_search_probed(qd, radii, nprobe, **kw)), want)
        for P in (2, 3):
            stride = max(int(((want[2] >= lo) & (want[2] < hi)).sum()) for lo, hi, _ in parts[P]) + 3
            records = []
            for lo, hi, ix in parts[P]:
                rec = torch.empty(ram._lib.range_record_words(nq, stride), dtype=torch.int64, device="cuda")
                lims, D, I = ram.sharded.range_record_views(rec, nq, stride)
                ix.range_search_probed_into(qd, radii, lims, D, I, nprobe=nprobe, idx_offset=lo, sel_bit0=lo if "selector" in kw else 0, **kw)
                records.append(rec)
            got = ram.range_merge_records(torch.cat(records), P, nq, stride)
            total = int(got[0][-1])
            assert rg.same((got[0].cpu().numpy(), got[1][:total].cpu().numpy(), got[2][:total].cpu().numpy()), want), (nprobe, flt, P)


# ------------------------------------------------------------------ (c) ranks sharing one GPU (gloo)
def _rank_worker(rank, world, port, name, train, tmp, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        c = shc.case(name)
        rows, q = c["rows"], c["q"]
        n, nq, d, nlist = len(rows), len(q), rows.shape[1], c["nlist"]
        qd = torch.from_numpy(q).cuda()
        lo, hi = ram.shard_bounds(n, world, rank)
        planted = not train                                                  # set_trained with the case's planted centroids, or train_global
        tie = c.get("tie")
        for dtype in (("sq8",) if tie else shc.STORAGES):                  # (the tie case is about the SQ8 rule alone)
            sq8 = c["sq8_params"] if dtype == "sq8" else None
            ix = ram.ShardedIvfIndex(d, nlist, dtype=dtype, device=0)
            full = ram.IvfIndex(d, nlist, dtype=dtype, device=0)             # the unsharded index, on every rank
            if planted:
                ix.set_trained(c["centroids"], sq8)
                full.set_centroids(c["centroids"])
                if sq8 is not None:
                    full.set_sq8_params(*sq8)
            else:
                ix.local.niter = full.niter = 2
                ix.train_global(rows)
                full.train(rows)
            cen = ix.centroids()
            assert ix.is_trained and np.array_equal(cen.view(np.uint32), full.centroids().view(np.uint32))
            if dtype == "sq8":
                assert all(np.array_equal(a, b) for a, b in zip(ix.local.flat.sq8_params(), full.flat.sq8_params()))    # the GLOBAL range
            ix.add_global(rows)
            ix.set_labels_global(c["row_labels"])
            full.add(rows)
            full.set_labels(c["row_labels"])
            assert ix.ntotal == n and ix.local.ntotal == hi - lo and (ix.lo, ix.hi) == (lo, hi)
            assert np.array_equal(ix.list_sizes_global(), full.list_sizes())
            if planted:
                case_now = c
            else:                                                           # the restatement on what was trained
                case_now = dict(c, centroids=cen, assign=full.assignments(), sq8_params=full.flat.sq8_params() if dtype == "sq8" else c["sq8_params"])
            kws = {"plain": {}, "selector": {"selector": c["sel"]}, "exclude": {"groups": c["q_labels"], "group_mode": "exclude"},
                   "only": {"groups": c["q_labels"], "group_mode": "only"}, "both": {"selector": c["sel"], "groups": c["q_labels"]}}

            def check_all(ix, full, case_now, what):
                for k, nprobe, flt in ((5, 1, "plain"), (5, 3, "both"), (29, nlist, "selector"), (30, 3, "only"), (100, nlist, "exclude")):
                    fn = ix.search_probed if k <= 29 else ix.search_probed_wide
                    got = fn(qd, k, nprobe, **kws[flt])                      # CUDA in -> CUDA out
                    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
                    ref = _np(full.search_probed_wide(qd, k, nprobe, **kws[flt]))
                    assert shc.same(_np(got), ref), (what, rank, dtype, k, nprobe, flt, "against the unsharded index")
                    assert shc.same(ref, shc.expected(case_now, dtype, k, nprobe, flt)), (what, rank, dtype, k, nprobe, flt, "restatement")
                got = ix.search_probed(q, 5, 3)                              # NumPy in -> NumPy out
                assert all(isinstance(t, np.ndarray) for t in got) and shc.same(got, shc.expected(case_now, dtype, 5, 3))
                for nprobe, flt in ((1, "plain"), (3, "both")):
                    radii = shc.radii_for(case_now, dtype, nprobe, flt)
                    want = shc.expected_range(case_now, dtype, radii, nprobe, flt)
                    got = ix.range_search_probed(qd, radii, nprobe, **kws[flt])
                    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got) and rg.same(_np(got), want), (what, rank, dtype, flt, "range")
                    assert rg.same(ix.range_search_probed(q, radii, nprobe, **kws[flt]), want)
                    total = int(want[0][-1])
                    lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
                    D = torch.empty(total + 3, dtype=torch.float32, device="cuda")
                    I = torch.empty(total + 3, dtype=torch.int64, device="cuda")
                    ix.range_search_probed_into(qd, radii, lims, D, I, part_cap=total + 1, nprobe=nprobe, **kws[flt])
                    assert rg.same((lims.cpu().numpy(), D[:total].cpu().numpy(), I[:total].cpu().numpy()), want)

            check_all(ix, full, case_now, "built")
            if tie:                                                         # equal D, different S on ranks 1 and 0: the order of S, on every rank
                got = _np(ix.search_probed(qd, tie["k"], nlist))
                assert shc.same(got, shc.expected(c, dtype, tie["k"], nlist)) and got[1][tie["query"], tie["rank"]:tie["rank"] + 2].tolist() == list(tie["rows"])
            ids = np.arange(n, dtype=np.int64)
            assert np.array_equal(ix.reconstruct_batch(ids).view(np.uint32), full.reconstruct_batch(ids).view(np.uint32))
            # rows rewritten by id on both sides of every border: they change lists, and the searches follow
            edges = [e for a, b in shc.bounds(n, world) for e in (a, b - 1)]     # (the same ids on every rank)
            upd = np.array(sorted({min(max(e, 0), n - 1) for e in edges} | {n // 2}), dtype=np.int64)
            newx = np.ascontiguousarray(rows[(upd * 7 + 3) % n] * np.float32(0.5) + q[upd % nq])
            ix.update_rows_global(upd, newx)
            full.update_rows(upd, newx)
            rows2 = rows.copy()
            rows2[upd] = newx
            case_upd = dict(case_now, rows=rows2, assign=full.assignments())
            assert np.array_equal(ix.list_sizes_global(), full.list_sizes())
            check_all(ix, full, case_upd, "updated")
            # save / load round trip: every rank its shard
            path = os.path.join(tmp, f"{name}_{dtype}_{world}")
            ix.save(path)
            back = ram.ShardedIvfIndex.load(path, device=0)
            assert back.ntotal == n and (back.lo, back.hi) == (lo, hi) and back.dtype == dtype
            check_all(back, full, case_upd, "loaded")
            # the training checksum: one rank with other centroids, every rank raises
            bad = ram.ShardedIvfIndex(d, nlist, dtype=dtype, device=0)
            other = cen.copy()
            if rank == world - 1:
                other[0, 0] = np.nextafter(other[0, 0], np.float32(2))
            with pytest.raises(RuntimeError, match="different centroids"):
                bad.set_trained(other, full.flat.sq8_params() if dtype == "sq8" else None)
        ret[rank] = True
    finally:
        dist.destroy_process_group()


def _run_ranks(fn, args, world, limit):
    """`world` child processes, each under its own time limit; every exit status is checked, and after a failure the others are
    ended and nothing further is started"""
    import torch.multiprocessing as mp

    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5):                                      # raises as soon as a child failed (and ends the others)
            if time.monotonic() > deadline:
                raise TimeoutError(f"a rank ran past its limit of {limit} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(30)
    assert [p.exitcode for p in ctx.processes] == [0] * world


@pytest.mark.parametrize("world,name,train", [(2, "planted", True), (3, "planted", False), (3, "tiny", False), (3, "sq8_tie", False)])
def test_sharded_ivf_index_on_ranks_sharing_one_gpu(world, name, train, tmp_path):
    """train_global (or set_trained with the planted centroids: the padding and the border ties of the planted case, and the 4-row
    case whose third shard is empty), add_global, search_probed / search_probed_wide /
    range_search_probed (+ _into), update_rows_global followed by the searches, a save / load round trip, reconstruct_batch and the
    checksum refusal, checked on every rank against the unsharded IvfIndex of the same process and the restatement."""
    import torch.multiprocessing as mp

    port = 29600 + (os.getpid() % 2000) + 7 * world + len(name)
    ret = mp.Manager().dict()
    _run_ranks(_rank_worker, (world, port, name, train, str(tmp_path), ret), world, limit=240)
    assert dict(ret) == {r: True for r in range(world)}


# ------------------------------------------------------------------ (d) refusals, one rank
def test_refusals_and_the_one_rank_result():
    c = shc.case("planted")
    n, nq, nlist = len(c["rows"]), len(c["q"]), c["nlist"]
    qd = torch.from_numpy(c["q"]).cuda()
    for dtype in ("bf16", "sq8"):
        ix = ram.ShardedIvfIndex(64, nlist, dtype=dtype, device=0)          # no process group: one rank, the same checks
        with pytest.raises(RuntimeError):
            ix.add_global(c["rows"])                                        # not trained
        ix.set_trained(c["centroids"], c["sq8_params"] if dtype == "sq8" else None)
        ix.add_global(c["rows"])
        ix.set_labels_global(c["row_labels"])
        with pytest.raises(ValueError):
            ix.add_global(c["rows"])                                        # the partition is made once
        with pytest.raises(ValueError):
            ix.search_probed(qd, 0)
        with pytest.raises(ValueError):
            ix.search_probed(qd, 5, nprobe=0)
        with pytest.raises(NotImplementedError):
            ix.search_probed(qd, ram.MAX_K_WIDE + 1)
        with pytest.raises(ValueError):
            ix.search_probed(qd, 5, selector=np.ones(n - 1, bool))          # shorter than ntotal
        with pytest.raises(ValueError):
            ix.set_labels_global(c["row_labels"][:-1])
        with pytest.raises(ValueError):
            ix.set_trained(c["centroids"][:, :32])
        for k, nprobe, flt in ((5, 1, "plain"), (100, 3, "both")):
            kw = {"plain": {}, "both": {"selector": c["sel"], "groups": c["q_labels"]}}[flt]
            want = shc.expected(c, dtype, k, nprobe, flt)
            assert shc.same(_np(ix.search_probed(qd, k, nprobe, **kw)), want) and shc.same(_np(ix.local.search_probed_wide(qd, k, nprobe, **kw)), want)
        radii = shc.radii_for(c, dtype, 3)
        assert rg.same(_np(ix.range_search_probed(qd, radii, 3)), shc.expected_range(c, dtype, radii, 3))
    # the C layer's refusals, with their codes (-1 MIPS_E_INVALID, -3 MIPS_E_UNSUPPORTED)
    lib = ram._lib.load()
    _, full, parts, _, _ = _built("planted", "sq8")
    h = full._h
    pk = torch.zeros((nq, 1024, 2), dtype=torch.int64, device="cuda")
    b = torch.zeros(nq, dtype=torch.float64, device="cuda")
    dev = ram._lib.Q_DEVICE | ram._lib.OUT_DEVICE

    def part(k=5, nprobe=2, packed=pk.data_ptr(), bias=b.data_ptr(), flags=dev, nq_=nq):
        return lib.mips_ivf_search_part(h, qd.data_ptr(), ram._lib.DTYPE_F32, nq_, k, nprobe, packed, bias, 0, flags, None, 0, 0, None, 0, None)

    assert part() == 0
    assert part(k=0) == -1 and part(nprobe=0) == -1 and part(packed=None) == -1 and part(bias=None) == -1    # (an SQ8 index needs out_bias)
    assert part(flags=dev | ram._lib.OUT_PACKED) == -1
    assert part(k=1025) == -3 and part(k=1024, nprobe=nlist) == 0 and part(nq_=0, packed=None, bias=None) == 0
    assert len(lib.mips_last_error()) > 0
    s = torch.zeros((nq, 1024), dtype=torch.float32, device="cuda")
    i = torch.zeros((nq, 1024), dtype=torch.int64, device="cuda")
    g = torch.zeros((2, nq, 1024, 2), dtype=torch.int64, device="cuda")

    def merge(gathered=g.data_ptr(), parts_=2, nq_=nq, k=5, out_s=s.data_ptr(), out_i=i.data_ptr()):
        return lib.mips_ivf_merge_parts(gathered, parts_, nq_, k, None, out_s, out_i, 0, None)

    assert merge() == 0 and merge(k=1024) == 0
    assert merge(parts_=0) == -1 and merge(k=0) == -1 and merge(nq_=-1) == -1 and merge(gathered=None) == -1 and merge(out_s=None) == -1 and merge(out_i=None) == -1
    assert merge(parts_=65, k=1024) == -3 and merge(k=1025) == -3 and merge(nq_=0, gathered=None) == 0
    with pytest.raises(ValueError):
        ram.ivf_merge_parts(g.cpu(), 2, nq, 1024)
    with pytest.raises(RuntimeError):
        ram.ivf_merge_parts(torch.zeros((65 * nq * 1024 * 2,), dtype=torch.int64, device="cuda"), 65, nq, 1024)     # parts * k > 65536
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (e) plain C
def test_c_abi_ivf_sharded_from_plain_c(tmp_path):
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_ivf_sharded_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_ivf_sharded_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
