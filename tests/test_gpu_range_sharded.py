"""Range search on the row-sharded index: the merge kernels (mips_range_merge_records) against their NumPy restatement on synthetic
records, row shards searched into records and merged in one process (plain, with a global selector read from bit `lo`, with
group labels), ShardedMipsIndex.range_search / range_search_into on ranks that share one GPU (gloo), the refusals, and the plain-C
consumer of the second header.  Every expectation of a search comes from the oracle's canonical arithmetic on ALL pairs
(tests/range_cases.py); every comparison is per query and bit for bit, counts, ids and scores."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from oracle import synth
from retrieval_augmented_mds_amd.mips import KnowledgeBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import range_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the merge kernels alone
def _merge_and_check(part_results, parts, nq, stride, what):
    g = rc.gather(part_results, stride)
    exp = rc.merge_records(g, parts, nq, stride)
    got = ram.range_merge_records(torch.from_numpy(g).cuda(), parts, nq, stride, cap=int(exp[0][-1]))
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
    rc._same(got, exp, what)
    I, D = got[2].cpu().numpy(), got[1].cpu().numpy()
    assert (I != rc.PAD_ID).all() and not np.isnan(D).any()       # no padding entry of a record reaches the output
    return g, exp


@pytest.mark.parametrize("nq", [1, 5, 257, 4099])
@pytest.mark.parametrize("parts", [1, 2, 3, 8])
def test_merge_kernel_equals_numpy(parts, nq):
    """About half of the per-(part, query) counts are 0.  The records are as large as the largest part, which leaves sentinel
    padding (id -7, score NaN) in every other part; the stride is odd for odd nq, so the score view ends in half a word."""
    pr = rc.synthetic_parts(parts, nq, seed=1000 * parts + nq)
    stride = max(int(p[0][-1]) for p in pr)
    stride += (stride + nq) % 2
    _merge_and_check(pr, parts, nq, stride, f"parts {parts}, nq {nq}, stride {stride}")


def test_merge_one_query_of_70000_hits_spans_many_tiles():
    counts = np.zeros((3, 5), np.int64)
    counts[0] = [3, 0, 41, 0, 2]
    counts[1] = [1, 0, 70000, 0, 4]                                # the queries before and after it are empty in every part
    pr = rc.synthetic_parts(3, 5, seed=5, counts=counts)          # part 2 has total 0
    assert int(pr[2][0][-1]) == 0
    _merge_and_check(pr, 3, 5, 70005, "70 000 hits, odd stride")
    _merge_and_check(pr, 3, 5, 70006, "70 000 hits, even stride")


def test_merge_stride_above_every_total_and_odd_stride():
    pr = rc.synthetic_parts(3, 33, seed=9)
    top = max(int(p[0][-1]) for p in pr)
    for stride in (top + 1000, (top + 1001) | 1):                  # sentinels behind every part; one stride odd
        g, _ = _merge_and_check(pr, 3, 33, stride, f"stride {stride}")
        for p in range(3):
            _, D, I = rc.split_record(g[p * rc.record_words(33, stride):(p + 1) * rc.record_words(33, stride)], 33, stride)
            assert (I[int(pr[p][0][-1]):] == rc.PAD_ID).all() and np.isnan(D[int(pr[p][0][-1]):]).all()


def test_merge_capacity_protocol():
    parts, nq = 3, 257
    pr = rc.synthetic_parts(parts, nq, seed=11)
    stride = max(int(p[0][-1]) for p in pr)
    g = rc.gather(pr, stride)
    exp = rc.merge_records(g, parts, nq, stride)
    total = int(exp[0][-1])
    gd = torch.from_numpy(g).cuda()
    # cap below the total: the counts are true and nothing at or past cap is written
    cap, guard = total // 2 + 1, 4096
    lims = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    D = torch.full((cap + guard,), 123.0, dtype=torch.float32, device="cuda")
    I = torch.full((cap + guard,), -99, dtype=torch.int64, device="cuda")
    out = ram.range_merge_records(gd, parts, nq, stride, out=(lims, D[:cap], I[:cap]))
    assert out[0] is lims
    assert np.array_equal(lims.cpu().numpy(), exp[0])
    assert bool((D[cap:] == 123.0).all()) and bool((I[cap:] == -99).all())
    # the counting call: cap = 0, NULL outputs
    lims0, D0, I0 = ram.range_merge_records(gd, parts, nq, stride, cap=0)
    assert np.array_equal(lims0.cpu().numpy(), exp[0]) and D0.numel() == I0.numel() == 0
    # the default capacity (parts * stride) holds every result of untruncated parts
    rc._same(tuple(t[:total] if i else t for i, t in enumerate(ram.range_merge_records(gd, parts, nq, stride))), exp, "default cap")
    # a truncated part: lims_p[nq] = stride + 5; true counts, MIPS_OK, nothing read past the record (the merged payload is unspecified)
    small = max(int(p[0][-1]) for p in pr) - 5
    assert any(int(p[0][-1]) == small + 5 for p in pr)
    gt = torch.from_numpy(rc.gather(pr, small)).cuda()
    lt, Dt, It = ram.range_merge_records(gt, parts, nq, small, cap=total)
    assert np.array_equal(lt.cpu().numpy(), exp[0])
    # nq == 0
    l0, _, _ = ram.range_merge_records(torch.zeros(2, dtype=torch.int64, device="cuda"), 2, 0, 0, cap=0)
    assert l0.cpu().tolist() == [0]


def test_merge_bad_arguments_return_invalid():
    lib = ram._lib.load()
    g = torch.zeros(2 * rc.record_words(3, 4), dtype=torch.int64, device="cuda")
    lims = torch.zeros(4, dtype=torch.int64, device="cuda")
    D = torch.zeros(8, dtype=torch.float32, device="cuda")
    I = torch.zeros(8, dtype=torch.int64, device="cuda")
    work = torch.zeros(6, dtype=torch.int64, device="cuda")

    def call(gathered=g.data_ptr(), parts=2, nq=3, stride=4, out_lims=lims.data_ptr(), out_s=D.data_ptr(), out_i=I.data_ptr(), cap=8,
             workspace=work.data_ptr()):
        return lib.mips_range_merge_records(gathered, parts, nq, stride, out_lims, out_s, out_i, cap, workspace, 0, None)

    assert call() == 0
    assert call(parts=0) == -1 and call(nq=-1) == -1 and call(stride=-1) == -1 and call(cap=-1) == -1      # MIPS_E_INVALID
    assert call(gathered=None) == -1 and call(out_lims=None) == -1
    assert call(out_s=None) == -1 and call(out_i=None) == -1 and call(workspace=None) == -1
    assert call(out_s=None, out_i=None, cap=0) == 0 and call(nq=0, workspace=None) == 0
    assert call(nq=(1 << 24) + 1) == -3                                                                      # MIPS_E_UNSUPPORTED
    assert len(ram._lib.load().mips_last_error()) > 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. shards in one process
N2, D2, NQ2 = 9001, 256, 77
BOUNDS2 = [(0, 2000), (2000, 2000), (2000, 2050), (2050, N2)]     # one part is empty, one tiny; 2050 is not a multiple of 8
_CASE2 = {}


def _case2(dtype, metric):
    """Rows, queries, boundary radii and all pair values of one (storage, metric): computed once, shared, not modified."""
    key = (dtype, metric)
    if key not in _CASE2:
        rng = np.random.default_rng(4)
        x = (synth.generate(153, 0, N2, D2, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (N2, 1))).astype(np.float32)
        if dtype == "bf16":
            x = synth.round_to_bf16(x)
        q = synth.generate(154, 0, NQ2, D2, synth.KIND_GAUSS)
        vals = rc._values(q, x, metric)
        _CASE2[key] = (x, q, rc._boundary_radii(vals, metric), vals)
    return _CASE2[key]


def _search_shards(x, q, r, metric, dtype, stride, labels=None, **kw):
    """-> (the full index, merged result): every part of BOUNDS2 searches into the views of its own record with
    idx_offset = lo, the records are concatenated as an all-gather would leave them, and merged."""
    dev = torch.device("cuda", 0)
    full = ram.MipsIndex(D2, metric=metric, dtype=dtype)
    full.add(x)
    if labels is not None:
        full.set_labels(labels)
    qd = torch.from_numpy(q).cuda()
    records = []
    for lo, hi in BOUNDS2:
        p = ram.MipsIndex(D2, metric=metric, dtype=dtype)
        if hi > lo:
            p.add(x[lo:hi])
            if labels is not None:
                p.set_labels(labels[lo:hi])
        if metric == 1:
            p.set_phi(full.phi())
        rec = torch.empty(ram._lib.range_record_words(NQ2, stride), dtype=torch.int64, device=dev)
        lims, D, I = ram.sharded.range_record_views(rec, NQ2, stride)
        extra = {"sel_bit0": lo} if "selector" in kw else {}
        p.range_search_into(qd, r, lims, D, I, idx_offset=lo, **kw, **extra)
        assert p.margin_stats()["unresolved"] == 0
        records.append(rec)
    return full, qd, ram.range_merge_records(torch.cat(records), len(BOUNDS2), NQ2, stride)


def _trim(got):
    total = int(got[0][-1])
    return got[0], got[1][:total], got[2][:total]


def _shard_stride(exp):
    return max(int(((exp[2] >= lo) & (exp[2] < hi)).sum()) for lo, hi in BOUNDS2) + 3


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ragged_shards_merge_to_the_unsharded_result(dtype, metric):
    x, q, r, vals = _case2(dtype, metric)
    exp = rc._expected(vals, r, metric)
    full, qd, got = _search_shards(x, q, r, metric, dtype, _shard_stride(exp))
    print(f"{dtype} metric {metric}: {exp[0][-1]} hits")
    rc._same(_trim(got), exp, "shards against the oracle")
    rc._same(_trim(got), full.range_search(qd, r), "shards against the unsharded search")


def test_ragged_shards_with_a_global_selector():
    x, q, r, vals = _case2("bf16", 1)
    mask = np.random.default_rng(8).random(N2) < 0.5
    exp = rc._expected(vals, r, 1, mask=mask)
    sel = ram.Selector.from_mask(mask, device=0)                   # GLOBAL: every part reads its rows' bits from bit `lo` on
    full, qd, got = _search_shards(x, q, r, 1, "bf16", _shard_stride(exp), selector=sel)
    rc._same(_trim(got), exp, "selector, shards against the oracle")
    rc._same(_trim(got), full.range_search(qd, r, selector=sel), "selector, shards against the unsharded search")


@pytest.mark.parametrize("mode", ["exclude", "only"])
def test_ragged_shards_with_group_labels_and_a_selector(mode):
    x, q, r, vals = _case2("bf16", 0)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 3, N2).astype(np.int32)
    qlab = rng.integers(0, 3, NQ2).astype(np.int32)
    qlab[::7] = ram.LABEL_NONE                                     # not group-filtered
    sel_mask = rng.random(N2) < 0.5
    same = labels[None, :] == qlab[:, None]
    admit = np.where((qlab == ram.LABEL_NONE)[:, None], True, same if mode == "only" else ~same)
    exp = rc._expected(vals, r, 0, mask=admit & sel_mask[None, :])  # the AND-ed mask
    sel = ram.Selector.from_mask(sel_mask, device=0)
    full, qd, got = _search_shards(x, q, r, 0, "bf16", _shard_stride(exp), labels=labels, selector=sel, groups=qlab, group_mode=mode)
    rc._same(_trim(got), exp, f"groups {mode}, shards against the oracle")
    rc._same(_trim(got), full.range_search(qd, r, selector=sel, groups=qlab, group_mode=mode), f"groups {mode}, against the unsharded search")


# ------------------------------------------------------------------ 3. ranks sharing one GPU (gloo)
def _rank_worker(rank, world, port, n, nq, d, facade, tmp, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        rng = np.random.default_rng(3)
        x = synth.round_to_bf16((synth.generate(151, 0, n, d, synth.KIND_GAUSS) * rng.uniform(0.3, 2.5, (n, 1))).astype(np.float32))
        qn = synth.round_to_bf16(synth.generate(152, 0, nq, d, synth.KIND_GAUSS))
        qd = torch.from_numpy(qn).cuda()
        lo, hi = ram.shard_bounds(n, world, rank)
        for metric in (0, 1):
            ix = ram.ShardedMipsIndex(d, metric=metric, device=0)
            ix.add_global(x)
            assert ix.local.ntotal == hi - lo
            vals = rc._values(qn, x, metric)
            r = rc._boundary_radii(vals, metric)                   # per query, +-inf included: some queries return every row
            exp = rc._expected(vals, r, metric)
            got = ix.range_search(qd, r)                           # CUDA in -> CUDA out
            assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
            rc._same(got, exp, f"rank {rank} metric {metric} cuda")
            assert ix.margin_stats()["unresolved"] == 0
            got = ix.range_search(qn, r)                           # NumPy in -> NumPy out
            assert all(isinstance(t, np.ndarray) for t in got)
            rc._same(got, exp, f"rank {rank} metric {metric} numpy")
            # the default first stride (65536 entries) holds every shard result of these shapes; a small one makes every shard
            # that found more repeat its search once with the common maximum
            own = int(((exp[2] >= lo) & (exp[2] < hi)).sum())
            ix._range_stride_guess = lambda nq_: 1 << 10
            searches = []
            into = ix.local.range_search_into
            ix.local.range_search_into = lambda *a, **k: (searches.append(a[4].shape[0]), into(*a, **k))[1]
            rc._same(ix.range_search(qd, r), exp, f"rank {rank} metric {metric} after the repeat")
            shard_max = max(int(((exp[2] >= a) & (exp[2] < b)).sum()) for a, b in (ram.shard_bounds(n, world, t) for t in range(world)))
            assert searches == ([1 << 10, shard_max] if own > (1 << 10) else [1 << 10]), (searches, own, shard_max)
            if n > 10000:
                assert own > (1 << 10)                             # (the repeat is exercised)
            ix.local.range_search_into = into
            del ix._range_stride_guess
            # the form that never synchronises: enough room in every part -> the same bits; part_cap = 1 -> lims still true
            total = int(exp[0][-1])
            lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
            D = torch.empty(total + 7, dtype=torch.float32, device="cuda")
            I = torch.empty(total + 7, dtype=torch.int64, device="cuda")
            assert ix.range_search_into(qd, r, lims, D, I, part_cap=shard_max) is None
            rc._same((lims, D[:total], I[:total]), exp, f"rank {rank} metric {metric} range_search_into")
            lims.fill_(-1)
            ix.range_search_into(qd, r, lims, D, I, part_cap=1)
            assert np.array_equal(lims.cpu().numpy(), exp[0])
            if metric == 1:
                v0 = rc._values(qn, x, 0)
                r0 = rc._boundary_radii(v0, 0)
                rc._same(ix.range_search(qd, r0, force_ip=True), rc._expected(v0, r0, 0), f"rank {rank} force_ip")
        if facade:                                                 # planted duplicates on both sides of the shard border
            border = ram.shard_bounds(n, world, 0)[1]
            xn = x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
            xn = synth.round_to_bf16(xn.astype(np.float32))
            a = np.array([5, border - 1, border, border + 700, n - 1])
            b = np.array([border - 2, border + 1])
            xn[a] = xn[a[0]]
            xn[b] = xn[b[0]]
            data = {"mips_column": [f"text {t}" for t in range(n)], "aid": [f"a{t}" for t in range(n)]}
            m = ram.Mips(ram.MipsArgs(mips_metric_type=0, mips_normalize=False, mips_tmp_folder=tmp, mips_shard=True, mips_device=0), data=data)
            m.build_index_sharded(xn)
            kb = m.embeddings
            index = kb.get_index(m.index_name).faiss_index
            assert isinstance(index, ram.ShardedMipsIndex) and isinstance(kb, KnowledgeBase)
            kb.columns["emb"] = xn                                 # the column the index was built from, under its name
            kb.add_faiss_index("emb", index_name=m.index_name, custom_index=index)
            i, j, s = kb.near_duplicates(m.index_name, 0.99, batch_rows=8192)
            want = sorted([(int(u), int(v)) for c in (a, b) for ui, u in enumerate(c) for v in c[ui + 1:]])
            assert list(zip(i.tolist(), j.tolist())) == want, (list(zip(i.tolist(), j.tolist()))[:20], want)
            assert np.array_equal(s, rc.orc.canonical_pairs(xn[i], xn, j[:, None])[:, 0].astype(np.float32))
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,facade", [(2, 20001, True), (3, 20001, False), (3, 100, False)])
def test_sharded_range_search_on_ranks_sharing_one_gpu(world, n, facade, tmp_path):
    """Row shards on `world` processes sharing cuda:0: the range search per shard into its record, the scalar all-reduce, the ONE
    all-gather of the records (gloo, host staged) and the merge kernels -- equal to the oracle on the unsharded rows on every rank,
    CUDA and NumPy queries, both metrics, force_ip, the repeat with a larger stride, and range_search_into.  One case also joins
    the index of the Mips facade (mips_shard=True) with itself through KnowledgeBase.near_duplicates."""
    import torch.multiprocessing as mp

    port = 28600 + (os.getpid() % 2000) + 5 * world + n % 7
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, n, 50, 256, facade, str(tmp_path), ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


# ------------------------------------------------------------------ 4. refusals, one rank
def test_refusals_and_the_one_rank_result():
    q = torch.from_numpy(synth.generate(4, 0, 3, 64, synth.KIND_GAUSS)).cuda()
    x = synth.generate(3, 0, 300, 64, synth.KIND_GAUSS)
    ix = ram.ShardedMipsIndex(64, device=0)                        # no process group: one rank, the same checks
    ix.add_global(x)
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, idx_offset=1)
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, selector=np.ones(299, bool))       # shorter than ntotal_global
    with pytest.raises(ValueError):
        ix.range_search(q, 0.0, selector=np.zeros(37, np.uint8))   # 296 bits
    f8 = ram.ShardedMipsIndex(64, dtype="fp8_e4m3", device=0)
    f8.add_global(x)
    with pytest.raises(NotImplementedError):
        f8.range_search(q, 0.0)
    with pytest.raises(NotImplementedError):
        f8.range_search_into(q, 0.0, None, None, None, part_cap=4)
    got = ix.range_search(q, 1.0)
    assert int(got[0][-1]) > 0
    rc._same(got, tuple(t.cpu().numpy() for t in ix.local.range_search(q, 1.0)), "one rank")
    mask = np.arange(300) % 2 == 0
    rc._same(ix.range_search(q, 1.0, selector=mask), tuple(t.cpu().numpy() for t in ix.local.range_search(q, 1.0, selector=mask)), "one rank, selector")


# ------------------------------------------------------------------ 5. plain C
def test_c_abi_range_merge_from_plain_c(tmp_path):
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_range_merge_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_range_merge_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout
