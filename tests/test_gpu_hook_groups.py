"""The grouped one-launch hook search on the GPU: MipsIndex.search_fused(groups=) / mips_search_fused_grp / Mips.search_device(
ignore_groups=) against the expectations of tests/hook_group_cases.py -- the oracle's full ranking of all rows, filtered per query
by the admission matrix, cut to k and padded.  Indices and score bits are compared for EQUALITY, no query is left out.  Wherever
the one-launch form is due last_kernel must name the grouped kernel, and wherever a settlement is not the point nothing may stay
unresolved."""
import os
import subprocess

import numpy as np
import pytest
import torch

import hook_group_cases as hg
import retrieval_augmented_mds_amd as ram
from oracle import synth

pytestmark = pytest.mark.gpu

HOOK = "mips::hook_grouped_kernel"
GROUPED = "mips::grouped_scan_kernel"
NONE, ABSENT = hg.NONE, hg.ABSENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, exp, what=""):
    s, i = got
    es, ei = exp
    if isinstance(s, torch.Tensor):
        s, i = s.cpu().numpy(), i.cpu().numpy()
    s, i = np.asarray(s, np.float32), np.asarray(i, np.int64)
    bad = np.flatnonzero((i != ei).any(axis=1))
    assert np.array_equal(i, ei), f"{what}: indices differ in {len(bad)} queries, first {bad[:5]}: got {i[bad[:1]]} expected {ei[bad[:1]]}"
    assert np.array_equal(s.view(np.int32), es.view(np.int32)), f"{what}: scores differ"


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


_CASES = {}


def _gauss_case(n, d):
    """Gaussian bf16 rows, 16 queries, and the full ranking under both metrics: computed once per shape, shared, never modified."""
    key = (n, d)
    if key not in _CASES:
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(synth.SEED_QUERIES, 0, 16, d, synth.KIND_GAUSS)
        dot = hg.dots(q, x)
        _CASES[key] = (x, q, {m: hg.ranking(hg.values(q, x, m, dot), m) for m in (0, 1)})
    return _CASES[key]


def _index(x, metric=0, dtype="bf16", labels=None):
    ix = ram.MipsIndex(x.shape[1], metric=metric, dtype=dtype)
    ix.add(x)
    if labels is not None:
        ix.set_labels(labels)
    return ix


def _hook_ok(ix, what=""):
    st = ix.margin_stats()
    assert ix.last_kernel.startswith(HOOK), f"{what}: last kernel {ix.last_kernel}"
    assert st["unresolved"] == 0, f"{what}: {st}"
    return st


# ------------------------------------------------------------------ 1. parity sweep on Gaussian bf16 rows
# nq, k, metric, mode, labelling, ignore, variant.  Every value of every column occurs with every shape; ignore needs k + 1 <= 6
SWEEP = [
    (1, 1, 0, "exclude", "row % 5", False, "host"),
    (8, 5, 0, "exclude", "row // 2", True, "device"),
    (16, 6, 1, "only", "random 7", False, "bf16"),
    (8, 1, 1, "exclude", "one label", True, "offset"),
    (16, 5, 1, "only", "row % 5", True, "host"),
    (1, 6, 0, "only", "row // 2", False, "device"),
    (16, 5, 0, "exclude", "random 7", True, "offset"),
    (8, 6, 1, "only", "one label", False, "bf16"),
    (16, 5, 0, "exclude", "row // 2", False, "normalize"),
]
SHAPES = [(33, 100), (4099, 768), (10000, 768), (20011, 1024), (65536, 128)]


def _run_combo(ix, x, q, fulls, labs, combo, what):
    nq, k, metric, mode, labelling, ignore, variant = combo
    labels = labs[labelling]
    ql = hg.query_labels(labels, nq)
    adm = hg.admit(labels, ql, mode)
    off = (1 << 33) if variant == "offset" else 0
    qq, full = q[:nq], (fulls[metric][0][:nq], fulls[metric][1][:nq])
    kw = {}
    if variant == "normalize":
        # float32 queries that are no bf16 values; the expectation takes the rows the library stages: l2_normalize_ (the same
        # arithmetic, on the device), rounded to the index's bf16
        qraw = (qq * np.float32(1.7) + np.float32(0.001)).astype(np.float32)
        staged = synth.round_to_bf16(ram.l2_normalize_(_cuda(qraw).clone()).cpu().numpy())
        full = hg.ranking(hg.values(staged, x, metric), metric)
        qd, kw = _cuda(qraw), {"normalize": True}
    elif variant == "bf16":
        qd = _cuda(qq, torch.bfloat16)
    else:
        qd = _cuda(qq)
    groups = _cuda(ql.astype(np.int32)) if variant in ("device", "bf16") else ql
    if ignore:
        exp1 = hg.filter_ranking(full, adm, k + 1, metric, idx_offset=off)
        banned = hg.pick_banned(exp1)
        exp = hg.drop_banned(exp1, banned, k, metric)
        kw["ignore"] = _cuda(banned)
    else:
        exp = hg.filter_ranking(full, adm, k, metric, idx_offset=off)
    got = ix.search_fused(qd, k, idx_offset=off, groups=groups, group_mode=mode, **kw)
    _hook_ok(ix, what)
    assert ix.last_kernel == f"{HOOK}<{'true' if metric else 'false'}, false>"
    _same(got, exp, what)
    if not ignore and variant != "normalize":                       # equal to the route it replaces, bit for bit
        wide = ix.search_wide(qd, k, idx_offset=off, groups=groups, group_mode=mode)
        assert ix.last_kernel == GROUPED
        assert torch.equal(got[1], wide[1][:, :k]) and torch.equal(got[0].view(torch.int32), wide[0][:, :k].view(torch.int32)), what


@pytest.mark.parametrize("n,d", SHAPES)
def test_parity_sweep_gaussian_bf16(n, d):
    x, q, fulls = _gauss_case(n, d)
    labs = hg.labellings(n)
    ixs = {m: _index(x, m) for m in (0, 1)}
    current = {0: None, 1: None}
    for combo in SWEEP:
        metric, labelling = combo[2], combo[4]
        if current[metric] != labelling:
            ixs[metric].set_labels(labs[labelling])
            current[metric] = labelling
        _run_combo(ixs[metric], x, q, fulls, labs, combo, f"n={n} d={d} {combo}")


# ------------------------------------------------------------------ 2. fall-back selections
def test_fallback_selection_and_sequential_rescore():
    n, d = 4099, 768
    x, q, fulls = _gauss_case(n, d)
    labs = hg.labellings(n)
    for metric in (0, 1):
        ix = _index(x, metric)
        ix.set_param("tiny", 2)
        current = None
        for combo in SWEEP:
            if combo[2] != metric:
                continue
            if current != combo[4]:
                ix.set_labels(labs[combo[4]])
                current = combo[4]
            _run_combo(ix, x, q, fulls, labs, combo, f"tiny=2 {combo}")


# ------------------------------------------------------------------ 3. fp32-exact index
def _f32_case():
    """The 30000 x 768 float32 case of tests/test_gpu_grouped.py (same generator, same draws) cut to 10000 rows and 16 queries."""
    if "f32" not in _CASES:
        rng = np.random.default_rng(31)
        x = rng.standard_normal((30000, 768)).astype(np.float32)[:10000]
        q = rng.standard_normal((40, 768)).astype(np.float32)[:16]
        dot = hg.dots(q, x)
        _CASES["f32"] = (np.ascontiguousarray(x), np.ascontiguousarray(q), {m: hg.ranking(hg.values(q, x, m, dot), m) for m in (0, 1)})
    return _CASES["f32"]


@pytest.mark.parametrize("metric", [0, 1])
def test_f32_exact_index(metric):
    x, q, fulls = _f32_case()
    n = x.shape[0]
    labels = np.random.default_rng(23).integers(0, 7, n)
    ix = _index(x, metric, "f32", labels)
    for mode in ("exclude", "only"):
        for nq, k, ignore in ((8, 5, False), (16, 5, True), (1, 6, False)):
            ql = hg.query_labels(labels, nq)
            adm = hg.admit(labels, ql, mode)
            full = (fulls[metric][0][:nq], fulls[metric][1][:nq])
            kw = {}
            if ignore:
                exp1 = hg.filter_ranking(full, adm, k + 1, metric)
                banned = hg.pick_banned(exp1)
                exp, kw = hg.drop_banned(exp1, banned, k, metric), {"ignore": _cuda(banned)}
            else:
                exp = hg.filter_ranking(full, adm, k, metric)
            got = ix.search_fused(_cuda(q[:nq]), k, groups=ql, group_mode=mode, **kw)
            st = _hook_ok(ix, f"f32 {mode} nq={nq}")
            print(f"f32 metric={metric} {mode} nq={nq} k={k} ignore={ignore}: {st}")
            assert ix.last_kernel == f"{HOOK}<{'true' if metric else 'false'}, true>"
            _same(got, exp, f"f32 metric={metric} {mode} nq={nq} k={k}")


# ------------------------------------------------------------------ 4. own group on top
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_own_group_on_top(dtype):
    x, q, labels, ql = hg.own_group_on_top(f32=dtype == "f32")
    nq, k = q.shape[0], 5
    for metric in (0, 1):
        full = hg.ranking(hg.values(q, x, metric), metric)
        ix = _index(x, metric, dtype, labels)
        for mode in ("exclude", "only"):
            exp = hg.filter_ranking(full, hg.admit(labels, ql, mode), k, metric)
            for groups in (ql, _cuda(ql.astype(np.int32))):
                got = ix.search_fused(_cuda(q), k, groups=groups, group_mode=mode)
                _hook_ok(ix, f"own group {dtype} {mode}")
                _same(got, exp, f"own group on top, {dtype}, metric {metric}, {mode}")
            if mode == "exclude":
                ids = got[1].cpu().numpy()
                assert not (labels[ids] == ql[:, None]).any(), "a row of the query's own group came back"


# ------------------------------------------------------------------ 5. ties at the k-th
@pytest.mark.parametrize("resolve", [1, 2])
@pytest.mark.parametrize("metric", [0, 1])
def test_ties_at_the_kth_are_flagged_and_settled_under_the_rule(metric, resolve):
    k = 5
    x, q, labels, ql, copies, twice = hg.ties_at_kth()
    full = hg.ranking(hg.values(q, x, metric), metric)
    ix = _index(x, metric, "bf16", labels)
    ix.set_param("resolve", resolve)
    for mode in ("exclude", "only"):
        adm = hg.admit(labels, ql, mode)
        exp = hg.filter_ranking(full, adm, k, metric)
        got = ix.search_fused(_cuda(q), k, groups=_cuda(ql.astype(np.int32)), group_mode=mode)
        st = ix.margin_stats()
        print(f"ties metric={metric} resolve={resolve} {mode}: {st}")
        assert ix.last_kernel.startswith(HOOK)
        assert st["flagged"] >= len(hg.TIE_CHOSEN) and st["unresolved"] == 0
        ids = got[1].cpu().numpy()
        for j in hg.TIE_CHOSEN:
            assert adm[j][ids[j]].all(), f"query {j}: the settlement brought back a row the rule does not admit"
        _same(got, exp, f"ties at the k-th, metric {metric}, {mode}")
        # with the ignore filter on top: the settlement ranks k + 1 hits and drops the banned one
        exp1 = hg.filter_ranking(full, adm, k + 1, metric)
        banned = hg.pick_banned(exp1)
        got = ix.search_fused(_cuda(q), k, ignore=_cuda(banned), groups=ql, group_mode=mode)
        assert ix.margin_stats()["unresolved"] == 0
        _same(got, hg.drop_banned(exp1, banned, k, metric), f"ties with ignore, metric {metric}, {mode}")


@pytest.mark.parametrize("metric", [0, 1])
def test_graded_ties_on_the_f32_index_only_the_settlement_can_be_right(metric):
    k = 5
    x, q, labels, ql, copies, twice = hg.ties_at_kth(graded=True)
    full = hg.ranking(hg.values(q, x, metric), metric)
    ix = _index(x, metric, "f32", labels)
    for mode in ("exclude", "only"):
        adm = hg.admit(labels, ql, mode)
        exp = hg.filter_ranking(full, adm, k, metric)
        got = ix.search_fused(_cuda(q), k, groups=ql, group_mode=mode)
        st = ix.margin_stats()
        print(f"graded metric={metric} {mode}: {st}")
        assert ix.last_kernel.startswith(HOOK) and st["flagged"] >= len(hg.TIE_CHOSEN) and st["unresolved"] == 0
        _same(got, exp, f"graded copies, metric {metric}, {mode}")


# ------------------------------------------------------------------ 6. short and empty results
@pytest.mark.parametrize("metric", [0, 1])
def test_short_and_empty_results(metric):
    n, d = 4099, 768
    x, q, fulls = _gauss_case(n, d)
    nq, k = 8, 5
    full = (fulls[metric][0][:nq], fulls[metric][1][:nq])
    pad = np.inf if metric else -np.inf
    # only mode on groups of 1 .. 4 rows: padded results, certified outright
    perm = np.random.default_rng(22).permutation(n)
    labels = np.full(n, 1000)
    start = 0
    for g in range(1, 5):
        labels[perm[start:start + g]] = g
        start += g
    ql = np.array([1, 2, 3, 4, 1, 2, ABSENT, 4])
    ix = _index(x, metric, "bf16", labels)
    exp = hg.filter_ranking(full, hg.admit(labels, ql, "only"), k, metric)
    for j in (0, 1, 2, 3, 4, 5, 7):
        assert (exp[1][j, :ql[j]] >= 0).all() and (exp[1][j, ql[j]:] == -1).all()
    assert (exp[1][6] == -1).all()
    got = ix.search_fused(_cuda(q[:nq]), k, groups=ql, group_mode="only")
    assert ix.last_kernel.startswith(HOOK)
    assert ix.margin_stats() == {"flagged": 0, "rescanned": 0, "unresolved": 0}
    _same(got, exp, "small groups")
    # excluding the only group: nothing is left; a LABEL_NONE query beside them is unfiltered
    ix.set_labels(np.full(n, 9, np.int32))
    ql = np.array([9, 9, NONE, 9, ABSENT, 9, 9, 9])
    s, i = ix.search_fused(_cuda(q[:nq]), k, groups=ql)
    assert ix.last_kernel.startswith(HOOK) and ix.margin_stats()["unresolved"] == 0
    s, i = s.cpu().numpy(), i.cpu().numpy()
    gone = ql == 9
    assert (i[gone] == -1).all() and (s[gone] == pad).all()
    _same((s, i), hg.filter_ranking(full, hg.admit(np.full(n, 9), ql, "exclude"), k, metric), "mixed")
    assert np.array_equal(i[2], full[1][2, :k])


# ------------------------------------------------------------------ 7. bit-for-bit equalities
@pytest.mark.parametrize("metric", [0, 1])
def test_bit_for_bit_equalities(metric):
    n, d = 10000, 768
    x, q, fulls = _gauss_case(n, d)
    labels = np.arange(n) // 4
    ix = _index(x, metric, "bf16", labels)
    qd = _cuda(q[:8])
    plain = ix.search_fused(qd, 5)
    assert ix.last_kernel.startswith("mips::tiny_search_kernel")
    for mode in ("exclude", "only"):
        got = ix.search_fused(qd, 5, groups=np.full(8, NONE), group_mode=mode)
        _hook_ok(ix)
        assert torch.equal(got[1], plain[1]) and torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
    ql = (np.arange(8) * 311) % (n // 4)
    got = ix.search_fused(qd, 5, groups=ql)
    _hook_ok(ix)
    wide = ix.search_wide(qd, 5, groups=ql)
    assert torch.equal(got[1], wide[1][:, :5]) and torch.equal(got[0].view(torch.int32), wide[0][:, :5].view(torch.int32))
    again = ix.compute_distance_subset(qd, got[1])
    assert torch.equal(again.view(torch.int32), got[0].view(torch.int32))
    ix.search_fused(qd, 5)                                          # groups=None makes the existing call
    assert ix.last_kernel.startswith("mips::tiny_search_kernel")


# ------------------------------------------------------------------ 8. general form
def test_general_form():
    # more than 16 queries; more than 2^16 rows; k + 1 > 6
    rng = np.random.default_rng(8)
    for n, d, nq, k in ((4099, 768, 17, 5), (66000, 128, 4, 5), (4099, 768, 8, 10)):
        x = synth.generate(synth.SEED_DOCS, 0, n, d, synth.KIND_GAUSS)
        q = synth.generate(synth.SEED_QUERIES, 0, nq, d, synth.KIND_GAUSS)
        full = hg.ranking(hg.values(q, x, 0), 0)
        labels = rng.integers(0, 7, n)
        ql = hg.query_labels(labels, nq)
        ix = _index(x, 0, "bf16", labels)
        for mode in ("exclude", "only"):
            adm = hg.admit(labels, ql, mode)
            got = ix.search_fused(_cuda(q), k, groups=ql, group_mode=mode)
            assert ix.last_kernel == GROUPED and ix.margin_stats()["unresolved"] == 0
            _same(got, hg.filter_ranking(full, adm, k, 0), f"general form n={n} nq={nq} k={k} {mode}")
            exp1 = hg.filter_ranking(full, adm, k + 1, 0, idx_offset=77)
            banned = hg.pick_banned(exp1)
            got = ix.search_fused(_cuda(q), k, ignore=_cuda(banned), idx_offset=77, groups=_cuda(ql.astype(np.int32)), group_mode=mode)
            assert ix.last_kernel == GROUPED
            _same(got, hg.drop_banned(exp1, banned, k, 0), f"general form with ignore n={n} nq={nq} k={k} {mode}")


# ------------------------------------------------------------------ 9. labels that move
def test_labels_that_move():
    n, d, k = 4099, 768, 5
    x, q, fulls = _gauss_case(n, d)
    qd = _cuda(q[:8])
    labels = np.arange(n) % 5
    ql = hg.query_labels(labels, 8)
    ix = ram.MipsIndex(d)
    ix.reserve(1000)
    ix.add(x[:900])
    ix.set_labels(labels[:900])
    dot = hg.dots(q[:8], x)

    def expect(rows, mode):
        full = hg.ranking(hg.values(q[:8], x[rows], 0, dot[:, rows]), 0)
        return hg.filter_ranking(full, hg.admit(labels[rows], ql, mode), k, 0)

    _same(ix.search_fused(qd, k, groups=ql), expect(np.arange(900), "exclude"), "900 rows")
    _hook_ok(ix)
    ix.add(x[900:])                                                 # the rows grow past the label array's tiles
    with pytest.raises(ValueError):                                 # rows added since the labels were set
        ix.search_fused(qd, k, groups=ql)
    ix.set_labels(labels[900:], row0=900)                           # reallocates the label array
    _same(ix.search_fused(qd, k, groups=ql), expect(np.arange(n), "exclude"), "all rows")
    _hook_ok(ix)
    gone = np.zeros(n, bool)
    gone[fulls[0][1][:8, :3].reshape(-1)] = True                    # the three best rows of every query, and a run of rows
    gone[1000:1300] = True
    assert ix.remove_ids(gone) == int(gone.sum())
    rows = np.flatnonzero(~gone)
    for mode in ("exclude", "only"):
        _same(ix.search_fused(qd, k, groups=ql, group_mode=mode), expect(rows, mode), f"after remove_ids, {mode}")
        _hook_ok(ix)


# ------------------------------------------------------------------ 10. refusals
def test_refusals():
    d = 128
    x = synth.generate(3, 0, 300, d, synth.KIND_GAUSS)
    qd = torch.zeros((2, d), dtype=torch.float32, device="cuda")
    ix = _index(x, 0, "bf16", np.arange(300) % 4)
    g = np.array([1, 2])
    with pytest.raises(ValueError):
        ix.search_fused(qd, 5, groups=g, group_mode="without")
    with pytest.raises(ValueError):
        ix.search_fused(qd, 5, groups=np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        ix.search_fused(qd, 5, groups=np.array([1, 1 << 31]))
    with pytest.raises(ValueError):
        ix.search_fused(qd, 5, groups=np.array([-(1 << 31) - 1, 0]))
    with pytest.raises(ValueError):
        ix.search_fused(qd, 5, groups=np.array([0.5, 1.0]))
    with pytest.raises(ValueError):
        ix.search_fused(np.zeros((2, d), np.float32), 5, groups=g)  # the hook takes CUDA tensors
    for dtype in ("fp8_e4m3", "fp8_e4m3_docs"):
        f8 = _index(x, 0, dtype, np.arange(300) % 4)
        with pytest.raises(NotImplementedError):
            f8.search_fused(qd, 5, groups=g)
    wide = _index(synth.generate(3, 0, 300, 1100, synth.KIND_GAUSS), 0, "bf16", np.arange(300) % 4)
    qw = torch.zeros((2, 1100), dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError):
        wide.search_fused(qw, 5, groups=g)
    bare = _index(x)
    with pytest.raises(ValueError):
        bare.search_fused(qd, 5, groups=g)
    # the C ABI itself: the same refusals, by return code
    lib = ram._lib.load()
    out_s = torch.empty((2, 29), dtype=torch.float32, device="cuda")
    out_i = torch.empty((2, 29), dtype=torch.int64, device="cuda")
    gd = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    ign = torch.tensor([0, 0], dtype=torch.int64, device="cuda")

    def rc(index, k, mode, q=qd, ignore=None, normalize=0, code=ram._lib.DTYPE_F32):
        return lib.mips_search_fused_grp(index._h, q.data_ptr(), code, 2, k, normalize, ignore, out_s.data_ptr(), out_i.data_ptr(), 0,
                                         gd.data_ptr(), mode, ram._lib.GRP_DEVICE, None)

    assert rc(ix, 5, 0) == 0 and rc(ix, 5, 1) == 0
    assert rc(ix, 5, 2) == -1 and b"grp_mode" in lib.mips_last_error()                       # MIPS_E_INVALID
    assert rc(ix, 5, -1) == -1
    assert rc(ix, ram.MAX_K, 0) == 0 and rc(ix, ram.MAX_K, 0, ignore=ign.data_ptr()) == -3      # k + 1 > MIPS_MAX_K: MIPS_E_UNSUPPORTED
    assert rc(ix, 5, 0, q=qd.to(torch.bfloat16), normalize=1, code=ram._lib.DTYPE_BF16) == -1  # normalize needs float32 queries
    assert rc(f8, 5, 0) == -3 and rc(wide, 5, 0, q=qw) == -3                                   # what the wide search refuses
    assert rc(bare, 5, 0) == -1 and b"mips_index_set_labels" in lib.mips_last_error()         # never labelled
    torch.cuda.synchronize()


def test_c_abi_hook_grp_from_plain_c(tmp_path):
    libdir = os.path.dirname(ram._lib.build())
    exe = str(tmp_path / "c_abi_hook_grp_smoke")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tests", "c_abi_hook_grp_smoke.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lmips_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64", "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches: 0" in out.stdout


# ------------------------------------------------------------------ 11. facade
def test_mips_search_device_with_ignore_groups():
    n, d, nq, k = 600, 128, 8, 5
    x = synth.generate(61, 0, n, d, synth.KIND_GAUSS)
    q = synth.generate(62, 0, nq, d, synth.KIND_GAUSS)
    aid = np.array([f"art{r // 3:04d}" for r in range(n)])
    q_aid = [str(aid[(97 * j) % n]) for j in range(nq)]
    q_aid[3] = "no such article"
    # every query is (nearly) a row of its own article: without the filter the article's rows come first
    for j in range(nq):
        if j != 3:
            q[j] = x[(97 * j) % n]
    args = ram.MipsArgs(mips_topk=k, mips_metric_type=0, mips_normalize=False, mips_index_dtype="bf16")
    m = ram.Mips(args, data={"mips_column": [f"text {r}" for r in range(n)], "aid": list(aid)})
    m.build_index(x)
    qd = _cuda(q)
    ds, di = m.search_device(qd, k=k, ignore_groups=q_aid)          # sets the groups on first use
    assert ds.is_cuda and di.is_cuda and m._index().last_kernel.startswith(HOOK)
    hs, hi = m.search(q, k=k, ignore_groups=q_aid)
    _same((ds, di), (np.asarray(hs, np.float32), np.asarray(hi, np.int64)), "search_device(ignore_groups)")
    assert float(m.retrieved_group_hits(di, q_aid).sum()) == 0.0
    plain_s, plain_i = m.search_device(qd, k=k)
    assert float(m.retrieved_group_hits(plain_i, q_aid).sum()) > 0  # (the filter had something to do)
    banned = [int(hi[j][1]) for j in range(nq)]
    fs, fi = m.search(q, ignore_indexes=banned, k=k, ignore_groups=q_aid)
    gs, gi = m.search_device(qd, ignore_indexes=torch.tensor(banned).cuda(), k=k, ignore_groups=q_aid)
    _same((gs, gi), (np.asarray(fs, np.float32), np.asarray(fi, np.int64)), "ignore_groups and ignore_indexes")
    rs, ri, rows = m.search_device(qd, k=k, ignore_groups=q_aid, return_rows=True)
    assert torch.equal(ri, di) and torch.equal(rs, ds) and rows.shape == (nq, k, d)
    assert np.array_equal(rows.cpu().numpy(), x[di.cpu().numpy()])
    assert float(m.retrieved_group_hits(gi, q_aid).sum()) == 0.0
