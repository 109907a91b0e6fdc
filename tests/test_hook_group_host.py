"""CPU tests of the grouped one-launch hook search: the builders of tests/hook_group_cases.py do what they say, the wrong
kernels they are meant to catch (labels dropped, the rule applied after the pool was selected, a settlement without the rule)
are wrong on them, the expectation agrees with the DEFINITION (the unfiltered search on an index without the non-admitted
rows), and include/mips_hip_hook.h declares exactly what the binding lists as EXPORTS_HOOK."""
import os
import re

import numpy as np

import hook_group_cases as hg
import retrieval_augmented_mds_amd as ram
from oracle import mips_oracle as orc
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _differs(a, b):
    """bool [nq]: the two results differ for the query (ids or score bits)."""
    return (a[1] != b[1]).any(axis=1) | (a[0].view(np.int32) != b[0].view(np.int32)).any(axis=1)


def _definition(q, x, adm, k):
    """The result by its definition (inner product): per query, the exact search on the admitted rows alone, row numbers kept."""
    s = np.full((q.shape[0], k), -np.inf, np.float32)
    i = np.full((q.shape[0], k), -1, np.int64)
    for j in range(q.shape[0]):
        rows = np.flatnonzero(adm[j])
        if len(rows):
            ss, ii = orc.search_exact_bruteforce(q[j:j + 1], x[rows], min(k, len(rows)))
            s[j, :ss.shape[1]] = ss[0]
            i[j, :ii.shape[1]] = rows[ii[0]]
    return s, i


def test_ranking_from_values_is_the_brute_force_ranking():
    x = synth.generate(synth.SEED_DOCS, 0, 777, 100, synth.KIND_GAUSS)
    q = synth.generate(synth.SEED_QUERIES, 0, 5, 100, synth.KIND_GAUSS)
    for metric in (0, 1):
        full = hg.ranking(hg.values(q, x, metric), metric)
        bs, bi = orc.search_exact_bruteforce(q, x, 777, metric=metric)
        assert np.array_equal(bi, full[1]) and np.array_equal(bs.view(np.int32), full[0].view(np.int32))


def test_own_group_on_top_rejects_kernels_that_drop_or_postpone_the_rule():
    for f32 in (False, True):
        x, q, labels, ql = hg.own_group_on_top(f32=f32)
        nq, k = q.shape[0], 5
        labelled = ql != hg.NONE
        assert labelled.sum() == nq - 1 and not labelled[-1]
        for metric in (0, 1):
            full = hg.ranking(hg.values(q, x, metric), metric)
            own = labels[full[1][:, :hg.OWN_POOL]] == ql[:, None]
            assert own[labelled].all(), "the unfiltered top 8 of a labelled query is not entirely own-group"
            assert (np.array([(labels == v).sum() for v in ql[labelled]]) == hg.OWN_M).all()
            adm = hg.admit(labels, ql, "exclude")
            exp = hg.filter_ranking(full, adm, k, metric)
            assert (exp[1] >= 0).all() and not (labels[exp[1]] == ql[:, None]).any()
            # a kernel that ignores the labels: wrong for every labelled query, right for the unlabelled one
            assert np.array_equal(_differs(hg.ignore_labels(full, k), exp), labelled)
            # a kernel that filters AFTER selecting its pool of 8: nothing is left for a labelled query
            late = hg.filter_after_pool(full, adm, k, metric)
            assert (late[1][labelled] == -1).all() and np.array_equal(_differs(late, exp), labelled)
            if metric == 0 and not f32:
                assert not _differs(_definition(q, x, adm, k), exp).any(), "the filtered ranking is not the definition's result"
            # only mode: the query's own 40 rows, best first = largest factor first
            only = hg.filter_ranking(full, hg.admit(labels, ql, "only"), k, metric)
            assert (labels[only[1][labelled]] == ql[labelled, None]).all()


def test_ties_at_the_kth_counts_and_expectation():
    k = 5
    x, q, labels, ql, copies, twice = hg.ties_at_kth()
    assert np.array_equal(synth.round_to_bf16(x), x) and np.array_equal(synth.round_to_bf16(q), q)   # exactly representable in bf16
    for metric in (0, 1):
        vals = hg.values(q, x, metric)
        full = hg.ranking(vals, metric)
        for mode, wrong_label in (("exclude", {0: hg.TIE_A, 3: hg.TIE_B}), ("only", {0: hg.TIE_B, 3: hg.TIE_A})):
            adm = hg.admit(labels, ql, mode)
            exp = hg.filter_ranking(full, adm, k, metric)
            for j in hg.TIE_CHOSEN:
                kth = exp[0][j, k - 1]
                tied = np.flatnonzero(vals[j] == kth)
                assert len(tied) >= 65 and np.array_equal(tied, copies)
                assert adm[j][tied].any() and (~adm[j][tied]).any()
                assert (vals[j][copies[0]] > np.delete(vals[j], np.concatenate([copies, twice]))).all() if metric == 0 else True
                good = tied[adm[j][tied]]
                # one admitted 2 u row first, then the LOWEST admitted copies
                assert exp[1][j, 0] in twice and adm[j][exp[1][j, 0]]
                assert np.array_equal(exp[1][j, 1:], good[:k - 1])
                # a settlement without the rule ranks all tied rows: it returns a non-admitted row
                blind = (full[0][j, :k], full[1][j, :k])
                assert (labels[blind[1]] == wrong_label[j]).any() and not np.array_equal(blind[1], exp[1][j])
            if metric == 0:
                assert not _differs(_definition(q, x, adm, k), exp).any()
    # exclude mode: more admitted tied rows than a hit list holds (the flood kernel runs under the rule); only mode: fewer
    n_adm = (labels[copies] == hg.TIE_B).sum()
    assert n_adm > 64 and 0 < len(copies) - n_adm <= 64


def test_graded_ties_only_the_settlement_can_be_right():
    k = 5
    x, q, labels, ql, copies, twice = hg.ties_at_kth(graded=True)
    assert np.array_equal(synth.round_to_bf16(x[copies]), np.tile(synth.round_to_bf16(x[copies[0]]), (len(copies), 1)))
    for metric in (0, 1):
        vals = hg.values(q, x, metric)
        full = hg.ranking(vals, metric)
        adm = hg.admit(labels, ql, "exclude")
        exp = hg.filter_ranking(full, adm, k, metric)
        for j in hg.TIE_CHOSEN:
            good = copies[adm[j][copies]]
            assert np.array_equal(exp[1][j, 1:], good[::-1][:k - 1]), "the best admitted copies are not the HIGHEST ones"
            # what a scan that sees the bf16 image alone keeps: the lowest admitted copies -- not one of them is a result
            assert not np.isin(good[:8], exp[1][j]).any()


def test_drop_banned_and_pick_banned():
    s1 = np.array([[9, 8, 7], [5, -np.inf, -np.inf], [-np.inf] * 3], np.float32)
    i1 = np.array([[4, 2, 6], [3, -1, -1], [-1, -1, -1]], np.int64)
    banned = hg.pick_banned((s1, i1))
    assert banned.tolist() == [2, 3, 1 << 40]
    s, i = hg.drop_banned((s1, i1), banned, 2, 0)
    assert i.tolist() == [[4, 6], [-1, -1], [-1, -1]] and s[0].tolist() == [9, 7]


def test_header_declares_exactly_the_hook_exports():
    lib_ = ram._lib
    header = open(os.path.join(ROOT, "include", "mips_hip_hook.h")).read()
    declared = re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert tuple(declared) == lib_.EXPORTS_HOOK == ("mips_search_fused_grp",)
    assert len(lib_.EXPORTS) == 41 and not set(lib_.EXPORTS) & set(lib_.EXPORTS_HOOK)
    m = re.search(r"int mips_search_fused_grp\(([^;]*)\);", header)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    base = open(os.path.join(ROOT, "include", "mips_hip.h")).read()
    fused = [" ".join(p.split()) for p in re.search(r"int mips_search_fused\(([^;]*)\);", base).group(1).split(",")]
    assert params[:len(fused) - 1] == fused[:-1]                   # the arguments of mips_search_fused ...
    assert params[len(fused) - 1:] == ["const int32_t* q_labels", "int grp_mode", "int flags", "void* hip_stream"]
    lib = lib_.load()                                              # builds, loads and binds: AttributeError if the symbol is missing
    assert len(lib.mips_search_fused_grp.argtypes) == len(params) == 14
    import inspect

    sig = inspect.signature(ram.MipsIndex.search_fused)
    assert list(sig.parameters)[1:] == ["x", "k", "normalize", "ignore", "idx_offset", "groups", "group_mode"]
    assert sig.parameters["groups"].default is None and sig.parameters["group_mode"].default == "exclude"
    sig = inspect.signature(ram.Mips.search_device)
    assert list(sig.parameters)[1:] == ["queries", "ignore_indexes", "k", "prepare", "return_rows", "ignore_groups"]
