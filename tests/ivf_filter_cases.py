"""The NumPy restatement of the filtered IVF search (include/mips_hip_ivf.h: mips_ivf_search_sel / _grp) and its cases, on top of
tests/ivf_search_cases.py and tests/ivf_cases.py.

Row i is admitted for query j iff bit sel_bit0 + i of the bitmap is set (when a bitmap is given) and the group rule holds (when query
labels are given): q_labels[j] == LABEL_NONE, or labels[i] != q_labels[j] under "exclude", or labels[i] == q_labels[j] under "only".
The result for query j is the best k of (the rows of the probed lists) n (the admitted rows): the storage's canonical score, SQ8
ranked on S and reported as D, order (score descending, row ascending), -1 / -inf padding, idx_offset added.

`wrong=` switches ONE deliberate mistake on; tests/test_ivf_filter_host.py shows that every one of them changes the result of at
least one case, so a kernel that makes it cannot pass:
    "post_filter"        the best k of the probed lists first, the rows not admitted dropped afterwards
    "modes_swapped"      exclude and only exchanged
    "none_is_a_group"    LABEL_NONE compared like any other label
    "bit0_ignored"       bit i instead of bit sel_bit0 + i
    "first_window_only"  the rule applied to the first 64 positions of every list segment only (needs `segments`)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ivf_cases as iv  # noqa: E402
import ivf_search_cases as sc  # noqa: E402
from oracle import mips_oracle as orc  # noqa: E402

F = np.float32
LABEL_NONE = -(1 << 31)
WRONG = ("post_filter", "modes_swapped", "none_is_a_group", "bit0_ignored", "first_window_only")


def segments(nq, p, k, cus=256):
    """S of csrc/ivf_search_math.hpp (choose_segments)"""
    S = 1
    while S < 32 and nq * p * S < 2 * cus:
        S *= 2
    while S > 1 and p * S * k > 65536:
        S //= 2
    return S


def admitted(ids, j, sel=None, sel_bit0=0, labels=None, q_labels=None, mode="exclude", wrong=None):
    """bool [len(ids)]: which of the rows `ids` answer query j"""
    ok = np.ones(len(ids), bool)
    if sel is not None:
        ok &= np.asarray(sel, dtype=bool)[ids + (0 if wrong == "bit0_ignored" else int(sel_bit0))]
    if q_labels is not None:
        assert mode in ("exclude", "only")
        ql = int(q_labels[j])
        only = (mode == "only") != (wrong == "modes_swapped")
        if ql != LABEL_NONE or wrong == "none_is_a_group":
            lab = np.asarray(labels)[ids]
            ok &= (lab == ql) if only else (lab != ql)
    return ok


def search(rows, q, assign, centroids, k, nprobe, dtype, sq8_params=None, sel=None, labels=None, q_labels=None, mode="exclude",
           wrong=None, idx_offset=0, sel_bit0=0, seg=None):
    """-> (D float32 [nq, k], I int64 [nq, k]).  sel: bool array, entry sel_bit0 + i decides row i"""
    q = np.asarray(q, dtype=F)
    assign = np.asarray(assign)
    nlist = len(centroids)
    p = min(int(nprobe), nlist)
    P = iv.nearest(q, centroids, p)
    X, Y, bias = sc.stored(rows, q, dtype, sq8_params)
    S = segments(len(q), p, k) if seg is None else seg
    members = {}
    D = np.full((len(q), k), -np.inf, F)
    I = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        ids, ok = [np.zeros(0, np.int64)], [np.zeros(0, bool)]
        for l in P[j]:
            if int(l) not in members:
                members[int(l)] = np.flatnonzero(assign == l).astype(np.int64)
            m = members[int(l)]
            a = admitted(m, j, sel, sel_bit0, labels, q_labels, mode, wrong)
            if wrong == "first_window_only":
                for s in range(S):
                    a[len(m) * s // S + 64:len(m) * (s + 1) // S] = True
            ids.append(m)
            ok.append(a)
        ids, ok = np.concatenate(ids), np.concatenate(ok)
        if wrong != "post_filter":
            ids = ids[ok]
        if len(ids) == 0:
            continue
        key = orc.canonical_pairs(Y[j:j + 1], X, ids[None, :])[0].astype(F)
        order = np.lexsort((ids, -key))[:k]
        if wrong == "post_filter":
            order = order[np.isin(ids[order], np.concatenate([np.zeros(0, np.int64), ids[ok]]))]
        out = key[order]
        if bias is not None:
            out = (out.astype(np.float64) + bias[j]).astype(F)
        D[j, :len(order)] = out
        I[j, :len(order)] = ids[order] + idx_offset
    return D, I


def bruteforce_on_admitted(rows, q, assign, centroids, k, nprobe, dtype, sq8_params=None, sel=None, labels=None, q_labels=None,
                           mode="exclude", sel_bit0=0):
    """the same result from the oracle's exact brute force over the probed AND admitted rows alone, row numbers mapped back"""
    q = np.asarray(q, dtype=F)
    P = iv.nearest(q, centroids, min(int(nprobe), len(centroids)))
    X, Y, bias = sc.stored(rows, q, dtype, sq8_params)
    D = np.full((len(q), k), -np.inf, F)
    I = np.full((len(q), k), -1, np.int64)
    for j in range(len(q)):
        ids = np.flatnonzero(np.isin(assign, P[j]))
        ids = ids[admitted(ids, j, sel, sel_bit0, labels, q_labels, mode)]
        if len(ids) == 0:
            continue
        s, i = orc.search_exact_bruteforce(Y[j:j + 1], np.ascontiguousarray(X[ids]), k)
        ok = i[0] >= 0
        I[j, ok] = ids[i[0, ok]]
        D[j, ok] = s[0, ok] if bias is None else (s[0, ok].astype(np.float64) + bias[j]).astype(F)
    return D, I


# ------------------------------------------------------------------ cases
def case_planted(d):
    """iv.case_planted(d) (lists of 0, 2500, 1, 63, 64, 65, 200 and 100 rows) with labels: groups of 8 consecutive rows (row // 8),
    except that list 5 is ONE group of its own (label 9000): a group that covers a whole list.  q_labels: every third query carries
    LABEL_NONE, the others the label of the FIRST row of their list (so a query of list 5 excludes, or keeps, the whole list, and
    the query of the one-row list 2 its only row); the queries of the empty list 0 carry a label no row has.
    sel: a bitmap with two rows of three set; sel_off: the same one, 13 bits further on (sel_bit0 = 13)."""
    c = iv.case_planted(d)
    lab, n = c["labels"], len(c["rows"])
    labels = (np.arange(n) // 8).astype(np.int32)
    labels[lab == 5] = 9000
    ql = np.full(len(c["q"]), LABEL_NONE, np.int64)
    for j, l in enumerate(c["qlabels"]):
        if j % 3 == 2:
            continue
        mem = np.flatnonzero(lab == l)
        ql[j] = labels[mem[0]] if len(mem) else 123456
    c["assign"] = lab
    c["row_labels"] = labels
    c["q_labels"] = ql.astype(np.int32)
    c["sel"] = (np.arange(n) * 2654435761 % 3 != 0)
    c["sel_off"] = np.concatenate([np.ones(13, bool), c["sel"], np.zeros(5, bool)])
    return c


def case_ties():
    """sc.case_ties() with a bitmap that clears every other one of the first 20 copies: the result is the lowest admitted copies,
    ascending.  Labels: copy c belongs to group c % 5, every other row to group 99."""
    c = sc.case_ties()
    n = len(c["rows"])
    sel = np.ones(n, bool)
    sel[c["copies"][0:20:2]] = False
    labels = np.full(n, 99, np.int32)
    labels[c["copies"]] = np.arange(sc.TIE_COPIES) % 5
    c["sel"], c["row_labels"] = sel, labels
    c["admitted_copies"] = np.array([r for r in c["copies"] if sel[r]], np.int64)
    return c


QUEUE_N, QUEUE_BIG = 24000, 20000
QUEUE_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129)


def case_queue(seed=8):
    """24 000 rows of d = 32 in four lists by PLANTED assignments (mips_ivf_set_assign): 20 000 rows in list 0, the rest spread over
    lists 1 .. 3.  The centroids are e_0 .. e_3 and every query is 2 e_0 + noise, so P(q) = (0) at nprobe = 1.
    Searched with 512 queries and nprobe = 1 the list is ONE segment (512 workgroups on 256 compute units): wave w of a workgroup
    walks the windows of 64 positions that begin at 64 w + 256 i.  bitmaps["c<N>"] admits exactly N rows of list 0, all of them in
    wave 0's stretch and scattered over its 79 windows, so the wave's queue fills slowly, reaches 64 in the middle of a window
    (or never), and is flushed with a remainder of 0, 1, 63, ... rows; "first64" admits the first 64 positions of the list and
    nothing else; "every65" every 65th position (every wave, a queue that never reaches a pass).  Searched with one query the list
    is cut into 32 segments and the same bitmaps fall differently."""
    rng = np.random.default_rng(seed)
    d = 32
    rows = rng.standard_normal((QUEUE_N, d)).astype(F)
    assign = np.empty(QUEUE_N, np.int32)
    perm = rng.permutation(QUEUE_N)
    assign[perm[:QUEUE_BIG]] = 0
    assign[perm[QUEUE_BIG:]] = rng.integers(1, 4, QUEUE_N - QUEUE_BIG)
    cen = np.zeros((4, d), F)
    cen[np.arange(4), np.arange(4)] = 1
    q = (2 * cen[0] + 0.05 * rng.standard_normal((512, d))).astype(F)
    big = np.flatnonzero(assign == 0)                      # list 0 in list order
    pos = np.arange(QUEUE_BIG)
    wave0 = pos[(pos % 256) < 64]
    bitmaps = {}
    for cnt in QUEUE_COUNTS:
        m = np.zeros(QUEUE_N, bool)
        m[big[np.sort(rng.choice(wave0, cnt, replace=False))]] = True
        bitmaps[f"c{cnt}"] = m
    m = np.zeros(QUEUE_N, bool)
    m[big[:64]] = True
    bitmaps["first64"] = m
    m = np.zeros(QUEUE_N, bool)
    m[big[::65]] = True
    bitmaps["every65"] = m
    labels = (np.arange(QUEUE_N) // 8).astype(np.int32)
    return {"rows": rows, "q": q, "nlist": 4, "centroids": cen, "assign": assign, "bitmaps": bitmaps, "row_labels": labels, "big": big}
