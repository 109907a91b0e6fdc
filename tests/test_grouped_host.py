"""CPU tests of the grouped-search surface: the C ABI declares and the binding binds mips_index_set_labels / mips_index_read_labels /
mips_search_wide_grp / mips_range_search_grp, route_search sends a call that carries groups= to search_wide, and KnowledgeBase /
Mips turn per-query VALUES of a column into the dense int32 codes the index is labelled with (checked against stub indexes)."""
import os
import re

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram
from retrieval_augmented_mds_amd.mips import KnowledgeBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(header, name):
    m = re.search(rf"int {name}\(([^;]*)\);", header)
    assert m, f"{name} is not declared in mips_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_binding_binds_the_grouped_entry_points():
    header = open(os.path.join(ROOT, "include", "mips_hip.h")).read()
    wide, rng = _params(header, "mips_search_wide_grp"), _params(header, "mips_range_search_grp")
    wide_sel, rng_sel = _params(header, "mips_search_wide_sel"), _params(header, "mips_range_search_sel")
    assert len(wide_sel) == 13 and len(rng_sel) == 15
    assert wide[:12] == wide_sel[:12] and wide[12:] == ["const int32_t* q_labels", "int grp_mode", "void* hip_stream"]
    assert rng[:14] == rng_sel[:14] and rng[14:] == ["const int32_t* q_labels", "int grp_mode", "void* hip_stream"]
    assert _params(header, "mips_index_set_labels") == ["mips_index_t* index", "const int32_t* labels", "int64_t row0", "int64_t n",
                                                        "int src_is_device", "void* hip_stream"]
    assert _params(header, "mips_index_read_labels") == ["mips_index_t* index", "int64_t row0", "int64_t n", "int32_t* out_host", "void* hip_stream"]
    lib_ = ram._lib
    assert int(re.search(r"#define MIPS_GRP_DEVICE (\d+)", header).group(1)) == lib_.GRP_DEVICE == 32
    assert int(re.search(r"#define MIPS_GRP_EXCLUDE (\d+)", header).group(1)) == lib_.GRP_EXCLUDE == 0
    assert int(re.search(r"#define MIPS_GRP_ONLY (\d+)", header).group(1)) == lib_.GRP_ONLY == 1
    assert re.search(r"#define MIPS_LABEL_NONE INT32_MIN\b", header) and lib_.LABEL_NONE == ram.LABEL_NONE == -2 ** 31 == np.iinfo(np.int32).min
    assert lib_.GRP_DEVICE & (lib_.Q_DEVICE | lib_.OUT_DEVICE | lib_.OUT_PACKED | lib_.FORCE_IP | lib_.SEL_DEVICE) == 0
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", header).group(1)) == lib_.ABI_VERSION == 1
    names = ("mips_index_set_labels", "mips_index_read_labels", "mips_search_wide_grp", "mips_range_search_grp")
    assert all(name in lib_.EXPORTS for name in names)
    assert set(lib_.EXPORTS) == set(re.findall(r"\b(mips_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))) and len(lib_.EXPORTS) == 41
    lib = lib_.load()                                              # builds, loads and binds: AttributeError if a symbol is missing
    # 12 + 3 and 14 + 3 parameters: those of the _sel calls before hip_stream, then q_labels, grp_mode, hip_stream.  (The issue that
    # asked for these entry points counted "16 and 18"; it took the _sel calls' 13 and 15 parameters, hip_stream included, for the
    # ones "up to sel_bit0".  Its prototypes, which the header follows word for word, have 15 and 17.)
    assert len(wide) == 15 and len(rng) == 17
    assert len(lib.mips_search_wide_grp.argtypes) == len(wide) and len(lib.mips_range_search_grp.argtypes) == len(rng)
    assert len(lib.mips_index_set_labels.argtypes) == 6 and len(lib.mips_index_read_labels.argtypes) == 5
    assert lib.mips_abi_version() == 1


class _Stub:
    """A duck-typed index that records which of its searches was called, and the labels it was given."""

    metric_type = 0
    d = 4

    def __init__(self):
        self.calls = []
        self.labelled = None

    def search(self, q, k, **kw):
        self.calls.append(("search", k, kw))
        return np.zeros((len(q), k), np.float32), np.zeros((len(q), k), np.int64)

    def search_wide(self, q, k, **kw):
        self.calls.append(("search_wide", k, kw))
        return np.zeros((len(q), k), np.float32), np.tile(np.arange(k, dtype=np.int64), (len(q), 1))

    def set_labels(self, labels, row0=0):
        self.labelled = np.asarray(labels)


def test_route_search_sends_a_grouped_call_to_search_wide():
    route = ram.index.route_search
    stub = _Stub()
    g = np.array([1, 2])
    q = np.zeros((2, 4), np.float32)
    route(stub, q, 5, groups=g)                                    # whatever k is
    route(stub, q, 100, groups=g, group_mode="only", force_ip=True)
    route(stub, q, 5, groups=None)                                 # groups=None is stripped, and its mode with it
    route(stub, q, 5, groups=None, group_mode="only", selector=None)
    route(stub, q, 100, groups=None)
    route(stub, q, 5)                                              # calls without it route as before
    route(stub, q, 100)
    sel = object()
    route(stub, q, 5, selector=sel, groups=None)
    route(stub, q, 5, selector=sel, groups=g)
    assert stub.calls == [("search_wide", 5, {"groups": g}), ("search_wide", 100, {"groups": g, "group_mode": "only", "force_ip": True}),
                          ("search", 5, {}), ("search", 5, {}), ("search_wide", 100, {}), ("search", 5, {}), ("search_wide", 100, {}),
                          ("search_wide", 5, {"selector": sel}), ("search_wide", 5, {"selector": sel, "groups": g})]


def test_as_labels_converts_and_refuses():
    import torch

    as_labels = ram.index.as_labels
    for src in ([3, -1, ram.LABEL_NONE], np.array([3, -1, ram.LABEL_NONE]), np.array([3, -1, ram.LABEL_NONE], np.int64),
                torch.tensor([3, -1, ram.LABEL_NONE])):
        out, is_dev = as_labels(src, "t")
        assert not is_dev and out.dtype == np.int32 and out.flags.c_contiguous and out.tolist() == [3, -1, -2 ** 31]
    assert as_labels(np.array([2 ** 31 - 1], np.uint32), "t")[0].tolist() == [2 ** 31 - 1]
    assert as_labels([], "t")[0].shape == (0,)
    for bad in (np.array([2 ** 31]), np.array([-2 ** 31 - 1]), np.array([1.0]), np.array(["a"]), np.array([True]), torch.tensor([0.5]),
                torch.tensor([2 ** 31]), np.array([2 ** 31], np.uint32)):
        with pytest.raises(ValueError):
            as_labels(bad, "t")


def test_knowledge_base_groups_are_dense_codes_of_the_column():
    aid = np.array(["b7", "a1", "c3", "a1", "b7", "b7", "zz"])
    kb = KnowledgeBase({"aid": aid, "row": np.arange(7)})
    stub = _Stub()
    kb.add_index("ix", stub)
    with pytest.raises(ValueError):
        kb.group_codes("ix", ["a1"])                               # no groups yet
    assert kb.set_groups("ix", "aid") is kb
    uniq = ["a1", "b7", "c3", "zz"]                                # np.unique's order: the codes are 0 .. U - 1
    assert stub.labelled.dtype == np.int32 and stub.labelled.tolist() == [uniq.index(v) for v in aid]
    q = np.zeros((5, 4), np.float32)
    vals = ["zz", "a1", "nobody", "c3", "b"]                       # two values the column does not contain ("b" sorts between members)
    scores, examples = kb.get_nearest_examples_batch("ix", q, 3, groups=vals)
    name, k, kw = stub.calls[-1]
    assert (name, k) == ("search_wide", 3) and kw["group_mode"] == "exclude" and set(kw) == {"groups", "group_mode"}
    assert kw["groups"].dtype == np.int32 and kw["groups"].tolist() == [3, 0, ram.LABEL_NONE, 2, ram.LABEL_NONE]    # nothing to exclude
    assert len(scores) == 5 and examples[0]["aid"] == ["b7", "a1", "c3"]
    kb.get_nearest_examples_batch("ix", q, 7, groups=np.array(vals), group_mode="only")
    name, k, kw = stub.calls[-1]
    assert (name, k) == ("search_wide", 7) and kw["group_mode"] == "only" and kw["groups"].tolist() == [3, 0, 4, 2, 4]   # U: no row has it
    with pytest.raises(ValueError):
        kb.get_nearest_examples_batch("ix", q, 3, groups=vals, group_mode="both")
    kb.get_nearest_examples_batch("ix", q, 3)                      # without groups: as before
    assert stub.calls[-1] == ("search", 3, {})
    ints = KnowledgeBase({"aid": [40, 10, 40, 30]})
    s2 = _Stub()
    ints.add_index("ix", s2)
    ints.set_groups("ix", "aid")
    assert s2.labelled.tolist() == [2, 0, 2, 1] and ints.group_codes("ix", [30, 20, 40], "only").tolist() == [1, 3, 2]
    kb.drop_index("ix")
    assert "ix" not in kb._groups


def test_mips_search_forwards_the_codes_of_ignore_groups():
    aid = ["p", "q", "p", "r", "q", "q"]
    m = ram.Mips(ram.MipsArgs(mips_normalize=False), data={"mips_column": [f"t{r}" for r in range(6)], "aid": aid})
    stub = _Stub()
    m.embeddings = KnowledgeBase(dict(m.data), stub, m.index_name)
    q = np.zeros((3, 4), np.float32)
    m.search(q, k=2)                                               # the defaults leave the call as it is
    assert stub.calls[-1] == ("search", 2, {}) and stub.labelled is None
    m.search(q, k=2, ignore_groups=["q", "x", "r"])                # the groups are set on first use
    assert stub.labelled.tolist() == [0, 1, 0, 2, 1, 1]
    name, k, kw = stub.calls[-1]
    assert (name, k) == ("search_wide", 2) and kw["group_mode"] == "exclude" and kw["groups"].tolist() == [1, ram.LABEL_NONE, 2]
    stub.labelled = None
    s, i = m.search(q, ignore_indexes=[1, 0, 5], k=2, ignore_groups=["q", "x", "r"])     # k + 1 fetch, then the drop
    name, k, kw = stub.calls[-1]
    assert (name, k) == ("search_wide", 3) and kw["groups"].tolist() == [1, ram.LABEL_NONE, 2] and stub.labelled is None   # set once
    assert [list(r) for r in i] == [[0, 2], [1, 2], [0, 1]]
    out = m.forward(queries=q, aid=["p", "q", "r"], k=2, ignore_own_group=True)
    name, k, kw = stub.calls[-1]
    assert (name, k) == ("search_wide", 2) and kw["groups"].tolist() == [0, 1, 2] and np.asarray(out.indices).tolist() == [[0, 1]] * 3
    m.forward(queries=q, aid=["p", "q", "r"], k=2)
    assert stub.calls[-1] == ("search", 2, {})
    with pytest.raises(ValueError):
        m.forward(queries=q, k=2, ignore_own_group=True)
