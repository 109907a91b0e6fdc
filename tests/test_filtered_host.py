"""CPU tests of the filtered-search surface: the C ABI declares and the binding binds mips_search_wide_sel / mips_range_search_sel,
the packing of ram.Selector and of every faiss_shim selector class agrees with np.packbits(bitorder="little"), and route_search
sends a call that carries selector= to search_wide."""
import os
import re

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(header, name):
    m = re.search(rf"int {name}\(([^;]*)\);", header)
    assert m, f"{name} is not declared in mips_hip.h"
    return [p.strip() for p in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_and_binding_binds_the_selector_entry_points():
    header = open(os.path.join(ROOT, "include", "mips_hip.h")).read()
    wide = _params(header, "mips_search_wide_sel")
    rng = _params(header, "mips_range_search_sel")
    assert len(wide) == 13 and wide[9].startswith("const uint8_t* sel_bits") and "sel_nbits" in wide[10] and "sel_bit0" in wide[11]
    assert len(rng) == 15 and rng[11].startswith("const uint8_t* sel_bits") and "sel_nbits" in rng[12] and "sel_bit0" in rng[13]
    assert wide[:9] == _params(header, "mips_search_wide")[:9] and rng[:11] == _params(header, "mips_range_search")[:11]
    assert int(re.search(r"#define MIPS_SEL_DEVICE (\d+)", header).group(1)) == ram._lib.SEL_DEVICE == 16
    assert int(re.search(r"#define MIPS_ABI_VERSION (\d+)", header).group(1)) == ram._lib.ABI_VERSION == 1
    assert "mips_search_wide_sel" in ram._lib.EXPORTS and "mips_range_search_sel" in ram._lib.EXPORTS
    lib = ram._lib.load()                                          # builds, loads and binds: AttributeError if a symbol is missing
    assert len(lib.mips_search_wide_sel.argtypes) == 13 and len(lib.mips_range_search_sel.argtypes) == 15
    assert lib.mips_abi_version() == 1


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 777, 4099])
def test_selector_packing_agrees_with_packbits(n):
    import torch

    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.4
    want = np.packbits(mask, bitorder="little")
    S = ram.Selector
    for built in (S.from_mask(mask, device="cpu"), S.from_mask(torch.from_numpy(mask), device="cpu"),
                  S.from_ids(np.flatnonzero(mask), n, device="cpu"), S.from_ids(np.repeat(np.flatnonzero(mask), 2)[::-1].copy(), n, device="cpu"),
                  S.from_bitmap(want, n, device="cpu"), S.from_bitmap(np.concatenate([want, [255, 255]]).astype(np.uint8), n, device="cpu")):
        assert built.nbits == n and built.bits.dtype == torch.uint8 and built.bits.shape == ((n + 7) // 8,)
        assert np.array_equal(built.numpy(), want) and np.array_equal(built.mask(), mask) and built.count() == int(mask.sum())
    inv = S.from_mask(mask, device="cpu").invert()
    assert np.array_equal(inv.numpy(), np.packbits(~mask, bitorder="little")) and inv.nbits == n    # bits past n stay clear
    assert np.array_equal(inv.invert().numpy(), want)
    lo, hi = n // 3, n - n // 4
    rmask = np.zeros(n, bool)
    rmask[lo:hi] = True
    assert np.array_equal(S.from_range(lo, hi, n, device="cpu").numpy(), np.packbits(rmask, bitorder="little"))
    assert np.array_equal(S.from_range(-5, n + 9, n, device="cpu").numpy(), np.packbits(np.ones(n, bool), bitorder="little"))
    assert S.from_bitmap(np.full((n + 7) // 8, 255, np.uint8), n, device="cpu").count() == n         # the tail of a bitmap is dropped
    with pytest.raises(ValueError):
        S.from_ids([n], n, device="cpu")
    with pytest.raises(ValueError):
        S.from_bitmap(np.zeros(max(0, (n + 7) // 8 - 1), np.uint8), n, device="cpu")


@pytest.mark.parametrize("n", [5, 64, 1001])
def test_faiss_shim_selector_bitmaps_agree_with_packbits(n):
    fs = ram.faiss_shim
    rng = np.random.default_rng(100 + n)
    mask = rng.random(n) < 0.3
    ids = np.flatnonzero(mask)
    want = np.packbits(mask, bitorder="little")
    for cls in (fs.IDSelectorBatch, fs.IDSelectorArray):
        assert np.array_equal(cls(ids).bitmap(n), want)
        assert np.array_equal(cls(np.concatenate([ids, [n, n + 100, -1]])).bitmap(n), want)         # ids the index does not hold select nothing
        assert np.array_equal(cls(len(ids), ids).bitmap(n), want)                                    # the SWIG spelling (n, ids)
    assert np.array_equal(fs.IDSelectorBitmap(want).bitmap(n), want)
    assert np.array_equal(fs.IDSelectorBitmap(len(want), want).bitmap(n), want)
    assert np.array_equal(fs.IDSelectorBitmap(want[:-1]).bitmap(n), np.packbits(np.where(np.arange(n) < 8 * (len(want) - 1), mask, False), bitorder="little"))
    assert np.array_equal(fs.IDSelectorNot(fs.IDSelectorBatch(ids)).bitmap(n), np.packbits(~mask, bitorder="little"))
    lo, hi = n // 4, n - 2
    rmask = (np.arange(n) >= lo) & (np.arange(n) < hi)
    assert np.array_equal(fs.IDSelectorRange(lo, hi).bitmap(n), np.packbits(rmask, bitorder="little"))
    assert np.array_equal(fs.IDSelectorNot(fs.IDSelectorRange(lo, hi)).bitmap(n), np.packbits(~rmask, bitorder="little"))
    assert fs.IDSelectorRange(lo, hi).is_member(lo) and not fs.IDSelectorRange(lo, hi).is_member(hi)
    assert fs.SearchParameters().sel is None and fs.SearchParameters(sel=fs.IDSelectorRange(0, 1)).sel.imax == 1


class _Stub:
    """A duck-typed index that records which of its two searches was called."""

    def __init__(self):
        self.calls = []

    def search(self, q, k, **kw):
        self.calls.append(("search", k, kw))
        return "narrow"

    def search_wide(self, q, k, **kw):
        self.calls.append(("search_wide", k, kw))
        return "wide"


def test_route_search_sends_a_selector_call_to_search_wide():
    route = ram.index.route_search
    stub = _Stub()
    sel = object()
    assert route(stub, None, 5, selector=sel) == "wide"                                  # whatever k is
    assert route(stub, None, 100, selector=sel, force_ip=True) == "wide"
    assert route(stub, None, 5) == "narrow" and route(stub, None, 5, selector=None) == "narrow"
    assert route(stub, None, 100, selector=None) == "wide"
    assert stub.calls == [("search_wide", 5, {"selector": sel}), ("search_wide", 100, {"selector": sel, "force_ip": True}),
                          ("search", 5, {}), ("search", 5, {}), ("search_wide", 100, {})]


def test_faiss_shim_passes_params_and_refuses_other_keywords():
    fs = ram.faiss_shim
    fx = fs.IndexFlatIP(16)
    stub = fx._inner = _Stub()
    stub.ntotal = 20
    q = np.zeros((2, 16), np.float32)
    assert fx.search(q, 5) == "narrow" and fx.search(q, 5, params=None) == "narrow" and fx.search(q, 5, params=fs.SearchParameters()) == "narrow"
    assert fx.search(q, 5, params=fs.SearchParameters(sel=fs.IDSelectorRange(3, 9))) == "wide"
    name, k, kw = stub.calls[-1]
    assert (name, k) == ("search_wide", 5) and np.array_equal(kw["selector"], np.packbits((np.arange(20) >= 3) & (np.arange(20) < 9), bitorder="little"))
    with pytest.raises(TypeError):
        fx.search(q, 5, parms=None)
    with pytest.raises(TypeError):
        fx.range_search(q, 0.5, sel=None)
