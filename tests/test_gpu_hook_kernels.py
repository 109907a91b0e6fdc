"""The kernels of the retriever scoring hook and of the facade (csrc/aux_kernels.hpp) at their edges, against float64: cosine
re-score forward and backward, l2_normalize_, rows_max_sumsq (host and device accumulator), filter_ignore, and the storage
rounding of the bf16 and e4m3 indexes.  Inputs, references, bounds and comparison functions live in tests/hook_cases.py;
tests/test_hook_cases_host.py shows on the CPU that those comparisons reject a kernel that drops a column, reads one element too
many, skips the j tail, stops at 64 memory tokens, takes the norm of the wrong row, or rounds the wrong way.

Conventions.  Numeric checks call the C ABI with raw pointers, so float32 results are seen before any cast.  Every buffer is an
interior window of a larger allocation whose guard zones hold a sentinel (floats: a NaN with a payload -- 1e30 for the maximum
norm, which ignores NaN --, int64: a fixed pattern): after each call the guards must be bit-identical, read-only inputs must
be bit-identical, and every output element must have been written.  Every output element is compared; where the float64
reference is non-finite the kernel's value must be non-finite, everywhere else the derived bound applies.

Worst error / bound ratios, MI355X next to the NumPy model of the summation order (tests/test_hook_cases_host.py):
  cosine forward               GPU 0.24   model 0.24
  cosine backward grad_query   GPU 0.14   model 0.14
  cosine backward grad_cls     GPU 0.20   model 0.20
  l2_normalize_                GPU 0.43   model 0.43
  rows_max_sumsq               GPU 0.22   model 0.22
(The tests print them; run with -s.  Several coincide with the model's to the digits shown: the model follows the kernel's order
of operations, and only the kernel's fused multiply-adds separate the two.)"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import retrieval_augmented_mds_amd as ram
from retrieval_augmented_mds_amd import _lib
from retrieval_augmented_mds_amd.index import rows_max_sumsq_into

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import hook_cases as hc
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -3
G = 256                                   # guard elements either side of every window
NAN_BITS = {2: 0x7FC1, 4: 0x7FC0CAFE, 8: 0x7FF8DEADBEEF0000}
BIG_BITS = int(np.float32(hc.MAX_GUARD).view(np.uint32))
_INT = {2: np.int16, 4: np.int32, 8: np.int64}
_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731
COSINE = [(s, t) for s in hc.FORWARD_SHAPES for t in hc.DTYPES]
BACKWARD = [(s, t) for s in hc.BACKWARD_SHAPES for t in hc.DTYPES]
_WORST = {}


def _note(key, r):
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    print(f"GPU error / bound, {key}: {r:.3f} (worst so far {_WORST[key]:.3f})")


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


class Buf:
    """A window of `data.size` elements inside one device allocation, G sentinel elements before and after it."""

    def __init__(self, data, sentinel=None):
        data = np.ascontiguousarray(data)
        it = _INT[data.dtype.itemsize]
        self.dtype, self.shape, self.n = data.dtype, data.shape, data.size
        self.sentinel = it(NAN_BITS[data.dtype.itemsize] if sentinel is None else sentinel)
        host = np.full(2 * G + self.n, self.sentinel, dtype=it)
        host[G:G + self.n] = data.view(it).ravel()
        self.before = host[G:G + self.n].copy()
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + G * host.itemsize

    @classmethod
    def out(cls, shape, dtype, sentinel=None):
        """An output window that holds the sentinel itself."""
        dtype = np.dtype(dtype)
        s = NAN_BITS[dtype.itemsize] if sentinel is None else sentinel
        return cls(np.full(shape, _INT[dtype.itemsize](s)).view(dtype), s)

    def read(self, written=False, unchanged=False):
        """The window after a call (synchronises).  The guards must hold the sentinel; written: no element of the window may
        still hold it; unchanged: the window must be what it was."""
        host = self.t.cpu().numpy()
        assert (host[:G] == self.sentinel).all(), "the guard zone before the window was written"
        assert (host[G + self.n:] == self.sentinel).all(), "the guard zone behind the window was written"
        win = host[G:G + self.n]
        if written:
            assert (win != self.sentinel).all(), f"{int((win == self.sentinel).sum())} output elements were never written"
        if unchanged:
            assert np.array_equal(win, self.before), "a read-only buffer was modified"
        return win.view(self.dtype).reshape(self.shape).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _operands(case):
    """-> (query Buf, cls Buf, dtype code): float32 as it is, bf16 as bit patterns (the case's values are bf16 values)."""
    if case.dtype == "bf16":
        return Buf(hc.bf16_round_bits(case.q)), Buf(hc.bf16_round_bits(case.c)), _lib.DTYPE_BF16
    return Buf(case.q), Buf(case.c), _lib.DTYPE_F32


# ------------------------------------------------------------------ 1. cosine re-score, forward
@pytest.mark.parametrize("shape,dtype", COSINE, ids=_ID)
def test_cosine_forward_against_float64(shape, dtype):
    lib, dev = _lib.load(), torch.cuda.current_device()
    case = hc.cosine_case(shape, dtype)
    b, k, d, L = shape
    q, c, code = _operands(case)
    out = Buf.out((b, k), np.float32)
    assert lib.mips_cosine_rescore(q.ptr, c.ptr, code, b, k, d, out.ptr, dev, _stream()) == 0
    s1 = out.read(written=True)
    _note("cosine forward", hc.compare_scores(case, s1))
    out2 = Buf.out((b, k), np.float32)
    bias = Buf.out((b, k * L), np.float32) if L else None
    assert lib.mips_cosine_rescore_bias(q.ptr, c.ptr, code, b, k, d, out2.ptr, L, bias.ptr if L else None, dev, _stream()) == 0
    s2 = out2.read(written=True)
    assert np.array_equal(_bits(s2), _bits(s1)), "the fused call scores differently"
    if L:
        assert np.array_equal(_bits(bias.read(written=True)), case.bias_ref_bits(_bits(s2)))
    q.read(unchanged=True)
    c.read(unchanged=True)


# ------------------------------------------------------------------ 2. cosine re-score, backward
def _backward(lib, dev, case, mode, q, c, code):
    b, k, d = case.b, case.k, case.d
    gs, gb, L = case.grads(mode)
    gsb = Buf(gs) if gs is not None else None
    gbb = None if gb is None else Buf(gb if gb.size else np.zeros(1, np.float32))   # (L == 0: a pointer, and nothing behind it)
    gq, gc = Buf.out((b, d), np.float32), Buf.out((b, k, d), np.float32)
    rc = lib.mips_cosine_rescore_backward(q.ptr, c.ptr, code, b, k, d, gsb.ptr if gsb else None, gbb.ptr if gbb else None, L,
                                          gq.ptr, gc.ptr, dev, _stream())
    for buf in (gsb, gbb):
        if buf is not None:
            buf.read(unchanged=True)
    return rc, gq, gc


@pytest.mark.parametrize("shape,dtype", BACKWARD, ids=_ID)
def test_cosine_backward_against_float64(shape, dtype):
    lib, dev = _lib.load(), torch.cuda.current_device()
    case = hc.cosine_case(shape, dtype)
    q, c, code = _operands(case)
    for mode in hc.BACKWARD_MODES:
        rc, gq, gc = _backward(lib, dev, case, mode, q, c, code)
        assert rc == 0
        rq, rc_ = hc.compare_backward(case, mode, gq.read(written=True), gc.read(written=True))
        _note("cosine backward grad_query", rq)
        _note("cosine backward grad_cls", rc_)
    q.read(unchanged=True)
    c.read(unchanged=True)


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_cosine_backward_refuses_k_65_and_writes_nothing(dtype):
    lib, dev = _lib.load(), torch.cuda.current_device()
    case = hc.cosine_case((1, 65, 128, 2), dtype)
    q, c, code = _operands(case)
    for mode in hc.BACKWARD_MODES:
        rc, gq, gc = _backward(lib, dev, case, mode, q, c, code)
        assert rc == E_UNSUPPORTED
        assert np.array_equal(gq.read().view(np.int32).ravel(), gq.before)
        assert np.array_equal(gc.read().view(np.int32).ravel(), gc.before)


def _leaf(values, dtype, pad_axis, requires_grad):
    """A leaf twice as long along pad_axis whose second half (axis 1: row 1 of 2) holds `values`: the view of that half is
    non-contiguous.  -> (leaf, view)."""
    v = torch.from_numpy(np.ascontiguousarray(values)).cuda().to(dtype)
    shape = list(v.shape)
    shape[pad_axis] *= 2
    leaf = torch.full(shape, 7.0, dtype=dtype, device="cuda")
    half = v.shape[pad_axis]
    leaf.narrow(pad_axis, half, half).copy_(v)
    leaf.requires_grad_(requires_grad)
    view = leaf.narrow(pad_axis, half, half)
    assert not view.is_contiguous()
    return leaf, view


def test_cosine_autograd_layer_plumbing():
    shape = (3, 5, 70, 3)
    b, k, d, L = shape
    # (a) float32, both inputs non-contiguous views of leaves, query [B, 1, d], loss over scores and bias
    case = hc.cosine_case(shape, "f32")
    qleaf, qv = _leaf(case.q.reshape(b, 1, d), torch.float32, 1, True)
    cleaf, cv = _leaf(case.c, torch.float32, 2, True)
    gs, gb = torch.from_numpy(case.gs).cuda(), torch.from_numpy(case.gb).cuda()
    sc, bias = ram.cosine_rescore(qv, cv, memory_seq_len=L)
    assert sc.dtype == torch.float32 and sc.shape == (b, k) and bias.shape == (b, k * L)
    hc.compare_scores(case, sc.detach().cpu().numpy())
    ((sc * gs).sum() + (bias * gb.reshape(b, k * L)).sum()).backward()
    assert qleaf.grad.dtype == torch.float32 and cleaf.grad.dtype == torch.float32
    assert not qleaf.grad[:, 0].any() and not cleaf.grad[:, :, :d].any()               # outside the views: nothing
    hc.compare_backward(case, "both", qleaf.grad[:, 1].cpu().numpy(), cleaf.grad[:, :, d:].cpu().numpy())

    # (b) bf16, only the query requires grad, the loss uses only the bias: bf16 gradient (2^-8 |ref| for the cast)
    case = hc.cosine_case(shape, "bf16")
    q = torch.from_numpy(case.q).cuda().bfloat16().requires_grad_(True)
    c = torch.from_numpy(case.c).cuda().bfloat16()
    gb = torch.from_numpy(case.gb).cuda()
    sc, bias = ram.cosine_rescore(q, c, memory_seq_len=L)
    (bias * gb.reshape(b, k * L)).sum().backward()
    assert q.grad.dtype == torch.bfloat16 and c.grad is None
    hc.compare_backward(case, "bias", q.grad.float().cpu().numpy(), None, cast_slack=2.0 ** -8)

    # (c) mixed dtypes: bf16 query, float32 cls, only cls requires grad, scores only
    mixed = hc.CosineCase(shape, "f32")
    mixed.q = hc.to_bf16(mixed.q)
    gs = torch.from_numpy(mixed.gs).cuda()
    q = torch.from_numpy(mixed.q).cuda().bfloat16()
    c = torch.from_numpy(mixed.c).cuda().requires_grad_(True)
    sc = ram.cosine_rescore(q, c)
    hc.compare_scores(mixed, sc.detach().cpu().numpy())
    (sc * gs).sum().backward()
    assert c.grad.dtype == torch.float32 and q.grad is None
    hc.compare_backward(mixed, "scores", None, c.grad.cpu().numpy())

    # (d) and the bf16 gradient of a bf16 query next to a float32 cls
    q = torch.from_numpy(mixed.q).cuda().bfloat16().requires_grad_(True)
    sc = ram.cosine_rescore(q, c.detach())
    (sc * gs).sum().backward()
    assert q.grad.dtype == torch.bfloat16
    hc.compare_backward(mixed, "scores", q.grad.float().cpu().numpy(), None, cast_slack=2.0 ** -8)

    # (e) no graph under no_grad
    with torch.no_grad():
        sc, bias = ram.cosine_rescore(q, c, memory_seq_len=L)
    assert not sc.requires_grad and sc.grad_fn is None and not bias.requires_grad and bias.grad_fn is None

    # (f) k = 65: the forward serves it, backward raises instead of returning garbage
    wide = hc.cosine_case((1, 65, 128, 2), "f32")
    q = torch.from_numpy(wide.q).cuda().requires_grad_(True)
    c = torch.from_numpy(wide.c).cuda().requires_grad_(True)
    sc = ram.cosine_rescore(q, c)
    hc.compare_scores(wide, sc.detach().cpu().numpy())
    with pytest.raises(RuntimeError, match="k = 65"):
        sc.sum().backward()
    assert q.grad is None and c.grad is None


# ------------------------------------------------------------------ 3. l2_normalize_
@pytest.mark.parametrize("n", hc.L2_N)
@pytest.mark.parametrize("d", hc.L2_D)
def test_l2_normalize_against_float64(n, d):
    lib, dev = _lib.load(), torch.cuda.current_device()
    case = hc.l2_case(n, d)
    x = Buf(case.x)
    assert lib.mips_l2_normalize(x.ptr, n, d, dev, _stream()) == 0
    _note("l2_normalize", hc.compare_l2(case, x.read()))


# ------------------------------------------------------------------ 4. rows_max_sumsq, rows_max_sumsq_into
def _max_host(lib, dev, xb, n, d):
    out = ctypes.c_double(-1.0)
    assert lib.mips_rows_max_sumsq(xb.ptr, n, d, ctypes.byref(out), dev, _stream()) == 0
    return out.value


def _max_into(lib, dev, xb, n, d, acc):
    assert lib.mips_rows_max_sumsq_device(xb.ptr, n, d, acc.ptr, dev, _stream()) == 0
    return acc.read()[0]


@pytest.mark.parametrize("n", hc.MAX_N)
@pytest.mark.parametrize("d", hc.MAX_D)
def test_rows_max_sumsq_against_float64(n, d):
    lib, dev = _lib.load(), torch.cuda.current_device()
    for plant in hc.max_plants(n):
        x = hc.max_matrix(n, d, plant)
        ref = hc.cached(("maxref", n, d, plant), lambda: hc.max_ref(x))
        xb = Buf(x, BIG_BITS)
        got = _max_host(lib, dev, xb, n, d)
        _note("rows_max_sumsq", hc.compare_max(d, got, ref))
        acc = Buf(np.zeros(1, np.float64))
        assert _max_into(lib, dev, xb, n, d, acc) == got          # the accumulator form: the same kernel from 0
        xb.read(unchanged=True)
    zb = Buf(np.zeros((n, d), np.float32), BIG_BITS)
    assert _max_host(lib, dev, zb, n, d) == 0.0


def test_rows_max_sumsq_accumulator_is_a_running_maximum():
    lib, dev = _lib.load(), torch.cuda.current_device()
    n, d = 20000, 3
    late = hc.max_matrix(n, d, 17000)                               # its maximum sits in the second stride pass
    small = (hc.max_matrix(n, d, 9, seed=1) * np.float32(0.25)).astype(np.float32)
    early = (hc.max_matrix(n, d, 5, seed=2) * np.float32(3.0)).astype(np.float32)    # first pass, and larger than `late`
    r_late, r_small, r_early = hc.max_ref(late), hc.max_ref(small), hc.max_ref(early)
    assert r_small < r_late < r_early
    bl, bs, be = Buf(late, BIG_BITS), Buf(small, BIG_BITS), Buf(early, BIG_BITS)
    acc = Buf(np.zeros(1, np.float64))
    a1 = _max_into(lib, dev, bl, n, d, acc)
    hc.compare_max(d, a1, r_late)                                   # 0 -> raised
    a2 = _max_into(lib, dev, bs, n, d, acc)
    assert np.float64(a2).view(np.uint64) == np.float64(a1).view(np.uint64)          # a smaller maximum: bit-identical
    a3 = _max_into(lib, dev, be, n, d, acc)
    hc.compare_max(d, a3, r_early)                                  # a larger one raises it
    a4 = _max_into(lib, dev, bl, n, d, acc)
    assert np.float64(a4).view(np.uint64) == np.float64(a3).view(np.uint64)
    # the other order: first-pass maximum first, then the larger one of the second pass
    acc = Buf(np.zeros(1, np.float64))
    _max_into(lib, dev, bs, n, d, acc)
    hc.compare_max(d, _max_into(lib, dev, bl, n, d, acc), max(r_small, r_late))
    for buf in (bl, bs, be):
        buf.read(unchanged=True)
    # the Python wrapper
    t = torch.zeros(1, dtype=torch.float64, device="cuda")
    rows_max_sumsq_into(torch.from_numpy(late).cuda(), t)
    rows_max_sumsq_into(torch.from_numpy(small).cuda(), t)
    assert t.item() == a1 and ram.rows_max_sumsq(torch.from_numpy(late).cuda()) == a1


# ------------------------------------------------------------------ 5. filter_ignore
@pytest.mark.parametrize("kf,k", hc.FILTER_K)
@pytest.mark.parametrize("nq", hc.FILTER_NQ)
def test_filter_ignore_pads_what_it_does_not_fill(nq, kf, k):
    lib, dev = _lib.load(), torch.cuda.current_device()
    case = hc.filter_case(nq, kf, k)
    s, i, ign = Buf(case.score_bits), Buf(case.ids, 0x5A5A5A5A5A5A5A5A), Buf(case.ignore, 0x5A5A5A5A5A5A5A5A)
    # twice, into buffers that held different things: what is stale in one run is not in the other
    for sent_i, sent_s in ((0x5A5A5A5A5A5A5A5A, 0x7FC0BEEF), (0x0707070707070707, 0x3F800000)):
        out_s, out_i = Buf.out((nq, k), np.uint32, sent_s), Buf.out((nq, k), np.int64, sent_i)
        assert lib.mips_filter_ignore(s.ptr, i.ptr, ign.ptr, nq, kf, k, out_s.ptr, out_i.ptr, dev, _stream()) == 0
        hc.compare_filter(case, out_s.read(), out_i.read(written=True))
    for buf in (s, i, ign):
        buf.read(unchanged=True)
    # the wrapper: the same through torch tensors
    ts = torch.from_numpy(case.score_bits.view(np.float32)).cuda()
    fs, fi = ram.filter_ignore(ts, torch.from_numpy(case.ids).cuda(), torch.from_numpy(case.ignore).cuda(), k)
    hc.compare_filter(case, _bits(fs.cpu().numpy()), fi.cpu().numpy())


# ------------------------------------------------------------------ 6. storage rounding, exhaustive
def _nan32(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def test_bf16_index_rounds_every_float32_pattern_to_nearest_even():
    x = hc.rounding_inputs_bf16()
    ix = ram.MipsIndex(768, dtype="bf16")
    ix.add(x)
    hc.compare_codes(ix.rows_bf16(), hc.bf16_round_bits(x), _nan32(x), 0x7F80, 0x8000)


def test_e4m3_index_rounds_every_bf16_pattern_to_the_nearest_code():
    b = hc.rounding_inputs_e4m3_from_bf16()
    x = hc.bf16_to_f32(b)
    ix = ram.MipsIndex(768, dtype="fp8_e4m3")
    ix.add(b)                                                        # np.uint16: bf16 bit patterns
    hc.compare_codes(ix.rows_raw(), hc.e4m3_nearest_bits(x), _nan32(x), 0x7F, 0x80)


def test_e4m3_index_rounds_float32_to_the_nearest_code():
    x = hc.rounding_inputs_e4m3_from_f32()
    ix = ram.MipsIndex(768, dtype="fp8_e4m3")
    ix.add(x)
    hc.compare_codes(ix.rows_raw(), hc.e4m3_nearest_bits(x), _nan32(x), 0x7F, 0x80)
