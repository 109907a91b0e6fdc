"""MipsIndex -- the faiss.IndexFlat-shaped object the reference reaches through
`self.embeddings.get_index(self.index_name).faiss_index` (sotasum/mips.py:383-386, 342-345).

Duck type kept:  d, ntotal, metric_type, nprobe (settable, ignored: the index is exact),
add(x), search(x, k) -> (D float32 [nq,k], I int64 [nq,k]), reset().
Extensions: torch CUDA tensors in -> torch CUDA tensors out (no host hop), add_synthetic,
save/load of the raw bf16 shard, last_scan_ms for the bench.

All arithmetic happens in libmips_hip.so (hand-written HIP, gfx950); this file only moves
pointers.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading

import numpy as np

from . import _lib

_FORMAT_VERSION = 1


def _stream_handle(device: int) -> int:
    import torch

    return int(torch.cuda.current_stream(device).cuda_stream)


def as_labels(a, what: str, device: int | None = None):
    """An int array (NumPy / sequence -> host, torch CUDA tensor -> device) as contiguous 1-d int32 labels; values outside
    int32 raise ValueError.  A CUDA tensor that is not int32 already is range-checked on the host, which synchronises.
    -> (np.ndarray | CUDA tensor, is_device)"""
    import torch

    lo, hi = -(1 << 31), (1 << 31) - 1
    if isinstance(a, torch.Tensor):
        if a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool:
            raise ValueError(f"{what}: expected integers, got {a.dtype}")
        a = a.reshape(-1)
        if a.is_cuda:
            if a.dtype != torch.int32:
                if a.numel() and (int(a.min()) < lo or int(a.max()) > hi):
                    raise ValueError(f"{what}: values outside int32")
                a = a.to(torch.int32)
            if device is not None and a.device.index != device:
                a = a.to(f"cuda:{device}")
            return a.contiguous(), True
        a = a.numpy()
    a = np.asarray(a).reshape(-1)
    if a.size == 0:
        return np.zeros(0, np.int32), False
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: expected integers, got {a.dtype}")
    if a.dtype != np.int32 and (int(a.min()) < lo or int(a.max()) > hi):
        raise ValueError(f"{what}: values outside int32")
    return np.ascontiguousarray(a, dtype=np.int32), False


_GROUP_MODES = {"exclude": _lib.GRP_EXCLUDE, "only": _lib.GRP_ONLY}


def route_search(index, q, k: int, **kwargs):
    """index.search(q, k), or index.search_wide(q, k) when k exceeds MAX_K and the index has a wide search (MipsIndex and
    ShardedMipsIndex do; foreign duck-typed indexes keep their own search and its limits).  A call carrying selector= (a
    filtered search) or groups= (a grouped one) goes to search_wide whatever k is: search() itself has neither."""
    if "groups" in kwargs and kwargs["groups"] is None:
        kwargs = {key: v for key, v in kwargs.items() if key not in ("groups", "group_mode")}
    if "selector" in kwargs and kwargs["selector"] is None:
        kwargs = {key: v for key, v in kwargs.items() if key != "selector"}
    if hasattr(index, "search_probed"):  # an IvfIndex: the probed lists under the same filters; its nprobe attribute decides
        if int(k) > _lib.MAX_K:
            raise NotImplementedError(f"an IVF index serves k <= {_lib.MAX_K} (search_probed); got k = {int(k)}")
        if kwargs.pop("force_ip", False):
            raise NotImplementedError("force_ip on an IVF index: the exhaustive cross-check goes to its flat index")
        return index.search_probed(q, int(k), **kwargs)
    if "selector" in kwargs or "groups" in kwargs:
        return index.search_wide(q, int(k), **kwargs)
    if int(k) > _lib.MAX_K and hasattr(index, "search_wide"):
        return index.search_wide(q, int(k), **kwargs)
    return index.search(q, k, **kwargs)


# file extension and element type of the stored rows, by index dtype (save / load)
_ROWS_FILE = {"bf16": ("bf16", np.uint16), "fp8_e4m3": ("e4m3", np.uint8), "fp8_e4m3_docs": ("e4m3", np.uint8), "f32": ("f32", np.float32),
              "sq8": ("sq8", np.uint8)}


class MipsIndex:
    def __init__(self, d: int, metric: int = _lib.METRIC_IP, dtype: str = "bf16", device: int | None = None):
        if dtype not in ("bf16", "fp8_e4m3", "fp8_e4m3_docs", "f32", "sq8"):
            raise NotImplementedError(f"index dtype {dtype!r}: this build stores 'bf16', 'fp8_e4m3' (queries e4m3 too), "
                                      "'fp8_e4m3_docs' (e4m3 rows, bf16 queries), 'sq8' (trained 8-bit codes) or 'f32'")
        if dtype == "sq8" and int(metric) != _lib.METRIC_IP:
            raise NotImplementedError("an 'sq8' index ranks by inner product only: the L2 rule |q|^2 + phi - 2 q.x presumes rows of "
                                      "constant norm, which decoded SQ8 rows are not")
        self._lib = _lib.load()
        self.device = _lib.require_gpu(device)
        self._h = ctypes.c_void_p()
        self._code = {"bf16": _lib.DTYPE_BF16, "fp8_e4m3": _lib.DTYPE_FP8_E4M3, "fp8_e4m3_docs": _lib.DTYPE_FP8_E4M3_DOCS,
                      "f32": _lib.DTYPE_F32, "sq8": _lib.DTYPE_SQ8}[dtype]
        self._f8 = self._code in (_lib.DTYPE_FP8_E4M3, _lib.DTYPE_FP8_E4M3_DOCS)   # e4m3 storage
        self._sq8 = self._code == _lib.DTYPE_SQ8   # trained 8-bit codes (faiss "SQ8"): train() before add()
        _lib.check(self._lib.mips_index_create(ctypes.byref(self._h), self.device, int(d), self._code,
                                               int(metric)), "mips_index_create")
        self._d = int(d)
        self._metric = int(metric)
        self.dtype = dtype
        self.nprobe = 1  # accepted for drop-in compatibility (mips.py:342-345); exact search ignores it
        self._mutex = threading.Lock()
        self._nlabelled = 0  # rows [0, _nlabelled) carry a group label (set_labels)

    # ------------------------------------------------------------------ faiss-like attributes
    @property
    def d(self) -> int:
        return self._d

    @property
    def ntotal(self) -> int:
        return int(self._lib.mips_index_ntotal(self._h))

    @property
    def metric_type(self) -> int:
        return self._metric

    @property
    def is_trained(self) -> bool:
        """faiss Index.is_trained: False only on an 'sq8' index before train() / set_sq8_params()."""
        return not self._sq8 or self._lib.mips_index_sq8_is_trained(self._h) == 1

    def __len__(self) -> int:
        return self.ntotal

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.mips_index_destroy(h)
            except Exception:
                pass
            h.value = None

    # ------------------------------------------------------------------ helpers
    def _as_buffer(self, x, what: str):
        """-> (pointer, dtype code, is_device, n, keepalive)"""
        import torch

        if isinstance(x, torch.Tensor):
            if x.dim() != 2 or x.shape[1] != self._d:
                raise ValueError(f"{what}: expected [n, {self._d}], got {tuple(x.shape)}")
            if x.dtype == torch.float32:
                code = _lib.DTYPE_F32
            elif x.dtype == torch.bfloat16:
                code = _lib.DTYPE_BF16
            elif x.dtype == getattr(torch, "float8_e4m3fn", None) and self._f8 and not (what == "search" and self._code == _lib.DTYPE_FP8_E4M3_DOCS):
                code = _lib.DTYPE_FP8_E4M3  # raw e4m3 bytes
            elif x.dtype == torch.uint8 and self._sq8:
                if what != "add":
                    raise ValueError(f"{what}: an 'sq8' index takes float32 / bfloat16 queries; uint8 codes are rows only")
                code = _lib.DTYPE_SQ8  # raw codes
            else:
                x = x.float()
                code = _lib.DTYPE_F32
            x = x.contiguous()
            if x.is_cuda:
                if x.device.index != self.device:
                    x = x.to(f"cuda:{self.device}")
                return x.data_ptr(), code, 1, x.shape[0], x
            return x.data_ptr(), code, 0, x.shape[0], x
        a = np.asarray(x)
        if a.ndim != 2 or a.shape[1] != self._d:
            raise ValueError(f"{what}: expected [n, {self._d}], got {a.shape}")
        if a.dtype == np.uint16:  # raw bf16 bit patterns
            a = np.ascontiguousarray(a)
            return a.ctypes.data, _lib.DTYPE_BF16, 0, a.shape[0], a
        if a.dtype == np.uint8 and self._f8 and not (what == "search" and self._code == _lib.DTYPE_FP8_E4M3_DOCS):  # raw e4m3 codes
            a = np.ascontiguousarray(a)
            return a.ctypes.data, _lib.DTYPE_FP8_E4M3, 0, a.shape[0], a
        if a.dtype == np.uint8 and self._sq8:
            if what != "add":
                raise ValueError(f"{what}: an 'sq8' index takes float32 queries; uint8 codes are rows only")
            a = np.ascontiguousarray(a)
            return a.ctypes.data, _lib.DTYPE_SQ8, 0, a.shape[0], a  # raw codes
        a = np.ascontiguousarray(a, dtype=np.float32)
        return a.ctypes.data, _lib.DTYPE_F32, 0, a.shape[0], a

    # ------------------------------------------------------------------ building
    def reserve(self, n: int) -> None:
        _lib.check(self._lib.mips_index_reserve(self._h, int(n)), "mips_index_reserve")

    def train(self, x) -> None:
        """faiss Index.train.  An 'sq8' index learns its per-column range from x [n, d] (float32 / bfloat16, host or device:
        vmin = column minimum, vdiff = column maximum - vmin; NaN or infinite values and n = 0 raise) and must be trained
        before add(); training again is possible while the index is empty.  Every other storage has nothing to train."""
        if not self._sq8:
            return
        ptr, code, is_dev, n, keep = self._as_buffer(x, "train")
        with self._mutex:
            _lib.check(self._lib.mips_index_sq8_train(self._h, ptr, n, code, _lib.Q_DEVICE if is_dev else 0, _stream_handle(self.device)),
                       "mips_index_sq8_train")
        del keep

    def sq8_params(self):
        """(vmin, vdiff): the trained per-column range of an 'sq8' index, np.float32 [d] each."""
        if not self._sq8:
            raise TypeError("sq8_params: not an 'sq8' index")
        vmin, vdiff = np.empty(self._d, np.float32), np.empty(self._d, np.float32)
        with self._mutex:
            _lib.check(self._lib.mips_index_sq8_get_params(self._h, vmin.ctypes.data, vdiff.ctypes.data), "mips_index_sq8_get_params")
        return vmin, vdiff

    def set_sq8_params(self, vmin, vdiff) -> None:
        """Set the per-column range of an EMPTY 'sq8' index instead of training it (load does; finite values, vdiff >= 0)."""
        if not self._sq8:
            raise TypeError("set_sq8_params: not an 'sq8' index")
        vmin = np.ascontiguousarray(np.asarray(vmin, dtype=np.float32).reshape(-1))
        vdiff = np.ascontiguousarray(np.asarray(vdiff, dtype=np.float32).reshape(-1))
        if vmin.shape != (self._d,) or vdiff.shape != (self._d,):
            raise ValueError(f"set_sq8_params: expected two arrays of {self._d}")
        with self._mutex:
            _lib.check(self._lib.mips_index_sq8_set_params(self._h, vmin.ctypes.data, vdiff.ctypes.data), "mips_index_sq8_set_params")

    def add(self, x) -> None:
        """faiss Index.add: append rows (np.float32 / np.uint16 bf16 bits / torch float32|bfloat16,
        host or device).  float32 is rounded to bf16 (RNE) on the device.  An 'sq8' index encodes with its trained range
        (np.uint8 / torch.uint8: raw codes) and raises before train()."""
        if self._sq8 and not self.is_trained:
            raise RuntimeError("add: the 'sq8' index is not trained (train(x) first, as faiss requires)")
        ptr, code, is_dev, n, keep = self._as_buffer(x, "add")
        with self._mutex:
            _lib.check(self._lib.mips_index_add(self._h, ptr, n, code, is_dev, _stream_handle(self.device)),
                       "mips_index_add")
        del keep

    def add_synthetic(self, n: int, row0: int = 0, seed: int = 0xD0C5, kind: int = _lib.SYNTH_GAUSS) -> None:
        with self._mutex:
            _lib.check(self._lib.mips_index_add_synthetic(self._h, int(n), int(row0), int(seed), int(kind),
                                                          _stream_handle(self.device)), "mips_index_add_synthetic")

    def reset(self) -> None:
        _lib.check(self._lib.mips_index_reset(self._h), "mips_index_reset")
        self._nlabelled = 0

    def remove_ids(self, sel, sel_bit0: int = 0) -> int:
        """faiss IndexFlat.remove_ids: take the selected rows out, in place (mips_index_remove).  The surviving rows keep their
        order and are renumbered 0 .. ntotal - 1; labels follow their rows; phi and the row-norm maxima follow the stored rows
        (a set_phi override stays).  sel: a Selector, a bool mask, a NumPy or torch uint8 bitmap, or an integer array / tensor
        of row ids (duplicates allowed); bit sel_bit0 + i of a bitmap or mask decides local row i, ids count from sel_bit0 too.
        SYNCHRONISES the current stream once.  -> the number of rows removed."""
        from .selector import Selector, is_id_list

        sel_bit0 = int(sel_bit0)
        is_ids = is_id_list(sel)
        with self._mutex:
            if is_ids:
                sel = Selector.from_ids(sel, sel_bit0 + self.ntotal, device=self.device)
            ptr, nbits, flag, keep = self._sel_args(sel, sel_bit0, "remove_ids")
            counts = (ctypes.c_int64 * 2)()
            _lib.check(self._lib.mips_index_remove(self._h, ptr, nbits, sel_bit0, flag, counts, _stream_handle(self.device)),
                       "mips_index_remove")
            self._nlabelled = int(counts[1])
        del keep
        return int(counts[0])

    def _update_args(self, ids, x, what: str):
        """(ids pointer, rows pointer, n, dtype code, flags, keepalives) of mips_index_update / mips_ivf_update."""
        iptr, shape, ids_dev, keep_ids = self._ids_arg(ids, what)
        if len(shape) != 1:
            raise ValueError(f"{what}: expected ids [n], got {shape}")
        xptr, code, x_dev, n, keep_x = self._as_buffer(x, "add")   # (rows are taken as add() takes them, raw codes included)
        if n != shape[0]:
            raise ValueError(f"{what}: {shape[0]} ids for {n} rows")
        flags = (_lib.IDS_DEVICE if ids_dev else 0) | (_lib.Q_DEVICE if x_dev else 0)
        return iptr, xptr, n, code, flags, (keep_ids, keep_x)

    def update_rows(self, ids, x, idx_offset: int = 0, return_count: bool = False):
        """Overwrite stored rows in place (mips_index_update): for p = 0 .. n - 1, row ids[p] - idx_offset becomes x[p], converted
        as add() converts it.  An id that names no local row (negative, below idx_offset, past the index) is skipped; of several
        positions that name one row the last wins.  Row numbers, labels and ntotal stay; afterwards the index equals a fresh one
        that was given the final rows -- stored bytes and every search, bit for bit.  ids: an integer array [n] (NumPy ->
        host, CUDA tensor -> device); x [n, d] as add() takes it, host or device.  With CUDA ids and rows and return_count=False
        nothing synchronises (an L2 index recomputes phi in its next search).  return_count=True -> the number of distinct rows
        written (synchronises)."""
        iptr, xptr, n, code, flags, keep = self._update_args(ids, x, "update_rows")
        count = ctypes.c_int64(0)
        with self._mutex:
            _lib.check(self._lib.mips_index_update(self._h, iptr, n, int(idx_offset), xptr, code, flags,
                                                   ctypes.byref(count) if return_count else None, _stream_handle(self.device)),
                       "mips_index_update")
        del keep
        return int(count.value) if return_count else None

    def set_labels(self, labels, row0: int = 0) -> None:
        """One int32 group label per row for rows [row0, row0 + len(labels)) (NumPy or torch int array, host or CUDA): what
        groups= of search_wide / range_search tests.  The labelled rows are a prefix of the index -- row0 may not lie behind
        the rows labelled so far -- so a build that adds in batches labels as it goes; labelled rows may be rewritten.  The
        labels survive reserve() and growth; reset() clears them."""
        lab, is_dev = as_labels(labels, "set_labels", self.device)
        n, row0 = int(lab.shape[0]), int(row0)
        if row0 < 0 or row0 + n > self.ntotal:
            raise ValueError(f"set_labels: rows [{row0}, {row0 + n}) of an index of {self.ntotal}")
        if row0 > self._nlabelled:
            raise ValueError(f"set_labels: row0 = {row0} leaves a gap behind the {self._nlabelled} labelled rows")
        with self._mutex:
            _lib.check(self._lib.mips_index_set_labels(self._h, lab.data_ptr() if is_dev else lab.ctypes.data, row0, n, int(is_dev),
                                                       _stream_handle(self.device)), "mips_index_set_labels")
            self._nlabelled = max(self._nlabelled, row0 + n)
        del lab

    def labels(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """The labels of the labelled rows [row0, row0 + n) as np.int32 (n = None: up to the last labelled row)."""
        n = self._nlabelled - int(row0) if n is None else int(n)
        if row0 < 0 or n < 0 or row0 + n > self._nlabelled:
            raise ValueError(f"labels: rows [{row0}, {row0 + n}) of {self._nlabelled} labelled rows")
        out = np.empty(n, dtype=np.int32)
        with self._mutex:
            _lib.check(self._lib.mips_index_read_labels(self._h, int(row0), n, out.ctypes.data, _stream_handle(self.device)),
                       "mips_index_read_labels")
        return out

    def _grp_args(self, groups, group_mode, nq: int, what: str):
        """groups (None | int array [nq]: NumPy -> host, CUDA tensor -> device) -> (pointer, mode, flag, keepalive) of the
        *_grp entry points."""
        if groups is None:
            return None, 0, 0, None
        if group_mode not in _GROUP_MODES:
            raise ValueError(f"{what}: group_mode must be 'exclude' or 'only', got {group_mode!r}")
        if self._nlabelled != self.ntotal:
            raise ValueError(f"{what}: groups= needs a label on every row; {self._nlabelled} of {self.ntotal} rows carry one (set_labels)")
        g, is_dev = as_labels(groups, what + ": groups", self.device)
        if g.shape[0] != nq:
            raise ValueError(f"{what}: expected {nq} group labels, got {g.shape[0]}")
        return (g.data_ptr() if is_dev else g.ctypes.data), _GROUP_MODES[group_mode], (_lib.GRP_DEVICE if is_dev else 0), g

    def phi(self) -> float:
        out = ctypes.c_double()
        _lib.check(self._lib.mips_index_phi(self._h, ctypes.byref(out), _stream_handle(self.device)), "mips_index_phi")
        return out.value

    def set_phi(self, phi: float) -> None:
        """Override phi (row-sharded L2 indexes: the maximum over all shards)."""
        _lib.check(self._lib.mips_index_set_phi(self._h, float(phi)), "mips_index_set_phi")

    def clear_phi(self) -> None:
        """Drop a set_phi override: phi() is this shard's own maximum again (recomputed from the stored rows)."""
        _lib.check(self._lib.mips_index_set_phi(self._h, -1.0), "mips_index_set_phi")

    def rows_raw(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """Stored rows in the index dtype: np.uint16 bf16 bits, np.uint8 e4m3 codes or np.float32, [n, d]."""
        n = self.ntotal - row0 if n is None else n
        npdt = self._RAW_NP[self._code]
        out = np.empty((n, self._d), dtype=npdt)
        _lib.check(self._lib.mips_index_read_rows(self._h, int(row0), int(n), out.ctypes.data,
                                                  _stream_handle(self.device)), "mips_index_read_rows")
        return out

    def rows_bf16(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """Stored rows as bf16 bit patterns, np.uint16 [n, d]."""
        if self._code != _lib.DTYPE_BF16:
            raise TypeError("rows_bf16 on an fp8 index: use rows_raw")
        n = self.ntotal - row0 if n is None else n
        out = np.empty((n, self._d), dtype=np.uint16)
        _lib.check(self._lib.mips_index_read_rows(self._h, int(row0), int(n), out.ctypes.data,
                                                  _stream_handle(self.device)), "mips_index_read_rows")
        return out

    # ------------------------------------------------------------------ rows by id (include/mips_hip_rows.h)
    _RAW_NP = {_lib.DTYPE_BF16: np.uint16, _lib.DTYPE_FP8_E4M3: np.uint8, _lib.DTYPE_FP8_E4M3_DOCS: np.uint8, _lib.DTYPE_F32: np.float32,
               _lib.DTYPE_SQ8: np.uint8}

    def _ids_arg(self, ids, what: str):
        """ids of any shape (NumPy / sequence -> host, CUDA tensor -> device) -> (pointer, shape, is_device, keepalive)."""
        import torch

        if isinstance(ids, torch.Tensor):
            if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
                raise ValueError(f"{what}: expected integer ids, got {ids.dtype}")
            if ids.is_cuda:
                if ids.device.index != self.device:
                    ids = ids.to(f"cuda:{self.device}")
                t = ids.to(torch.int64).contiguous()
                return t.data_ptr(), tuple(t.shape), True, t
            ids = ids.numpy()
        a = np.asarray(ids)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"{what}: expected integer ids, got {a.dtype}")
        if a.size and a.dtype.kind == "u" and int(a.max()) > np.iinfo(np.int64).max:
            raise ValueError(f"{what}: id {int(a.max())} does not fit int64")   # (the cast below would make it negative: "no row")
        a = np.ascontiguousarray(a, dtype=np.int64)
        return a.ctypes.data, a.shape, False, a

    def reconstruct_batch(self, ids, raw: bool = False, idx_offset: int = 0, out=None, zero_missing: bool = False):
        """The stored rows ids[...] - idx_offset -> [..., d] (faiss Index.reconstruct_batch; mips_index_reconstruct, one
        launch).  float32: the decoded values, exactly what the searches score (an "f32" index: the float32 values it was
        given, bit for bit); raw=True: the storage's own bits (np.uint16 / torch.bfloat16, np.uint8 / torch.uint8 e4m3 codes,
        float32).  NumPy ids -> NumPy result; an id >= ntotal raises.  A CUDA tensor -> a CUDA tensor, stream-ordered, nothing
        synchronises, and an id that names no row (negative, as the -1 padding of a search, or past the index) gives a NaN
        row -- zero_missing=True: zero bytes.  out= (CUDA ids only): a caller-allocated CUDA tensor [..., d] of the result's
        dtype whose last dimension is contiguous and whose leading dimensions collapse to one row pitch >= d (a slice of
        wider rows); the elements between its rows are not written."""
        import torch

        ptr, shape, is_dev, keep = self._ids_arg(ids, "reconstruct_batch")
        n = int(np.prod(shape, dtype=np.int64))
        out_dtype = _lib.DTYPE_F32 if not raw else (_lib.DTYPE_FP8_E4M3 if self._f8 else self._code)
        flags = _lib.ROWS_ZERO_MISSING if zero_missing else 0
        if is_dev:
            tdt = torch.float32 if (not raw or self._code == _lib.DTYPE_F32) else torch.uint8 if (self._f8 or self._sq8) else torch.bfloat16
            if out is None:
                out = torch.empty(shape + (self._d,), dtype=tdt, device=f"cuda:{self.device}")
                out_ld = self._d
            else:
                if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device.index == self.device and out.dtype == tdt
                        and tuple(out.shape) == shape + (self._d,)):
                    raise ValueError(f"reconstruct_batch: out must be a CUDA {tdt} tensor {shape + (self._d,)} on cuda:{self.device}")
                try:
                    flat = out.view(n, self._d) if n else out
                except RuntimeError:                         # the leading dimensions have no common pitch
                    raise ValueError("reconstruct_batch: the leading dimensions of out do not collapse to one row pitch") from None
                out_ld = int(flat.stride(0)) if n > 1 else self._d
                if n and (flat.stride(1) != 1 or out_ld < self._d):
                    raise ValueError("reconstruct_batch: out needs a contiguous last dimension and a row pitch >= d")
            optr, flags = out.data_ptr(), flags | _lib.IDS_DEVICE | _lib.OUT_DEVICE
        else:
            if out is not None:
                raise ValueError("reconstruct_batch: out= goes with CUDA ids")
            out = np.empty(shape + (self._d,), dtype=self._RAW_NP[self._code] if raw else np.float32)
            optr, out_ld = out.ctypes.data, self._d
        with self._mutex:
            _lib.check(self._lib.mips_index_reconstruct(self._h, ptr, n, int(idx_offset), optr, out_dtype, out_ld, flags,
                                                        _stream_handle(self.device)), "mips_index_reconstruct")
        del keep
        return out

    def reconstruct(self, key: int) -> np.ndarray:
        """faiss Index.reconstruct: stored row `key` as np.float32 [d]; IndexError outside [0, ntotal)."""
        key = int(key)
        if not 0 <= key < self.ntotal:
            raise IndexError(f"reconstruct: row {key} of an index of {self.ntotal}")
        return self.reconstruct_batch(np.array([key], dtype=np.int64))[0]

    def reconstruct_n(self, n0: int = 0, ni: int | None = None) -> np.ndarray:
        """faiss Index.reconstruct_n: stored rows [n0, n0 + ni) as np.float32 [ni, d] (ni = None: up to the last row)."""
        n0 = int(n0)
        ni = self.ntotal - n0 if ni is None else int(ni)
        if n0 < 0 or ni < 0 or n0 + ni > self.ntotal:
            raise IndexError(f"reconstruct_n: rows [{n0}, {n0 + ni}) of an index of {self.ntotal}")
        return self.reconstruct_batch(np.arange(n0, n0 + ni, dtype=np.int64))

    def labels_of(self, ids, idx_offset: int = 0):
        """The labels (set_labels) of rows ids[...] - idx_offset -> int32 [...]; LABEL_NONE for an id that names no row and for
        rows behind the labelled prefix.  NumPy ids -> NumPy; a CUDA tensor -> a CUDA tensor, nothing synchronises."""
        import torch

        ptr, shape, is_dev, keep = self._ids_arg(ids, "labels_of")
        n = int(np.prod(shape, dtype=np.int64))
        if is_dev:
            out = torch.empty(shape, dtype=torch.int32, device=f"cuda:{self.device}")
            optr, flags = out.data_ptr(), _lib.IDS_DEVICE | _lib.OUT_DEVICE
        else:
            out = np.empty(shape, dtype=np.int32)
            optr, flags = out.ctypes.data, 0
        with self._mutex:
            _lib.check(self._lib.mips_index_gather_labels(self._h, ptr, n, int(idx_offset), optr, flags, _stream_handle(self.device)),
                       "mips_index_gather_labels")
        del keep
        return out

    def compute_distance_subset(self, x, ids, force_ip: bool = False, idx_offset: int = 0):
        """faiss Index.compute_distance_subset: out[j, t] = the canonical score of (x[j], row ids[j, t] - idx_offset), float32
        [nq, k] in the caller's order (mips_score_subset).  The score is what the searches return -- scoring the I of a search
        gives its D bit for bit --: the inner product, on an L2 index the distance unless force_ip.  An id that names no row
        scores -inf (L2: +inf).  Any k, every storage.  x and ids on the host -> NumPy (an id >= ntotal raises); x a CUDA tensor
        -> a CUDA tensor (host ids are copied over first)."""
        import torch

        if self._sq8 and not self.is_trained:
            raise RuntimeError("compute_distance_subset: the 'sq8' index is not trained (train(x) first)")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        if is_dev and not (isinstance(ids, torch.Tensor) and ids.is_cuda):
            ids = torch.as_tensor(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids), dtype=torch.int64).to(f"cuda:{self.device}")
        iptr, shape, ids_dev, ikeep = self._ids_arg(ids, "compute_distance_subset")
        if len(shape) != 2 or shape[0] != nq:
            raise ValueError(f"compute_distance_subset: expected ids [{nq}, k], got {shape}")
        k = int(shape[1])
        flags = (_lib.FORCE_IP if force_ip else 0) | (_lib.IDS_DEVICE if ids_dev else 0)
        if is_dev:
            out = torch.empty((nq, k), dtype=torch.float32, device=f"cuda:{self.device}")
            optr, flags = out.data_ptr(), flags | _lib.Q_DEVICE | _lib.OUT_DEVICE
        else:
            out = np.empty((nq, k), dtype=np.float32)
            optr = out.ctypes.data
        with self._mutex:
            _lib.check(self._lib.mips_score_subset(self._h, ptr, code, nq, iptr, k, optr, int(idx_offset), flags,
                                                   _stream_handle(self.device)), "mips_score_subset")
        del keep, ikeep
        return out

    def rerank(self, x, ids, k: int, idx_offset: int = 0):
        """(D, I) [nq, k]: the best k of the SET of valid ids in each query's row of ids int64 [nq, kc], 1 <= k <= kc <= MAX_K_WIDE,
        scored exactly (mips_index_rerank; faiss IndexRefineFlat's second stage).  An id is valid iff 0 <= id - idx_offset < ntotal;
        every other value, the -1 padding of a search among them, is no row (host ids too: nothing raises), and a repeated id
        counts once.  D is the score compute_distance_subset reports -- compute_distance_subset(x, I) reproduces it bit for bit --
        and an id whose score is a NaN is dropped.  Order: (D descending, id ascending), -1 / -inf padding; I carries the ids as
        given.  Inner-product indexes; on 'sq8' the order is that of the reported D, which need not be the order in which search
        ranks the integer sums.  x on the host -> NumPy; x a CUDA tensor -> CUDA tensors (host ids are copied over first), and
        with CUDA ids nothing synchronises (graph-capturable in steady state)."""
        import torch

        k = int(k)
        if self._metric != _lib.METRIC_IP:
            raise NotImplementedError("rerank: an inner-product index only (the order is score descending)")
        if self._sq8 and not self.is_trained:
            raise RuntimeError("rerank: the 'sq8' index is not trained (train(x) first)")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        if is_dev and not (isinstance(ids, torch.Tensor) and ids.is_cuda):
            ids = torch.as_tensor(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids), dtype=torch.int64).to(f"cuda:{self.device}")
        iptr, shape, ids_dev, ikeep = self._ids_arg(ids, "rerank")
        if len(shape) != 2 or shape[0] != nq:
            raise ValueError(f"rerank: expected ids [{nq}, kc], got {shape}")
        kc = int(shape[1])
        if kc > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"rerank: kc = {kc} exceeds MAX_K_WIDE = {_lib.MAX_K_WIDE}")
        if not 1 <= k <= kc:
            raise ValueError(f"rerank: 1 <= k <= kc = {kc}, got k = {k}")
        flags = _lib.IDS_DEVICE if ids_dev else 0
        if is_dev:
            dev = f"cuda:{self.device}"
            D = torch.empty((nq, k), dtype=torch.float32, device=dev)
            I = torch.empty((nq, k), dtype=torch.int64, device=dev)
            dp, ip, flags = D.data_ptr(), I.data_ptr(), flags | _lib.Q_DEVICE | _lib.OUT_DEVICE
        else:
            D = np.empty((nq, k), dtype=np.float32)
            I = np.empty((nq, k), dtype=np.int64)
            dp, ip = D.ctypes.data, I.ctypes.data
        with self._mutex:
            _lib.check(self._lib.mips_index_rerank(self._h, ptr, code, nq, iptr, kc, k, dp, ip, int(idx_offset), flags,
                                                   _stream_handle(self.device)), "mips_index_rerank")
        del keep, ikeep
        return D, I

    def search_and_reconstruct(self, x, k: int, **kw):
        """faiss Index.search_and_reconstruct -> (D, I, R [nq, k, d] float32): route_search(x, k, **kw) -- selector, groups and
        force_ip as there, k > MAX_K goes to the wide search -- and the rows of I.  The rows of the -1 slots are NaN."""
        D, I = route_search(self, x, int(k), **kw)
        return D, I, self.reconstruct_batch(I, idx_offset=int(kw.get("idx_offset", 0)))

    # ------------------------------------------------------------------ search
    def search(self, x, k: int, idx_offset: int = 0, force_ip: bool = False, tail_stream=None):
        """faiss Index.search(x, k) -> (D, I)  (sotasum/mips.py:383-386).
        NumPy in -> NumPy out; torch CUDA tensor in -> torch CUDA tensors out (stream-ordered, no
        synchronisation).  tail_stream (a torch.cuda.Stream, CUDA tensors only): candidate selection and exact
        re-score run there instead of on the current stream (mips_search_split) -- the results are complete on
        THAT stream."""
        import torch

        k = int(k)
        if k < 0:
            raise ValueError("k must be >= 0")
        if k > _lib.MAX_K:
            raise NotImplementedError(f"k = {k} > {_lib.MAX_K} is not supported by this build")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        stream = _stream_handle(self.device)
        if is_dev:
            dev = f"cuda:{self.device}"
            D = torch.empty((nq, k), dtype=torch.float32, device=dev)
            I = torch.empty((nq, k), dtype=torch.int64, device=dev)
            flags = _lib.Q_DEVICE | _lib.OUT_DEVICE
            ds, di = D.data_ptr(), I.data_ptr()
        else:
            D = np.empty((nq, k), dtype=np.float32)
            I = np.empty((nq, k), dtype=np.int64)
            flags = 0
            ds, di = D.ctypes.data, I.ctypes.data
        if force_ip:
            flags |= _lib.FORCE_IP  # inner-product ranking on an L2 index (Mips.np_search)
        with self._mutex:
            if tail_stream is not None and is_dev:
                D.record_stream(tail_stream)
                I.record_stream(tail_stream)
                _lib.check(self._lib.mips_search_split(self._h, ptr, code, nq, k, ds, di, int(idx_offset), flags, stream,
                                                       int(tail_stream.cuda_stream)), "mips_search_split")
            else:
                _lib.check(self._lib.mips_search(self._h, ptr, code, nq, k, ds, di, int(idx_offset), flags, stream),
                           "mips_search")
        del keep
        return D, I

    def _sel_args(self, selector, sel_bit0: int, what: str):
        """selector (None | Selector | bool mask | NumPy uint8 bitmap) -> (pointer, nbits, flag, keepalive) of the *_sel entry
        points.  A Selector or a bool mask is a device bitmap; a NumPy uint8 array is passed as the host bitmap it is."""
        import torch

        from .selector import Selector

        if selector is None:
            return None, 0, 0, None
        sel_bit0 = int(sel_bit0)
        if sel_bit0 < 0:
            raise ValueError(f"{what}: sel_bit0 must be >= 0")
        if isinstance(selector, np.ndarray) and selector.dtype == np.uint8:
            host = np.ascontiguousarray(selector.reshape(-1))
            ptr, nbits, flag, keep = host.ctypes.data, 8 * host.shape[0], 0, host
        else:
            if not isinstance(selector, Selector):
                if isinstance(selector, torch.Tensor) and selector.dtype == torch.uint8:
                    selector = Selector.from_bitmap(selector, 8 * selector.numel(), device=self.device)
                else:
                    selector = Selector.from_mask(selector, device=self.device)
            selector = selector.to(self.device)
            bits = selector.bits.contiguous()
            ptr, nbits, flag, keep = bits.data_ptr(), selector.nbits, _lib.SEL_DEVICE, bits
        if nbits < sel_bit0 + self.ntotal:
            raise ValueError(f"{what}: the selector has {nbits} bits; rows {sel_bit0} .. {sel_bit0 + self.ntotal} of it are needed")
        return ptr, nbits, flag, keep

    def search_wide(self, x, k: int, idx_offset: int = 0, force_ip: bool = False, selector=None, sel_bit0: int = 0, groups=None,
                    group_mode: str = "exclude"):
        """search() for k up to MAX_K_WIDE = 1024 (mips_search_wide: threshold scan, streaming select, exact re-score; every
        query certified or settled exactly in the same call).  bf16 and f32 indexes of at most 1024 columns.  NumPy in ->
        NumPy out; torch CUDA tensor in -> torch CUDA tensors out, stream-ordered, no synchronisation.
        selector (a Selector, a bool mask or a NumPy uint8 bitmap; one for all queries): only the selected rows can be results
        -- what the search returns on an index from which the others were deleted, row numbers, phi and maximal norm kept;
        fewer than k selected rows leave the -1 / -+inf padding.  Bit sel_bit0 + i of the selector decides local row i.
        groups (an int array [nq], NumPy -> host, CUDA tensor -> device) with group_mode: one label per query, tested against
        the row labels of set_labels -- "exclude": only rows of ANOTHER label answer the query, "only": only rows of ITS label;
        a query labelled LABEL_NONE is not filtered.  Applies on top of the selector, with the same definition per query."""
        import torch

        k = int(k)
        self._check_wide(k)
        sel_ptr, sel_nbits, sel_flag, sel_keep = self._sel_args(selector, sel_bit0, "search_wide")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        grp_ptr, grp_mode, grp_flag, grp_keep = self._grp_args(groups, group_mode, nq, "search_wide")
        stream = _stream_handle(self.device)
        if is_dev:
            dev = f"cuda:{self.device}"
            D = torch.empty((nq, k), dtype=torch.float32, device=dev)
            I = torch.empty((nq, k), dtype=torch.int64, device=dev)
            flags = _lib.Q_DEVICE | _lib.OUT_DEVICE
            ds, di = D.data_ptr(), I.data_ptr()
        else:
            D = np.empty((nq, k), dtype=np.float32)
            I = np.empty((nq, k), dtype=np.int64)
            flags = 0
            ds, di = D.ctypes.data, I.ctypes.data
        if force_ip:
            flags |= _lib.FORCE_IP
        with self._mutex:
            if groups is not None:
                _lib.check(self._lib.mips_search_wide_grp(self._h, ptr, code, nq, k, ds, di, int(idx_offset), flags | sel_flag | grp_flag,
                                                          sel_ptr, sel_nbits, int(sel_bit0), grp_ptr, grp_mode, stream),
                           "mips_search_wide_grp")
            elif selector is None:
                _lib.check(self._lib.mips_search_wide(self._h, ptr, code, nq, k, ds, di, int(idx_offset), flags, stream),
                           "mips_search_wide")
            else:
                _lib.check(self._lib.mips_search_wide_sel(self._h, ptr, code, nq, k, ds, di, int(idx_offset), flags | sel_flag,
                                                          sel_ptr, sel_nbits, int(sel_bit0), stream), "mips_search_wide_sel")
        del keep, sel_keep, grp_keep
        return D, I

    def _check_wide(self, k: int) -> None:
        if k < 0:
            raise ValueError("k must be >= 0")
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"k = {k} > {_lib.MAX_K_WIDE} is not supported by this build")
        if self._f8 or self._sq8:
            raise NotImplementedError("search_wide serves 'bf16' and 'f32' indexes; e4m3 and sq8 storage is limited to search()")
        if self._d > 1024:
            raise NotImplementedError("search_wide serves rows of at most 1024 columns")

    # ------------------------------------------------------------------ range search
    def _check_range(self) -> None:
        if self._f8 or self._sq8:
            raise NotImplementedError("range_search serves 'bf16' and 'f32' indexes; e4m3 and sq8 storage is limited to search()")
        if self._d > 1024:
            raise NotImplementedError("range_search serves rows of at most 1024 columns")

    @staticmethod
    def _radii(radius, nq: int) -> np.ndarray:
        """A scalar or an array-like of length nq -> host float32 [nq] (mips_range_search takes the radii from the host)."""
        r = np.asarray(radius.detach().cpu() if hasattr(radius, "detach") else radius, dtype=np.float32)
        if r.ndim == 0:
            r = np.full(nq, r, dtype=np.float32)
        r = np.ascontiguousarray(r.reshape(-1))
        if r.shape[0] != nq:
            raise ValueError(f"range_search: expected a scalar radius or {nq} radii, got {r.shape[0]}")
        if np.isnan(r).any():
            raise ValueError("range_search: a radius is NaN")
        return r

    def range_search_into(self, x, radius, lims, D, I, idx_offset: int = 0, force_ip: bool = False, selector=None, groups=None,
                          group_mode: str = "exclude", sel_bit0: int = 0) -> None:
        """The non-synchronising form of range_search: the caller allocates the CUDA tensors lims (int64 [nq + 1]), D (float32
        [cap]) and I (int64 [cap]); everything is enqueued on the current stream.  lims always receives the true counts; when
        lims[-1] > cap the contents of D and I are unspecified and the call is to be repeated with larger tensors.  cap = 0
        (empty D and I) is a counting call.  `radius` is host data (a scalar or nq values).  selector, sel_bit0, groups and
        group_mode: as in search_wide (a row shard passes the global selector and its first global row)."""
        import torch

        self._check_range()
        sel_ptr, sel_nbits, sel_flag, sel_keep = self._sel_args(selector, sel_bit0, "range_search")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        grp_ptr, grp_mode, grp_flag, grp_keep = self._grp_args(groups, group_mode, nq, "range_search")
        r = self._radii(radius, nq)
        dev = torch.device("cuda", self.device)
        for t, dt, what in ((lims, torch.int64, "lims"), (D, torch.float32, "D"), (I, torch.int64, "I")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
                raise ValueError(f"range_search_into: {what} must be a contiguous 1-d CUDA {dt} tensor on cuda:{self.device}")
        if lims.shape[0] != nq + 1 or D.shape[0] != I.shape[0]:
            raise ValueError(f"range_search_into: lims must have {nq + 1} entries and D, I one length")
        cap = int(D.shape[0])
        flags = _lib.OUT_DEVICE | (_lib.Q_DEVICE if is_dev else 0) | (_lib.FORCE_IP if force_ip else 0)
        with self._mutex:
            if groups is not None:
                _lib.check(self._lib.mips_range_search_grp(self._h, ptr, code, nq, r.ctypes.data, lims.data_ptr(),
                                                           D.data_ptr() if cap else None, I.data_ptr() if cap else None, cap,
                                                           int(idx_offset), flags | sel_flag | grp_flag, sel_ptr, sel_nbits, int(sel_bit0), grp_ptr,
                                                           grp_mode, _stream_handle(self.device)), "mips_range_search_grp")
            elif selector is None:
                _lib.check(self._lib.mips_range_search(self._h, ptr, code, nq, r.ctypes.data, lims.data_ptr(),
                                                       D.data_ptr() if cap else None, I.data_ptr() if cap else None, cap,
                                                       int(idx_offset), flags, _stream_handle(self.device)), "mips_range_search")
            else:
                _lib.check(self._lib.mips_range_search_sel(self._h, ptr, code, nq, r.ctypes.data, lims.data_ptr(),
                                                           D.data_ptr() if cap else None, I.data_ptr() if cap else None, cap,
                                                           int(idx_offset), flags | sel_flag, sel_ptr, sel_nbits, int(sel_bit0),
                                                           _stream_handle(self.device)), "mips_range_search_sel")
        del keep, sel_keep, grp_keep

    def range_search(self, x, radius, idx_offset: int = 0, force_ip: bool = False, selector=None, groups=None,
                     group_mode: str = "exclude", sel_bit0: int = 0):
        """faiss Index.range_search(x, radius) -> (lims, D, I): every stored row whose canonical score is strictly above the
        radius (inner product; L2: whose distance |q|^2 + phi - 2 q.x is strictly below it).  `radius` is a scalar or nq
        values.  The hits of query j are D / I [lims[j] : lims[j + 1]], in ascending row order; lims is int64 [nq + 1].
        NumPy in -> NumPy out; torch CUDA tensor in -> torch CUDA tensors out.  The result's size is not known beforehand: a
        first call runs with a guessed capacity, lims[-1] is READ ON THE HOST -- THIS SYNCHRONISES the stream -- and one repeat
        with the exact size follows if the guess was too small (range_search_into is the form that never synchronises).
        bf16 and f32 indexes of at most 1024 columns.  selector and sel_bit0 (as in search_wide): only selected rows can be hits;
        groups and group_mode (as in search_wide): only rows the group rule admits for the query."""
        import torch

        from .selector import Selector

        self._check_range()
        if selector is not None and not isinstance(selector, (Selector, np.ndarray)):
            selector = Selector.from_mask(selector, device=self.device)   # packed once for the repeat call
        if isinstance(selector, np.ndarray) and selector.dtype != np.uint8:
            selector = Selector.from_mask(selector, device=self.device)
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        r = self._radii(radius, nq)
        dev = f"cuda:{self.device}"
        lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        cap = max(1 << 16, 256 * nq)
        while True:
            D = torch.empty(cap, dtype=torch.float32, device=dev)
            I = torch.empty(cap, dtype=torch.int64, device=dev)
            self.range_search_into(keep, r, lims, D, I, idx_offset=idx_offset, force_ip=force_ip, selector=selector, groups=groups,
                                   group_mode=group_mode, sel_bit0=sel_bit0)
            total = int(lims[-1].item())   # the synchronisation
            if total <= cap:
                break
            cap = total
        D, I = D[:total], I[:total]
        if is_dev:
            return lims, D.clone() if total < cap else D, I.clone() if total < cap else I
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    def search_wide_packed(self, x, k: int, idx_offset: int = 0, force_ip: bool = False, selector=None, sel_bit0: int = 0, groups=None,
                           group_mode: str = "exclude"):
        """Device-only search_wide returning the all-gather payload: CUDA int64 [nq, k, 2] = {float32 score bits,
        index + idx_offset}, row for row what search_wide returns (padding included).  selector / sel_bit0 as in search_wide:
        a row shard passes the global selector and its first global row.  groups / group_mode as in search_wide (the row labels
        are the shard's own)."""
        import torch

        k = int(k)
        self._check_wide(k)
        sel_ptr, sel_nbits, sel_flag, sel_keep = self._sel_args(selector, sel_bit0, "search_wide_packed")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        if not is_dev:
            raise ValueError("search_wide_packed needs a CUDA tensor")
        grp_ptr, grp_mode, grp_flag, grp_keep = self._grp_args(groups, group_mode, nq, "search_wide_packed")
        out = torch.empty((nq, k, 2), dtype=torch.int64, device=f"cuda:{self.device}")
        flags = _lib.Q_DEVICE | _lib.OUT_DEVICE | _lib.OUT_PACKED | (_lib.FORCE_IP if force_ip else 0)
        with self._mutex:
            if groups is not None:
                _lib.check(self._lib.mips_search_wide_grp(self._h, ptr, code, nq, k, None, out.data_ptr(), int(idx_offset),
                                                          flags | sel_flag | grp_flag, sel_ptr, sel_nbits, int(sel_bit0), grp_ptr, grp_mode,
                                                          _stream_handle(self.device)), "mips_search_wide_grp")
            elif selector is None:
                _lib.check(self._lib.mips_search_wide(self._h, ptr, code, nq, k, None, out.data_ptr(), int(idx_offset), flags,
                                                      _stream_handle(self.device)), "mips_search_wide")
            else:
                _lib.check(self._lib.mips_search_wide_sel(self._h, ptr, code, nq, k, None, out.data_ptr(), int(idx_offset),
                                                          flags | sel_flag, sel_ptr, sel_nbits, int(sel_bit0),
                                                          _stream_handle(self.device)), "mips_search_wide_sel")
        del keep, sel_keep, grp_keep
        return out

    def search_fused(self, x, k: int, normalize: bool = False, ignore=None, idx_offset: int = 0, groups=None, group_mode: str = "exclude"):
        """The scoring hook's search in one call on CUDA tensors (include/mips_hip.h, mips_search_fused): optional
        row normalisation of float32 queries (the caller's tensor is not modified), top-k, and the ignore filter of
        sotasum/mips.py:388-398 (`ignore`: int64 ids, one per query).  One kernel launch for <= 16 queries on a small
        index; nothing synchronises.
        groups (an int array [nq], NumPy -> host, CUDA tensor -> device) with group_mode: the group rule of search_wide, applied
        in the same one launch (include/mips_hip_hook.h, mips_search_fused_grp); `ignore` applies on top of it.  bf16 and f32
        indexes of at most 1024 columns, as search_wide."""
        import torch

        k = int(k)
        if groups is not None:  # (the storages and widths the grouped wide search serves)
            if self._f8 or self._sq8:
                raise NotImplementedError("search_fused(groups=) serves 'bf16' and 'f32' indexes, not e4m3 or sq8 storage")
            if self._d > 1024:
                raise NotImplementedError("search_fused(groups=) serves rows of at most 1024 columns")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        if not is_dev:
            raise ValueError("search_fused needs a CUDA tensor")
        grp_ptr, grp_mode, grp_flag, grp_keep = self._grp_args(groups, group_mode, nq, "search_fused")
        dev = f"cuda:{self.device}"
        ig = None
        if ignore is not None:
            ig = torch.as_tensor(ignore, device=dev, dtype=torch.int64).contiguous()
            if ig.shape != (nq,):
                raise ValueError(f"ignore_indexes: expected {nq} ids, got {tuple(ig.shape)}")
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        with self._mutex:
            if groups is not None:
                _lib.check(self._lib.mips_search_fused_grp(self._h, ptr, code, nq, k, int(bool(normalize)),
                                                           ig.data_ptr() if ig is not None else None, D.data_ptr(), I.data_ptr(),
                                                           int(idx_offset), grp_ptr, grp_mode, grp_flag, _stream_handle(self.device)),
                           "mips_search_fused_grp")
            else:
                _lib.check(self._lib.mips_search_fused(self._h, ptr, code, nq, k, int(bool(normalize)),
                                                       ig.data_ptr() if ig is not None else None, D.data_ptr(), I.data_ptr(),
                                                       int(idx_offset), _stream_handle(self.device)), "mips_search_fused")
        del keep, ig, grp_keep
        return D, I

    def search_packed(self, x, k: int, idx_offset: int = 0, tail_stream=None):
        """Device-only search returning the all-gather payload: CUDA int64 [nq, k, 2] =
        {float32 score bits, index + idx_offset} (sharded.py).  tail_stream: as in search()."""
        import torch

        k = int(k)
        if k > _lib.MAX_K:
            raise NotImplementedError(f"k = {k} > {_lib.MAX_K} is not supported by this build")
        ptr, code, is_dev, nq, keep = self._as_buffer(x, "search")
        if not is_dev:
            raise ValueError("search_packed needs a CUDA tensor")
        out = torch.empty((nq, k, 2), dtype=torch.int64, device=f"cuda:{self.device}")
        flags = _lib.Q_DEVICE | _lib.OUT_DEVICE | _lib.OUT_PACKED
        with self._mutex:
            if tail_stream is not None:
                out.record_stream(tail_stream)
                _lib.check(self._lib.mips_search_split(self._h, ptr, code, nq, k, None, out.data_ptr(), int(idx_offset), flags,
                                                       _stream_handle(self.device), int(tail_stream.cuda_stream)),
                           "mips_search_split")
            else:
                _lib.check(self._lib.mips_search(self._h, ptr, code, nq, k, None, out.data_ptr(), int(idx_offset), flags,
                                                 _stream_handle(self.device)), "mips_search")
        del keep
        return out

    def set_param(self, name: str, value: int) -> None:
        """Launch tuning knob ("nsplit", "qgroups", "variant", "f32_fast": two-stage search of an fp32-exact index,
        0 off / 1 when the call may synchronise / 2 always); never changes certified results.  ("spin_limit" is the
        test-only bound of the scan's block barrier, include/mips_hip.h.)"""
        _lib.check(self._lib.mips_index_set_param(self._h, name.encode(), int(value)), "mips_index_set_param")

    def check(self, synchronize: bool = True) -> None:
        """Raise RuntimeError if a scan kernel of an earlier search on this index gave up on its block barrier
        (that search returned idx = IDX_POISON / NaN in every slot).  synchronize=True first waits for the
        current stream, so every search enqueued so far is covered; False only looks at the host-visible flag.
        Device-output searches never synchronise by themselves: call this where a sync is affordable (end of a
        batch, before results leave the process).  The next search on the index performs the same check."""
        _lib.check(self._lib.mips_index_check_error(self._h, int(bool(synchronize)), _stream_handle(self.device)),
                   "mips_index_check_error")

    def margin_stats(self, synchronize: bool = True) -> dict:
        """Margin check of the LAST search (include/mips_hip.h, mips_index_margin_stats): {"flagged": queries whose
        candidate pool was not provably wide enough, "rescanned": of those settled (exactly, by the brute-force pass, or by the
        re-scan with the widest lists), "unresolved": left with their first result}.  set_param("margin_check", m): 0 off,
        1 (default) certify -- NumPy searches with a synchronisation, CUDA searches stream-ordered, without one --,
        2 certify and synchronise, 3 stream-ordered explicitly, 4 count only."""
        f, r, u = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._lib.mips_index_margin_stats(self._h, ctypes.byref(f), ctypes.byref(r), ctypes.byref(u),
                                                     int(bool(synchronize)), _stream_handle(self.device)),
                   "mips_index_margin_stats")
        return {"flagged": f.value, "rescanned": r.value, "unresolved": u.value}

    @property
    def last_kernel(self) -> str:
        """Scan-kernel instance the last search dispatched to (rocprofv3 spelling)."""
        return self._lib.mips_index_last_kernel(self._h).decode()

    def scan_timing(self, reset: bool = False):
        """(summed ms, launches) of the fused scan kernel in the current measurement window, from HIP events
        on the search stream (synchronise first).  reset=True opens a new window (at most 128 launches);
        outside a window no events are recorded."""
        ms, cnt = ctypes.c_float(), ctypes.c_int()
        _lib.check(self._lib.mips_scan_timing(self._h, ctypes.byref(ms), ctypes.byref(cnt), int(reset)),
                   "mips_scan_timing")
        return ms.value, cnt.value

    def last_scan_ms(self) -> float:
        """Mean scan-kernel time of the searches since scan_timing(reset=True) opened a measurement window
        (-1.0 outside a window: events are not recorded then)."""
        import torch

        torch.cuda.synchronize(self.device)
        ms, cnt = self.scan_timing()
        return ms / cnt if cnt else -1.0

    # ------------------------------------------------------------------ persistence
    # Own format (the on-disk format is free, the call surface is kept):
    #   <path>/meta.json   {"format":1,"d":..,"ntotal":..,"metric":..,"dtype":"bf16", ...}
    #   <path>/rows.bf16   raw little-endian bf16 bit patterns [ntotal, d]   (rows.e4m3: e4m3 bytes; rows.sq8: codes, with
    #                      "sq8_vmin" / "sq8_vdiff" in meta.json: the float32 parameters as exact hexadecimal strings)
    #   <path>/labels.i32  little-endian int32 [ntotal], only with "labels": true in meta.json (a fully labelled index)
    def save(self, path: str, extra: dict | None = None, chunk_rows: int = 1 << 16) -> None:
        """Replaces Dataset.save_faiss_index (sotasum/mips.py:536)."""
        os.makedirs(path, exist_ok=True)
        n = self.ntotal
        with open(os.path.join(path, "rows." + _ROWS_FILE[self.dtype][0]), "wb") as f:
            for r0 in range(0, n, chunk_rows):
                f.write(self.rows_raw(r0, min(chunk_rows, n - r0)).tobytes())
        meta = {"format": _FORMAT_VERSION, "d": self._d, "ntotal": n, "metric": self._metric, "dtype": self.dtype}
        if self._metric == _lib.METRIC_L2 and n > 0:
            # phi of the WHOLE file: a rank that loads one row range of it must not fall back to its own rows' maximum
            # (L2 distances of different shards would not be comparable)
            meta["phi"] = self.phi()
        if self._sq8 and self.is_trained:
            vmin, vdiff = self.sq8_params()
            meta["sq8_vmin"], meta["sq8_vdiff"] = [float(v).hex() for v in vmin], [float(v).hex() for v in vdiff]
        if n > 0 and self._nlabelled == n:
            with open(os.path.join(path, "labels.i32"), "wb") as f:
                f.write(self.labels().astype("<i4").tobytes())
            meta["labels"] = True
        if extra:
            meta.update({k: v for k, v in extra.items() if v is not None or k not in meta})
        with open(os.path.join(path, "meta.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def load(cls, path: str, device: int | None = None, row_range: tuple | None = None,
             chunk_rows: int = 1 << 16) -> "MipsIndex":
        """Replaces Dataset.load_faiss_index (sotasum/mips.py:547).  row_range=(lo, hi) loads one
        row shard of the file (multi-GPU: every rank maps the same file and keeps its own rows)."""
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("format") != _FORMAT_VERSION:
            raise ValueError(f"unknown index format {meta.get('format')}")
        ix = cls(meta["d"], metric=meta["metric"], dtype=meta["dtype"], device=device)
        n, d = meta["ntotal"], meta["d"]
        lo, hi = (0, n) if row_range is None else row_range
        if meta.get("sq8_vmin") is not None:  # (the whole file's parameters, whichever row range is loaded)
            ix.set_sq8_params([float.fromhex(v) for v in meta["sq8_vmin"]], [float.fromhex(v) for v in meta["sq8_vdiff"]])
        if hi > lo:
            ext, npdt = _ROWS_FILE[meta["dtype"]]
            mm = np.memmap(os.path.join(path, "rows." + ext), dtype=npdt, mode="r", shape=(n, d))
            ix.reserve(hi - lo)
            for r0 in range(lo, hi, chunk_rows):
                ix.add(np.asarray(mm[r0:min(hi, r0 + chunk_rows)]))
            del mm
            if meta.get("labels"):
                lab = np.memmap(os.path.join(path, "labels.i32"), dtype="<i4", mode="r", shape=(n,))
                ix.set_labels(np.asarray(lab[lo:hi]))
                del lab
        if row_range is not None and meta["metric"] == _lib.METRIC_L2 and meta.get("phi") is not None:
            ix.set_phi(float(meta["phi"]))  # the file's phi, not this row range's
        ix.meta = meta
        return ix


def synth_fill(n: int, d: int, row0: int, seed: int, kind: int, dtype="bf16", device: int | None = None):
    """Device tensor [n, d] of generator values: torch.bfloat16 ("bf16"), torch.float32 ("f32") or
    e4m3 codes as torch.uint8 ("fp8_e4m3")."""
    import torch

    lib = _lib.load()
    dev = _lib.require_gpu(device)
    tdt = {"bf16": torch.bfloat16, "f32": torch.float32, "fp8_e4m3": torch.uint8}[dtype]
    code = {"bf16": _lib.DTYPE_BF16, "f32": _lib.DTYPE_F32, "fp8_e4m3": _lib.DTYPE_FP8_E4M3}[dtype]
    out = torch.empty((n, d), dtype=tdt, device=f"cuda:{dev}")
    _lib.check(lib.mips_synth_fill(out.data_ptr(), n, d, row0, seed, kind, code, dev, _stream_handle(dev)),
               "mips_synth_fill")
    return out


def l2_normalize_(x):
    """In-place row normalisation of a CUDA float32 tensor (faiss.normalize_L2 semantics,
    sotasum/mips.py:521-525)."""
    import torch

    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2):
        raise ValueError("l2_normalize_: expected a contiguous CUDA float32 matrix")
    lib = _lib.load()
    _lib.check(lib.mips_l2_normalize(x.data_ptr(), x.shape[0], x.shape[1], x.device.index,
                                     _stream_handle(x.device.index)), "mips_l2_normalize")
    return x


def rows_max_sumsq(x) -> float:
    """max_i |x_i|^2 of a CUDA float32 matrix (its sqrt is max_norm, sotasum/mips.py:298-304)."""
    import torch

    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2):
        raise ValueError("rows_max_sumsq: expected a contiguous CUDA float32 matrix")
    lib = _lib.load()
    out = ctypes.c_double()
    _lib.check(lib.mips_rows_max_sumsq(x.data_ptr(), x.shape[0], x.shape[1], ctypes.byref(out), x.device.index,
                                       _stream_handle(x.device.index)), "mips_rows_max_sumsq")
    return out.value


def rows_max_sumsq_into(x, acc) -> None:
    """acc = max(acc, max_i |x_i|^2): `acc` is a CUDA float64 tensor of one element that stays on the device -- no host copy,
    no synchronisation (the running max-norm of a streaming index build; read it once, at the end)."""
    import torch

    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2):
        raise ValueError("rows_max_sumsq_into: expected a contiguous CUDA float32 matrix")
    if not (isinstance(acc, torch.Tensor) and acc.is_cuda and acc.dtype == torch.float64 and acc.numel() == 1 and acc.device == x.device):
        raise ValueError("rows_max_sumsq_into: the accumulator must be a one-element CUDA float64 tensor on the rows' device")
    lib = _lib.load()
    _lib.check(lib.mips_rows_max_sumsq_device(x.data_ptr(), x.shape[0], x.shape[1], acc.data_ptr(), x.device.index,
                                              _stream_handle(x.device.index)), "mips_rows_max_sumsq_device")


def merge_topk_packed(gathered, nq: int, parts: int, k: int, metric: int = _lib.METRIC_IP):
    """Device merge straight from the gathered payload: CUDA int64 [parts * nq, k, 2] (rank-major)."""
    import torch

    lib = _lib.load()
    dev = gathered.device.index
    out_s = torch.empty((nq, k), dtype=torch.float32, device=gathered.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=gathered.device)
    _lib.check(lib.mips_merge_topk_packed(gathered.data_ptr(), nq, parts, k, metric, out_s.data_ptr(), out_i.data_ptr(),
                                          dev, _stream_handle(dev)), "mips_merge_topk_packed")
    return out_s, out_i


def merge_topk_sorted_packed(gathered, nq: int, parts: int, k: int, metric: int = _lib.METRIC_IP):
    """merge_topk_packed for wide lists (k up to MAX_K_WIDE): same payload, same result, but every part must arrive in result
    order (what search_packed and search_wide_packed emit) -- ranks come from binary searches in the other parts."""
    import torch

    lib = _lib.load()
    dev = gathered.device.index
    out_s = torch.empty((nq, k), dtype=torch.float32, device=gathered.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=gathered.device)
    _lib.check(lib.mips_merge_topk_sorted_packed(gathered.data_ptr(), nq, parts, k, metric, out_s.data_ptr(), out_i.data_ptr(),
                                                 dev, _stream_handle(dev)), "mips_merge_topk_sorted_packed")
    return out_s, out_i


def range_merge_records(gathered, parts: int, nq: int, stride: int, cap: int | None = None, out=None):
    """Device merge of the range-search records of `parts` row shards (include/mips_hip_sharded.h, mips_range_merge_records):
    gathered is a CUDA int64 tensor of parts * range_record_words(nq, stride) words, the records end to end in ascending row
    order of their shards, as an all-gather leaves them.  -> (lims int64 [nq + 1], D float32 [cap], I int64 [cap]) CUDA tensors;
    nothing synchronises.  lims holds the true global counts; D and I are complete iff lims[-1] <= cap and no part exceeded its
    stride.  cap = None: parts * stride, which no result of untruncated parts exceeds; cap = 0 only counts.  out = (lims, D, I):
    the caller's contiguous CUDA tensors of those dtypes are written instead (cap is then len(D) = len(I)) and returned."""
    import torch

    lib = _lib.load()
    parts, nq, stride = int(parts), int(nq), int(stride)
    words = _lib.range_record_words(nq, stride)
    if not (isinstance(gathered, torch.Tensor) and gathered.is_cuda and gathered.dtype == torch.int64 and gathered.is_contiguous()):
        raise ValueError("range_merge_records: gathered must be a contiguous CUDA int64 tensor")
    if parts < 1 or nq < 0 or stride < 0 or gathered.numel() != parts * words:
        raise ValueError(f"range_merge_records: {gathered.numel()} words for {parts} records of {words}")
    dev = gathered.device.index
    if out is not None:
        lims, D, I = out
        for t, dt, n in ((lims, torch.int64, nq + 1), (D, torch.float32, None), (I, torch.int64, D.shape[0])):
            if not (isinstance(t, torch.Tensor) and t.device == gathered.device and t.dtype == dt and t.dim() == 1 and t.is_contiguous()
                    and (n is None or t.shape[0] == n)):
                raise ValueError(f"range_merge_records: out must be contiguous 1-d tensors on {gathered.device}: int64 [nq + 1], "
                                 "float32 [cap], int64 [cap]")
        cap = int(D.shape[0])
    else:
        cap = parts * stride if cap is None else int(cap)
        lims = torch.empty(nq + 1, dtype=torch.int64, device=gathered.device)
        D = torch.empty(cap, dtype=torch.float32, device=gathered.device)
        I = torch.empty(cap, dtype=torch.int64, device=gathered.device)
    work = torch.empty(parts * nq, dtype=torch.int64, device=gathered.device)
    _lib.check(lib.mips_range_merge_records(gathered.data_ptr(), parts, nq, stride, lims.data_ptr(), D.data_ptr() if cap else None,
                                            I.data_ptr() if cap else None, cap, work.data_ptr() if nq else None, dev,
                                            _stream_handle(dev)), "mips_range_merge_records")
    return lims, D, I   # (the workspace goes back to the allocator of the stream the kernels run on: stream-ordered reuse)


def merge_topk(cand_s, cand_i, parts: int, k: int, metric: int = _lib.METRIC_IP):
    """Device merge of `parts` per-shard top-k lists: cand_* CUDA [nq, parts*k] -> ([nq,k], [nq,k])."""
    import torch

    lib = _lib.load()
    nq = cand_s.shape[0]
    if cand_s.shape != cand_i.shape or cand_s.shape[1] != parts * k:
        raise ValueError(f"merge_topk: candidates {tuple(cand_s.shape)} / {tuple(cand_i.shape)} != [nq, parts*k = {parts * k}]")
    cand_s = cand_s.contiguous()
    cand_i = cand_i.contiguous()
    dev = cand_s.device.index
    out_s = torch.empty((nq, k), dtype=torch.float32, device=cand_s.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=cand_s.device)
    _lib.check(lib.mips_merge_topk(cand_s.data_ptr(), cand_i.data_ptr(), nq, parts, k, metric, out_s.data_ptr(),
                                   out_i.data_ptr(), dev, _stream_handle(dev)), "mips_merge_topk")
    return out_s, out_i


def filter_ignore(scores, idx, ignore, k: int):
    """Device form of the ignore filter of sotasum/mips.py:388-398: CUDA scores/idx [nq, k+1] and
    ignore [nq] -> ([nq, k], [nq, k])."""
    import torch

    lib = _lib.load()
    nq, k1 = scores.shape
    dev = scores.device.index
    scores, idx = scores.contiguous(), idx.contiguous()
    ignore = torch.as_tensor(ignore, device=scores.device, dtype=torch.int64).contiguous()
    if ignore.shape != (nq,):
        raise ValueError(f"ignore_indexes: expected {nq} ids, got {tuple(ignore.shape)}")
    out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    _lib.check(lib.mips_filter_ignore(scores.data_ptr(), idx.data_ptr(), ignore.data_ptr(), nq, k1, k, out_s.data_ptr(),
                                      out_i.data_ptr(), dev, _stream_handle(dev)), "mips_filter_ignore")
    return out_s, out_i


def _cosine_rescore_raw(query, mips_cls, memory_seq_len: int):
    """One launch: float32 scores [B, k] (+ memory_bias [B, k * memory_seq_len]) of CUDA query [B, d], cls [B, k, d]."""
    import torch

    lib = _lib.load()
    b, k, d = mips_cls.shape
    code = _lib.DTYPE_BF16 if mips_cls.dtype == torch.bfloat16 else _lib.DTYPE_F32
    dev = query.device.index
    out = torch.empty((b, k), dtype=torch.float32, device=query.device)
    if memory_seq_len == 0:
        _lib.check(lib.mips_cosine_rescore(query.data_ptr(), mips_cls.data_ptr(), code, b, k, d, out.data_ptr(), dev,
                                           _stream_handle(dev)), "mips_cosine_rescore")
        return out, None
    bias = torch.empty((b, k * memory_seq_len), dtype=torch.float32, device=query.device)
    _lib.check(lib.mips_cosine_rescore_bias(query.data_ptr(), mips_cls.data_ptr(), code, b, k, d, out.data_ptr(),
                                            memory_seq_len, bias.data_ptr(), dev, _stream_handle(dev)),
               "mips_cosine_rescore_bias")
    return out, bias


def _make_cosine_function():
    import torch

    class _CosineRescore(torch.autograd.Function):
        """Autograd wrapper of the hook's re-score: backward = the reference's (retriever_generator.py:158-172) --
        gradient of `query @ mips_cls.transpose(1, 2)` only, the norms are constants (they are computed under
        torch.no_grad() there).  memory_bias is an expand of the scores, its gradient folds back over the tokens."""

        @staticmethod
        def forward(ctx, query, mips_cls, memory_seq_len):
            ctx.save_for_backward(query, mips_cls)
            ctx.memory_seq_len = int(memory_seq_len)
            out, bias = _cosine_rescore_raw(query, mips_cls, ctx.memory_seq_len)
            if bias is None:
                return out
            return out, bias

        @staticmethod
        def backward(ctx, g_scores, g_bias=None):
            query, mips_cls = ctx.saved_tensors
            lib = _lib.load()
            b, k, d = mips_cls.shape
            code = _lib.DTYPE_BF16 if mips_cls.dtype == torch.bfloat16 else _lib.DTYPE_F32
            dev = query.device.index
            gs = g_scores.float().contiguous() if g_scores is not None else None
            gb = g_bias.float().contiguous() if (g_bias is not None and ctx.memory_seq_len > 0) else None
            gq = torch.empty((b, d), dtype=torch.float32, device=query.device)
            gc = torch.empty((b, k, d), dtype=torch.float32, device=query.device)
            if gs is None and gb is None:
                return None, None, None
            _lib.check(lib.mips_cosine_rescore_backward(query.data_ptr(), mips_cls.data_ptr(), code, b, k, d,
                                                        gs.data_ptr() if gs is not None else None,
                                                        gb.data_ptr() if gb is not None else None, ctx.memory_seq_len,
                                                        gq.data_ptr(), gc.data_ptr(), dev, _stream_handle(dev)),
                       "mips_cosine_rescore_backward")
            return gq.to(query.dtype), gc.to(mips_cls.dtype), None

    return _CosineRescore


_COSINE_FN = None


def cosine_rescore(query, mips_cls, memory_seq_len: int = 0):
    """retriever_generator.py:158-172 on the device: query [B, 1, d] or [B, d], mips_cls [B, k, d]
    (CUDA float32 or bfloat16) -> float32 [B, k] = q . c / (|q| |c|).  With memory_seq_len > 0 the
    same launch also writes the hook's memory_bias (retriever_generator.py:188-192), float32
    [B, k * memory_seq_len], and (scores, memory_bias) is returned.
    Differentiable like the reference's expression: when an input requires grad the call goes through a
    torch.autograd.Function whose backward (a HIP kernel as well) is the gradient of the dot product with the
    norms held constant -- memory_bias is how the retriever's encoders are trained."""
    import torch

    global _COSINE_FN
    squeeze_grad_shape = query.dim() == 3
    if squeeze_grad_shape:
        query = query[:, 0, :]
    b, k, d = mips_cls.shape
    if query.shape != (b, d) or not (query.is_cuda and mips_cls.is_cuda):
        raise ValueError("cosine_rescore: expected CUDA query [B,(1,)d] and mips_cls [B,k,d]")
    if memory_seq_len < 0:
        raise ValueError("cosine_rescore: memory_seq_len must be >= 0")
    if not (mips_cls.dtype == torch.bfloat16 and query.dtype == torch.bfloat16):
        query, mips_cls = query.float(), mips_cls.float()
    query, mips_cls = query.contiguous(), mips_cls.contiguous()
    if torch.is_grad_enabled() and (query.requires_grad or mips_cls.requires_grad):
        if _COSINE_FN is None:
            _COSINE_FN = _make_cosine_function()
        return _COSINE_FN.apply(query, mips_cls, int(memory_seq_len))
    out, bias = _cosine_rescore_raw(query, mips_cls, int(memory_seq_len))
    return out if bias is None else (out, bias)
