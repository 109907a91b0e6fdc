"""IvfIndex -- an inverted file (k-means lists, nprobe) over the rows of a flat index (include/mips_hip_ivf.h).

Building and maintaining the file: deterministic k-means training, the list of every added row, the list table, the probed lists
P(q) of a query, removal, reset, save / load.  Searching it: `search_probed` scores every row of the probed lists exactly and
returns what `flat.search` would return if the other rows were deleted; `range_search_probed` returns every probed row above a
per-query radius in CSR form (include/mips_hip_ivf_range.h); `flat` is the inner MipsIndex over the same rows and searches all of
them.  `search_part` + `ivf_merge_parts` are the search cut behind its merge, for the row shards of a ShardedIvfIndex
(include/mips_hip_ivf_sharded.h).

All arithmetic happens in libmips_hip.so; this file moves pointers.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading

import numpy as np

from . import _lib
from .index import _FORMAT_VERSION, _ROWS_FILE, MipsIndex, _stream_handle

_DTYPES = {"bf16": _lib.DTYPE_BF16, "f32": _lib.DTYPE_F32, "sq8": _lib.DTYPE_SQ8}


class _FlatView(MipsIndex):
    """The inner flat index of an IvfIndex, borrowed: reads (reconstruct*, labels, rows_raw, sq8_params, compute_distance_subset)
    work unchanged; what would change its rows behind the list table is refused."""

    def __init__(self, owner: "IvfIndex"):
        self._lib = owner._lib
        self.device = owner.device
        self._h = ctypes.c_void_p(owner._lib.mips_ivf_flat(owner._h))
        self._code = _DTYPES[owner.dtype]
        self._f8 = False
        self._sq8 = owner.dtype == "sq8"
        self._d = owner.d
        self._metric = _lib.METRIC_IP
        self.dtype = owner.dtype
        self.nprobe = 1
        self._mutex = owner._mutex
        self._nlabelled = 0
        self._owner = owner  # (keeps the handle alive)

    def __del__(self):  # borrowed: the IvfIndex destroys it
        pass

    def _refuse(self, *a, **kw):
        raise RuntimeError("the inner flat index of an IvfIndex is changed through the IvfIndex (train / add / remove_ids / reset)")

    train = add = add_synthetic = reset = remove_ids = reserve = _refuse


class IvfIndex:
    def __init__(self, d: int, nlist: int, dtype: str = "bf16", metric: int = _lib.METRIC_IP, device: int | None = None):
        if dtype not in _DTYPES:
            raise NotImplementedError(f"IvfIndex dtype {dtype!r}: 'bf16', 'f32' or 'sq8' (the e4m3 storages are not served)")
        if int(metric) != _lib.METRIC_IP:
            raise NotImplementedError("an IvfIndex ranks by inner product only (the index's L2 is the MIPS->L2 reduction)")
        if int(d) > 1024:
            raise NotImplementedError("IvfIndex: rows of more than 1024 columns are not served")
        if not 1 <= int(nlist) <= 65536:
            raise NotImplementedError(f"IvfIndex: nlist must be 1 .. 65536, got {nlist}")
        self._lib = _lib.load()
        self.device = _lib.require_gpu(device)
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.mips_ivf_create(ctypes.byref(self._h), self.device, int(d), _DTYPES[dtype], int(metric), int(nlist)), "mips_ivf_create")
        self._d, self._nlist, self.dtype = int(d), int(nlist), dtype
        self.nprobe = 1  # lists probe() returns by default (faiss IndexIVF.nprobe)
        self._niter = 10
        self._mutex = threading.RLock()
        self.flat = _FlatView(self)

    # ------------------------------------------------------------------ faiss-like attributes
    @property
    def d(self) -> int:
        return self._d

    @property
    def nlist(self) -> int:
        return self._nlist

    @property
    def ntotal(self) -> int:
        return self.flat.ntotal

    @property
    def metric_type(self) -> int:
        return _lib.METRIC_IP

    @property
    def is_trained(self) -> bool:
        return self._lib.mips_ivf_is_trained(self._h) == 1

    @property
    def niter(self) -> int:
        return self._niter

    @niter.setter
    def niter(self, v: int) -> None:
        _lib.check(self._lib.mips_ivf_set_param(self._h, b"ivf_niter", int(v)), "mips_ivf_set_param")
        self._niter = int(v)

    def __len__(self) -> int:
        return self.ntotal

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.mips_ivf_destroy(h)
            except Exception:
                pass
            h.value = None

    def _rows(self, x, what: str):
        """float32 / bfloat16 rows or queries, host or device -> (pointer, dtype code, is_device, n, keepalive)"""
        import torch

        if isinstance(x, torch.Tensor):
            if x.dtype not in (torch.float32, torch.bfloat16):
                if not x.dtype.is_floating_point:
                    raise NotImplementedError(f"{what}: raw codes cannot be assigned to a list (float32 or bfloat16 values)")
                x = x.float()
        elif np.asarray(x).dtype.kind in "iub":
            raise NotImplementedError(f"{what}: raw codes (uint8 SQ8 codes, uint16 bf16 bits) cannot be assigned to a list")
        return self.flat._as_buffer(x, what)

    # ------------------------------------------------------------------ building
    def train(self, x) -> None:
        """Deterministic k-means (include/mips_hip_ivf.h): niter iterations from evenly spaced initial rows; an 'sq8' index also
        trains its per-column range on x.  Raises on n < nlist, on NaN / infinity and on an index that holds rows."""
        ptr, code, is_dev, n, keep = self._rows(x, "train")
        with self._mutex:
            _lib.check(self._lib.mips_ivf_train(self._h, ptr, n, code, _lib.Q_DEVICE if is_dev else 0, _stream_handle(self.device)), "mips_ivf_train")
        del keep

    def centroids(self) -> np.ndarray:
        out = np.empty((self._nlist, self._d), np.float32)
        with self._mutex:
            _lib.check(self._lib.mips_ivf_get_centroids(self._h, out.ctypes.data), "mips_ivf_get_centroids")
        return out

    def set_centroids(self, c) -> None:
        """Plant the centroids (stored as given, not normalised) of an EMPTY index; an 'sq8' index needs flat.set_sq8_params too."""
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
        if c.shape != (self._nlist, self._d):
            raise ValueError(f"set_centroids: expected [{self._nlist}, {self._d}], got {c.shape}")
        with self._mutex:
            _lib.check(self._lib.mips_ivf_set_centroids(self._h, c.ctypes.data), "mips_ivf_set_centroids")

    def set_sq8_params(self, vmin, vdiff) -> None:
        MipsIndex.set_sq8_params(self.flat, vmin, vdiff)

    def add(self, x) -> None:
        if not self.is_trained:
            raise RuntimeError("add: the IvfIndex is not trained (train(x) first, as faiss requires)")
        ptr, code, is_dev, n, keep = self._rows(x, "add")
        with self._mutex:
            _lib.check(self._lib.mips_ivf_add(self._h, ptr, n, code, is_dev, _stream_handle(self.device)), "mips_ivf_add")
        del keep

    def reset(self) -> None:
        with self._mutex:
            _lib.check(self._lib.mips_ivf_reset(self._h), "mips_ivf_reset")
            self.flat._nlabelled = 0

    def remove_ids(self, sel, sel_bit0: int = 0) -> int:
        """faiss remove_ids: as MipsIndex.remove_ids; the assignments follow their rows and the list table is rebuilt."""
        from .selector import Selector, is_id_list

        sel_bit0 = int(sel_bit0)
        with self._mutex:
            if is_id_list(sel):
                sel = Selector.from_ids(sel, sel_bit0 + self.ntotal, device=self.device)
            ptr, nbits, flag, keep = self.flat._sel_args(sel, sel_bit0, "remove_ids")
            counts = (ctypes.c_int64 * 2)()
            _lib.check(self._lib.mips_ivf_remove(self._h, ptr, nbits, sel_bit0, flag, counts, _stream_handle(self.device)), "mips_ivf_remove")
            self.flat._nlabelled = int(counts[1])
        del keep
        return int(counts[0])

    def update_rows(self, ids, x, idx_offset: int = 0, return_count: bool = False):
        """faiss IndexIVF.update_vectors: MipsIndex.update_rows on the stored rows, and every written row moves to the list add()
        would give its new value (mips_ivf_update); the list table is rebuilt.  float32 / bfloat16 values only, as add().
        Afterwards the index equals a fresh IvfIndex with the same centroids that was given the final rows.  flat.update_rows
        alone changes the row and leaves it in its old list."""
        if not self.is_trained:
            raise RuntimeError("update_rows: the IvfIndex is not trained (train(x) first, as faiss requires)")
        xptr, code, x_dev, n, keep = self._rows(x, "update_rows")  # (refuses raw codes)
        iptr, shape, ids_dev, keep_ids = self.flat._ids_arg(ids, "update_rows")
        if shape != (n,):
            raise ValueError(f"update_rows: ids {shape} for {n} rows")
        flags = (_lib.IDS_DEVICE if ids_dev else 0) | (_lib.Q_DEVICE if x_dev else 0)
        count = ctypes.c_int64(0)
        with self._mutex:
            _lib.check(self._lib.mips_ivf_update(self._h, iptr, n, int(idx_offset), xptr, code, flags,
                                                 ctypes.byref(count) if return_count else None, _stream_handle(self.device)), "mips_ivf_update")
        del keep, keep_ids
        return int(count.value) if return_count else None

    def list_sizes(self) -> np.ndarray:
        out = np.empty(self._nlist, np.int64)
        with self._mutex:
            _lib.check(self._lib.mips_ivf_list_sizes(self._h, out.ctypes.data, _stream_handle(self.device)), "mips_ivf_list_sizes")
        return out

    def assignments(self) -> np.ndarray:
        """int32 [ntotal]: the list of every row"""
        out = np.empty(self.ntotal, np.int32)
        with self._mutex:
            _lib.check(self._lib.mips_ivf_read_assign(self._h, 0, out.shape[0], out.ctypes.data, _stream_handle(self.device)), "mips_ivf_read_assign")
        return out

    # ------------------------------------------------------------------ searching
    def probe(self, x, nprobe: int | None = None, device_out: bool = False):
        """P(q): int32 [nq, min(nprobe, nlist)], the probed lists of every query, nearest first.  A NumPy array; with device_out
        (CUDA queries only) a CUDA tensor, stream-ordered: nothing synchronises, so the call may be captured into a graph."""
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        ptr, code, is_dev, nq, keep = self._rows(x, "probe")
        if nprobe < 1:
            raise ValueError("nprobe must be >= 1")
        if device_out:
            import torch

            if not is_dev:
                raise ValueError("probe(device_out=True) takes CUDA queries")
            out = torch.empty((nq, min(nprobe, self._nlist)), dtype=torch.int32, device=f"cuda:{self.device}")
            with self._mutex:
                _lib.check(self._lib.mips_ivf_probe(self._h, ptr, code, nq, nprobe, out.data_ptr(), _lib.Q_DEVICE | _lib.OUT_DEVICE,
                                                    _stream_handle(self.device)), "mips_ivf_probe")
            del keep
            return out
        out = np.empty((nq, min(nprobe, self._nlist)), np.int32)
        with self._mutex:
            _lib.check(self._lib.mips_ivf_probe(self._h, ptr, code, nq, nprobe, out.ctypes.data, _lib.Q_DEVICE if is_dev else 0,
                                                _stream_handle(self.device)), "mips_ivf_probe")
        del keep
        return out

    def set_labels(self, labels, row0: int = 0) -> None:
        """One int32 group label per row (MipsIndex.set_labels on the inner flat index): what groups= of search_probed tests.  The
        labels follow their rows through remove_ids, save and load; rows added later need theirs before the next grouped search."""
        self.flat.set_labels(labels, row0)

    def labels(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        return self.flat.labels(row0, n)

    def labels_of(self, ids, idx_offset: int = 0):
        return self.flat.labels_of(ids, idx_offset)

    def search_probed(self, x, k: int, nprobe: int | None = None, idx_offset: int = 0, selector=None, groups=None, group_mode: str = "exclude",
                      sel_bit0: int = 0):
        """(D, I) [nq, k]: for every query the best k of the rows whose list lies in P(q) -- the flat storage's canonical score, ordered
        by (score descending, row ascending), -1 / -inf padding (include/mips_hip_ivf.h).  nprobe defaults to self.nprobe.  NumPy in
        gives NumPy out; a CUDA tensor in gives CUDA tensors out, stream-ordered (graph-capturable in steady state).
        selector (a Selector, a list of row ids, a bool mask or a NumPy uint8 bitmap; one for all queries; bit sel_bit0 + i decides row
        i) and groups (an int array [nq], NumPy -> host, CUDA tensor -> device) with group_mode "exclude" / "only" are those of
        MipsIndex.search_wide: only admitted rows can be results -- what the search returns on an index from which the others were
        deleted, row numbers kept.  The rows are refused inside the list scan, so nothing is fetched in excess and dropped."""
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        k = int(k)
        ptr, code, is_dev, nq, keep = self._rows(x, "search_probed")
        if selector is not None:
            from .selector import Selector, is_id_list

            if is_id_list(selector):
                selector = Selector.from_ids(selector, int(sel_bit0) + self.ntotal, device=self.device)
        sel_ptr, sel_nbits, sel_flag, sel_keep = self.flat._sel_args(selector, sel_bit0, "search_probed")
        grp_ptr, grp_mode, grp_flag, grp_keep = self.flat._grp_args(groups, group_mode, nq, "search_probed")
        stream = _stream_handle(self.device)
        if is_dev:
            import torch

            dev = f"cuda:{self.device}"
            D = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
            I = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
            dp, ip, flags = D.data_ptr(), I.data_ptr(), _lib.Q_DEVICE | _lib.OUT_DEVICE
        else:
            D = np.empty((nq, max(k, 0)), np.float32)
            I = np.empty((nq, max(k, 0)), np.int64)
            dp, ip, flags = D.ctypes.data, I.ctypes.data, 0
        with self._mutex:
            if groups is not None:
                _lib.check(self._lib.mips_ivf_search_grp(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags | sel_flag | grp_flag,
                                                         sel_ptr, sel_nbits, int(sel_bit0), grp_ptr, grp_mode, stream), "mips_ivf_search_grp")
            elif selector is not None:
                _lib.check(self._lib.mips_ivf_search_sel(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags | sel_flag,
                                                         sel_ptr, sel_nbits, int(sel_bit0), stream), "mips_ivf_search_sel")
            else:
                _lib.check(self._lib.mips_ivf_search(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags, stream), "mips_ivf_search")
        del keep, sel_keep, grp_keep
        return D, I

    def search_probed_wide(self, x, k: int, nprobe: int | None = None, idx_offset: int = 0, selector=None, groups=None, group_mode: str = "exclude",
                           sel_bit0: int = 0):
        """search_probed for 1 <= k <= MAX_K_WIDE (include/mips_hip_ivf.h: mips_ivf_search_wide / _grp): the same definition, the same
        arguments, the same contract -- NumPy in gives NumPy out; a CUDA tensor in gives CUDA tensors out, stream-ordered
        (graph-capturable in steady state).  Every probed row is scored exactly, so nothing is approximated or certified; for k' <= k
        the first k' columns are the result for k', and for k' <= MAX_K those of search_probed.  Raises NotImplementedError for
        k > MAX_K_WIDE (as MipsIndex.search_wide does) and RuntimeError for what the library refuses, min(nprobe, nlist) * k > 65536
        among it."""
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        k = int(k)
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"search_probed_wide: k = {k} exceeds MAX_K_WIDE = {_lib.MAX_K_WIDE}")
        ptr, code, is_dev, nq, keep = self._rows(x, "search_probed_wide")
        if selector is not None:
            from .selector import Selector, is_id_list

            if is_id_list(selector):
                selector = Selector.from_ids(selector, int(sel_bit0) + self.ntotal, device=self.device)
        sel_ptr, sel_nbits, sel_flag, sel_keep = self.flat._sel_args(selector, sel_bit0, "search_probed_wide")
        grp_ptr, grp_mode, grp_flag, grp_keep = self.flat._grp_args(groups, group_mode, nq, "search_probed_wide")
        stream = _stream_handle(self.device)
        if is_dev:
            import torch

            dev = f"cuda:{self.device}"
            D = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
            I = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
            dp, ip, flags = D.data_ptr(), I.data_ptr(), _lib.Q_DEVICE | _lib.OUT_DEVICE
        else:
            D = np.empty((nq, max(k, 0)), np.float32)
            I = np.empty((nq, max(k, 0)), np.int64)
            dp, ip, flags = D.ctypes.data, I.ctypes.data, 0
        with self._mutex:
            if selector is not None or groups is not None:  # a bitmap alone is q_labels == NULL
                _lib.check(self._lib.mips_ivf_search_wide_grp(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags | sel_flag | grp_flag,
                                                              sel_ptr, sel_nbits, int(sel_bit0), grp_ptr, grp_mode, stream), "mips_ivf_search_wide_grp")
            else:
                _lib.check(self._lib.mips_ivf_search_wide(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags, stream), "mips_ivf_search_wide")
        del keep, sel_keep, grp_keep
        return D, I

    def search_part(self, x, k: int, nprobe: int | None = None, idx_offset: int = 0, selector=None, groups=None, group_mode: str = "exclude",
                    sel_bit0: int = 0):
        """The search of ONE PART of a row-sharded IVF index (include/mips_hip_ivf_sharded.h: mips_ivf_search_part): search_probed_wide
        cut behind its merge.  -> (payload, bias): payload int64 [nq, k, 2] = {float32 bits of the RANKING score (an 'sq8' index: S, not
        D), row + idx_offset}, padding {bits of -inf, -1}; bias float64 [nq] = B_q on an 'sq8' index, None otherwise.  ivf_merge_parts
        over the payloads of all parts finishes the search.  Arguments and NumPy / CUDA forms as search_probed_wide; nothing of the
        call stays in the index."""
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        k = int(k)
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"search_part: k = {k} exceeds MAX_K_WIDE = {_lib.MAX_K_WIDE}")
        ptr, code, is_dev, nq, keep = self._rows(x, "search_part")
        if selector is not None:
            from .selector import Selector, is_id_list

            if is_id_list(selector):
                selector = Selector.from_ids(selector, int(sel_bit0) + self.ntotal, device=self.device)
        sel_ptr, sel_nbits, sel_flag, sel_keep = self.flat._sel_args(selector, sel_bit0, "search_part")
        grp_ptr, grp_mode, grp_flag, grp_keep = self.flat._grp_args(groups, group_mode, nq, "search_part")
        sq8 = self.dtype == "sq8"
        if is_dev:
            import torch

            dev = f"cuda:{self.device}"
            P = torch.empty((nq, max(k, 0), 2), dtype=torch.int64, device=dev)
            B = torch.empty(nq, dtype=torch.float64, device=dev) if sq8 else None
            pp, bp, flags = P.data_ptr(), (B.data_ptr() if sq8 else None), _lib.Q_DEVICE | _lib.OUT_DEVICE
        else:
            P = np.empty((nq, max(k, 0), 2), np.int64)
            B = np.empty(nq, np.float64) if sq8 else None
            pp, bp, flags = P.ctypes.data, (B.ctypes.data if sq8 else None), 0
        with self._mutex:
            _lib.check(self._lib.mips_ivf_search_part(self._h, ptr, code, nq, k, nprobe, pp, bp, int(idx_offset), flags | sel_flag | grp_flag,
                                                      sel_ptr, sel_nbits, int(sel_bit0), grp_ptr, grp_mode, _stream_handle(self.device)),
                       "mips_ivf_search_part")
        del keep, sel_keep, grp_keep
        return P, B

    # ------------------------------------------------------------------ range search over the probed lists
    def _range_radii(self, radius, nq: int):
        """-> (pointer, flag, keepalive): a CUDA float32 tensor [nq] is read where it is (MIPS_RADII_DEVICE); anything else becomes
        host float32 [nq], a NaN refused"""
        import torch

        if isinstance(radius, torch.Tensor) and radius.is_cuda:
            if radius.dtype != torch.float32 or radius.dim() != 1 or radius.shape[0] != nq or not radius.is_contiguous() or radius.device.index != self.device:
                raise ValueError(f"range_search_probed: device radii must be a contiguous CUDA float32 tensor [{nq}] on cuda:{self.device}")
            return radius.data_ptr(), _lib.RADII_DEVICE, radius
        r = MipsIndex._radii(radius, nq)
        return r.ctypes.data, 0, r

    def range_search_probed_into(self, x, radius, lims, D, I, nprobe: int | None = None, idx_offset: int = 0, selector=None, groups=None,
                                 group_mode: str = "exclude", sel_bit0: int = 0) -> None:
        """The non-synchronising form of range_search_probed (include/mips_hip_ivf_range.h): the caller allocates the CUDA tensors lims
        (int64 [nq + 1]), D (float32 [cap]) and I (int64 [cap]); everything is enqueued on the current stream, so with CUDA queries
        (and CUDA radii, groups and a device selector) the call may be captured into a graph.  lims always receives the true counts;
        when lims[-1] > cap the contents of D and I are unspecified and the call is to be repeated with larger tensors.  cap = 0
        (empty D and I) is a counting call.  `radius`: a scalar, nq host values, or a CUDA float32 tensor [nq] that is read on the
        device (a NaN there makes its query hit nothing; a host NaN raises)."""
        import torch

        nprobe = int(self.nprobe if nprobe is None else nprobe)
        ptr, code, is_dev, nq, keep = self._rows(x, "range_search_probed")
        if selector is not None:
            from .selector import Selector, is_id_list

            if is_id_list(selector):
                selector = Selector.from_ids(selector, int(sel_bit0) + self.ntotal, device=self.device)
        sel_ptr, sel_nbits, sel_flag, sel_keep = self.flat._sel_args(selector, sel_bit0, "range_search_probed")
        grp_ptr, grp_mode, grp_flag, grp_keep = self.flat._grp_args(groups, group_mode, nq, "range_search_probed")
        rad_ptr, rad_flag, rad_keep = self._range_radii(radius, nq)
        dev = torch.device("cuda", self.device)
        for t, dt, what in ((lims, torch.int64, "lims"), (D, torch.float32, "D"), (I, torch.int64, "I")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
                raise ValueError(f"range_search_probed_into: {what} must be a contiguous 1-d CUDA {dt} tensor on cuda:{self.device}")
        if lims.shape[0] != nq + 1 or D.shape[0] != I.shape[0]:
            raise ValueError(f"range_search_probed_into: lims must have {nq + 1} entries and D, I one length")
        cap = int(D.shape[0])
        flags = _lib.OUT_DEVICE | (_lib.Q_DEVICE if is_dev else 0) | rad_flag
        dp, ip = (D.data_ptr(), I.data_ptr()) if cap else (None, None)
        stream = _stream_handle(self.device)
        with self._mutex:
            if selector is not None or groups is not None:  # a bitmap alone is q_labels == NULL
                _lib.check(self._lib.mips_ivf_range_search_grp(self._h, ptr, code, nq, rad_ptr, nprobe, lims.data_ptr(), dp, ip, cap, int(idx_offset),
                                                               flags | sel_flag | grp_flag, sel_ptr, sel_nbits, int(sel_bit0), grp_ptr, grp_mode, stream),
                           "mips_ivf_range_search_grp")
            else:
                _lib.check(self._lib.mips_ivf_range_search(self._h, ptr, code, nq, rad_ptr, nprobe, lims.data_ptr(), dp, ip, cap, int(idx_offset), flags,
                                                           stream), "mips_ivf_range_search")
        del keep, sel_keep, grp_keep, rad_keep

    def range_search_probed(self, x, radius, nprobe: int | None = None, idx_offset: int = 0, selector=None, groups=None, group_mode: str = "exclude",
                            sel_bit0: int = 0):
        """(lims, D, I): for every query the rows of the probed lists that the filter admits and whose reported score is strictly above
        the radius (include/mips_hip_ivf_range.h) -- the flat storage's canonical score, an 'sq8' index's D -- in CSR form as
        MipsIndex.range_search returns it: the hits of query j are D / I [lims[j] : lims[j + 1]], in ascending row order.  `radius` is
        a scalar, nq values, or a CUDA float32 tensor [nq].  NumPy in gives NumPy out; a CUDA tensor in gives CUDA tensors out.  The
        result's size is not known beforehand: a first call runs with a guessed capacity, lims[-1] is READ ON THE HOST -- THIS
        SYNCHRONISES the stream -- and one repeat with the exact size follows if the guess was too small
        (range_search_probed_into is the form that never synchronises).  selector, groups, group_mode, sel_bit0: as search_probed."""
        import torch

        from .selector import Selector, is_id_list

        if selector is not None and not isinstance(selector, (Selector, np.ndarray)):   # packed once for the repeat call
            selector = Selector.from_ids(selector, int(sel_bit0) + self.ntotal, device=self.device) if is_id_list(selector) else \
                Selector.from_mask(selector, device=self.device)
        if isinstance(selector, np.ndarray) and selector.dtype != np.uint8:
            selector = Selector.from_mask(selector, device=self.device)
        ptr, code, is_dev, nq, keep = self._rows(x, "range_search_probed")
        if not (isinstance(radius, torch.Tensor) and radius.is_cuda):
            radius = MipsIndex._radii(radius, nq)
        dev = f"cuda:{self.device}"
        lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        cap = max(1 << 16, 256 * nq)
        while True:
            D = torch.empty(cap, dtype=torch.float32, device=dev)
            I = torch.empty(cap, dtype=torch.int64, device=dev)
            self.range_search_probed_into(keep, radius, lims, D, I, nprobe=nprobe, idx_offset=idx_offset, selector=selector, groups=groups,
                                          group_mode=group_mode, sel_bit0=sel_bit0)
            total = int(lims[-1].item())   # the synchronisation
            if total <= cap:
                break
            cap = total
        D, I = D[:total], I[:total]
        if is_dev:
            return lims, D.clone() if total < cap else D, I.clone() if total < cap else I
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    # rows by id: the inner flat index's (row ids are the flat ids)
    def reconstruct(self, key: int):
        return self.flat.reconstruct(key)

    def reconstruct_n(self, n0: int = 0, ni: int | None = None):
        return self.flat.reconstruct_n(n0, ni)

    def reconstruct_batch(self, ids, **kw):
        return self.flat.reconstruct_batch(ids, **kw)

    def _refused(self, *a, **kw):
        raise NotImplementedError("IvfIndex: the search over the probed lists is search_probed(x, k, nprobe) (DESIGN.md 4j); the faiss-shaped "
                                  "forms are not served on an IVF index, and `flat` searches all rows exactly")

    search = search_packed = search_wide = range_search = search_fused = search_wide_packed = _refused

    # ------------------------------------------------------------------ persistence
    #   the inner index's files (MipsIndex.save) + centroids.f32 (raw float32 [nlist, d]) + assign.i32 (int32 [ntotal]);
    #   meta.json carries "nlist" and "niter"
    def save(self, path: str, extra: dict | None = None) -> None:
        if not self.is_trained:
            raise RuntimeError("save: the IvfIndex is not trained")
        ext = {"nlist": self._nlist, "niter": self._niter}
        ext.update(extra or {})
        MipsIndex.save(self.flat, path, extra=ext)
        with open(os.path.join(path, "centroids.f32"), "wb") as f:
            f.write(self.centroids().astype("<f4").tobytes())
        with open(os.path.join(path, "assign.i32"), "wb") as f:
            f.write(self.assignments().astype("<i4").tobytes())

    @classmethod
    def load(cls, path: str, device: int | None = None, chunk_rows: int = 1 << 16) -> "IvfIndex":
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("format") != _FORMAT_VERSION or "nlist" not in meta:
            raise ValueError("not a saved IvfIndex")
        n, d = meta["ntotal"], meta["d"]
        ix = cls(d, meta["nlist"], dtype=meta["dtype"], device=device)
        ix.niter = meta.get("niter", 10)
        ix.set_centroids(np.fromfile(os.path.join(path, "centroids.f32"), dtype="<f4").reshape(ix.nlist, d))
        if meta.get("sq8_vmin") is not None:
            ix.set_sq8_params([float.fromhex(v) for v in meta["sq8_vmin"]], [float.fromhex(v) for v in meta["sq8_vdiff"]])
        if n > 0:
            fext, npdt = _ROWS_FILE[meta["dtype"]]
            mm = np.memmap(os.path.join(path, "rows." + fext), dtype=npdt, mode="r", shape=(n, d))
            for r0 in range(0, n, chunk_rows):  # the rows in their stored form, straight into the inner index
                MipsIndex.add(ix.flat, np.asarray(mm[r0:min(n, r0 + chunk_rows)]))
            del mm
            assign = np.ascontiguousarray(np.fromfile(os.path.join(path, "assign.i32"), dtype="<i4").astype(np.int32))
            with ix._mutex:
                _lib.check(ix._lib.mips_ivf_set_assign(ix._h, assign.ctypes.data, n, _stream_handle(ix.device)), "mips_ivf_set_assign")
            if meta.get("labels"):
                ix.flat.set_labels(np.fromfile(os.path.join(path, "labels.i32"), dtype="<i4"))
        ix.meta = meta
        return ix


def ivf_merge_parts(gathered, parts: int, nq: int, k: int, bias=None):
    """The merge of the gathered payloads of IvfIndex.search_part (include/mips_hip_ivf_sharded.h: mips_ivf_merge_parts): gathered is
    a contiguous CUDA int64 tensor of parts * nq * k * 2 words, part p (lower global rows than part p + 1) first; bias a CUDA float64
    tensor [nq] (any part's B_q: an 'sq8' index) or None.  -> (D float32 [nq, k], I int64 [nq, k]) on gathered's device,
    stream-ordered; the order is fixed on the ranking scores and S becomes D = (float)((double)S + B_q) behind it."""
    import torch

    parts, nq, k = int(parts), int(nq), int(k)
    if not (isinstance(gathered, torch.Tensor) and gathered.is_cuda and gathered.dtype == torch.int64 and gathered.is_contiguous()
            and gathered.numel() == parts * nq * k * 2):
        raise ValueError(f"ivf_merge_parts: gathered must be a contiguous CUDA int64 tensor of {parts} x {nq} x {k} x 2 words")
    dev = gathered.device
    if bias is not None and not (isinstance(bias, torch.Tensor) and bias.device == dev and bias.dtype == torch.float64 and bias.is_contiguous()
                                 and bias.numel() == nq):
        raise ValueError(f"ivf_merge_parts: bias must be a contiguous float64 tensor [{nq}] on {dev}")
    D = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
    I = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().mips_ivf_merge_parts(gathered.data_ptr(), parts, nq, k, bias.data_ptr() if bias is not None else None, D.data_ptr(),
                                                I.data_ptr(), dev.index, _stream_handle(dev.index)), "mips_ivf_merge_parts")
    return D, I
