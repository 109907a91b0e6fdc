"""IvfPqIndex -- an inverted file over product-quantised codes (faiss IndexIVFPQ; include/mips_hip_ivfpq.h): k-means
lists and nprobe as in IvfIndex, M one-byte codes per row as in PqIndex, the codes taken on the row's RESIDUAL against its list's
centroid.  A search reads only the codes of the probed lists; the score of a row is the probe's score of its list plus the ADC sum.

Reached by name only: the factory strings ("IVF4096,PQ32"), Mips, KnowledgeBase and faiss_shim do not route here.  Inner product
only, 8 bits per code, M <= 128, d <= 1024, nlist <= 65536, min(nprobe, nlist) <= 1024, search k <= MAX_K (search_candidates:
k <= MAX_K_WIDE); no range search, selectors, groups, remove_ids, update_rows, sharding or OPQ.

All arithmetic happens in libmips_hip.so; this file moves pointers.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading

import numpy as np

from . import _lib
from .index import _FORMAT_VERSION, _stream_handle
from .pq import PqIndex

_KSUB = 256


class IvfPqIndex:
    def __init__(self, d: int, nlist: int, M: int, nbits: int = 8, by_residual: bool = True, metric: int = _lib.METRIC_IP, device: int | None = None):
        d, nlist, M = int(d), int(nlist), int(M)
        if int(metric) != _lib.METRIC_IP:
            raise NotImplementedError("an IvfPqIndex ranks by inner product only (coarse term plus a table of inner products)")
        if int(nbits) != 8:
            raise NotImplementedError(f"IvfPqIndex: {nbits} bits per code are not served (8: 256 centroids per sub-quantiser)")
        if d > 1024:
            raise NotImplementedError("IvfPqIndex: rows of more than 1024 columns are not served")
        if M > 128:
            raise NotImplementedError(f"IvfPqIndex: M = {M} exceeds 128 (the query's table is M KiB of LDS)")
        if not 1 <= nlist <= 65536:
            raise NotImplementedError(f"IvfPqIndex: nlist must be 1 .. 65536, got {nlist}")
        if M < 1 or d < 1 or d % M != 0:
            raise ValueError(f"IvfPqIndex: d = {d} must be a positive multiple of M = {M} >= 1")
        self._lib = _lib.load()
        self.device = _lib.require_gpu(device)
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.mips_ivfpq_create(ctypes.byref(self._h), self.device, d, nlist, M, int(nbits), 1 if by_residual else 0, int(metric)),
                   "mips_ivfpq_create")
        self._d, self._nlist, self._M, self._by_residual = d, nlist, M, bool(by_residual)
        self.nprobe = 1  # lists a search probes by default (faiss IndexIVF.nprobe)
        self._niter = 10
        self._pq_niter = 10
        self._query_slice = 256
        self._scan_segments = 0
        self._mutex = threading.RLock()

    # ------------------------------------------------------------------ faiss-like attributes
    d = property(lambda self: self._d)
    nlist = property(lambda self: self._nlist)
    M = property(lambda self: self._M)
    dsub = property(lambda self: self._d // self._M)
    nbits = property(lambda self: 8)
    by_residual = property(lambda self: self._by_residual)
    metric_type = property(lambda self: _lib.METRIC_IP)

    @property
    def ntotal(self) -> int:
        return int(self._lib.mips_ivfpq_ntotal(self._h))

    @property
    def is_trained(self) -> bool:
        return self._lib.mips_ivfpq_is_trained(self._h) == 1

    @property
    def bytes_per_row(self) -> int:
        """bytes of one row: M codes and its int32 list number; centroids (4 nlist d bytes) and codebook (1024 d bytes) are shared"""
        return self._M + 4

    def _param(name: str, attr: str, doc: str):  # noqa: N805 -- a property over mips_ivfpq_set_param
        def get(self) -> int:
            return getattr(self, attr)

        def put(self, v: int) -> None:
            _lib.check(self._lib.mips_ivfpq_set_param(self._h, name.encode(), int(v)), "mips_ivfpq_set_param")
            setattr(self, attr, int(v))

        return property(get, put, doc=doc)

    niter = _param("ivf_niter", "_niter", "k-means iterations of the coarse quantiser")
    pq_niter = _param("pq_niter", "_pq_niter", "k-means iterations of the sub-quantisers")
    query_slice = _param("pq_query_slice", "_query_slice", "queries one pass of a search serves")
    scan_segments = _param("scan_segments", "_scan_segments", "0: the library chooses the scan's segments per query; else forced")
    del _param

    def __len__(self) -> int:
        return self.ntotal

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.mips_ivfpq_destroy(h)
            except Exception:
                pass
            h.value = None

    _rows = PqIndex._rows          # float32 / bfloat16 rows or queries -> (pointer, dtype code, is_device, n, keepalive)
    _ids_arg = PqIndex._ids_arg    # ids of any shape -> (pointer, shape, is_device, keepalive)

    # ------------------------------------------------------------------ building
    def train(self, x) -> None:
        """The centroids IvfIndex.train gives on x (niter), then the codebook PqIndex.train gives (pq_niter) on the residuals of at
        most 65536 evenly spaced rows of x.  Raises on n < max(nlist, 256), on a NaN or an infinity and on an index that holds rows."""
        ptr, code, is_dev, n, keep = self._rows(x, "train")
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_train(self._h, ptr, n, code, _lib.Q_DEVICE if is_dev else 0, _stream_handle(self.device)), "mips_ivfpq_train")
        del keep

    def centroids(self) -> np.ndarray:
        """float32 [nlist, d]"""
        out = np.empty((self._nlist, self._d), np.float32)
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_get_centroids(self._h, out.ctypes.data), "mips_ivfpq_get_centroids")
        return out

    def set_centroids(self, c) -> None:
        """Plant the centroids [nlist, d] (stored as given) of an EMPTY index; with a codebook too the index is trained."""
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
        if c.shape != (self._nlist, self._d):
            raise ValueError(f"set_centroids: expected [{self._nlist}, {self._d}], got {c.shape}")
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_set_centroids(self._h, c.ctypes.data), "mips_ivfpq_set_centroids")

    def codebook(self) -> np.ndarray:
        """float32 [M, 256, dsub]"""
        out = np.empty((self._M, _KSUB, self.dsub), np.float32)
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_get_codebook(self._h, out.ctypes.data), "mips_ivfpq_get_codebook")
        return out

    def set_codebook(self, c) -> None:
        """Plant the codebook [M, 256, dsub] (stored as given) of an EMPTY index; with centroids too the index is trained."""
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
        if c.shape != (self._M, _KSUB, self.dsub):
            raise ValueError(f"set_codebook: expected [{self._M}, {_KSUB}, {self.dsub}], got {c.shape}")
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_set_codebook(self._h, c.ctypes.data), "mips_ivfpq_set_codebook")

    def add(self, x) -> None:
        """Assign, encode (the residual) and append float32 / bfloat16 rows (NumPy, or a torch tensor on the host or the device)."""
        if not self.is_trained:
            raise RuntimeError("add: the IvfPqIndex is not trained (train(x) first, as faiss requires)")
        ptr, code, is_dev, n, keep = self._rows(x, "add")
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_add(self._h, ptr, n, code, is_dev, _stream_handle(self.device)), "mips_ivfpq_add")
        del keep

    def add_codes(self, codes, assign) -> None:
        """Append rows given as their codes uint8 [n, M] and their lists int32 [n] (both NumPy or both CUDA tensors), stored as given."""
        import torch

        if not self.is_trained:
            raise RuntimeError("add_codes: the IvfPqIndex is not trained (train(x), or set_centroids and set_codebook)")
        if isinstance(codes, torch.Tensor) and codes.is_cuda:
            if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != self._M:
                raise ValueError(f"add_codes: expected uint8 [n, {self._M}], got {codes.dtype} {tuple(codes.shape)}")
            dev = f"cuda:{self.device}"
            codes = codes.to(dev).contiguous()
            assign = torch.as_tensor(assign).to(dev).to(torch.int32).contiguous()
            if tuple(assign.shape) != (codes.shape[0],):
                raise ValueError(f"add_codes: {tuple(assign.shape)} assignments for {codes.shape[0]} rows")
            cp, ap, n, is_dev = codes.data_ptr(), assign.data_ptr(), codes.shape[0], 1
        else:
            codes = codes.numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
            if codes.dtype != np.uint8 or codes.ndim != 2 or codes.shape[1] != self._M:
                raise ValueError(f"add_codes: expected uint8 [n, {self._M}], got {codes.dtype} {codes.shape}")
            codes = np.ascontiguousarray(codes)
            assign = assign.cpu().numpy() if isinstance(assign, torch.Tensor) else np.asarray(assign)
            if assign.shape != (codes.shape[0],) or (assign.size and assign.dtype.kind not in "iu"):
                raise ValueError(f"add_codes: assignments {assign.dtype} {assign.shape} for {codes.shape[0]} rows")
            if assign.size and (assign.min() < 0 or assign.max() >= self._nlist):
                raise ValueError(f"add_codes: assignments must lie in [0, {self._nlist})")
            assign = np.ascontiguousarray(assign, dtype=np.int32)
            cp, ap, n, is_dev = codes.ctypes.data, assign.ctypes.data, codes.shape[0], 0
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_add_codes(self._h, cp, ap, n, is_dev, _stream_handle(self.device)), "mips_ivfpq_add_codes")

    def codes(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """uint8 [n, M]: the codes of rows [row0, row0 + n)"""
        row0 = int(row0)
        n = self.ntotal - row0 if n is None else int(n)
        out = np.empty((max(n, 0), self._M), np.uint8)
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_read_codes(self._h, row0, n, out.ctypes.data, _stream_handle(self.device)), "mips_ivfpq_read_codes")
        return out

    def assignments(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """int32 [n]: the lists of rows [row0, row0 + n)"""
        row0 = int(row0)
        n = self.ntotal - row0 if n is None else int(n)
        out = np.empty(max(n, 0), np.int32)
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_read_assign(self._h, row0, n, out.ctypes.data, _stream_handle(self.device)), "mips_ivfpq_read_assign")
        return out

    def list_sizes(self) -> np.ndarray:
        out = np.empty(self._nlist, np.int64)
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_list_sizes(self._h, out.ctypes.data, _stream_handle(self.device)), "mips_ivfpq_list_sizes")
        return out

    def reset(self) -> None:
        """Drop all rows; centroids and codebook stay."""
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_reset(self._h), "mips_ivfpq_reset")

    # ------------------------------------------------------------------ searching
    def probe(self, x, nprobe: int | None = None, return_scores: bool = False):
        """P(q): int32 [nq, min(nprobe, nlist)], the probed lists of every query, nearest first; with return_scores also the coarse
        terms T float32 of the same shape.  NumPy in gives NumPy out; a CUDA tensor in gives CUDA tensors out, stream-ordered."""
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        if nprobe < 1:
            raise ValueError("nprobe must be >= 1")
        ptr, code, is_dev, nq, keep = self._rows(x, "probe")
        p = min(nprobe, self._nlist)
        if is_dev:
            import torch

            dev = f"cuda:{self.device}"
            L = torch.empty((nq, p), dtype=torch.int32, device=dev)
            T = torch.empty((nq, p), dtype=torch.float32, device=dev) if return_scores else None
            lp, tp, flags = L.data_ptr(), T.data_ptr() if return_scores else None, _lib.Q_DEVICE | _lib.OUT_DEVICE
        else:
            L = np.empty((nq, p), np.int32)
            T = np.empty((nq, p), np.float32) if return_scores else None
            lp, tp, flags = L.ctypes.data, T.ctypes.data if return_scores else None, 0
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_probe(self._h, ptr, code, nq, nprobe, lp, tp, flags, _stream_handle(self.device)), "mips_ivfpq_probe")
        del keep
        return (L, T) if return_scores else L

    def search(self, x, k: int, nprobe: int | None = None, idx_offset: int = 0):
        """(D, I) [nq, k]: the best k of the rows whose list is among the query's min(nprobe, nlist) nearest, by (D descending, row
        ascending); D = the probe's score of the row's list, then the query's table entries at the row's codes added in ascending m,
        all in float32; -1 / -inf padding.  nprobe defaults to self.nprobe.  NumPy in gives NumPy out; a CUDA tensor in gives CUDA
        tensors out, stream-ordered, never synchronising (graph-capturable in steady state)."""
        k = int(k)
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        if k > _lib.MAX_K:
            raise NotImplementedError(f"IvfPqIndex.search: k = {k} exceeds MAX_K = {_lib.MAX_K} (search_candidates serves k <= MAX_K_WIDE on PQ codes)")
        if min(nprobe, self._nlist) > 1024:
            raise NotImplementedError(f"IvfPqIndex.search: min(nprobe, nlist) = {min(nprobe, self._nlist)} exceeds 1024")
        ptr, code, is_dev, nq, keep = self._rows(x, "search")
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
            _lib.check(self._lib.mips_ivfpq_search(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags, _stream_handle(self.device)),
                       "mips_ivfpq_search")
        del keep
        return D, I

    def search_candidates(self, x, k: int, nprobe: int | None = None, idx_offset: int = 0):
        """(D, I) [nq, k] for 1 <= k <= MAX_K_WIDE: the definition of search, unchanged -- every row of the probed lists scored, the
        best k by (D descending, row ascending), -1 / -inf padding; the first k' columns are the result for k'.  k <= MAX_K issues
        search's own launches.  The candidate generator in front of MipsIndex.rerank (RefinedIndex).  NumPy in gives
        NumPy out; a CUDA tensor in gives CUDA tensors out, stream-ordered, never synchronising (graph-capturable in steady state)."""
        k = int(k)
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"IvfPqIndex.search_candidates: k = {k} exceeds MAX_K_WIDE = {_lib.MAX_K_WIDE}")
        if min(nprobe, self._nlist) > 1024:
            raise NotImplementedError(f"IvfPqIndex.search_candidates: min(nprobe, nlist) = {min(nprobe, self._nlist)} exceeds 1024")
        ptr, code, is_dev, nq, keep = self._rows(x, "search_candidates")
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
            _lib.check(self._lib.mips_ivfpq_search_candidates(self._h, ptr, code, nq, k, nprobe, dp, ip, int(idx_offset), flags,
                                                              _stream_handle(self.device)), "mips_ivfpq_search_candidates")
        del keep
        return D, I

    def reconstruct_batch(self, ids, idx_offset: int = 0, out=None):
        """The decoded rows ids[...] - idx_offset -> float32 [..., d]: the centroid of the row's list plus the centroids its codes name
        (by_residual=False: the latter alone).  NumPy ids give a NumPy result and an id >= ntotal raises; a CUDA tensor gives a CUDA
        tensor, stream-ordered, and an id that names no row gives a NaN row.  out= (CUDA ids only): a contiguous CUDA float32 tensor."""
        import torch

        ptr, shape, is_dev, keep = self._ids_arg(ids, "reconstruct_batch")
        n = int(np.prod(shape, dtype=np.int64))
        if is_dev:
            if out is None:
                out = torch.empty(shape + (self._d,), dtype=torch.float32, device=f"cuda:{self.device}")
            elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device.index == self.device and out.dtype == torch.float32
                      and tuple(out.shape) == shape + (self._d,) and out.is_contiguous()):
                raise ValueError(f"reconstruct_batch: out must be a contiguous CUDA float32 tensor {shape + (self._d,)} on cuda:{self.device}")
            op, flags = out.data_ptr(), _lib.IDS_DEVICE | _lib.OUT_DEVICE
        else:
            if out is not None:
                raise ValueError("reconstruct_batch: out= goes with CUDA ids")
            out = np.empty(shape + (self._d,), np.float32)
            op, flags = out.ctypes.data, 0
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_reconstruct(self._h, ptr, n, int(idx_offset), op, _lib.DTYPE_F32, self._d, flags, _stream_handle(self.device)),
                       "mips_ivfpq_reconstruct")
        del keep
        return out

    reconstruct = PqIndex.reconstruct
    reconstruct_n = PqIndex.reconstruct_n

    def compute_distance_subset(self, x, ids, idx_offset: int = 0):
        """The score of rows ids[j, t] - idx_offset for query j -> float32 [nq, k], with the coarse term of each row's OWN list, probed
        or not: scoring the I of a search reproduces its D bit for bit.  An id that names no row scores -inf.  NumPy in gives NumPy
        out; CUDA queries and CUDA ids give a CUDA tensor, stream-ordered."""
        import torch

        ptr, code, q_dev, nq, keep = self._rows(x, "compute_distance_subset")
        iptr, shape, ids_dev, keep_ids = self._ids_arg(ids, "compute_distance_subset")
        if len(shape) != 2 or shape[0] != nq:
            raise ValueError(f"compute_distance_subset: ids must be [{nq}, k], got {shape}")
        k = int(shape[1])
        flags = (_lib.Q_DEVICE if q_dev else 0) | (_lib.IDS_DEVICE if ids_dev else 0)
        if q_dev and ids_dev:
            out = torch.empty((nq, k), dtype=torch.float32, device=f"cuda:{self.device}")
            op, flags = out.data_ptr(), flags | _lib.OUT_DEVICE
        else:
            out = np.empty((nq, k), np.float32)
            op = out.ctypes.data
        with self._mutex:
            _lib.check(self._lib.mips_ivfpq_score_subset(self._h, ptr, code, nq, iptr, k, op, int(idx_offset), flags, _stream_handle(self.device)),
                       "mips_ivfpq_score_subset")
        del keep, keep_ids
        return out

    def _refused(self, *a, **kw):
        raise NotImplementedError("IvfPqIndex serves search(x, k <= MAX_K, nprobe), search_candidates(x, k <= MAX_K_WIDE, nprobe), probe, reconstruct* and "
                                  "compute_distance_subset; search_wide, range "
                                  "search, selectors, groups, remove_ids, update_rows and sharding are not served on PQ codes (DESIGN.md 4m)")

    search_wide = range_search = search_packed = search_fused = remove_ids = update_rows = search_probed_wide = range_search_probed = _refused

    # ------------------------------------------------------------------ persistence
    #   meta.json + codes.u8 (uint8 [ntotal, M]) + assign.i32 (little-endian int32 [ntotal]) + codebook.f32 ([M, 256, dsub]) +
    #   centroids.f32 ([nlist, d]), the last two raw little-endian float32
    def save(self, path: str, chunk_rows: int = 1 << 20) -> None:
        if not self.is_trained:
            raise RuntimeError("save: the IvfPqIndex is not trained")
        os.makedirs(path, exist_ok=True)
        n = self.ntotal
        with open(os.path.join(path, "codebook.f32"), "wb") as f:
            f.write(self.codebook().astype("<f4").tobytes())
        with open(os.path.join(path, "centroids.f32"), "wb") as f:
            f.write(self.centroids().astype("<f4").tobytes())
        with open(os.path.join(path, "codes.u8"), "wb") as f, open(os.path.join(path, "assign.i32"), "wb") as g:
            for r0 in range(0, n, chunk_rows):
                nr = min(chunk_rows, n - r0)
                f.write(self.codes(r0, nr).tobytes())
                g.write(self.assignments(r0, nr).astype("<i4").tobytes())
        meta = {"format": _FORMAT_VERSION, "kind": "ivfpq", "d": self._d, "nlist": self._nlist, "M": self._M, "nbits": 8, "by_residual": self._by_residual,
                "ntotal": n, "metric": _lib.METRIC_IP, "niter": self._niter, "pq_niter": self._pq_niter, "nprobe": int(self.nprobe)}
        with open(os.path.join(path, "meta.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def load(cls, path: str, device: int | None = None, chunk_rows: int = 1 << 20) -> "IvfPqIndex":
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("format") != _FORMAT_VERSION or meta.get("kind") != "ivfpq":
            raise ValueError("not a saved IvfPqIndex")
        n, d, nlist, M = meta["ntotal"], meta["d"], meta["nlist"], meta["M"]
        ix = cls(d, nlist, M, nbits=meta.get("nbits", 8), by_residual=meta.get("by_residual", True), device=device)
        ix.niter = meta.get("niter", 10)
        ix.pq_niter = meta.get("pq_niter", 10)
        ix.nprobe = meta.get("nprobe", 1)
        ix.set_centroids(np.fromfile(os.path.join(path, "centroids.f32"), dtype="<f4").reshape(nlist, d))
        ix.set_codebook(np.fromfile(os.path.join(path, "codebook.f32"), dtype="<f4").reshape(M, _KSUB, d // M))
        if n > 0:
            mm = np.memmap(os.path.join(path, "codes.u8"), dtype=np.uint8, mode="r", shape=(n, M))
            ma = np.memmap(os.path.join(path, "assign.i32"), dtype="<i4", mode="r", shape=(n,))
            for r0 in range(0, n, chunk_rows):
                ix.add_codes(np.asarray(mm[r0:min(n, r0 + chunk_rows)]), np.asarray(ma[r0:min(n, r0 + chunk_rows)]))
            del mm, ma
        ix.meta = meta
        return ix
