"""PqIndex -- a product-quantised index (faiss IndexPQ; include/mips_hip_pq.h): M one-byte codes per row, trained
sub-quantisers of 256 centroids, asymmetric-distance search through a per-query lookup table.

Reached by name only: the factory strings ("PQ16", "IVF4096,PQ32"), Mips, KnowledgeBase and faiss_shim do not route here.  Inner
product only, 8 bits per code, M <= 128, d <= 1024, search k <= MAX_K (search_candidates: k <= MAX_K_WIDE); no range
search, selectors, groups, remove_ids, update_rows, sharding or OPQ; lists over the codes are IvfPqIndex (ivfpq.py).  Large query batches are served but are not what the index is for: the scan costs
nq * ntotal * M table reads and shares nothing between queries.

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

_KSUB = 256


class PqIndex:
    def __init__(self, d: int, M: int, nbits: int = 8, metric: int = _lib.METRIC_IP, device: int | None = None):
        d, M = int(d), int(M)
        if int(metric) != _lib.METRIC_IP:
            raise NotImplementedError("a PqIndex ranks by inner product only (the lookup table holds inner products)")
        if int(nbits) != 8:
            raise NotImplementedError(f"PqIndex: {nbits} bits per code are not served (8: 256 centroids per sub-quantiser)")
        if d > 1024:
            raise NotImplementedError("PqIndex: rows of more than 1024 columns are not served")
        if M > 128:
            raise NotImplementedError(f"PqIndex: M = {M} exceeds 128 (the query's table is M KiB of LDS)")
        if M < 1 or d < 1 or d % M != 0:
            raise ValueError(f"PqIndex: d = {d} must be a positive multiple of M = {M} >= 1")
        self._lib = _lib.load()
        self.device = _lib.require_gpu(device)
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.mips_pq_create(ctypes.byref(self._h), self.device, d, M, int(nbits), int(metric)), "mips_pq_create")
        self._d, self._M = d, M
        self._niter = 10
        self._query_slice = 256
        self._mutex = threading.RLock()

    # ------------------------------------------------------------------ faiss-like attributes
    @property
    def d(self) -> int:
        return self._d

    @property
    def M(self) -> int:
        return self._M

    @property
    def dsub(self) -> int:
        return self._d // self._M

    @property
    def nbits(self) -> int:
        return 8

    @property
    def ntotal(self) -> int:
        return int(self._lib.mips_pq_ntotal(self._h))

    @property
    def metric_type(self) -> int:
        return _lib.METRIC_IP

    @property
    def is_trained(self) -> bool:
        return self._lib.mips_pq_is_trained(self._h) == 1

    @property
    def bytes_per_row(self) -> int:
        """bytes of one row's codes (M); the codebook's 1024 * d bytes are shared by all rows"""
        return self._M

    @property
    def niter(self) -> int:
        return self._niter

    @niter.setter
    def niter(self, v: int) -> None:
        _lib.check(self._lib.mips_pq_set_param(self._h, b"pq_niter", int(v)), "mips_pq_set_param")
        self._niter = int(v)

    @property
    def query_slice(self) -> int:
        return self._query_slice

    @query_slice.setter
    def query_slice(self, v: int) -> None:
        _lib.check(self._lib.mips_pq_set_param(self._h, b"pq_query_slice", int(v)), "mips_pq_set_param")
        self._query_slice = int(v)

    def __len__(self) -> int:
        return self.ntotal

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.mips_pq_destroy(h)
            except Exception:
                pass
            h.value = None

    def _rows(self, x, what: str):
        """float32 / bfloat16 rows or queries, host or device -> (pointer, dtype code, is_device, n, keepalive)"""
        import torch

        if isinstance(x, torch.Tensor):
            if x.dim() != 2 or x.shape[1] != self._d:
                raise ValueError(f"{what}: expected [n, {self._d}], got {tuple(x.shape)}")
            if not x.dtype.is_floating_point:
                raise NotImplementedError(f"{what}: float32 or bfloat16 values (codes go through add_codes)")
            if x.dtype not in (torch.float32, torch.bfloat16):
                x = x.float()
            code = _lib.DTYPE_F32 if x.dtype == torch.float32 else _lib.DTYPE_BF16
            x = x.contiguous()
            if x.is_cuda and x.device.index != self.device:
                x = x.to(f"cuda:{self.device}")
            return x.data_ptr(), code, 1 if x.is_cuda else 0, x.shape[0], x
        a = np.asarray(x)
        if a.ndim != 2 or a.shape[1] != self._d:
            raise ValueError(f"{what}: expected [n, {self._d}], got {a.shape}")
        if a.dtype == np.uint16:  # raw bf16 bit patterns
            a = np.ascontiguousarray(a)
            return a.ctypes.data, _lib.DTYPE_BF16, 0, a.shape[0], a
        if a.dtype.kind in "iub":
            raise NotImplementedError(f"{what}: float32 values or bf16 bit patterns (codes go through add_codes)")
        a = np.ascontiguousarray(a, dtype=np.float32)
        return a.ctypes.data, _lib.DTYPE_F32, 0, a.shape[0], a

    # ------------------------------------------------------------------ building
    def train(self, x) -> None:
        """Deterministic k-means per sub-quantiser (include/mips_hip_pq.h): niter iterations from evenly spaced initial rows, on at
        most 65536 evenly spaced rows of x.  Raises on n < 256, on a NaN or an infinity and on an index that holds rows."""
        ptr, code, is_dev, n, keep = self._rows(x, "train")
        with self._mutex:
            _lib.check(self._lib.mips_pq_train(self._h, ptr, n, code, _lib.Q_DEVICE if is_dev else 0, _stream_handle(self.device)), "mips_pq_train")
        del keep

    def codebook(self) -> np.ndarray:
        """float32 [M, 256, dsub]"""
        out = np.empty((self._M, _KSUB, self.dsub), np.float32)
        with self._mutex:
            _lib.check(self._lib.mips_pq_get_codebook(self._h, out.ctypes.data), "mips_pq_get_codebook")
        return out

    def set_codebook(self, c) -> None:
        """Plant the codebook [M, 256, dsub] (stored as given) of an EMPTY index; the index is trained afterwards."""
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
        if c.shape != (self._M, _KSUB, self.dsub):
            raise ValueError(f"set_codebook: expected [{self._M}, {_KSUB}, {self.dsub}], got {c.shape}")
        with self._mutex:
            _lib.check(self._lib.mips_pq_set_codebook(self._h, c.ctypes.data), "mips_pq_set_codebook")

    def add(self, x) -> None:
        """Encode and append float32 / bfloat16 rows (NumPy, or a torch tensor on the host or the device)."""
        if not self.is_trained:
            raise RuntimeError("add: the PqIndex is not trained (train(x) first, as faiss requires)")
        ptr, code, is_dev, n, keep = self._rows(x, "add")
        with self._mutex:
            _lib.check(self._lib.mips_pq_add(self._h, ptr, n, code, is_dev, _stream_handle(self.device)), "mips_pq_add")
        del keep

    def add_codes(self, codes) -> None:
        """Append rows given as their codes, uint8 [n, M] (NumPy or a torch tensor), stored as they are."""
        import torch

        if not self.is_trained:
            raise RuntimeError("add_codes: the PqIndex is not trained (train(x) or set_codebook first)")
        if isinstance(codes, torch.Tensor):
            if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != self._M:
                raise ValueError(f"add_codes: expected uint8 [n, {self._M}], got {codes.dtype} {tuple(codes.shape)}")
            codes = codes.contiguous()
            if codes.is_cuda and codes.device.index != self.device:
                codes = codes.to(f"cuda:{self.device}")
            ptr, n, is_dev = codes.data_ptr(), codes.shape[0], 1 if codes.is_cuda else 0
        else:
            codes = np.asarray(codes)
            if codes.dtype != np.uint8 or codes.ndim != 2 or codes.shape[1] != self._M:
                raise ValueError(f"add_codes: expected uint8 [n, {self._M}], got {codes.dtype} {codes.shape}")
            codes = np.ascontiguousarray(codes)
            ptr, n, is_dev = codes.ctypes.data, codes.shape[0], 0
        with self._mutex:
            _lib.check(self._lib.mips_pq_add_codes(self._h, ptr, n, is_dev, _stream_handle(self.device)), "mips_pq_add_codes")

    def codes(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """uint8 [n, M]: the codes of rows [row0, row0 + n)"""
        row0 = int(row0)
        n = self.ntotal - row0 if n is None else int(n)
        out = np.empty((max(n, 0), self._M), np.uint8)
        with self._mutex:
            _lib.check(self._lib.mips_pq_read_codes(self._h, row0, n, out.ctypes.data, _stream_handle(self.device)), "mips_pq_read_codes")
        return out

    def reset(self) -> None:
        """Drop all rows; the codebook stays."""
        with self._mutex:
            _lib.check(self._lib.mips_pq_reset(self._h), "mips_pq_reset")

    # ------------------------------------------------------------------ searching
    def search(self, x, k: int, idx_offset: int = 0):
        """(D, I) [nq, k]: the best k rows by (D descending, row ascending), D the float32 sum in ascending m of the query's table
        entries at the row's codes; -1 / -inf padding.  NumPy in gives NumPy out; a CUDA tensor in gives CUDA tensors out,
        stream-ordered, never synchronising (graph-capturable in steady state)."""
        k = int(k)
        if k > _lib.MAX_K:
            raise NotImplementedError(f"PqIndex.search: k = {k} exceeds MAX_K = {_lib.MAX_K} (search_candidates serves k <= MAX_K_WIDE on PQ codes)")
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
            _lib.check(self._lib.mips_pq_search(self._h, ptr, code, nq, k, dp, ip, int(idx_offset), flags, _stream_handle(self.device)), "mips_pq_search")
        del keep
        return D, I

    def search_candidates(self, x, k: int, idx_offset: int = 0):
        """(D, I) [nq, k] for 1 <= k <= MAX_K_WIDE: the definition of search, unchanged -- every row scored, the best k by (D
        descending, row ascending), -1 / -inf padding; the first k' columns are the result for k'.  k <= MAX_K issues search's own
        launches.  The candidate generator in front of MipsIndex.rerank (RefinedIndex).  NumPy in gives NumPy out; a
        CUDA tensor in gives CUDA tensors out, stream-ordered, never synchronising (graph-capturable in steady state)."""
        k = int(k)
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"PqIndex.search_candidates: k = {k} exceeds MAX_K_WIDE = {_lib.MAX_K_WIDE}")
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
            _lib.check(self._lib.mips_pq_search_candidates(self._h, ptr, code, nq, k, dp, ip, int(idx_offset), flags, _stream_handle(self.device)),
                       "mips_pq_search_candidates")
        del keep
        return D, I

    def _ids_arg(self, ids, what: str):
        """ids of any shape (NumPy / sequence -> host, CUDA tensor -> device) -> (pointer, shape, is_device, keepalive)"""
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
        a = np.ascontiguousarray(a, dtype=np.int64)
        return a.ctypes.data, a.shape, False, a

    def reconstruct_batch(self, ids, idx_offset: int = 0, out=None):
        """The decoded rows ids[...] - idx_offset -> float32 [..., d]: the concatenation of the centroids the codes name.  NumPy ids
        give a NumPy result and an id >= ntotal raises; a CUDA tensor gives a CUDA tensor, stream-ordered, and an id that names no
        row (the -1 padding of a search, or past the index) gives a NaN row.  out= (CUDA ids only): a contiguous CUDA float32
        tensor [..., d]."""
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
            _lib.check(self._lib.mips_pq_reconstruct(self._h, ptr, n, int(idx_offset), op, _lib.DTYPE_F32, self._d, flags, _stream_handle(self.device)),
                       "mips_pq_reconstruct")
        del keep
        return out

    def reconstruct(self, key: int) -> np.ndarray:
        key = int(key)
        if not 0 <= key < self.ntotal:
            raise IndexError(f"reconstruct: row {key} of {self.ntotal}")
        return self.reconstruct_batch(np.array([key], np.int64))[0]

    def reconstruct_n(self, n0: int = 0, ni: int | None = None) -> np.ndarray:
        n0 = int(n0)
        ni = self.ntotal - n0 if ni is None else int(ni)
        if n0 < 0 or ni < 0 or n0 + ni > self.ntotal:
            raise IndexError(f"reconstruct_n: rows [{n0}, {n0 + ni}) of {self.ntotal}")
        return self.reconstruct_batch(np.arange(n0, n0 + ni, dtype=np.int64))

    def compute_distance_subset(self, x, ids, idx_offset: int = 0):
        """D(q_j, ids[j, t] - idx_offset) -> float32 [nq, k], nothing ranked: scoring the I of a search reproduces its D bit for bit.
        An id that names no row scores -inf.  NumPy in gives NumPy out; CUDA queries and CUDA ids give a CUDA tensor, stream-ordered."""
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
            _lib.check(self._lib.mips_pq_score_subset(self._h, ptr, code, nq, iptr, k, op, int(idx_offset), flags, _stream_handle(self.device)),
                       "mips_pq_score_subset")
        del keep, keep_ids
        return out

    def _refused(self, *a, **kw):
        raise NotImplementedError("PqIndex serves search(x, k <= MAX_K), search_candidates(x, k <= MAX_K_WIDE), reconstruct* and compute_distance_subset; "
                                  "search_wide, range search, selectors, "
                                  "groups, remove_ids, update_rows and sharding are not served on PQ codes (DESIGN.md 4l)")

    search_wide = range_search = search_packed = search_fused = remove_ids = update_rows = _refused

    # ------------------------------------------------------------------ persistence
    #   meta.json + codes.u8 (uint8 [ntotal, M]) + codebook.f32 (raw little-endian float32 [M, 256, dsub])
    def save(self, path: str, chunk_rows: int = 1 << 20) -> None:
        if not self.is_trained:
            raise RuntimeError("save: the PqIndex is not trained")
        os.makedirs(path, exist_ok=True)
        n = self.ntotal
        with open(os.path.join(path, "codebook.f32"), "wb") as f:
            f.write(self.codebook().astype("<f4").tobytes())
        with open(os.path.join(path, "codes.u8"), "wb") as f:
            for r0 in range(0, n, chunk_rows):
                f.write(self.codes(r0, min(chunk_rows, n - r0)).tobytes())
        meta = {"format": _FORMAT_VERSION, "kind": "pq", "d": self._d, "M": self._M, "nbits": 8, "ntotal": n, "metric": _lib.METRIC_IP,
                "niter": self._niter}
        with open(os.path.join(path, "meta.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def load(cls, path: str, device: int | None = None, chunk_rows: int = 1 << 20) -> "PqIndex":
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("format") != _FORMAT_VERSION or meta.get("kind") != "pq":
            raise ValueError("not a saved PqIndex")
        n, d, M = meta["ntotal"], meta["d"], meta["M"]
        ix = cls(d, M, nbits=meta.get("nbits", 8), device=device)
        ix.niter = meta.get("niter", 10)
        ix.set_codebook(np.fromfile(os.path.join(path, "codebook.f32"), dtype="<f4").reshape(M, _KSUB, d // M))
        if n > 0:
            mm = np.memmap(os.path.join(path, "codes.u8"), dtype=np.uint8, mode="r", shape=(n, M))
            for r0 in range(0, n, chunk_rows):
                ix.add_codes(np.asarray(mm[r0:min(n, r0 + chunk_rows)]))
            del mm
        ix.meta = meta
        return ix
