"""The slice of the `faiss` module surface that sotasum's retrieval path touches, answered by the MI355X backend.

The reference never calls its search code directly: it goes through HF `datasets`, which imports `faiss` by name
(sotasum/mips.py:1, 306, 316, 333-345, 383-386, 524, 536, 547; retriever_lightning.py:395-404, 317-321):

    faiss.METRIC_INNER_PRODUCT / faiss.METRIC_L2                      mips.py:306, 316, 369, 371
    faiss.normalize_L2(x)                                             mips.py:524
    Dataset.add_faiss_index(column=..., string_factory="Flat", metric_type=..., train_size=..., faiss_verbose=...)
        -> faiss.index_factory(d, "Flat", metric) / faiss.IndexFlat(d, metric), index.train, index.add   (HF search.py)
    Dataset.get_index(name).faiss_index.search(q, k) / .nprobe        mips.py:343-345, 383-386
    Dataset.get_nearest_examples_batch(name, q, k)                    retriever_lightning.py:317-321
    Dataset.save_faiss_index / load_faiss_index -> faiss.write_index / read_index through Python callbacks   mips.py:536, 547

`install()` registers this module as `faiss` (only if no real faiss is importable) and tells an already imported
`datasets.search` that faiss exists, after which the reference's call text runs UNCHANGED on a real `datasets.Dataset` and
lands in `MipsIndex` (fp32-exact storage by default: `DEFAULT_DTYPE`).  HF's own hook works as well without any of this:
`Dataset.add_faiss_index(column=..., custom_index=MipsIndex(d, metric))` -- it only needs `faiss` importable for its check.

Exact indexes only -- "Flat", and "SQ8" storage (IndexScalarQuantizer, QT_8bit): every other factory string raises
NotImplementedError, like Mips.build_index.

L2: the reference only ever puts phi-AUGMENTED vectors into an L2 index (augment_xb, mips.py:59-65, 316-331): rows of constant
norm sqrt(phi) whose last column is sqrt(phi - |x|^2), queries with a zero last column.  `IndexFlat(d + 1, METRIC_L2)` checks
that, stores the un-augmented d columns and reproduces the augmented squared distances |q|^2 + phi - 2 q.x (the kernel stays
an inner-product kernel); plain L2 on rows of different norms is not this path and is refused.
"""
from __future__ import annotations

import json
import struct
import sys

import numpy as np

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1

DEFAULT_DTYPE = "f32"   # storage of the MipsIndex behind IndexFlat: "f32" (exact on fp32 data) | "bf16" | "fp8_e4m3"
DEFAULT_DEVICE = None   # GPU ordinal (None = torch's current device)

__version__ = "mips-hip-shim"


def normalize_L2(x: np.ndarray) -> None:
    """faiss.normalize_L2: in-place row normalisation of a C-contiguous float32 matrix, rows of norm 0 untouched."""
    if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 2 and x.flags.c_contiguous):
        raise TypeError("normalize_L2: a C-contiguous float32 matrix is expected (as faiss does)")
    nr = np.einsum("ij,ij->i", x, x, dtype=np.float32)
    scale = np.ones_like(nr)
    np.divide(np.float32(1.0), np.sqrt(nr), out=scale, where=nr > 0)
    x *= scale[:, None]


# ---- faiss.IDSelector*: "search only these rows".  Each class answers bitmap(ntotal) -> uint8 [(ntotal + 7) // 8] in the
# IDSelectorBitmap layout (row i is selected iff bitmap[i >> 3] >> (i & 7) & 1), bits at and past ntotal clear; ids the index does
# not hold select nothing, as in faiss.
class IDSelector:
    def mask(self, ntotal: int) -> np.ndarray:   # bool [ntotal]
        raise NotImplementedError

    def bitmap(self, ntotal: int) -> np.ndarray:
        return np.packbits(self.mask(int(ntotal)), bitorder="little")

    def is_member(self, i: int) -> bool:
        return bool(self.mask(int(i) + 1)[int(i)]) if i >= 0 else False


class IDSelectorRange(IDSelector):
    """Rows imin <= i < imax."""

    def __init__(self, imin: int, imax: int, assume_sorted: bool = False):
        self.imin, self.imax = int(imin), int(imax)

    def mask(self, ntotal: int) -> np.ndarray:
        r = np.arange(ntotal)
        return (r >= self.imin) & (r < self.imax)


class IDSelectorBatch(IDSelector):
    """The listed rows (faiss: a hash set; IDSelectorArray: the plain list -- the same selection)."""

    def __init__(self, ids, *more):
        if more:   # the SWIG spelling IDSelectorBatch(n, ids)
            ids = np.asarray(more[0]).reshape(-1)[: int(ids)]
        self.ids = np.asarray(ids, dtype=np.int64).reshape(-1)

    def mask(self, ntotal: int) -> np.ndarray:
        m = np.zeros(ntotal, dtype=np.bool_)
        m[self.ids[(self.ids >= 0) & (self.ids < ntotal)]] = True
        return m


IDSelectorArray = IDSelectorBatch


class IDSelectorBitmap(IDSelector):
    """A ready bitmap (uint8, bit i of the array = row i); rows past its end are not selected."""

    def __init__(self, bitmap, *more):
        if more:   # the SWIG spelling IDSelectorBitmap(n, bitmap)
            bitmap = np.asarray(more[0], dtype=np.uint8).reshape(-1)[: int(bitmap)]
        self.bits = np.ascontiguousarray(np.asarray(bitmap, dtype=np.uint8).reshape(-1))

    def mask(self, ntotal: int) -> np.ndarray:
        m = np.zeros(ntotal, dtype=np.bool_)
        have = np.unpackbits(self.bits, bitorder="little")[:ntotal]
        m[: have.shape[0]] = have != 0
        return m


class IDSelectorNot(IDSelector):
    def __init__(self, sel: IDSelector):
        self.sel = sel

    def mask(self, ntotal: int) -> np.ndarray:
        return ~self.sel.mask(ntotal)


class IDSelectorAll(IDSelector):
    def mask(self, ntotal: int) -> np.ndarray:
        return np.ones(ntotal, dtype=np.bool_)


class SearchParameters:
    """faiss.SearchParameters(sel=...): the one field a flat index has."""

    def __init__(self, sel=None):
        self.sel = sel


def _selector_of(params, ntotal: int):
    """params (None | SearchParameters) -> what MipsIndex takes as selector=: the host bitmap of a shim selector; a
    ram.Selector or a bool mask placed in params.sel passes through."""
    sel = None if params is None else getattr(params, "sel", None)
    if sel is None:
        return None
    return sel.bitmap(ntotal) if isinstance(sel, IDSelector) else sel


def removal_mask(sel, ntotal: int) -> np.ndarray:
    """What IndexFlat.remove_ids takes (an IDSelector, or ids as faiss's IDSelectorBatch reads them) -> bool [ntotal], True = the
    row leaves.  Ids the index does not hold remove nothing, as in faiss."""
    if not isinstance(sel, IDSelector):
        sel = IDSelectorBatch(sel)
    return np.ascontiguousarray(sel.mask(int(ntotal)), dtype=np.bool_)


def _no_other_keywords(what: str, kwargs: dict) -> None:
    if kwargs:
        raise TypeError(f"{what}() got an unexpected keyword argument {sorted(kwargs)[0]!r} (params= is the one it takes)")


class IndexFlat:
    """faiss.IndexFlat(d, metric): d, ntotal, metric_type, is_trained, verbose, nprobe, add / train / search / range_search /
    reset / remove_ids / reconstruct / reconstruct_n / reconstruct_batch / search_and_reconstruct / compute_distance_subset."""

    is_trained = True

    def __init__(self, d: int, metric: int = METRIC_L2, dtype: str = None, device: int = None):
        if metric not in (METRIC_INNER_PRODUCT, METRIC_L2):
            raise NotImplementedError(f"metric {metric!r}: inner product (0) and L2 (1) only")
        self.d = int(d)
        self.metric_type = int(metric)
        self.verbose = False
        self.nprobe = 1
        self._dtype = dtype or DEFAULT_DTYPE
        self._device = DEFAULT_DEVICE if device is None else device
        self._inner = None

    # the MipsIndex behind it: d columns for inner product, d - 1 (augmentation column stripped) for L2
    def _index(self):
        if self._inner is None:
            from .index import MipsIndex

            dd = self.d - 1 if self.metric_type == METRIC_L2 else self.d
            if dd < 1:
                raise ValueError("IndexFlat(METRIC_L2) needs d >= 2 (phi-augmented vectors)")
            self._inner = MipsIndex(dd, metric=self.metric_type, dtype=self._dtype, device=self._device)
        return self._inner

    @property
    def ntotal(self) -> int:
        return 0 if self._inner is None else self._inner.ntotal

    @property
    def mips_index(self):
        """The backend object (MipsIndex): device-tensor searches, margin_stats(), set_param(), ..."""
        return self._index()

    def train(self, x=None) -> None:   # exact index: nothing to train (HF calls it when train_size is given)
        return None

    def reset(self) -> None:
        if self._inner is not None:
            self._inner.reset()

    def remove_ids(self, sel) -> int:
        """faiss Index.remove_ids(sel) -> the number of rows removed: any IDSelector of this module, or an int64 array of ids
        (faiss wraps it into an IDSelectorBatch).  The surviving rows keep their order and are renumbered, as in
        faiss.IndexFlat.  L2: phi follows the stored rows, so the index equals one built from the surviving rows."""
        if self._inner is None or self._inner.ntotal == 0:
            return 0
        return self._inner.remove_ids(np.packbits(removal_mask(sel, self._inner.ntotal), bitorder="little"))

    def _stored_form(self, x, what: str):
        """float32 rows [n, d] as the backend stores them: L2 rows are checked to be phi-augmented and lose that column."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"{what}: expected [n, {self.d}], got {x.shape}")
        if self.metric_type == METRIC_L2:
            sq = np.square(x.astype(np.float64)).sum(axis=1)
            phi = getattr(self, "_phi_seen", None)
            ref = float(sq.max()) if phi is None else phi
            if not (len(sq) > 0 and np.all(np.abs(sq - ref) <= 1e-4 * max(ref, 1e-30)) and (x[:, -1] >= 0).all()):
                raise NotImplementedError(
                    f"IndexFlat(METRIC_L2).{what}: the rows are not phi-augmented (constant norm, last column sqrt(phi - |x|^2) as "
                    "augment_xb produces, sotasum/mips.py:59-65); this backend's L2 is that MIPS->L2 reduction")
            self._phi_seen = ref
            x = np.ascontiguousarray(x[:, :-1])
        return x

    def add(self, x) -> None:
        x = self._stored_form(x, "add")   # (checked before the backend is touched)
        self._index().add(x)

    def update_vectors(self, ids, x) -> int:
        """faiss IndexIVF.update_vectors(ids, x), served on every index class: row ids[p] takes the value x[p] in place (a
        repeated id: its last occurrence); row numbers and ntotal stay.  Unlike faiss, an id outside [0, ntotal) raises
        nothing and writes nothing.  L2: the rows are phi-augmented as for add(), and phi follows the stored rows, so the
        index equals one built from the final rows.  -> the number of distinct rows written."""
        ids = np.asarray(ids)
        if ids.ndim != 1:
            raise ValueError(f"update_vectors: expected ids [n], got {ids.shape}")
        if len(ids) == 0 or self._inner is None:
            return 0
        return self._inner.update_rows(ids, self._stored_form(x, "update_vectors"), return_count=True)

    def search(self, x, k: int, params=None, **kwargs):
        """(D float32 [nq, k], I int64 [nq, k]); NumPy in, NumPy out -- the call of mips.py:383-386 and of HF's search_batch.
        params=SearchParameters(sel=IDSelector...) restricts the search to the selected rows (the filtered wide search)."""
        _no_other_keywords("search", kwargs)
        ix = self._index()
        q = np.ascontiguousarray(x, dtype=np.float32)
        if self.metric_type == METRIC_L2:
            if q.ndim != 2 or q.shape[1] != self.d:
                raise ValueError(f"search: expected [nq, {self.d}], got {q.shape}")
            if np.any(q[:, -1] != 0):
                raise ValueError("L2 search: the queries' last (augmentation) column is not zero; this index answers queries "
                                 "prepared by augment_xq (sotasum/mips.py:68-70)")
            q = np.ascontiguousarray(q[:, :-1])
        from .index import route_search

        sel = _selector_of(params, ix.ntotal)
        if sel is not None:
            return route_search(ix, q, int(k), selector=sel)
        return route_search(ix, q, int(k))   # k > MAX_K: the wide search (k <= MAX_K_WIDE = 1024)

    def range_search(self, x, thresh, params=None, **kwargs):
        """faiss Index.range_search(x, thresh) -> (lims uint64 [nq + 1], D float32, I int64): inner product, every row scoring
        strictly above thresh; L2 (queries prepared by augment_xq, as in search), every row whose augmented squared distance
        |q|^2 + phi - 2 q.x is strictly below it.  The hits of query j are D / I [lims[j] : lims[j + 1]], in ascending row order
        (faiss leaves the order undefined).  NumPy in, NumPy out.  params=SearchParameters(sel=...): selected rows only."""
        _no_other_keywords("range_search", kwargs)
        ix = self._index()
        q = np.ascontiguousarray(x, dtype=np.float32)
        if self.metric_type == METRIC_L2:
            if q.ndim != 2 or q.shape[1] != self.d:
                raise ValueError(f"range_search: expected [nq, {self.d}], got {q.shape}")
            if np.any(q[:, -1] != 0):
                raise ValueError("L2 range_search: the queries' last (augmentation) column is not zero; this index answers "
                                 "queries prepared by augment_xq (sotasum/mips.py:68-70)")
            q = np.ascontiguousarray(q[:, :-1])
        sel = _selector_of(params, ix.ntotal)
        lims, D, I = ix.range_search(q, thresh) if sel is None else ix.range_search(q, thresh, selector=sel)
        return (np.asarray(lims).astype(np.uint64), np.ascontiguousarray(D, dtype=np.float32), np.ascontiguousarray(I, dtype=np.int64))

    # ---- rows by id.  L2: the index stores the un-augmented d - 1 columns; the augmentation column of a row handed back is
    # RECOMPUTED from the stored values (l2_augmentation_column), not stored -- it equals the column that was added up to the
    # storage's rounding of the other columns and float32 rounding of the square root.
    def _rows_out(self, rows: np.ndarray) -> np.ndarray:
        if self.metric_type != METRIC_L2:
            return rows
        flat = rows.reshape(-1, rows.shape[-1])
        col = l2_augmentation_column(flat, self._inner.phi() if flat.shape[0] else 0.0)
        return np.concatenate((flat, col[:, None]), axis=1).reshape(rows.shape[:-1] + (self.d,))

    def _l2_queries(self, x, what: str) -> np.ndarray:
        q = np.ascontiguousarray(x, dtype=np.float32)
        if self.metric_type == METRIC_L2:
            if q.ndim != 2 or q.shape[1] != self.d:
                raise ValueError(f"{what}: expected [nq, {self.d}], got {q.shape}")
            if np.any(q[:, -1] != 0):
                raise ValueError(f"L2 {what}: the queries' last (augmentation) column is not zero; this index answers queries "
                                 "prepared by augment_xq (sotasum/mips.py:68-70)")
            q = np.ascontiguousarray(q[:, :-1])
        return q

    def reconstruct(self, key: int) -> np.ndarray:
        """faiss Index.reconstruct(key) -> float32 [d]; IndexError outside [0, ntotal) (an empty index: always)."""
        key = int(key)
        if not 0 <= key < self.ntotal:
            raise IndexError(f"reconstruct: row {key} of an index of {self.ntotal}")
        return self._rows_out(self._inner.reconstruct(key))

    def reconstruct_n(self, n0: int = 0, ni: int = -1) -> np.ndarray:
        """faiss Index.reconstruct_n(n0, ni) -> float32 [ni, d]; ni = -1 (or None): up to the last row."""
        n0 = int(n0)
        ni = self.ntotal - n0 if ni is None or int(ni) < 0 else int(ni)
        if n0 < 0 or ni < 0 or n0 + ni > self.ntotal:
            raise IndexError(f"reconstruct_n: rows [{n0}, {n0 + ni}) of an index of {self.ntotal}")
        if ni == 0:
            return np.empty((0, self.d), dtype=np.float32)
        return self._rows_out(self._inner.reconstruct_n(n0, ni))

    def reconstruct_batch(self, ids) -> np.ndarray:
        """faiss Index.reconstruct_batch(ids) -> float32 [..., d] for int64 ids [...]; negative ids (the -1 padding of a search)
        give NaN rows, an id >= ntotal raises IndexError."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.size and int(ids.max()) >= self.ntotal:
            raise IndexError(f"reconstruct_batch: id {int(ids.max())} of an index of {self.ntotal}")
        if ids.size == 0 or self._inner is None:
            return np.full(ids.shape + (self.d,), np.nan, dtype=np.float32)
        return self._rows_out(self._inner.reconstruct_batch(ids))

    def search_and_reconstruct(self, x, k: int, params=None, **kwargs):
        """faiss Index.search_and_reconstruct(x, k) -> (D, I, R float32 [nq, k, d]): search(x, k, params) and the rows of I; the
        rows of the -1 slots are NaN."""
        _no_other_keywords("search_and_reconstruct", kwargs)
        D, I = self.search(x, k, params=params)
        return D, I, self.reconstruct_batch(I)

    def compute_distance_subset(self, x, labels) -> np.ndarray:
        """faiss Index.compute_distance_subset, spelled for NumPy (the SWIG pointer form cannot be taken): x float32 [nq, d],
        labels int64 [nq, k] -> D float32 [nq, k], the index's own score of every pair (what search returns for it); negative
        labels give -inf (L2: +inf)."""
        q = self._l2_queries(x, "compute_distance_subset")
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        if labels.ndim != 2 or labels.shape[0] != q.shape[0]:
            raise ValueError(f"compute_distance_subset: expected labels [{q.shape[0]}, k], got {labels.shape}")
        if labels.size and int(labels.max()) >= self.ntotal:
            raise IndexError(f"compute_distance_subset: id {int(labels.max())} of an index of {self.ntotal}")
        return self._index().compute_distance_subset(q, labels)


def l2_augmentation_column(rows: np.ndarray, phi: float) -> np.ndarray:
    """The last column of the phi-augmented form of `rows` (float32 [n, d - 1], as stored): float32(sqrt(max(phi - sum x^2, 0)))
    with the sum taken sequentially in fp64 over the columns (augment_xb, sotasum/mips.py:59-65).  NaN rows stay NaN."""
    x = np.asarray(rows, dtype=np.float64)
    sq = np.cumsum(x * x, axis=1)[:, -1] if x.shape[1] else np.zeros(x.shape[0])
    return np.sqrt(np.maximum(float(phi) - sq, 0.0)).astype(np.float32)


class IndexFlatIP(IndexFlat):
    def __init__(self, d: int):
        super().__init__(d, METRIC_INNER_PRODUCT)


class IndexFlatL2(IndexFlat):
    def __init__(self, d: int):
        super().__init__(d, METRIC_L2)


class ScalarQuantizer:
    """faiss.ScalarQuantizer: the one quantiser type this backend stores."""
    QT_8bit = 0


class IndexScalarQuantizer(IndexFlat):
    """faiss.IndexScalarQuantizer(d, ScalarQuantizer.QT_8bit, metric): one byte per element, 256 uniform levels over each
    column's trained range (MipsIndex dtype "sq8").  train(x) before add(x); inner product only."""

    def __init__(self, d: int, qtype: int = ScalarQuantizer.QT_8bit, metric: int = METRIC_L2, device: int = None):
        if qtype != ScalarQuantizer.QT_8bit:
            raise NotImplementedError(f"IndexScalarQuantizer: quantiser type {qtype!r}: QT_8bit only")
        if metric != METRIC_INNER_PRODUCT:
            raise NotImplementedError("IndexScalarQuantizer: inner product only -- this backend's L2 is the MIPS->L2 reduction over rows "
                                      "of constant norm, which decoded SQ8 rows are not")
        super().__init__(d, metric, dtype="sq8", device=device)

    @property
    def is_trained(self) -> bool:
        return self._index().is_trained

    def train(self, x=None) -> None:
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"train: expected [n, {self.d}], got {x.shape}")
        self._index().train(x)


Index = IndexFlat   # (type annotations in HF spell `faiss.Index`)


def index_factory(d: int, description: str, metric: int = METRIC_L2) -> IndexFlat:
    """faiss.index_factory: "Flat" (what the reference ships with, mips_string_factory) and "SQ8" (the storage half of its
    "IVF256,SQ8" configuration).  The index is exact: IVF, HNSW and PQ -- alone or in front of a storage -- are refused."""
    if description == "Flat":
        return IndexFlat(d, metric)
    if description == "SQ8":
        return IndexScalarQuantizer(d, ScalarQuantizer.QT_8bit, metric)
    raise NotImplementedError(f"index_factory({description!r}): the exact 'Flat' index and 'SQ8' storage are implemented "
                              "(no IVF, HNSW or PQ: every search is exact)")


# ---- write_index / read_index as HF drives them: faiss.write_index(index, faiss.BufferedIOWriter(faiss.PyCallbackIOWriter(f.write)))
class PyCallbackIOWriter:
    def __init__(self, write, bs: int = 1 << 20):
        self.write = write


class PyCallbackIOReader:
    def __init__(self, read, bs: int = 1 << 20):
        self.read = read


class BufferedIOWriter:
    def __init__(self, writer, bsz: int = 1 << 20):
        self.write = writer.write


class BufferedIOReader:
    def __init__(self, reader, bsz: int = 1 << 20):
        self.read = reader.read


_MAGIC = b"MIPSHIP1"


def write_index(index: IndexFlat, writer) -> None:
    """Own byte format (the on-disk format is free): magic, JSON header, raw rows in the storage dtype."""
    if isinstance(writer, str):
        with open(writer, "wb") as f:
            return write_index(index, PyCallbackIOWriter(f.write))
    inner = index._index()
    head = {"d": index.d, "metric": index.metric_type, "dtype": inner.dtype, "ntotal": inner.ntotal, "inner_d": inner.d,
            "phi_seen": getattr(index, "_phi_seen", None)}
    if inner.dtype == "sq8" and inner.is_trained:   # float32 parameters as exact hexadecimal strings
        head["sq8_vmin"], head["sq8_vdiff"] = ([float(v).hex() for v in a] for a in inner.sq8_params())
    hb = json.dumps(head).encode()
    writer.write(_MAGIC + struct.pack("<q", len(hb)) + hb)
    for r0 in range(0, inner.ntotal, 1 << 16):
        writer.write(inner.rows_raw(r0, min(1 << 16, inner.ntotal - r0)).tobytes())


def _read_exact(reader, n: int) -> bytes:
    out = bytearray()
    while len(out) < n:
        b = reader.read(n - len(out))
        if not b:
            raise EOFError("read_index: truncated index file")
        out += b
    return bytes(out)


def read_index(reader) -> IndexFlat:
    if isinstance(reader, str):
        with open(reader, "rb") as f:
            return read_index(PyCallbackIOReader(f.read))
    if _read_exact(reader, 8) != _MAGIC:
        raise ValueError("read_index: not an index written by this backend's write_index")
    (hl,) = struct.unpack("<q", _read_exact(reader, 8))
    head = json.loads(_read_exact(reader, hl))
    if head["dtype"] == "sq8":
        index = IndexScalarQuantizer(head["d"], ScalarQuantizer.QT_8bit, head["metric"])
    else:
        index = IndexFlat(head["d"], head["metric"], dtype=head["dtype"])
    if head.get("phi_seen") is not None:
        index._phi_seen = head["phi_seen"]
    inner = index._index()
    if head.get("sq8_vmin") is not None:
        inner.set_sq8_params([float.fromhex(v) for v in head["sq8_vmin"]], [float.fromhex(v) for v in head["sq8_vdiff"]])
    npdt = {"bf16": np.uint16, "fp8_e4m3": np.uint8, "fp8_e4m3_docs": np.uint8, "f32": np.float32, "sq8": np.uint8}[head["dtype"]]
    row_bytes = head["inner_d"] * np.dtype(npdt).itemsize
    inner.reserve(head["ntotal"])
    for r0 in range(0, head["ntotal"], 1 << 16):
        n = min(1 << 16, head["ntotal"] - r0)
        inner.add(np.frombuffer(_read_exact(reader, n * row_bytes), dtype=npdt).reshape(n, head["inner_d"]))
    return index


def index_gpu_to_cpu(index):   # (HF calls it when a device was given: the index lives on the GPU either way)
    return index


def index_cpu_to_gpu(resources, device, index):
    return index


def index_cpu_to_all_gpus(index):
    return index


class StandardGpuResources:
    pass


def install(force: bool = False):
    """Make `import faiss` resolve to this module (unless a real faiss is importable and force is False) and let an already
    imported HF `datasets.search` know.  Returns the module."""
    import importlib.util

    me = sys.modules[__name__]
    real = None
    if "faiss" in sys.modules and sys.modules["faiss"] is not me:
        real = sys.modules["faiss"]
    elif "faiss" not in sys.modules:
        try:
            real = importlib.util.find_spec("faiss")
        except (ImportError, ValueError):
            real = None
    if real is not None and not force:
        raise RuntimeError("a real `faiss` is importable: pass force=True to shadow it with the MI355X backend")
    sys.modules["faiss"] = me
    search = sys.modules.get("datasets.search")
    if search is not None:
        search._has_faiss = True
    return me
