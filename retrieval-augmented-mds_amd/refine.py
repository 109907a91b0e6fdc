"""RefinedIndex -- a PQ index in front of an exact store (faiss IndexRefine / IndexRefineFlat, IndexIVFPQR; include/mips_hip_refine.h,
DESIGN.md 4n).  A search asks the base index (PqIndex or IvfPqIndex) for min(k * k_factor, MAX_K_WIDE) candidates by its quantised
score and the store (a MipsIndex that holds the same rows in the same order) for the best k of them by its exact score.

All arithmetic happens in libmips_hip.so; this file calls base.search_candidates and store.rerank.  No CPU fallback.
"""
from __future__ import annotations

import json
import os

from . import _lib
from .index import _FORMAT_VERSION, MipsIndex
from .ivfpq import IvfPqIndex
from .pq import PqIndex


class RefinedIndex:
    def __init__(self, base, store, k_factor: int = 4):
        if not isinstance(base, (PqIndex, IvfPqIndex)):
            raise TypeError("RefinedIndex: base must be a PqIndex or an IvfPqIndex")
        if not isinstance(store, MipsIndex):
            raise TypeError("RefinedIndex: store must be a MipsIndex")
        if base.d != store.d:
            raise ValueError(f"RefinedIndex: base.d = {base.d} but store.d = {store.d}")
        if store.metric_type != _lib.METRIC_IP:
            raise NotImplementedError("RefinedIndex: an inner-product store only (PQ codes rank by inner product)")
        if int(k_factor) < 1:
            raise ValueError("RefinedIndex: k_factor must be >= 1")
        self.base, self.store, self.k_factor = base, store, int(k_factor)

    d = property(lambda self: self.base.d)

    @property
    def ntotal(self) -> int:
        n = self.base.ntotal
        if self.store.ntotal != n:
            raise RuntimeError(f"RefinedIndex: base holds {n} rows but store holds {self.store.ntotal}")
        return n

    @property
    def is_trained(self) -> bool:
        return self.base.is_trained and self.store.is_trained

    def __len__(self) -> int:
        return self.ntotal

    def train(self, x) -> None:
        """base.train(x); an 'sq8' store learns its ranges from x too."""
        self.base.train(x)
        if self.store.dtype == "sq8":
            self.store.train(x)

    def add(self, x) -> None:
        """The rows go to both parts, which must hold the same number of rows before and after."""
        self.ntotal  # noqa: B018 -- raises when the parts disagree
        self.base.add(x)
        self.store.add(x)
        self.ntotal  # noqa: B018

    def reset(self) -> None:
        self.base.reset()
        self.store.reset()

    def search(self, x, k: int, k_factor: int | None = None, nprobe: int | None = None, idx_offset: int = 0):
        """(D, I) [nq, k]: store.rerank of base.search_candidates(x, min(k * k_factor, MAX_K_WIDE)) -- D the store's exact scores, by (D
        descending, row ascending), -1 / -inf padding.  nprobe goes to an IvfPqIndex base.  CUDA tensors in give CUDA tensors out
        without a synchronisation."""
        k = int(k)
        kf = self.k_factor if k_factor is None else int(k_factor)
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"RefinedIndex.search: k = {k} exceeds MAX_K_WIDE = {_lib.MAX_K_WIDE}")
        if k < 1 or kf < 1:
            raise ValueError(f"RefinedIndex.search: k and k_factor must be >= 1, got {k}, {kf}")
        self.ntotal  # noqa: B018
        kc = min(k * kf, _lib.MAX_K_WIDE)
        if isinstance(self.base, IvfPqIndex):
            _, cand = self.base.search_candidates(x, kc, nprobe=nprobe, idx_offset=idx_offset)
        else:
            if nprobe is not None:
                raise ValueError("RefinedIndex.search: nprobe goes with an IvfPqIndex base")
            _, cand = self.base.search_candidates(x, kc, idx_offset=idx_offset)
        return self.store.rerank(x, cand, k, idx_offset=idx_offset)

    # ------------------------------------------------------------------ persistence: meta.json, base/ and store/ in the parts' own formats
    def save(self, path: str) -> None:
        self.ntotal  # noqa: B018
        os.makedirs(path, exist_ok=True)
        self.base.save(os.path.join(path, "base"))
        self.store.save(os.path.join(path, "store"))
        meta = {"format": _FORMAT_VERSION, "kind": "refined", "base": "ivfpq" if isinstance(self.base, IvfPqIndex) else "pq", "k_factor": self.k_factor}
        with open(os.path.join(path, "meta.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def load(cls, path: str, device: int | None = None) -> "RefinedIndex":
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("format") != _FORMAT_VERSION or meta.get("kind") != "refined":
            raise ValueError("not a saved RefinedIndex")
        base_cls = IvfPqIndex if meta.get("base") == "ivfpq" else PqIndex
        base = base_cls.load(os.path.join(path, "base"), device=device)
        store = MipsIndex.load(os.path.join(path, "store"), device=device)
        return cls(base, store, k_factor=meta.get("k_factor", 4))
