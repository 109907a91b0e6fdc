"""ShardedIvfIndex -- one logical IvfIndex whose rows are split contiguously over the ranks of a torch.distributed group
(include/mips_hip_ivf_sharded.h).

Every rank holds the same centroids (and, for 'sq8', the same per-column range) and an IvfIndex over its own row range
shard_bounds(N, world, rank).  The list of a row depends on the float32 row and the centroids only, so the lists of a shard are the
global lists restricted to its rows; the probe depends on the query and the centroids only, so it is the same on every rank; and the
best k of a union are the best k of the shards' best k.  A search is therefore IvfIndex.search_probed_wide cut behind its merge:
every rank searches its part (IvfIndex.search_part, idx_offset = lo, a GLOBAL selector read from bit lo), ONE all-gather moves the
payloads, and a replicated merge (ivf_merge_parts) finishes -- bit for bit the result of the unsharded IvfIndex over all the rows in
global order, on every rank.  'sq8' is ranked and merged on S across the shards too and becomes D only behind the merge.  The range
search takes the record protocol of ShardedMipsIndex.range_search.

Not served: remove_ids_global, an exact `.flat` search across the shards, per-rank training on disjoint rows, the Mips /
KnowledgeBase / faiss_shim routing (mips_nlist with mips_shard stays refused) and factory strings.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from . import _lib
from .sharded import ShardedMipsIndex, pack_topk, range_record_exchange, range_record_fill, shard_bounds

_DTYPES = ("bf16", "f32", "sq8")


def training_checksum(centroids, sq8_params=None) -> int:
    """A 64-bit checksum (as a signed int64) of the bits of the centroids and, when given, of the SQ8 range (vmin, vdiff)."""
    h = hashlib.blake2b(digest_size=8)
    h.update(np.ascontiguousarray(centroids, dtype="<f4").tobytes())
    if sq8_params is not None:
        for a in sq8_params:
            h.update(np.ascontiguousarray(a, dtype="<f4").tobytes())
    return int.from_bytes(h.digest(), "little", signed=True)


class ShardedIvfIndex:
    """One logical IvfIndex, row-sharded across the ranks of a torch.distributed group.

    The local steps default to the HIP path (IvfIndex.search_part / ivf_merge_parts, IvfIndex.range_search_probed_into /
    mips_range_merge_records).  They are injectable, so that the partition + selector offset + pack + all-gather + merge plumbing
    runs with the gloo backend on machines without a GPU, where tests substitute NumPy restatements:
      local_search(q, k, nprobe, idx_offset, **kw) -> (S float32 [nq, k] RANKING scores, I int64 [nq, k] rows + idx_offset with -1
          padding, bias float64 [nq] or None), kw carrying selector + sel_bit0 and groups + group_mode when the call has them;
      merge(gathered int64 [parts, nq, k, 2], parts, nq, k, bias) -> (D, I);
      local_range_search(q, radius, nprobe, idx_offset, **kw) -> (lims, D, I);  range_merge(gathered, parts, nq, stride) -> (lims, D, I).
    local_search and merge are injected together; an index with injected steps holds no rows (set_global_size names their count).
    """

    def __init__(self, d: int, nlist: int, dtype: str = "bf16", group=None, device=None, local_search=None, merge=None,
                 local_range_search=None, range_merge=None, local_reconstruct=None, _local_index=None):
        import torch.distributed as dist

        if dtype not in _DTYPES:
            raise NotImplementedError(f"ShardedIvfIndex dtype {dtype!r}: 'bf16', 'f32' or 'sq8'")
        if (local_search is None) != (merge is None) or (local_range_search is None) != (range_merge is None):
            raise ValueError("ShardedIvfIndex: a local step and its merge are injected together")
        self.d, self.nlist, self.dtype = int(d), int(nlist), dtype
        self.group = group
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.ntotal_global = 0
        self.lo = self.hi = 0
        self.nprobe = 1
        self.local = None
        self._local_search, self._merge = local_search, merge
        self._local_range_search, self._range_merge = local_range_search, range_merge
        self._local_reconstruct = local_reconstruct
        self._trained = None  # injected steps: (centroids, sq8_params) as set_trained got them
        if _local_index is not None:  # (load: the shard's index comes from its files)
            self.local = _local_index
        elif local_search is None and local_range_search is None and local_reconstruct is None:
            from .ivf import IvfIndex

            self.local = IvfIndex(d, nlist, dtype=dtype, device=device)

    # ------------------------------------------------------------------ building
    def _need_local(self, what: str):
        if self.local is None:
            raise ValueError(f"{what} needs the library's own local index (injected steps hold no rows)")

    def _small_gather(self, values):
        """int64 values of this rank -> int64 [world, len(values)] of every rank: one small all-gather"""
        import torch
        import torch.distributed as dist

        mine = torch.tensor([int(v) for v in values], dtype=torch.int64)
        if self.world == 1:
            return mine[None, :]
        if dist.get_backend(self.group) == "nccl":
            mine = mine.to(f"cuda:{self.local.device}" if self.local is not None else "cuda")
        every = torch.empty(self.world * mine.shape[0], dtype=torch.int64, device=mine.device)
        dist.all_gather_into_tensor(every, mine, group=self.group)
        return every.cpu().view(self.world, -1)

    def check_trained_global(self) -> None:
        """COLLECTIVE: one small all-gather of a 64-bit checksum of the centroid bits (and of the SQ8 range bits of an 'sq8' index);
        raises on EVERY rank when the ranks do not hold the same ones -- shards with different centroids or ranges have lists and
        scores that do not merge."""
        if self.local is not None:
            mine = training_checksum(self.local.centroids(), self.local.flat.sq8_params() if self.dtype == "sq8" else None)
        else:
            if self._trained is None:
                raise RuntimeError("check_trained_global: the index is not trained")
            mine = training_checksum(*self._trained)
        every = self._small_gather([mine])[:, 0].tolist()
        if len(set(every)) != 1:
            raise RuntimeError(f"ShardedIvfIndex: the ranks hold different centroids or SQ8 ranges (checksums {every}); every rank must train "
                               "on the same rows or be given the same set_trained() arguments")

    def train_global(self, x) -> None:
        """Every rank passes the SAME full [n, d] array and runs IvfIndex.train(x) on it: the training is deterministic, so the ranks
        agree without communicating, and an 'sq8' index gets its range from the whole x -- the global range.  Ends with
        check_trained_global()."""
        self._need_local("train_global")
        self.local.train(x)
        self.check_trained_global()

    def set_trained(self, centroids, sq8_params=None) -> None:
        """Plant the centroids [nlist, d] (and (vmin, vdiff) of an 'sq8' index) on an empty index: for load() and for callers that
        train elsewhere.  The same on every rank; ends with check_trained_global()."""
        centroids = np.ascontiguousarray(np.asarray(centroids, dtype=np.float32))
        if centroids.shape != (self.nlist, self.d):
            raise ValueError(f"set_trained: expected centroids [{self.nlist}, {self.d}], got {centroids.shape}")
        if (self.dtype == "sq8") != (sq8_params is not None):
            raise ValueError("set_trained: sq8_params = (vmin, vdiff) goes with an 'sq8' index, and only with one")
        if self.local is not None:
            self.local.set_centroids(centroids)
            if sq8_params is not None:
                self.local.set_sq8_params(*sq8_params)
        else:
            self._trained = (centroids, sq8_params)
        self.check_trained_global()

    @property
    def is_trained(self) -> bool:
        return self.local.is_trained if self.local is not None else self._trained is not None

    def set_global_size(self, n: int):
        self.ntotal_global = int(n)
        self.lo, self.hi = shard_bounds(n, self.world, self.rank)
        return self.lo, self.hi

    def add_global(self, x) -> None:
        """Every rank sees the full [N, d] array (NumPy / memmap / torch) and keeps its own rows, shard_bounds(N, world, rank)."""
        if self.ntotal_global:
            raise ValueError("add_global: the index holds rows already; the even partition is made once (update_rows_global changes rows)")
        if not self.is_trained:
            raise RuntimeError("add_global: the index is not trained (train_global(x) or set_trained(...) first)")
        lo, hi = self.set_global_size(len(x))
        if self.local is not None and hi > lo:
            self.local.add(x[lo:hi])

    def set_labels_global(self, labels) -> None:
        """Every rank sees the full [N] int array of row labels (IvfIndex.set_labels) and keeps those of its own rows."""
        if len(labels) != self.ntotal_global:
            raise ValueError(f"set_labels_global: {len(labels)} labels for {self.ntotal_global} rows")
        if self.local is not None and self.hi > self.lo:
            self.local.set_labels(labels[self.lo:self.hi])

    def update_rows_global(self, ids, x) -> None:
        """IvfIndex.update_rows over the shards: every rank passes the same GLOBAL row ids [n] and the same rows x [n, d]; each shard
        writes the rows it holds and moves them to their new lists (ids outside [lo, hi) name no local row and are skipped).  No
        communication."""
        self._need_local("update_rows_global")
        self.local.update_rows(ids, x, idx_offset=self.lo)

    @property
    def ntotal(self) -> int:
        return self.ntotal_global

    def centroids(self) -> np.ndarray:
        return self.local.centroids() if self.local is not None else self._trained[0]

    def list_sizes_global(self) -> np.ndarray:
        """int64 [nlist]: the sizes of the global lists -- the shards' list sizes summed, ONE integer all-reduce."""
        import torch
        import torch.distributed as dist

        self._need_local("list_sizes_global")
        t = torch.from_numpy(self.local.list_sizes())
        if self.world > 1:
            if dist.get_backend(self.group) == "nccl":
                t = t.to(f"cuda:{self.local.device}")
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy()

    # The collectives below are ShardedMipsIndex's own code, borrowed as plain functions.  They touch nothing of `self` but: local
    # (.device, .reconstruct_batch(ids, idx_offset=, zero_missing=)), lo, world, group, d, ntotal_global, _local_reconstruct
    # (reconstruct_batch); world, group (_range_gather).  A change there that reads more has to be mirrored in __init__ here.
    reconstruct_batch = ShardedMipsIndex.reconstruct_batch  # each shard's rows, zero elsewhere, ONE integer all-reduce

    # ------------------------------------------------------------------ persistence
    def save(self, path: str) -> None:
        """COLLECTIVE: every rank writes its shard with IvfIndex.save into path/shard_<rank>, rank 0 writes path/meta.json."""
        import torch.distributed as dist

        self._need_local("save")
        if self.rank == 0:
            os.makedirs(path, exist_ok=True)
        if self.world > 1:
            dist.barrier(group=self.group)
        self.local.save(os.path.join(path, f"shard_{self.rank}"))
        if self.rank == 0:
            with open(os.path.join(path, "meta.json"), "w") as f:
                json.dump({"format": 1, "sharded_ivf": self.world, "d": self.d, "nlist": self.nlist, "dtype": self.dtype,
                           "ntotal": self.ntotal_global}, f)
        if self.world > 1:
            dist.barrier(group=self.group)

    @classmethod
    def load(cls, path: str, group=None, device=None) -> "ShardedIvfIndex":
        """COLLECTIVE: every rank loads its own shard (IvfIndex.load of path/shard_<rank>); the group must have as many ranks as the
        one that saved.  Ends with check_trained_global()."""
        from .ivf import IvfIndex

        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if "sharded_ivf" not in meta:
            raise ValueError("not a saved ShardedIvfIndex")
        import torch.distributed as dist

        rank = dist.get_rank(group) if dist.is_initialized() else 0
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        if meta["sharded_ivf"] != world:
            raise ValueError(f"load: saved by {meta['sharded_ivf']} ranks, loaded by {world}; the shards are files of their own")
        self = cls(meta["d"], meta["nlist"], dtype=meta["dtype"], group=group, device=device,
                   _local_index=IvfIndex.load(os.path.join(path, f"shard_{rank}"), device=device))
        lo, hi = self.set_global_size(meta["ntotal"])
        if self.local.ntotal != hi - lo:
            raise ValueError(f"load: shard {self.rank} holds {self.local.ntotal} rows, the partition gives it {hi - lo}")
        self.meta = meta
        self.check_trained_global()
        return self

    # ------------------------------------------------------------------ searching
    def _filter_kw(self, what: str, selector, groups, group_mode: str) -> dict:
        """-> the keywords of the local step: a GLOBAL selector (one bit per global row, the same on every rank) read from bit lo"""
        kw = {}
        if selector is not None:
            from .selector import Selector

            if self.local is not None and not (isinstance(selector, Selector) or (isinstance(selector, np.ndarray) and selector.dtype == np.uint8)):
                selector = Selector.from_mask(selector, device=self.local.device)  # packed once (the range search may repeat its call)
            nbits = selector.nbits if isinstance(selector, Selector) else (
                8 * selector.size if isinstance(selector, np.ndarray) and selector.dtype == np.uint8 else len(selector))
            if nbits < self.ntotal_global:
                raise ValueError(f"{what}: the selector has {nbits} bits, the sharded index {self.ntotal_global} rows")
            kw.update(selector=selector, sel_bit0=self.lo)
        if groups is not None:
            if group_mode not in ("exclude", "only"):
                raise ValueError(f"{what}: group_mode must be 'exclude' or 'only', got {group_mode!r}")
            kw.update(groups=groups, group_mode=group_mode)
        return kw

    def _home(self):
        import torch

        return torch.device("cuda", self.local.device) if self.local is not None else torch.device("cpu")

    def search_probed(self, q, k: int, nprobe: int | None = None, selector=None, groups=None, group_mode: str = "exclude"):
        """(D, I) [nq, k], 1 <= k <= MAX_K_WIDE: replicated queries in, the result of the unsharded IvfIndex.search_probed /
        search_probed_wide out, global row numbers, the same bits on every rank.  NumPy in gives NumPy out, a CUDA tensor CUDA
        tensors.  selector: GLOBAL (one bit per global row, the same on every rank); groups / group_mode: one label per query,
        replicated like the queries, against set_labels_global.  COLLECTIVE: the part search, ONE all-gather of the payloads (nq * k
        * 16 bytes per rank; host-staged under gloo), the merge.  Raises ValueError for k < 1 or nprobe < 1, NotImplementedError for
        k > MAX_K_WIDE, min(nprobe, nlist) > 1024, min(nprobe, nlist) * k > 65536 and world * k > 65536 (the entries a merge takes)."""
        import torch
        import torch.distributed as dist

        k = int(k)
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        if k < 1 or nprobe < 1:
            raise ValueError(f"search_probed: k and nprobe must be >= 1, got k = {k}, nprobe = {nprobe}")
        p = min(nprobe, self.nlist)
        if k > _lib.MAX_K_WIDE or p > 1024 or p * k > 65536 or self.world * k > 65536:
            raise NotImplementedError(f"search_probed: k = {k} with min(nprobe, nlist) = {p} on {self.world} ranks is not served (k <= "
                                      f"{_lib.MAX_K_WIDE}, lists <= 1024, lists * k <= 65536, ranks * k <= 65536)")
        kw = self._filter_kw("search_probed", selector, groups, group_mode)
        as_numpy = not isinstance(q, torch.Tensor)
        if self.local is not None:
            if self.world == 1:
                return self.local.search_probed_wide(q, k, nprobe, idx_offset=self.lo, **kw)
            home = self._home()
            qd = (torch.from_numpy(np.ascontiguousarray(q)) if as_numpy else q).to(home)
            packed, bias = self.local.search_part(qd, k, nprobe, idx_offset=self.lo, **kw)
        else:
            hq = q.detach().cpu().numpy() if not as_numpy else np.asarray(q)
            s, i, bias = self._local_search(hq, k, nprobe, self.lo, **kw)
            packed = pack_topk(torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(i, dtype=np.int64)))
        nq = int(packed.shape[0])
        gathered = packed
        if self.world > 1:
            if dist.get_backend(self.group) == "gloo" and packed.is_cuda:
                packed = packed.cpu()  # gloo moves host memory; RCCL takes the device tensor
            gathered = torch.empty((self.world * nq, k, 2), dtype=torch.int64, device=packed.device)
            dist.all_gather_into_tensor(gathered, packed, group=self.group)  # the ONE collective of the path
        if self.local is not None:
            from .ivf import ivf_merge_parts

            D, I = ivf_merge_parts(gathered.to(home).contiguous(), self.world, nq, k, bias)
            if as_numpy:
                return D.cpu().numpy(), I.cpu().numpy()
            return (D, I) if D.device == q.device else (D.to(q.device), I.to(q.device))
        D, I = self._merge(gathered.cpu().numpy().reshape(self.world, nq, k, 2), self.world, nq, k, bias)
        if as_numpy:
            return np.asarray(D), np.asarray(I)
        return torch.as_tensor(D).to(q.device), torch.as_tensor(I).to(q.device)

    search_probed_wide = search_probed  # one definition for 1 <= k <= MAX_K_WIDE: the sharded class takes the wide range under one name

    # ------------------------------------------------------------------ range search: the record protocol of ShardedMipsIndex
    _range_stride_guess = staticmethod(ShardedMipsIndex._range_stride_guess)
    _range_gather = ShardedMipsIndex._range_gather

    def _range_local_record(self, q, r, nq: int, stride: int, nprobe: int, kw: dict):
        """This shard's hits as a record of `stride` entries on _home(); the lims are the true counts whatever the stride is."""
        import torch

        if self._local_range_search is None:
            return range_record_fill(self._home(), nq, stride, search_into=lambda lims, D, I: self.local.range_search_probed_into(
                q, r, lims, D, I, nprobe=nprobe, idx_offset=self.lo, **kw))
        hq = q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else q
        return range_record_fill(self._home(), nq, stride, search_host=lambda: self._local_range_search(hq, r, nprobe, self.lo, **kw))

    def _range_args(self, what: str, nprobe, selector, groups, group_mode):
        nprobe = int(self.nprobe if nprobe is None else nprobe)
        if nprobe < 1:
            raise ValueError(f"{what}: nprobe must be >= 1")
        if min(nprobe, self.nlist) > 1024:
            raise NotImplementedError(f"{what}: min(nprobe, nlist) > 1024 is not served")
        if self.local is None and self._local_range_search is None:
            raise ValueError(f"{what}: no local range step was injected")
        return nprobe, self._filter_kw(what, selector, groups, group_mode)

    def range_search_probed(self, q, radius, nprobe: int | None = None, selector=None, groups=None, group_mode: str = "exclude"):
        """IvfIndex.range_search_probed over the row shards: replicated queries and radii in, (lims, D, I) with global row numbers
        out, the same on every rank, the hits of a query in ascending row order.  NumPy in -> NumPy out, CUDA tensor in -> CUDA
        tensors out.  An 'sq8' hit is decided on D per row, so nothing is compared across shards.  COLLECTIVE and SYNCHRONISING:
        every shard searches into a record with a guessed capacity, ONE scalar all-reduce (MAX) of the shards' totals is read on the
        host, a shard that found more than its record holds repeats its search once with that maximum, ONE all-gather moves the
        records and mips_range_merge_records lays the shards' segments end to end per query."""
        import torch

        from .index import MipsIndex

        nprobe, kw = self._range_args("range_search_probed", nprobe, selector, groups, group_mode)
        as_numpy = not isinstance(q, torch.Tensor)
        if self.world == 1:
            if self._local_range_search is None:
                return self.local.range_search_probed(q, radius, nprobe, idx_offset=self.lo, **kw)
            return self._local_range_search(q.detach().cpu().numpy() if not as_numpy else q, radius, nprobe, self.lo, **kw)
        nq = int(q.shape[0])
        r = MipsIndex._radii(radius, nq)
        if self.local is not None and as_numpy:
            q = torch.from_numpy(np.ascontiguousarray(q)).to(self._home())  # staged once for the repeat call
        return range_record_exchange(self, q, nq, lambda stride: self._range_local_record(q, r, nq, stride, nprobe, kw), as_numpy)

    def range_search_probed_into(self, q, radius, lims, D, I, part_cap: int, nprobe: int | None = None, selector=None, groups=None,
                                 group_mode: str = "exclude") -> None:
        """The form of range_search_probed that never synchronises on the GPU: every shard searches into a record of `part_cap`
        entries, then ONE all-gather and ONE merge into the caller's CUDA tensors lims (int64 [nq + 1]), D (float32 [cap]) and I
        (int64 [cap]).  lims receives the true global counts whatever happens; D and I are valid iff no shard found more than
        part_cap hits and lims[-1] <= cap.  Device steps only; under gloo the all-gather is host-staged, which waits for the record."""
        from .index import MipsIndex, range_merge_records

        nprobe, kw = self._range_args("range_search_probed_into", nprobe, selector, groups, group_mode)
        if self.local is None:
            raise ValueError("range_search_probed_into runs the library's own device steps; injected steps serve range_search_probed only")
        if self.world == 1:
            return self.local.range_search_probed_into(q, radius, lims, D, I, nprobe=nprobe, idx_offset=self.lo, **kw)
        nq, part_cap = int(q.shape[0]), int(part_cap)
        if part_cap < 0:
            raise ValueError("range_search_probed_into: part_cap must be >= 0")
        rec = self._range_local_record(q, MipsIndex._radii(radius, nq), nq, part_cap, nprobe, kw)
        range_merge_records(self._range_gather(rec)[1], self.world, nq, part_cap, out=(lims, D, I))
