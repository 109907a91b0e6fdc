"""Row-sharded search over the GPUs of one node.

The reference replicates the whole FAISS index on every rank (lightning_model.py:180,
mips.py:545-549).  Here rank r of G keeps rows [r*ceil(N/G), min(N, (r+1)*ceil(N/G))) in its own
HBM, every rank scores ALL queries against its shard with the fused HIP kernel, and ONE collective
-- an all-gather (RCCL over xGMI when the backend is "nccl") of the packed per-rank top-k -- is
followed by a replicated k-way merge, identical on every rank.  No other data-path collective.

The all-gather payload is one int64 tensor [nq, k, 2] per rank (float32 score bits, global row id):
4096 x 5 x 16 B = 320 KiB at the headline config -- latency bound on xGMI.  The wide search (search_wide, 30 <= k <= 1024)
takes the same route with a payload that is bandwidth-sized instead: 6.5 MB per rank at 4096 x 100, 64 MiB at 4096 x 1024, and
the gathered buffer is `world` times that.

The range search (range_search) has a result of variable size: every rank searches into ONE int64 record -- lims, global ids and
scores side by side (range_record_views; include/mips_hip_sharded.h) -- the ranks agree on a common record size with one scalar
all-reduce, the records travel in the same ONE all-gather, and a replicated merge lays the shards' segments end to end per query.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def shard_bounds(n: int, world: int, rank: int):
    """Contiguous row partition, ceil(N/G) rows per rank (same contiguous-chunk idea as the
    reference's encode sharding, sotasum/mips.py:227-229)."""
    per = -(-int(n) // int(world))
    lo = min(int(n), rank * per)
    hi = min(int(n), (rank + 1) * per)
    return lo, hi


def shard_offsets(counts, rank: int):
    """Row ranges of shards that hold counts[r] rows each, laid end to end in rank order: -> (lo, hi, total) of `rank`.  What
    the shards of an index are after remove_ids_global (shard_bounds describes them only until then)."""
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts) or not 0 <= int(rank) < len(counts):
        raise ValueError(f"shard_offsets: rank {rank} of counts {counts}")
    lo = sum(counts[:int(rank)])
    return lo, lo + counts[int(rank)], sum(counts)


def pack_topk(scores, idx):
    """(float32 [nq,k], int64 [nq,k]) torch tensors -> int64 [nq,k,2]."""
    import torch

    bits = scores.contiguous().view(torch.int32).to(torch.int64)
    return torch.stack((bits, idx.to(torch.int64)), dim=-1).contiguous()


def unpack_gathered(gathered, world: int):
    """int64 [world, nq, k, 2] -> (float32 [nq, world*k], int64 [nq, world*k]), shard-major rows."""
    import torch

    nq, k = gathered.shape[1], gathered.shape[2]
    g = gathered.permute(1, 0, 2, 3).reshape(nq, world * k, 2)
    s = g[..., 0].to(torch.int32).contiguous().view(torch.float32)
    return s, g[..., 1].contiguous()


def range_record_views(rec, nq: int, stride: int):
    """The three regions of a range-search record (a contiguous int64 torch tensor of range_record_words(nq, stride) words) as
    contiguous 1-d views: lims int64 [nq + 1], D float32 [stride], I int64 [stride] -- what MipsIndex.range_search_into takes."""
    import torch

    if rec.dtype != torch.int64 or rec.dim() != 1 or not rec.is_contiguous() or rec.shape[0] != _lib.range_record_words(nq, stride):
        raise ValueError(f"range_record_views: expected {_lib.range_record_words(nq, stride)} contiguous int64 words")
    return rec[:nq + 1], rec[nq + 1 + stride:].view(torch.float32)[:stride], rec[nq + 1:nq + 1 + stride]


def range_record_fill(home, nq: int, stride: int, search_into=None, search_host=None):
    """A shard's range-search hits as a record of `stride` entries on the device `home`: search_into(lims, D, I) searches straight
    into the record's three views (the device step), or search_host() -> NumPy (lims, D, I) is copied into it (an injected step).
    The lims are the true counts whatever the stride is; entries past it are dropped, as mips_range_search drops them."""
    import torch

    if search_into is not None:
        rec = torch.empty(_lib.range_record_words(nq, stride), dtype=torch.int64, device=home)
        search_into(*range_record_views(rec, nq, stride))
        return rec
    lims, D, I = search_host()
    rec = torch.zeros(_lib.range_record_words(nq, stride), dtype=torch.int64)
    v_lims, v_D, v_I = range_record_views(rec, nq, stride)
    m = min(stride, len(I))
    v_lims.copy_(torch.from_numpy(np.ascontiguousarray(lims, dtype=np.int64)))
    v_D[:m].copy_(torch.from_numpy(np.ascontiguousarray(D[:m], dtype=np.float32)))
    v_I[:m].copy_(torch.from_numpy(np.ascontiguousarray(I[:m], dtype=np.int64)))
    return rec.to(home)


def range_record_exchange(ix, q, nq: int, local_record, as_numpy: bool):
    """The record protocol of a sharded range search, for any index `ix` with world, group, _range_stride_guess, _range_gather and
    _range_merge: local_record(stride) -> this shard's record.  Every shard searches into a record of the guessed capacity, ONE
    scalar all-reduce (MAX) of the shards' totals is read on the host -- the call's synchronisation --, a shard that found more than
    its record holds repeats its search once with that maximum, every record is brought to that common size, ONE all-gather moves
    the records and the merge lays the shards' segments end to end per query.  -> (lims, D, I): NumPy when as_numpy, else on q's
    device."""
    import torch
    import torch.distributed as dist

    from .index import range_merge_records

    stride = int(ix._range_stride_guess(nq))
    rec = local_record(stride)
    # the shards' totals: one scalar all-reduce, read on the host -- the call's synchronisation
    if dist.get_backend(ix.group) == "nccl":
        total = rec[nq:nq + 1].clone()
        dist.all_reduce(total, op=dist.ReduceOp.MAX, group=ix.group)
        common, own = (int(v) for v in torch.cat((total, rec[nq:nq + 1])).tolist())
    else:
        total = rec[nq:nq + 1].to("cpu", copy=True)  # (a copy also of a host record: the all-reduce writes in place)
        own = int(total.item())
        dist.all_reduce(total, op=dist.ReduceOp.MAX, group=ix.group)
        common = int(total.item())
    if own > stride:  # the guess was too small HERE: once more, with room for the largest shard result
        stride = common
        rec = local_record(stride)
    if stride != common:  # the record at the common size: the lims and the `own` entries that count
        fit = torch.empty(_lib.range_record_words(nq, common), dtype=torch.int64, device=rec.device)
        for dst, src, n in zip(range_record_views(fit, nq, common), range_record_views(rec, nq, stride), (nq + 1, own, own)):
            dst[:n].copy_(src[:n])
        rec = fit
    arrived, gathered = ix._range_gather(rec)
    if ix._range_merge is None:
        cap = int(arrived.view(ix.world, -1)[:, nq].sum().item())  # (on the host already under gloo)
        out = range_merge_records(gathered, ix.world, nq, common, cap)
    else:
        out = ix._range_merge(arrived.cpu().numpy(), ix.world, nq, common)
    if as_numpy:
        return tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in out)
    return tuple(t if isinstance(t, torch.Tensor) and t.device == q.device else torch.as_tensor(t).to(q.device) for t in out)


class ShardedMipsIndex:
    """One logical exact index, row-sharded across the ranks of a torch.distributed group.

    local_search(q, k, idx_offset) and merge(cand_s, cand_i, parts, k, metric) default to the HIP
    path (MipsIndex.search / mips_merge_topk).  They are injectable so that the partition + pack +
    all-gather + unpack plumbing can be exercised with the gloo backend on CPU-only machines, where
    tests substitute the CPU oracle for the two device steps.  local_search_wide(q, k, idx_offset) is the
    local step of search_wide (default MipsIndex.search_wide); when only one of the two local steps is
    injected it stands in for the other.  local_range_search(q, radius, idx_offset, **kw) -> NumPy (lims, D, I) and
    range_merge(gathered, parts, nq, stride) -> (lims, D, I) are the two steps of range_search (defaults
    MipsIndex.range_search_into / mips_range_merge_records); kw carries force_ip, selector + sel_bit0, groups + group_mode when
    the call has them, `gathered` is a NumPy int64 array of the records end to end.  With an injected local step the record is
    assembled on the host.  local_reconstruct(ids, lo) -> np.float32 [n, d] is the local step of reconstruct_batch (default
    MipsIndex.reconstruct_batch with idx_offset = lo and zero_missing): this shard's rows of the flat int64 `ids`, zero bytes for
    every id that names no row here.
    """

    def __init__(self, d: int, metric: int = _lib.METRIC_IP, dtype: str = "bf16", group=None, device=None,
                 local_search=None, merge=None, local_search_wide=None, local_range_search=None, range_merge=None,
                 local_reconstruct=None):
        import torch.distributed as dist

        if dtype == "sq8":
            raise NotImplementedError("ShardedMipsIndex: 'sq8' storage is not served -- every shard would train its own column range, "
                                      "and scores of different ranges do not merge (a global min / max is not implemented)")
        self.d = int(d)
        self.metric_type = int(metric)
        self.group = group
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.ntotal_global = 0
        self.lo = self.hi = 0
        self._even = True  # the shards are shard_bounds(ntotal_global, ...): until remove_ids_global
        self.local = None
        self._local_range_search = local_range_search
        self._range_merge = range_merge
        self._local_reconstruct = local_reconstruct
        if local_search is None and local_search_wide is None and local_range_search is None and local_reconstruct is None:
            from .index import MipsIndex

            self.local = MipsIndex(d, metric=metric, dtype=dtype, device=device)
            local_search, local_search_wide = self.local.search, self.local.search_wide
        self._fast = self.local is not None and merge is None  # both device steps are the library's own
        self._device_merge = merge is None  # mips_merge_topk: candidates must be on the GPU whatever moved them
        if merge is None:
            from .index import merge_topk as merge
        self._local_search = local_search if local_search is not None else local_search_wide
        self._local_search_wide = local_search_wide if local_search_wide is not None else local_search
        self._merge = merge

    # ------------------------------------------------------------------ building
    def set_global_size(self, n: int):
        self.ntotal_global = int(n)
        self.lo, self.hi = shard_bounds(n, self.world, self.rank)
        return self.lo, self.hi

    def add_global(self, x) -> None:
        """Every rank sees the full [N, d] array (NumPy / memmap / torch) and keeps its own rows."""
        self._refuse_after_removal("add_global")
        lo, hi = self.set_global_size(len(x))
        if self.local is not None and hi > lo:
            self.local.reserve(hi - lo)
            self.local.add(x[lo:hi])
        self._sync_phi()

    def add_synthetic_global(self, n: int, seed: int, kind: int) -> None:
        self._refuse_after_removal("add_synthetic_global")
        lo, hi = self.set_global_size(n)
        if hi > lo:
            self.local.reserve(hi - lo)
            self.local.add_synthetic(hi - lo, row0=lo, seed=seed, kind=kind)
        self._sync_phi()

    def _refuse_after_removal(self, what: str) -> None:
        if not self._even:
            raise ValueError(f"{what}: remove_ids_global left shards of unequal size (rows [{self.lo}, {self.hi}) here), and this "
                             "call places rows by the even partition shard_bounds(); save() and load() the index to re-partition it")

    def remove_ids_global(self, sel) -> int:
        """COLLECTIVE MipsIndex.remove_ids: every rank passes the same GLOBAL selector (Selector, bool mask, uint8 bitmap; one
        bit per global row) or the same global row ids; each shard removes its own rows (its bits start at `lo`), ONE small
        all-gather of the shards' new sizes renumbers the shards (shard_offsets), and an L2 index agrees on the new phi.
        Searches, selectors and save() go on working with the new lo / hi; the shards are no longer the even partition, so
        add_global is refused from here on.  -> the number of rows removed from the whole index."""
        import torch
        import torch.distributed as dist

        from .selector import Selector, is_id_list

        if self.local is None:
            raise ValueError("remove_ids_global needs the library's own local index (injected steps hold no rows)")
        if is_id_list(sel):
            sel = Selector.from_ids(sel, self.ntotal_global, device=self.local.device)
        nbits = sel.nbits if isinstance(sel, Selector) else (
            8 * sel.numel() if isinstance(sel, torch.Tensor) and sel.dtype == torch.uint8 else
            8 * sel.size if isinstance(sel, np.ndarray) and sel.dtype == np.uint8 else len(sel))
        if nbits < self.ntotal_global:
            raise ValueError(f"remove_ids_global: the selector has {nbits} bits, the sharded index {self.ntotal_global} rows")
        before = self.ntotal_global
        self.local.remove_ids(sel, sel_bit0=self.lo)
        counts = [self.local.ntotal]
        if self.world > 1:
            nccl = dist.get_backend(self.group) == "nccl"
            mine = torch.tensor(counts, dtype=torch.int64, device=f"cuda:{self.local.device}" if nccl else "cpu")
            every = torch.empty(self.world, dtype=torch.int64, device=mine.device)
            dist.all_gather_into_tensor(every, mine, group=self.group)
            counts = every.tolist()
        self.lo, self.hi, self.ntotal_global = shard_offsets(counts, self.rank)
        if self.ntotal_global != before:
            self._even = False
        self._sync_phi()
        return before - self.ntotal_global

    def update_rows_global(self, ids, x) -> None:
        """COLLECTIVE MipsIndex.update_rows: every rank passes the same GLOBAL row ids [n] and the same rows x [n, d]; each
        shard writes the rows it holds (ids outside [lo, hi) name no local row and are skipped; lo follows remove_ids_global,
        as in reconstruct_batch).  Row numbers, labels and the shard sizes stay.  An inner-product index needs no communication
        and, with CUDA ids and rows, nothing synchronises; an L2 index agrees on the new phi (one scalar all-reduce)."""
        if self.local is None:
            raise ValueError("update_rows_global needs the library's own local index (injected steps hold no rows)")
        self.local.update_rows(ids, x, idx_offset=self.lo)
        self._sync_phi()

    def set_labels_global(self, labels) -> None:
        """Every rank sees the full [N] int array of row labels (MipsIndex.set_labels) and keeps those of its own rows."""
        if len(labels) != self.ntotal_global:
            raise ValueError(f"set_labels_global: {len(labels)} labels for {self.ntotal_global} rows")
        if self.local is not None and self.hi > self.lo:
            self.local.set_labels(labels[self.lo:self.hi])

    def _sync_phi(self) -> None:
        """L2 mode: phi = max_i |x_i|^2 must be the GLOBAL maximum (mips.py:316-324 computes it over the
        whole knowledge base); one scalar all-reduce at build time, not on the search path."""
        import torch
        import torch.distributed as dist

        if self.metric_type != _lib.METRIC_L2 or self.local is None or self.world == 1:
            return
        self.local.clear_phi()  # a previous global value must not mask rows added since (incremental add_global)
        local = self.local.phi() if self.local.ntotal > 0 else 0.0
        backend = dist.get_backend(self.group)
        t = torch.tensor([local], dtype=torch.float64, device=f"cuda:{self.local.device}" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        self.local.set_phi(float(t.item()))

    @property
    def ntotal(self) -> int:
        return self.ntotal_global

    @property
    def dtype(self):
        return self.local.dtype if self.local is not None else None

    nprobe = 1  # accepted like MipsIndex.nprobe (mips.py:342-345); exact search ignores it

    def phi(self) -> float:
        """The global phi (after _sync_phi every shard holds the same override)."""
        return self.local.phi()

    # ------------------------------------------------------------------ persistence
    def save(self, path: str, extra: dict = None) -> None:
        """Collective: the shards are written into ONE file set in rank order (rank 0 writes meta.json), so the
        result is the same directory MipsIndex.save produces for the unsharded index and can be loaded by any
        number of ranks (or by a single MipsIndex.load)."""
        import json
        import os

        import torch.distributed as dist

        ext = {"bf16": "bf16", "fp8_e4m3": "e4m3", "fp8_e4m3_docs": "e4m3", "f32": "f32"}[self.local.dtype]
        if self.rank == 0:
            os.makedirs(path, exist_ok=True)
            open(os.path.join(path, "rows." + ext), "wb").close()
        for r in range(self.world):  # append in rank order; barriers keep the order
            if self.world > 1:
                dist.barrier(group=self.group)
            if r == self.rank and self.local.ntotal > 0:
                with open(os.path.join(path, "rows." + ext), "ab") as f:
                    n = self.local.ntotal
                    for r0 in range(0, n, 1 << 16):
                        f.write(self.local.rows_raw(r0, min(1 << 16, n - r0)).tobytes())
        if self.world > 1:
            dist.barrier(group=self.group)
        if self.rank == 0:
            meta = {"format": 1, "d": self.d, "ntotal": self.ntotal_global, "metric": self.metric_type,
                    "dtype": self.local.dtype}
            if self.metric_type == _lib.METRIC_L2 and self.ntotal_global > 0:
                meta["phi"] = self.phi()
            if extra:
                meta.update({k: v for k, v in extra.items() if v is not None or k not in meta})
            with open(os.path.join(path, "meta.json"), "w") as f:
                json.dump(meta, f)
        if self.world > 1:
            dist.barrier(group=self.group)

    @classmethod
    def load(cls, path: str, group=None, device=None) -> "ShardedMipsIndex":
        """Every rank maps the same file set and keeps its own row range (MipsIndex.load(row_range)); an L2
        index takes the file's global phi.  Replaces `load()` on every rank of lightning_model.py:180."""
        import json
        import os

        from .index import MipsIndex

        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        self = cls.__new__(cls)
        ShardedMipsIndex.__init__(self, meta["d"], metric=meta["metric"], dtype=meta["dtype"], group=group, device=device,
                                  local_search=lambda *a, **k: None)  # placeholder: the local index comes from the file
        lo, hi = self.set_global_size(meta["ntotal"])
        self.local = MipsIndex.load(path, device=device, row_range=(lo, hi))
        self._local_search, self._local_search_wide = self.local.search, self.local.search_wide
        self._fast = True
        self.meta = meta
        if self.metric_type == _lib.METRIC_L2 and meta.get("phi") is None:
            self._sync_phi()  # files written before phi was persisted
        return self

    def set_param(self, name: str, value: int) -> None:
        """Knob of the LOCAL scan (MipsIndex.set_param) -- every rank sets its own.  The default margin mode already certifies
        the local device-output searches without synchronising (the exact pass of the queries they flag is enqueued behind the
        scan), which keeps the optimistic / two-stage paths (8 <= k <= 29, fp32-exact shards) open to the sharded search."""
        self.local.set_param(name, value)

    def margin_stats(self, synchronize: bool = True, reduce: bool = True) -> dict:
        """Margin statistics of the last search: the shards' counts (MipsIndex.margin_stats) SUMMED over the ranks -- a query
        left unresolved on any shard is unresolved in the merged result, so `unresolved` must be visible everywhere.  The sum
        is one small all-reduce: COLLECTIVE, every rank calls it (synchronize=True only; reduce=False or synchronize=False
        return this rank's own counts without communicating)."""
        st = self.local.margin_stats(synchronize)
        if not (reduce and synchronize and self.world > 1):
            return st
        import torch
        import torch.distributed as dist

        backend = dist.get_backend(self.group)
        t = torch.tensor([st["flagged"], st["rescanned"], st["unresolved"]], dtype=torch.int64,
                         device=f"cuda:{self.local.device}" if backend == "nccl" else "cpu")
        t = torch.clamp(t, min=0)  # (-1 = "only counted on the device" cannot survive a synchronising read)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        f, r, u = (int(v) for v in t.cpu().tolist())
        return {"flagged": f, "rescanned": r, "unresolved": u}

    def check(self, synchronize: bool = True) -> None:
        """MipsIndex.check for this rank's shard.  A shard whose scan timed out hands poisoned rows (idx -2, NaN)
        to the all-gather and the merge kernel propagates them, so every rank SEES the failure in its results;
        the rank it happened on also raises here (and on its next search)."""
        if self.local is not None:
            self.local.check(synchronize)

    # ------------------------------------------------------------------ pipelined search
    class _Pending:
        """Result of search_async: .result() makes the CURRENT stream wait for the merged top-k and returns it."""

        def __init__(self, out, done_event, keep, index=None):
            self._out, self._done, self._keep, self._index = out, done_event, keep, index

        def result(self):
            import torch

            if self._done is not None:
                cur = torch.cuda.current_stream(self._out[0].device)
                cur.wait_event(self._done)
                for t in self._out:
                    t.record_stream(cur)  # allocated on the side stream, consumed on this one
                self._done, self._keep = None, None
            if self._index is not None:
                self._index.check(synchronize=False)  # host-visible flag only: no synchronisation on this path
            return self._out

    def search_async(self, q, k: int, _force_collective: bool = False):
        """search() split over two streams so that consecutive, independent query batches overlap:
          current stream   query staging + the fused scan of this shard (mips_search_split);
          side stream      candidate selection + exact re-score, then the exchange step -- the ONE all-gather and the
                           replicated merge (ranks > 1).
        The caller can enqueue the NEXT batch's scan before asking for this batch's result(): the scan of batch t + 1
        starts right behind the scan of batch t, the ~45 us tail and the latency-bound collective (tens of us against a
        ~0.6 ms shard scan at 8 GPUs) run beside it.  Falls back to the synchronous path when there is nothing to
        overlap with (host queries, injected device steps, gloo).  k > MAX_K: the result of search_wide, already complete --
        the wide search has no two-stream form."""
        import torch
        import torch.distributed as dist

        if int(k) > _lib.MAX_K:
            return ShardedMipsIndex._Pending(self.search_wide(q, k), None, None)
        backend = dist.get_backend(self.group) if dist.is_initialized() else None
        collective = self.world > 1 or _force_collective
        fast = (self.local is not None and self._fast and isinstance(q, torch.Tensor) and q.is_cuda
                and (backend == "nccl" or not collective))
        if not fast:
            return ShardedMipsIndex._Pending(self.search(q, k), None, None)
        from .index import merge_topk_packed

        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=q.device, priority=-1)  # its short kernels go first when CUs free up
        side = self._side
        main = torch.cuda.current_stream(q.device)
        if not collective:
            out = self.local.search(q, k, self.lo, tail_stream=side)  # scan here, select + re-score on the side stream
            done = torch.cuda.Event()
            done.record(side)
            return ShardedMipsIndex._Pending(out, done, (q,), self.local)
        packed = self.local.search_packed(q, k, self.lo, tail_stream=side)
        nq = packed.shape[0]
        ready = torch.cuda.Event()
        ready.record(main)  # (the one-launch kernel of tiny searches writes its results on the main stream)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            gathered = torch.empty((self.world * nq, k, 2), dtype=torch.int64, device=packed.device)
            dist.all_gather_into_tensor(gathered, packed, group=self.group)  # the ONE collective of the path
            out = merge_topk_packed(gathered, nq, self.world, k, self.metric_type)
            done = torch.cuda.Event()
            done.record(side)
        return ShardedMipsIndex._Pending(out, done, (packed, gathered, q), self.local)

    # ------------------------------------------------------------------ search
    def search(self, q, k: int, idx_offset: int = 0, force_ip: bool = False, selector=None, groups=None, group_mode: str = "exclude"):
        """Replicated queries in, global top-k out (same on every rank).  force_ip: rank by inner product on an
        L2 index (Mips.np_search); idx_offset exists for signature compatibility with MipsIndex.search and must
        be 0 (global row numbers are the shard offsets' business).  selector / groups: a filtered or grouped search, served
        by search_wide."""
        import torch
        import torch.distributed as dist

        if selector is not None or groups is not None:
            return self.search_wide(q, k, idx_offset=idx_offset, force_ip=force_ip, selector=selector, groups=groups, group_mode=group_mode)
        if idx_offset:
            raise ValueError("ShardedMipsIndex.search returns global row numbers; idx_offset must be 0")
        if force_ip:
            return self._search_force_ip(q, k)
        backend = dist.get_backend(self.group) if self.world > 1 else None
        if (self.world > 1 and self.local is not None and self._fast and isinstance(q, torch.Tensor) and q.is_cuda):
            # device fast path: the re-score kernel writes the all-gather payload, the merge kernel reads
            # the gathered buffer as it arrives -- no tensor reshuffling between scan and collective
            from .index import merge_topk_packed

            packed = self.local.search_packed(q, k, self.lo)
            nq = packed.shape[0]
            if backend == "gloo":
                packed = packed.cpu()
            gathered = torch.empty((self.world * nq, k, 2), dtype=torch.int64, device=packed.device)
            dist.all_gather_into_tensor(gathered, packed, group=self.group)  # the ONE collective of the path
            if not gathered.is_cuda:
                gathered = gathered.to(q.device)
            return merge_topk_packed(gathered, nq, self.world, k, self.metric_type)
        s, i = self._local_search(q, k, self.lo)
        return self._exchange(s, i, k, self.metric_type)

    def search_wide(self, q, k: int, idx_offset: int = 0, force_ip: bool = False, selector=None, groups=None, group_mode: str = "exclude"):
        """search() for k up to MAX_K_WIDE = 1024 (route_search sends k > MAX_K here): every shard runs MipsIndex.search_wide,
        then the same ONE all-gather, then the merge for sorted lists (mips_merge_topk_sorted_packed: the counting merge of
        search() is quadratic in world * k).  bf16 and f32 shards of at most 1024 columns; idx_offset must be 0; force_ip as in
        search().  Every query is certified or settled on its shard, so margin_stats() reports unresolved = 0.  The payload is
        nq * k * 16 bytes per rank -- bandwidth- rather than latency-sized -- and the gathered buffer `world` times that.
        selector: a GLOBAL selector (one bit per global row, the same on every rank; Selector, bool mask or NumPy bitmap); each
        shard reads its own rows' bits from bit `lo` on, the exchange and the merge are those of the unfiltered search.
        groups / group_mode: one label per query, replicated like the queries, tested by every shard against the labels of its
        own rows (set_labels_global); exchange and merge untouched."""
        import torch
        import torch.distributed as dist

        sel_kw = {}
        if selector is not None:
            from .selector import Selector

            nbits = selector.nbits if isinstance(selector, Selector) else (
                8 * selector.size if isinstance(selector, np.ndarray) and selector.dtype == np.uint8 else len(selector))
            if nbits < self.ntotal_global:
                raise ValueError(f"search_wide: the selector has {nbits} bits, the sharded index {self.ntotal_global} rows")
            sel_kw = {"selector": selector, "sel_bit0": self.lo}
        if groups is not None:
            sel_kw.update(groups=groups, group_mode=group_mode)

        if idx_offset:
            raise ValueError("ShardedMipsIndex.search_wide returns global row numbers; idx_offset must be 0")
        k = int(k)
        if k > _lib.MAX_K_WIDE:
            raise NotImplementedError(f"k = {k} > {_lib.MAX_K_WIDE} is not supported by this build")
        if self.local is not None:
            self.local._check_wide(k)  # e4m3 storage, more than 1024 columns: refused as MipsIndex refuses them
        metric = _lib.METRIC_IP if force_ip else self.metric_type
        if (self.world > 1 and self.local is not None and self._fast and isinstance(q, torch.Tensor) and q.is_cuda):
            # device fast path, as in search(): the shard's result leaves as the payload, the merge reads it as it arrives
            from .index import merge_topk_sorted_packed

            packed = self.local.search_wide_packed(q, k, self.lo, force_ip=force_ip, **sel_kw)
            nq = packed.shape[0]
            if dist.get_backend(self.group) == "gloo":
                packed = packed.cpu()
            gathered = torch.empty((self.world * nq, k, 2), dtype=torch.int64, device=packed.device)
            dist.all_gather_into_tensor(gathered, packed, group=self.group)  # the ONE collective of the path
            if not gathered.is_cuda:
                gathered = gathered.to(q.device)
            return merge_topk_sorted_packed(gathered, nq, self.world, k, metric)
        s, i = self._local_search_wide(q, k, self.lo, **({"force_ip": True} if force_ip else {}), **sel_kw)
        return self._exchange(s, i, k, metric)

    # ------------------------------------------------------------------ rows by id
    def reconstruct_batch(self, ids):
        """COLLECTIVE MipsIndex.reconstruct_batch: every rank passes the same GLOBAL row ids [...] (NumPy -> NumPy, CUDA tensor
        -> CUDA tensor) and gets the same float32 rows [..., d], bit for bit those of the unsharded index.  Each shard gathers
        the rows it holds and leaves zero bytes elsewhere (idx_offset = lo, zero_missing), ONE all-reduce (SUM) of the buffers
        viewed as int32 assembles the rows -- exactly one shard contributes to a row, and an integer sum keeps its bits (a
        float sum would turn -0.0 + 0.0 into +0.0 and quieten NaN payloads) --, and the ids that name no row of the whole index
        become NaN rows.  Works on the uneven shards remove_ids_global leaves."""
        import torch
        import torch.distributed as dist

        as_numpy = not isinstance(ids, torch.Tensor)
        t_ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)) if as_numpy else ids.to(torch.int64)
        shape = tuple(t_ids.shape)
        flat = t_ids.reshape(-1)
        if self._local_reconstruct is not None:
            rows = torch.from_numpy(np.ascontiguousarray(self._local_reconstruct(flat.cpu().numpy(), self.lo), dtype=np.float32))
        else:
            rows = self.local.reconstruct_batch(flat.to(f"cuda:{self.local.device}"), idx_offset=self.lo, zero_missing=True)
        home = rows.device
        bits = rows.view(torch.int32)
        if self.world > 1:
            if dist.get_backend(self.group) == "gloo" and bits.is_cuda:
                bits = bits.cpu()  # gloo moves host memory
            dist.all_reduce(bits, op=dist.ReduceOp.SUM, group=self.group)  # the ONE collective of the call
            bits = bits.to(home)
        flat = flat.to(home)
        bits[(flat < 0) | (flat >= self.ntotal_global)] = 0x7FC00000
        out = bits.view(torch.float32).reshape(shape + (self.d,))
        if as_numpy:
            return out.cpu().numpy()
        return out if out.device == ids.device else out.to(ids.device)

    # ------------------------------------------------------------------ range search
    @staticmethod
    def _range_stride_guess(nq: int) -> int:
        """Room for hits in the first local call of range_search: MipsIndex.range_search's guess, the same on every rank."""
        return max(1 << 16, 256 * int(nq))

    def _range_kw(self, what: str, idx_offset: int, force_ip: bool, selector, groups, group_mode: str) -> dict:
        """Checks shared by the two range calls; -> the keywords of the local step."""
        if idx_offset:
            raise ValueError(f"ShardedMipsIndex.{what} returns global row numbers; idx_offset must be 0")
        if self.local is not None:
            self.local._check_range()  # e4m3 storage, more than 1024 columns: refused as MipsIndex refuses them
        kw = {"force_ip": True} if force_ip else {}
        if selector is not None:
            from .selector import Selector

            if self.local is not None and not (isinstance(selector, Selector) or (isinstance(selector, np.ndarray) and selector.dtype == np.uint8)):
                selector = Selector.from_mask(selector, device=self.local.device)  # packed once for the repeat call
            nbits = selector.nbits if isinstance(selector, Selector) else (
                8 * selector.size if isinstance(selector, np.ndarray) and selector.dtype == np.uint8 else len(selector))
            if nbits < self.ntotal_global:
                raise ValueError(f"{what}: the selector has {nbits} bits, the sharded index {self.ntotal_global} rows")
            kw.update(selector=selector, sel_bit0=self.lo)
        if groups is not None:
            kw.update(groups=groups, group_mode=group_mode)
        return kw

    def _range_home(self):
        """Where this rank's record is written and merged: the shard's GPU; the host when both steps are injected."""
        import torch

        if self.local is not None:
            return torch.device("cuda", self.local.device)
        return torch.device("cuda") if self._range_merge is None else torch.device("cpu")

    def _range_local_record(self, q, r, nq: int, stride: int, kw: dict):
        """This shard's hits as a record of `stride` entries on _range_home().  The lims are the true counts whatever the stride
        is; entries past it are dropped, as mips_range_search drops them."""
        import torch

        home = self._range_home()
        if self._local_range_search is None:
            return range_record_fill(home, nq, stride, search_into=lambda lims, D, I: self.local.range_search_into(q, r, lims, D, I, idx_offset=self.lo, **kw))
        hq = q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else q
        return range_record_fill(home, nq, stride, search_host=lambda: self._local_range_search(hq, r, self.lo, **kw))

    def _range_gather(self, rec):
        """The ONE collective of the range calls: this rank's record in, the records end to end out -- as they arrived (on the
        host under gloo, which moves host memory) and on the record's own device."""
        import torch
        import torch.distributed as dist

        home = rec.device
        if dist.get_backend(self.group) == "gloo" and rec.is_cuda:
            rec = rec.cpu()
        arrived = torch.empty(self.world * rec.shape[0], dtype=torch.int64, device=rec.device)
        dist.all_gather_into_tensor(arrived, rec, group=self.group)
        return arrived, (arrived if arrived.device == home else arrived.to(home))

    def range_search(self, q, radius, idx_offset: int = 0, force_ip: bool = False, selector=None, groups=None, group_mode: str = "exclude"):
        """MipsIndex.range_search over the row shards: replicated queries and radii in, (lims, D, I) with global row numbers out,
        the same on every rank; hits of a query in ascending row order.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors
        out.  idx_offset must be 0; force_ip, selector (GLOBAL, one bit per global row, the same on every rank), groups /
        group_mode (replicated like the queries, against set_labels_global) as in search_wide.  bf16 and f32 shards of at most
        1024 columns.  COLLECTIVE and SYNCHRONISING: every shard searches into a record with MipsIndex.range_search's guess of
        a capacity, ONE scalar all-reduce (MAX) of the shards' totals is read on the host, a shard that found more than its
        record holds repeats its search once with that maximum, every record is brought to that common size, ONE all-gather
        moves the records and mips_range_merge_records lays the shards' segments end to end per query."""
        import torch
        import torch.distributed as dist

        from .index import MipsIndex, range_merge_records

        kw = self._range_kw("range_search", idx_offset, force_ip, selector, groups, group_mode)
        as_numpy = not isinstance(q, torch.Tensor)
        if self.world == 1:
            if self._local_range_search is None:
                return self.local.range_search(q, radius, self.lo, **kw)
            return self._local_range_search(q.detach().cpu().numpy() if not as_numpy else q, radius, self.lo, **kw)
        nq = int(q.shape[0])
        r = MipsIndex._radii(radius, nq)
        return range_record_exchange(self, q, nq, lambda stride: self._range_local_record(q, r, nq, stride, kw), as_numpy)

    def range_search_into(self, q, radius, lims, D, I, part_cap: int, idx_offset: int = 0, force_ip: bool = False, selector=None,
                          groups=None, group_mode: str = "exclude") -> None:
        """The form of range_search that never synchronises on the GPU: every shard searches into a record of `part_cap` entries,
        then ONE all-gather and ONE merge into the caller's CUDA tensors lims (int64 [nq + 1]), D (float32 [cap]) and I (int64
        [cap]).  lims receives the true global counts whatever happens; D and I are valid iff no shard found more than part_cap
        hits and lims[-1] <= cap -- the caller reads lims when it needs to know, and a shard's own count is lims of
        local.range_search_into.  Device steps only (no injection); under gloo the all-gather is host-staged, which waits for
        the record."""
        import torch

        from .index import MipsIndex, range_merge_records

        kw = self._range_kw("range_search_into", idx_offset, force_ip, selector, groups, group_mode)
        if self.local is None or self._range_merge is not None:
            raise ValueError("range_search_into runs the library's own device steps; injected steps serve range_search only")
        if self.world == 1:
            return self.local.range_search_into(q, radius, lims, D, I, idx_offset=self.lo, **kw)
        nq, part_cap = int(q.shape[0]), int(part_cap)
        if part_cap < 0:
            raise ValueError("range_search_into: part_cap must be >= 0")
        rec = self._range_local_record(q, MipsIndex._radii(radius, nq), nq, part_cap, kw)
        range_merge_records(self._range_gather(rec)[1], self.world, nq, part_cap, out=(lims, D, I))

    def _search_force_ip(self, q, k: int):
        s, i = self.local.search(q, k, self.lo, force_ip=True)
        return self._exchange(s, i, k, _lib.METRIC_IP)

    def _exchange(self, s, i, k: int, metric: int):
        """Generic form of the exchange step: pack the local top-k, ONE all-gather, unpack, merge.  k > MAX_K with the
        library's own device merge: the gathered payload goes to the merge for sorted lists as it is (the local lists must be
        in result order, which every local search of the library and the oracle emits)."""
        import torch
        import torch.distributed as dist

        if self.world == 1:
            return s, i
        backend = dist.get_backend(self.group)
        as_numpy = not isinstance(s, torch.Tensor)
        if as_numpy:
            s, i = torch.from_numpy(np.ascontiguousarray(s)), torch.from_numpy(np.ascontiguousarray(i))
        home = s.device
        if (backend == "nccl" or self._device_merge) and not s.is_cuda:
            home = torch.device(f"cuda:{self.local.device}" if self.local is not None else "cuda")
            s, i = s.to(home), i.to(home)
        packed = pack_topk(s, i)
        if backend == "gloo" and packed.is_cuda:
            packed = packed.cpu()  # rehearsal / CPU clusters: gloo moves host memory; RCCL takes the device tensor
        nq = packed.shape[0]
        # rank-major concatenation along dim 0 (the layout both RCCL and gloo accept)
        gathered = torch.empty((self.world * nq,) + tuple(packed.shape[1:]), dtype=torch.int64, device=packed.device)
        dist.all_gather_into_tensor(gathered, packed, group=self.group)  # the ONE collective of the path
        if gathered.device != home:
            gathered = gathered.to(home)
        if self._device_merge and k > _lib.MAX_K:
            from .index import merge_topk_sorted_packed

            out_s, out_i = merge_topk_sorted_packed(gathered, nq, self.world, k, metric)
        else:
            cs, ci = unpack_gathered(gathered.view((self.world, nq) + tuple(packed.shape[1:])), self.world)
            out_s, out_i = self._merge(cs, ci, self.world, k, metric)
        if as_numpy:
            return out_s.cpu().numpy(), out_i.cpu().numpy()
        return out_s, out_i
