"""Selector -- "search only these rows": the row subset a filtered search_wide / range_search looks at.

A selector is a bitmap in the faiss IDSelectorBitmap layout: a uint8 tensor in which row i is selected iff
bits[i >> 3] >> (i & 7) & 1 (what np.packbits(mask, bitorder="little") produces), plus the number of rows it speaks about
(nbits).  It is built once, lives on the GPU and is reusable across calls; one selector applies to all queries of a call.
Packing is plumbing and uses torch ops on the selector's device; the searches read the bitmap in libmips_hip.so.
"""
from __future__ import annotations

import numpy as np


def is_id_list(sel) -> bool:
    """Does `sel` list row ids (an integer array, tensor or sequence) rather than flag rows (bool mask, uint8 bitmap)?"""
    import torch

    if isinstance(sel, torch.Tensor):
        return sel.dtype not in (torch.bool, torch.uint8) and not sel.dtype.is_floating_point
    if isinstance(sel, np.ndarray):
        return sel.dtype.kind in "iu" and sel.dtype != np.uint8
    return isinstance(sel, (list, tuple)) and (len(sel) == 0 or not isinstance(sel[0], (bool, np.bool_)))


class Selector:
    def __init__(self, bits, nbits: int):
        """bits: uint8 tensor of (nbits + 7) // 8 bytes whose bits at and past nbits are clear (use the from_* constructors)."""
        self.bits = bits
        self.nbits = int(nbits)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def _device(device):
        import torch

        if device is None:
            return torch.device("cuda", torch.cuda.current_device())
        if isinstance(device, int):
            return torch.device("cuda", device)
        return torch.device(device)

    @classmethod
    def from_mask(cls, mask, device=None) -> "Selector":
        """mask: bool array / tensor of one entry per row (True = selected)."""
        import torch

        dev = cls._device(device)
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask).astype(np.bool_)))
        m = m.to(dev).reshape(-1) != 0
        nbits = int(m.shape[0])
        nbytes = (nbits + 7) // 8
        padded = torch.zeros(nbytes * 8, dtype=torch.uint8, device=dev)
        padded[:nbits] = m.to(torch.uint8)
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
        bits = (padded.view(nbytes, 8) * weights).sum(dim=1, dtype=torch.uint8)
        return cls(bits.contiguous(), nbits)

    @classmethod
    def from_ids(cls, ids, nbits: int, device=None) -> "Selector":
        """The rows listed in ids (int array / tensor; duplicates allowed) of an index of nbits rows."""
        import torch

        dev = cls._device(device)
        nbits = int(nbits)
        t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1)))
        t = t.to(dev).reshape(-1).long()
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= nbits):
            raise ValueError(f"Selector.from_ids: an id lies outside [0, {nbits})")
        mask = torch.zeros(nbits, dtype=torch.bool, device=dev)
        mask[t] = True
        return cls.from_mask(mask, device=dev)

    @classmethod
    def from_range(cls, lo: int, hi: int, nbits: int, device=None) -> "Selector":
        """Rows lo <= i < hi (clipped to [0, nbits))."""
        import torch

        dev = cls._device(device)
        r = torch.arange(int(nbits), device=dev)
        return cls.from_mask((r >= int(lo)) & (r < int(hi)), device=dev)

    @classmethod
    def from_bitmap(cls, bitmap, nbits: int, device=None) -> "Selector":
        """An existing bitmap (uint8 array / tensor of at least (nbits + 7) // 8 bytes); bits at and past nbits are dropped."""
        import torch

        dev = cls._device(device)
        nbits = int(nbits)
        nbytes = (nbits + 7) // 8
        b = bitmap if isinstance(bitmap, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(bitmap, dtype=np.uint8).reshape(-1)))
        if b.dtype != torch.uint8 or b.numel() < nbytes:
            raise ValueError(f"Selector.from_bitmap: {nbits} bits need a uint8 bitmap of at least {nbytes} bytes")
        return cls(b.reshape(-1)[:nbytes].to(dev).clone(), nbits)._clear_tail()

    def _clear_tail(self) -> "Selector":
        if self.nbits & 7:
            self.bits[-1] &= (1 << (self.nbits & 7)) - 1
        return self

    def invert(self) -> "Selector":
        """A new selector of the rows this one leaves out."""
        return Selector(~self.bits, self.nbits)._clear_tail()

    # ------------------------------------------------------------------ views
    def to(self, device) -> "Selector":
        dev = self._device(device)
        return self if self.bits.device == dev else Selector(self.bits.to(dev), self.nbits)

    def numpy(self) -> np.ndarray:
        """The bitmap as a host uint8 array (np.packbits(mask, bitorder="little"))."""
        return self.bits.cpu().numpy()

    def mask(self) -> np.ndarray:
        """One bool per row, on the host."""
        return np.unpackbits(self.numpy(), bitorder="little")[: self.nbits].astype(np.bool_)

    def count(self) -> int:
        return int(self.mask().sum())

    def __len__(self) -> int:
        return self.nbits

    def __repr__(self) -> str:
        return f"Selector(nbits={self.nbits}, device={self.bits.device})"
