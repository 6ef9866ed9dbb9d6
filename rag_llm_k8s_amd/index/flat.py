"""HBM-resident exact L2 index (faiss IndexFlatL2 semantics) + IVF-Flat.

Reference: faiss.IndexFlatL2(1024), index.add, index.search(q, k) (/root/reference/llm/rag.py:61,80,116),
with the whole index re-read from the PVC on every request (:153-155).

Here the vectors live in GPU memory in a column-major [d][capacity] fp32 layout (fully
coalesced streaming in the search kernel), capacity doubles on growth, and search is
the gfx950 l2_block_topk + topk_merge kernels. On CPU the same class uses torch.
Results follow faiss: squared L2, ascending, (-1, FLT_MAX) padding when k > ntotal.
"""
from __future__ import annotations

import threading

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------- filtered search: id bitmaps
# masks: uint32 [n_masks, words], bit (id & 31) of word (id >> 5) set = the id may be returned; an id
# past 32 * words is not allowed. qmask: int [nq], the bitmap row of each query, -1 = unfiltered.
def pack_masks(allowed) -> np.ndarray:
    """bool [n_masks, n_ids] -> uint32 [n_masks, ceil(n_ids / 32)] bitmap rows."""
    a = np.atleast_2d(np.asarray(allowed, dtype=bool))
    pad = (-a.shape[1]) % 32
    if pad:
        a = np.concatenate([a, np.zeros((a.shape[0], pad), bool)], axis=1)
    return np.ascontiguousarray(np.packbits(a, axis=1, bitorder="little")).view(np.uint32).reshape(a.shape[0], -1)


def masks_host(masks) -> np.ndarray:
    """Bitmap rows (numpy or torch, int32 or uint32) as a uint32 numpy array [n_masks, words]."""
    if isinstance(masks, torch.Tensor):
        masks = masks.detach().cpu().view(torch.int32).numpy()
    m = np.ascontiguousarray(masks)
    if m.dtype != np.uint32:
        if m.dtype != np.int32:
            raise ValueError("masks must be uint32 / int32 words")
        m = m.view(np.uint32)
    if m.ndim != 2:
        raise ValueError("masks must be [n_masks, words]")
    return m


def masks_device(masks, device) -> torch.Tensor:
    """Bitmap rows as the int32 device tensor the kernels take (a device tensor passes through)."""
    if isinstance(masks, torch.Tensor) and masks.is_cuda:
        return masks
    return torch.from_numpy(masks_host(masks).view(np.int32)).to(device)


def qmask_host(qmask, nq, n_masks) -> np.ndarray:
    qm = np.asarray(qmask.cpu() if isinstance(qmask, torch.Tensor) else qmask).astype(np.int64).reshape(-1)
    if qm.shape[0] != nq or (nq and (qm.min() < -1 or qm.max() >= n_masks)):
        raise ValueError("qmask: one entry in [-1, n_masks) per query")
    return qm


def mask_allowed(masks, qmask, ids) -> np.ndarray:
    """bool [nq, len(ids)]: may query j return ids[i]? (host form of the kernels' test)"""
    m = masks_host(masks)
    ids = np.asarray(ids, dtype=np.int64)
    if qmask is None or masks is None:
        raise ValueError("masks and qmask go together")
    qm = qmask_host(qmask, len(qmask), m.shape[0])
    inb = (ids >= 0) & (ids < 32 * m.shape[1])
    word, bit = np.where(inb, ids >> 5, 0), (ids & 31).astype(np.uint32)
    out = np.ones((qm.shape[0], ids.shape[0]), dtype=bool)
    for r in np.unique(qm[qm >= 0]):
        row = (((m[r][word] >> bit) & 1).astype(bool) & inb) if m.shape[1] else np.zeros(ids.shape[0], bool)
        out[qm == r] = row
    return out


def pair_sqdist(x, q) -> torch.Tensor:
    """fp32 sum((x[j] - q[j]) ** 2) per row (the indexes' distances())."""
    df = x.float() - q.float()
    return (df * df).sum(1)


COMPACT_PIECE_FLOATS = 4 << 20  # FlatL2Index.compact on the device moves rows in pieces of <= 16 MB


def check_keep(keep, ntotal) -> np.ndarray:
    """compact(keep): the ids to keep, strictly ascending, within [0, ntotal)."""
    keep = np.asarray(keep, dtype=np.int64).reshape(-1)
    if len(keep) and (keep[0] < 0 or keep[-1] >= ntotal or bool((np.diff(keep) <= 0).any())):
        raise ValueError("keep must be strictly ascending ids within [0, ntotal)")
    return keep


class FlatL2Index:
    def __init__(self, d: int, device="cpu", capacity: int = 1024):
        self.d = int(d)
        self.device = torch.device(device)
        self.ntotal = 0
        self.metric = 1
        self._cap = max(1, capacity)
        self._lock = threading.RLock()
        if self.device.type == "cuda":
            from ..ops import native

            self._n = native
            self._xt = torch.zeros(self.d, self._cap, dtype=torch.float32, device=self.device)
        else:
            self._n = None
            self._xb = torch.zeros(self._cap, self.d, dtype=torch.float32)

    # ---------------------------------------------------------------- mutation
    def _grow(self, need):
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap)
        if self._n is not None:
            nxt = torch.zeros(self.d, cap, dtype=torch.float32, device=self.device)
            nxt[:, :self.ntotal] = self._xt[:, :self.ntotal]
            self._xt = nxt
        else:
            nxb = torch.zeros(cap, self.d, dtype=torch.float32)
            nxb[:self.ntotal] = self._xb[:self.ntotal]
            self._xb = nxb
        self._cap = cap

    def add(self, x):
        x = torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x)
        x = x.reshape(-1, self.d).float().contiguous()
        n = x.shape[0]
        if n == 0:
            return
        with self._lock:
            self._grow(self.ntotal + n)
            if self._n is not None:
                self._n.l2_append(self._xt, self._cap, self.ntotal, x.to(self.device))
            else:
                self._xb[self.ntotal:self.ntotal + n] = x
            self.ntotal += n

    def reset(self):
        with self._lock:
            self.ntotal = 0

    def compact(self, keep):
        """Drop every vector whose id is not in `keep` (sorted ids): afterwards the index equals a fresh one
        to which the kept vectors were added in their original order (new id = rank among the kept).
        In place: a kept row only ever moves down, so pieces of rows are gathered (l2_gather) and written
        back (l2_append) in ascending order -- one bounded row-major piece is the only temporary."""
        with self._lock:
            keep = check_keep(keep, self.ntotal)
            m = len(keep)
            if m == self.ntotal:
                return
            if self._n is not None:
                step = max(1, COMPACT_PIECE_FLOATS // self.d)
                idx = torch.from_numpy(keep.astype(np.int32)).to(self.device)
                for i in range(0, m, step):
                    # stream order: the piece is read completely before its (lower) slots are written
                    self._n.l2_append(self._xt, self._cap, i, self._n.l2_gather(self._xt, self._cap, idx[i:i + step]))
            elif m:
                self._xb[:m] = self._xb[torch.from_numpy(keep)]
            self.ntotal = m

    # ---------------------------------------------------------------- query
    def search(self, q, k, masks=None, qmask=None):
        """q: [nq, d] -> (D fp32 [nq,k], I int64 [nq,k]) on the host. masks / qmask: filtered search
        (id bitmaps, see pack_masks) -- query j only returns ids allowed by bitmap row qmask[j]."""
        q = torch.as_tensor(q).reshape(-1, self.d).float().contiguous()
        nq = q.shape[0]
        if nq == 0:
            return torch.zeros(0, k), torch.zeros(0, k, dtype=torch.int64)
        with self._lock:
            if self._n is not None:
                if k > 64:
                    raise ValueError("k <= 64 on the GPU path")
                D, I = self.search_device(q.to(self.device), k, masks, qmask)
                return D.cpu(), I.cpu()
            return self._cpu_search(q, k, masks, qmask)

    def search_device(self, q, k, masks=None, qmask=None):
        """GPU-only: q on device -> (D, I) on device (no host sync without a filter)."""
        with self._lock:
            if masks is None and qmask is None:
                return self._n.l2_search(self._xt, self._cap, self.ntotal, q, k)
            md = masks_device(masks, self.device)
            qm = qmask if isinstance(qmask, torch.Tensor) else torch.from_numpy(np.asarray(qmask, dtype=np.int32))
            return self._n.l2_search(self._xt, self._cap, self.ntotal, q, k, masks=md, qmask=qm.int().contiguous())

    def _cpu_search(self, q, k, masks=None, qmask=None):
        n = self.ntotal
        D = torch.full((q.shape[0], k), FLT_MAX)
        I = torch.full((q.shape[0], k), -1, dtype=torch.int64)
        if n == 0:
            return D, I
        xb = self._xb[:n]
        # faiss' BLAS path: ||x||^2 + ||q||^2 - 2 q.x (clamped at 0), ties -> lower id
        d = (q * q).sum(1, keepdim=True) + (xb * xb).sum(1)[None, :] - 2.0 * (q @ xb.t())
        d = d.clamp_min_(0.0)
        kk = min(k, n)
        if masks is not None or qmask is not None:
            # rows a query may not return sort last (inf; real distances are finite) and become padding
            d[~torch.from_numpy(mask_allowed(masks, qmask, np.arange(n)))] = float("inf")
            dv, di = torch.sort(d, dim=1, stable=True)
            live = dv[:, :kk] != float("inf")
            D[:, :kk] = torch.where(live, dv[:, :kk], D[:, :kk])
            I[:, :kk] = torch.where(live, di[:, :kk], I[:, :kk])
            return D, I
        dv, di = torch.sort(d, dim=1, stable=True)
        D[:, :kk] = dv[:, :kk]
        I[:, :kk] = di[:, :kk]
        return D, I

    def distances(self, q, ids):
        """Squared L2 between query row q[j] and stored vector ids[j], pairwise: q [m, d], ids [m] (each in
        [0, ntotal)) -> fp32 [m] on the host. The rows are gathered (l2_gather on the GPU) and the squares
        summed by torch in fp32 -- the distance of a chunk that entered a result list by another route."""
        q = torch.as_tensor(q).reshape(-1, self.d).float()
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) != q.shape[0]:
            raise ValueError("distances: one id per query row")
        with self._lock:
            if len(ids) and (ids.min() < 0 or ids.max() >= self.ntotal):
                raise ValueError("distances: ids within [0, ntotal)")
            if len(ids) == 0:
                return torch.zeros(0)
            if self._n is not None:
                x = self._n.l2_gather(self._xt, self._cap, torch.from_numpy(ids.astype(np.int32)).to(self.device))
                return pair_sqdist(x, q.to(self.device)).cpu()
            return pair_sqdist(self._xb[torch.from_numpy(ids)], q)

    def reconstruct_all(self) -> np.ndarray:
        with self._lock:
            if self._n is not None:
                return self._xt[:, :self.ntotal].t().contiguous().cpu().numpy()
            return self._xb[:self.ntotal].numpy().copy()

    # ---------------------------------------------------------------- persistence
    def snapshot_writer(self):
        """Host copy of the vectors now; the returned callable writes it (faiss IxF2) atomically."""
        xb = self.reconstruct_all()
        d = self.d

        def write(path):
            from ..runtime import native_rt
            from .faiss_io import atomic_write, write_flat_l2

            rt = native_rt()
            if rt is not None:  # C++ writer: temp file + fsync + rename
                rt.write_flat_index(path, xb.reshape(-1, d))
            else:
                atomic_write(path, lambda f: write_flat_l2(f, xb))
        return write

    def write(self, path):
        self.snapshot_writer()(path)

    @classmethod
    def read(cls, path, device="cpu"):
        from .faiss_io import read_index

        r = read_index(path)
        if r["type"] != "flat":
            raise ValueError("not an IndexFlat file")
        idx = cls(r["d"], device=device, capacity=max(1024, r["ntotal"]))
        if r["ntotal"]:
            idx.add(torch.from_numpy(r["xb"]))
        return idx

    def memory_bytes(self):
        return self.d * self._cap * 4
