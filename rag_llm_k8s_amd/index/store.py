"""Document store = vector index + chunk metadata, with the reference's on-disk layout.

Reference behaviour and its fixes:
  ensure_index_exists / update_index / search_documents   /root/reference/llm/rag.py:57-86,114-120
  * index + metadata re-read from disk on every request    -> kept resident (HBM), reloaded
    only if the files on disk change (mtime check);
  * unlocked read-modify-write of both files               -> single writer lock + atomic
    os.replace snapshots, so readers never see torn files; an /upload_pdf append returns as soon
    as the vectors are in HBM and the snapshot is written by a background thread (the state is
    copied under the lock, the file I/O runs outside it; bursts of appends coalesce into one
    write), so a 1M x 1024 index (4 GB) is not rewritten on the request path;
  * faiss label -1 mapped to metadata[-1] (last chunk)     -> -1 results are dropped, making the
    "No relevant information found" branch reachable;
  * startup re-ingest duplicates chunks                    -> idempotent by (filename, chunk_id)
    unless reingest_append=True (legacy behaviour);
  * a document can never be removed, replaced or excluded  -> delete(filename) / add(replace=True) and
    search(filters=...). A delete clears the chunks' bits in a LIVE BITMAP (a tombstone): the very next
    search runs masked (the kernels' top-k over the rows a per-query bitmap allows) and no longer sees
    them. The next snapshot first COMPACTS (index.compact + metadata filtered, bitmap reset), so the
    files on disk are always plain reference-format files of exactly the live chunks and the resident
    ids stay aligned with them. A filename filter is one more bitmap row, ANDed with the live one.
"""
from __future__ import annotations

import contextlib
import logging
import os
import threading
import time

import numpy as np

from ..utils import faults, metrics
from .faiss_io import load_metadata, read_index, save_metadata
from .flat import FlatL2Index, pack_masks

log = logging.getLogger(__name__)


class DocumentStore:
    def __init__(self, index_path, dim, device="cpu", index_type="flat", ivf_nlist=1024, ivf_nprobe=32,
                 recovery="rebuild", shard=None, lexical=False, hybrid_candidates=32, bm25_k1=1.2, bm25_b=0.75,
                 rrf_k=60.0):
        """lexical=True: the store also owns a LexicalIndex (index/lexical.py, BM25 over the chunk texts, row i =
        metadata entry i) kept in step with the dense index under _wlock; search(texts=...) then fuses the two
        result lists by reciprocal rank (hybrid_candidates deep each, BM25 k1 / b, fusion constant rrf_k). It is
        not persisted: load() rebuilds it from the metadata texts.
        shard = (group, rank, world): INDEX_SHARDED tensor-parallel mode -- this rank keeps the rows
        g % world == rank of the index (parallel/dp.py ShardedFlatIndex) in `<index_path>.shard<r>of<W>`
        (a faiss IxF2 file of its rows); every rank keeps the full metadata list, rank 0 persists it.
        search() is then a collective (all ranks call it together, followers with no queries)."""
        self.sharded = shard is not None
        self.shard = shard
        if lexical and self.sharded:
            raise ValueError(self.SHARDED_REFUSAL % "hybrid (lexical) search")
        if lexical and not 1 <= int(hybrid_candidates) <= 64:
            raise ValueError("hybrid_candidates must be in 1..64 (the width of the search kernels' top lists)")
        if lexical and not (float(bm25_k1) >= 0 and 0 <= float(bm25_b) <= 1 and float(rrf_k) > 0):
            raise ValueError("hybrid search needs bm25_k1 >= 0, 0 <= bm25_b <= 1 and rrf_k > 0")
        self.hybrid_candidates = int(hybrid_candidates)
        self.bm25_k1, self.bm25_b, self.rrf_k = float(bm25_k1), float(bm25_b), float(rrf_k)
        self.index_path = index_path
        self.index_file = index_path if shard is None else "%s.shard%dof%d" % (index_path, shard[1], shard[2])
        self.persist_meta = shard is None or shard[1] == 0
        self.recovery = recovery  # rebuild: quarantine an unreadable index and start empty | fail
        self.meta_path = index_path + ".metadata"
        self.dim = dim
        self.device = device
        self.index_type = index_type
        self.ivf_nlist, self.ivf_nprobe = ivf_nlist, ivf_nprobe
        self.index = self._new_index()
        self.lexical = self._new_lexical() if lexical else None
        self.metadata = []
        self._keys = set()
        self._wlock = threading.RLock()
        self._mtimes = None
        self.recovered = None
        self._dirty = False
        self._writing = 0  # snapshot writes in flight (their file replacements are not "other writers")
        self._persister = None
        self._persist_error = None
        self._reset_live()

    def _reset_live(self):
        """No tombstones: every metadata entry is live (state after a load or a compaction)."""
        self._live = None  # bool [len(metadata)] once a chunk was deleted; None = all live
        self._dead = 0     # tombstoned chunks still in the index
        self._by_file = None  # filename -> ids of its chunks (cache; rebuilt after any change)

    def _new_index(self):
        if self.sharded:
            if self.index_type != "flat":
                raise ValueError("INDEX_SHARDED supports the flat index only")
            from ..parallel.dp import ShardedFlatIndex

            return ShardedFlatIndex(self.dim, device=self.device, group=self.shard[0])
        if self.index_type == "ivf":
            from .ivf import IVFFlatIndex

            return IVFFlatIndex(self.dim, device=self.device, nlist=self.ivf_nlist, nprobe=self.ivf_nprobe)
        return FlatL2Index(self.dim, device=self.device)

    def _new_lexical(self, meta=()):
        """A LexicalIndex of the metadata entries' texts (an entry without one is an empty document)."""
        from .lexical import LexicalIndex, doc_text

        lex = LexicalIndex(device=self.device)
        if len(meta):
            lex.add([doc_text(m) for m in meta])
        return lex

    # ------------------------------------------------------------------ lifecycle
    def ensure_exists(self):
        """Reference ensure_index_exists(): create an empty index + [] metadata if missing."""
        if not os.path.exists(self.index_file):
            log.info("Faiss index not found. Creating a new one.")
            self.persist()
        else:
            log.info("Faiss index found.")
            try:
                self.load()
            except Exception as e:
                if self.recovery != "rebuild":
                    raise
                self._quarantine(e)
                self.persist()
        return self

    def _quarantine(self, err):
        """Move an unreadable index (+ metadata) aside and start empty; the startup directory
        ingest then rebuilds it from PDF_DIR. The reference would crash-loop instead."""
        tag = ".corrupt-%d" % int(time.time())
        for p in (self.index_file, self.meta_path) if self.persist_meta else (self.index_file,):
            if os.path.exists(p):
                os.replace(p, p + tag)
        log.error("index %s unreadable (%s); moved aside as *%s, starting empty", self.index_file, err, tag)
        self.index = self._new_index()
        if self.lexical is not None:
            self.lexical = self._new_lexical()
        self.metadata = []
        self._keys = set()
        self._reset_live()
        self.recovered = tag

    def _disk_mtimes(self):
        try:
            return (os.path.getmtime(self.index_file), os.path.getmtime(self.meta_path))
        except OSError:
            return None

    def load(self):
        faults.check("index_read_error", self.index_file)
        r = read_index(self.index_file)
        meta = load_metadata(self.meta_path) if os.path.exists(self.meta_path) else []
        if r["d"] != self.dim:
            raise ValueError("index dimension %d != embedder dimension %d" % (r["d"], self.dim))
        idx = self._new_index()
        if self.sharded:  # this rank's rows only; the global count comes from the metadata
            world, rank = self.shard[2], self.shard[1]
            if r["ntotal"] != len(range(rank, len(meta), world)):
                raise ValueError("shard has %d vectors, metadata implies %d" % (r["ntotal"], len(range(rank, len(meta), world))))
            idx.load_local(r["xb"] if r["ntotal"] else None, len(meta))
            self.index, self.metadata = idx, list(meta)
            self._keys = {(m.get("filename"), m.get("chunk_id")) for m in self.metadata if isinstance(m, dict)}
            self._reset_live()
            self._mtimes = self._disk_mtimes()
            return
        if len(meta) != r["ntotal"]:
            raise ValueError("index has %d vectors but metadata %d entries (torn write?)" % (r["ntotal"], len(meta)))
        if r["type"] == "flat":
            if r["ntotal"]:
                if self.index_type == "ivf":
                    idx.train(r["xb"])
                idx.add(r["xb"])
        else:
            from .ivf import IVFFlatIndex

            idx = IVFFlatIndex.from_lists(r, device=self.device)
        lex = self._new_lexical(meta) if self.lexical is not None else None  # not persisted: rebuilt from the texts
        self.index = idx
        self.lexical = lex
        self.metadata = list(meta)
        self._keys = {(m.get("filename"), m.get("chunk_id")) for m in self.metadata if isinstance(m, dict)}
        self._reset_live()
        self._mtimes = self._disk_mtimes()

    def maybe_reload(self):
        """Pick up index files replaced on disk by another writer (e.g. an offline ingest job)."""
        if self.sharded:  # a reload would have to be collective; shards change only through ingest jobs
            return
        m = self._disk_mtimes()
        if m is None or self._mtimes is None or m == self._mtimes:
            return
        with self._wlock:
            # Our own snapshot writer replaces the files outside the lock: while it runs (or while
            # appends are waiting for it) the disk lags HBM, and reloading would drop those appends.
            if self._writing or self._dirty:
                return
            m = self._disk_mtimes()  # re-check under the lock: a write may have finished meanwhile
            if m is None or m == self._mtimes:
                return
            try:
                self.load()
            except Exception as e:  # keep serving the resident snapshot; retry on the next change
                log.warning("index on disk changed but is unreadable (%s); keeping the resident copy", e)
                self._mtimes = m

    def _compact(self):
        """Drop the tombstoned chunks from the index and the metadata (caller holds _wlock): ids are
        renumbered by rank among the live ones, on both sides, and the live bitmap is reset."""
        if not self._dead:
            return
        keep = np.nonzero(self._live)[0]
        self.index.compact(keep)
        if self.lexical is not None:
            self.lexical.compact(keep)
        self.metadata = [self.metadata[i] for i in keep.tolist()]  # a new list: searches in flight keep theirs
        self._reset_live()
        metrics.inc("index_compactions")
        metrics.set_gauge("index_tombstones", 0)
        metrics.set_gauge("index", self.index.ntotal)
        log.info("Index compacted. Total vectors: %d", self.index.ntotal)

    def _snapshot(self):
        """(index writer, metadata copy) of the current state, compacted first, so the files only ever
        hold live chunks; caller holds _wlock."""
        self._compact()
        return self.index.snapshot_writer(), list(self.metadata)

    def _write(self, writer, meta):
        """Write a snapshot. The caller registered it in _writing under _wlock; the mtimes the store
        itself produced are recorded under the lock, so maybe_reload never mistakes them for another
        writer's files."""
        try:
            writer(self.index_file)
            if self.persist_meta:
                save_metadata(self.meta_path, meta)
        finally:
            with self._wlock:
                self._mtimes = self._disk_mtimes()
                self._writing -= 1

    def persist(self):
        """Synchronous snapshot (startup / directory ingest / shutdown)."""
        with self._wlock:
            writer, meta = self._snapshot()
            self._dirty = False
            self._writing += 1
            self._write(writer, meta)

    def persist_async(self):
        """Schedule a background snapshot; appends made meanwhile are folded into the same write."""
        with self._wlock:
            self._dirty = True
            if self._persister is None:  # cleared under the lock by the writer when it exits
                self._persister = threading.Thread(target=self._persist_loop, name="index-snapshot", daemon=True)
                self._persister.start()

    def _persist_loop(self):
        clean = False
        try:
            while True:
                with self._wlock:
                    if not self._dirty:
                        # deregister while still holding the lock: an add() after this point sees
                        # _persister None and starts a new writer (no lost wake-up)
                        self._persister = None
                        clean = True
                        return
                    # host copy under the lock (consistent vectors + metadata); a failure here (e.g. the
                    # device copy after a GPU fault) leaves _dirty set, so the next append retries
                    writer, meta = self._snapshot()
                    self._dirty = False
                    self._writing += 1
                try:
                    self._write(writer, meta)  # file I/O outside the lock: searches and appends continue
                except Exception as e:  # keep serving from HBM; the next append retries the snapshot
                    self._persist_error = e
                    log.error("index snapshot failed: %s", e)
        except Exception as e:
            self._persist_error = e
            log.error("index snapshot thread failed: %s", e)
        finally:
            if not clean:  # any abnormal exit deregisters too: the next persist_async starts a new writer
                with self._wlock:
                    if self._persister is threading.current_thread():
                        self._persister = None

    def flush(self):
        """Wait until every scheduled snapshot is on disk."""
        t = self._persister
        if t is not None:
            t.join()
        with self._wlock:
            if self._dirty:
                writer, meta = self._snapshot()
                self._dirty = False
                self._writing += 1
                self._write(writer, meta)

    # ------------------------------------------------------------------ writes
    def add(self, vectors, metadata, dedupe=True, persist=True, replace=False):
        """Append vectors + metadata (reference update_index). Returns number added.
        replace: first delete every chunk of the documents named in `metadata`, under the same lock -- no
        search sees neither or both versions of a document."""
        vecs = np.asarray(vectors.cpu() if hasattr(vectors, "cpu") else vectors, dtype=np.float32)
        if vecs.ndim == 1:
            vecs = vecs.reshape(1, -1)
        if replace and self.sharded:
            raise ValueError(self.SHARDED_REFUSAL % "replace")
        with self._wlock:
            if replace:
                for fn in dict.fromkeys(m["filename"] for m in metadata):
                    self.delete(fn, persist=False)
            keep = list(range(len(metadata)))
            if dedupe:
                keep = [i for i, m in enumerate(metadata) if (m["filename"], m["chunk_id"]) not in self._keys]
            if keep:
                if self.index_type == "ivf" and not self.index.is_trained:
                    self.index.train(vecs[keep])
                self.index.add(vecs[keep])
                if self.lexical is not None:
                    from .lexical import doc_text

                    self.lexical.add([doc_text(metadata[i]) for i in keep])
                for i in keep:
                    self.metadata.append(metadata[i])
                    self._keys.add((metadata[i]["filename"], metadata[i]["chunk_id"]))
                if self._live is not None:
                    self._live = np.concatenate([self._live, np.ones(len(keep), dtype=bool)])
                self._by_file = None
            if keep or (replace and self._dead):
                if persist:
                    self.persist_async()
            log.info("Index updated. Total vectors: %d, Dimension: %d", self.index.ntotal, self.dim)
            return len(keep)

    SHARDED_REFUSAL = ("document %s is not supported on a row-sharded index (INDEX_SHARDED): the shards would "
                       "have to be re-balanced and the filter broadcast to every rank")

    def delete(self, filename, persist=True):
        """Remove every chunk of a document. Returns the number of chunks removed (0: unknown document).
        The chunks' bits are cleared in the live bitmap (they are gone for the very next search), their
        (filename, chunk_id) keys dropped (the document can be uploaded again), and a snapshot -- which
        compacts index and metadata first -- is scheduled."""
        if self.sharded:
            raise ValueError(self.SHARDED_REFUSAL % "delete")
        with self._wlock:
            ids = self._file_ids().get(filename)
            if ids is not None and self._live is not None:
                ids = ids[self._live[ids]]
            if ids is None or not len(ids):
                return 0
            if self._live is None:
                self._live = np.ones(len(self.metadata), dtype=bool)
            self._live[ids] = False
            self._dead += len(ids)
            for i in ids.tolist():
                self._keys.discard((filename, self.metadata[i].get("chunk_id")))
            metrics.inc("index_chunks_deleted", len(ids))
            metrics.set_gauge("index_tombstones", self._dead)
            log.info("Deleted %d chunks of %s. Live vectors: %d", len(ids), filename, self.index.ntotal - self._dead)
            if persist:
                self.persist_async()
            return int(len(ids))

    # ------------------------------------------------------------------ reads
    def _file_ids(self):
        """filename -> int64 ids of its chunks, tombstoned ones included (caller holds _wlock)."""
        if self._by_file is None:
            by = {}
            for i, m in enumerate(self.metadata):
                if isinstance(m, dict):
                    by.setdefault(m.get("filename"), []).append(i)
            self._by_file = {fn: np.asarray(v, dtype=np.int64) for fn, v in by.items()}
        return self._by_file

    def documents(self):
        """[{"filename", "chunks"}] of the live chunks, in first-seen order."""
        with self._wlock:
            out = []
            for fn, ids in self._file_ids().items():
                n = int(len(ids) if self._live is None else self._live[ids].sum())
                if n:
                    out.append({"filename": fn, "chunks": n})
            return out

    def _filter_masks(self, filters, nq):
        """Per-query filename filters -> (bitmap rows uint32 [n_rows, words], qmask int32 [nq]) for one masked
        search, or (None, None) when nothing restricts it. One row per DISTINCT filter of the batch, each
        ANDed with the live bitmap; unfiltered queries use the live row while tombstones exist, else -1.
        Caller holds _wlock."""
        filters = list(filters) if filters is not None else [None] * nq
        if len(filters) != nq:
            raise ValueError("filters: one entry (None or filenames) per query")
        if self._dead == 0 and all(f is None for f in filters):
            return None, None
        n = len(self.metadata)
        live = self._live if self._live is not None else np.ones(n, dtype=bool)
        rows, row_of, qmask = [], {}, np.full(nq, -1, dtype=np.int32)
        for j, f in enumerate(filters):
            if f is None and self._dead == 0:
                continue
            key = None if f is None else frozenset([f] if isinstance(f, str) else f)
            if key not in row_of:
                if key is None:
                    al = live
                else:
                    al = np.zeros(n, dtype=bool)
                    for fn in key:
                        ids = self._file_ids().get(fn)
                        if ids is not None:
                            al[ids] = True
                    al &= live
                row_of[key] = len(rows)
                rows.append(al)
            qmask[j] = row_of[key]
        return pack_masks(np.stack(rows)), qmask

    def search(self, qvecs, k, filters=None, texts=None, trace=None):
        """Batched search -> list (per query) of [(metadata, squared_l2)] ascending, -1 dropped.
        filters: per query None or a collection of filenames the results must come from (a filter naming
        no known document yields no results for that query).
        texts (a store with lexical=True): per query its text, or None for a query that stays dense-only. A
        query with a text gets the hybrid result (_search_hybrid); the others are searched exactly as without
        `texts`, in a call of their own. trace (utils.metrics.Trace): receives the spans "lexical" and "fuse"."""
        if texts is not None and any(t is not None for t in texts):
            return self._search_mixed(qvecs, k, filters, list(texts), trace)
        if self.sharded and filters is not None and any(f is not None for f in filters):
            raise ValueError(self.SHARDED_REFUSAL % "filtering")
        with self._wlock:  # consistent (index, metadata) pair: an append cannot land in between
            nq = int(np.prod(np.shape(qvecs))) // self.dim if (filters is not None or self._dead) else 0
            masks, qmask = self._filter_masks(filters, nq) if nq else (None, None)
            if masks is None:
                D, I = self.index.search(qvecs, k)
            else:
                D, I = self.index.search(qvecs, k, masks=masks, qmask=qmask)
            meta = self.metadata
            n = len(meta)
        out = []
        for drow, irow in zip(D.tolist(), I.tolist()):
            res = []
            for d, i in zip(drow, irow):
                if 0 <= i < n:
                    res.append((meta[i], float(d)))
            out.append(res)
        return out

    def _search_mixed(self, qvecs, k, filters, texts, trace=None):
        """search() of a batch in which some queries carry a text: those go through _search_hybrid together,
        the rest through the plain search together; the results return in the batch's order."""
        if self.lexical is None:
            raise ValueError("hybrid search needs a store built with lexical=True")
        import torch

        q = torch.as_tensor(np.asarray(qvecs.cpu() if hasattr(qvecs, "cpu") else qvecs, dtype=np.float32))
        q = q.reshape(-1, self.dim)
        if len(texts) != q.shape[0]:
            raise ValueError("texts: one entry (a string or None) per query")
        filters = list(filters) if filters is not None else [None] * len(texts)
        if len(filters) != len(texts):
            raise ValueError("filters: one entry (None or filenames) per query")
        hyb = [i for i, t in enumerate(texts) if t is not None]
        rest = [i for i, t in enumerate(texts) if t is None]
        out = [None] * len(texts)
        for i, r in zip(hyb, self._search_hybrid(q[hyb], k, [filters[i] for i in hyb], [texts[i] for i in hyb],
                                                    trace)):
            out[i] = r
        if rest:
            fr = [filters[i] for i in rest]
            for i, r in zip(rest, self.search(q[rest], k, filters=fr if any(f is not None for f in fr) else None)):
                out[i] = r
        return out

    def _search_hybrid(self, q, k, filters, texts, trace=None):
        """Dense search and BM25 search, both hybrid_candidates deep and under the same per-query masks, fused by
        reciprocal rank: fused(d) = sum over the lists holding d of 1 / (rrf_k + rank), ordered by fused
        descending then id ascending, cut to k. The tuples stay (metadata, squared_l2): a chunk of the dense list
        keeps the distance the search returned, a lexical-only chunk gets index.distances(). The metadata dicts
        are copies that also carry dense_rank / lexical_rank (1-based, None = not in that list) and
        lexical_score (None likewise)."""
        from .lexical import rrf_fuse

        span = trace.span if trace is not None else (lambda stage: contextlib.nullcontext())
        depth = self.hybrid_candidates
        nq = q.shape[0]
        with self._wlock:
            masks, qmask = self._filter_masks(filters, nq)
            if masks is None:
                D, I = self.index.search(q, depth)
            else:
                D, I = self.index.search(q, depth, masks=masks, qmask=qmask)
            live = self._live if self._dead else None
            with span("lexical"):
                S, L = self.lexical.search(texts, depth, k1=self.bm25_k1, b=self.bm25_b, masks=masks, qmask=qmask,
                                           live=live)
            with span("fuse"):
                meta = self.metadata
                n = len(meta)
                D, I, S, L = D.tolist(), I.tolist(), S.tolist(), L.tolist()
                picked, need_q, need_id = [], [], []
                for j in range(nq):
                    dense = {i: (r + 1, d) for r, (d, i) in enumerate((d, i) for d, i in zip(D[j], I[j]) if 0 <= i < n)}
                    lex = {i: (r + 1, s) for r, (s, i) in enumerate((s, i) for s, i in zip(S[j], L[j]) if 0 <= i < n)}
                    rows = []
                    for i, _ in rrf_fuse([list(dense), list(lex)], self.rrf_k, k):
                        if i not in dense:
                            need_q.append(j)
                            need_id.append(i)
                        rows.append((i, dense.get(i), lex.get(i)))
                    picked.append(rows)
                extra = {}
                if need_id:  # lexical-only chunks: their real distance, one gather for the whole batch
                    dist = self.index.distances(q[need_q], need_id).tolist()
                    extra = {(j, i): d for j, i, d in zip(need_q, need_id, dist)}
        out = []
        for j, rows in enumerate(picked):
            res = []
            for i, de, le in rows:
                m = dict(meta[i]) if isinstance(meta[i], dict) else {"text": ""}
                m["dense_rank"] = de[0] if de else None
                m["lexical_rank"] = le[0] if le else None
                m["lexical_score"] = float(le[1]) if le else None
                res.append((m, float(de[1]) if de else float(extra[(j, i)])))
            out.append(res)
        return out

    def info(self):
        with self._wlock:
            if not self._dead:
                return {"total_vectors": int(self.index.ntotal), "dimension": int(self.dim),
                        "total_chunks": len(self.metadata),
                        "sample_chunks": self.metadata[:5] if self.metadata else []}
            live = [self.metadata[i] for i in np.nonzero(self._live)[0][:5].tolist()]  # tombstones not counted
            return {"total_vectors": int(self.index.ntotal) - self._dead, "dimension": int(self.dim),
                    "total_chunks": len(self.metadata) - self._dead, "sample_chunks": live}
