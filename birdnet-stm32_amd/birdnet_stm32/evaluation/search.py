"""Query by example: the nearest embeddings of query clips in archives written by ``embed``.

``search_reference`` is the specification in numpy; ``EmbeddingIndex.search`` runs the same search on the device (``csrc/bn_search.hip``,
C ABI ``bn_search_inv_norms`` / ``bn_search_topk``) and is tested against it for equality.

Scores.  ``dot[q, i]`` is the float32 inner product (summation order free); ``n[i]`` the float32 sum of squares;
``inv[i] = fl(1 / fl(sqrt(n[i])))`` with correctly rounded square root and division, 0 for a zero row.  ``"cosine"`` is
``fl(fl(dot * inv_q) * inv_row)``, ``"dot"`` is ``dot``.  An int8 database holds the raw bytes of ``embed --dtype int8``: dot and sums of
squares are exact int32 over ``byte - zero_point``, rounded once to float32, and the cosine is formed from them in the same way; the
Python layer multiplies a reported int8 dot score by ``fl(scale * scale)``.

Order.  Per query by score descending and, among equal scores, by row index ascending: a total order, so the best k are one set however
the work is split.  Fewer than k qualifying rows leave ``idx = -1`` and ``score = -inf``.  With groups a row of the query's own group does
not qualify (the command uses the file a query came from).  Inputs are finite.
"""

from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

METRICS = ("cosine", "dot")
MAX_K, MAX_D = 128, 2048   # BN_SEARCH_MAX_K / BN_SEARCH_MAX_D (include/birdnet_hip.h)
QUERY_POOLINGS = ("none", "avg", "max")


def _check_metric(metric: str) -> str:
    metric = str(metric).lower()
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    return metric


def inv_norms_reference(rows: np.ndarray, zero_point: int = 0) -> np.ndarray:
    """``inv`` of the module docstring for float32 rows or int8 bytes with their zero point."""
    rows = np.asarray(rows)
    if rows.dtype == np.int8:
        x = rows.astype(np.int64) - int(zero_point)
        n = (x * x).sum(axis=1).astype(np.float32)
    else:
        x = rows.astype(np.float32)
        n = (x * x).sum(axis=1, dtype=np.float32)
    inv = np.zeros(n.shape, np.float32)
    nz = n != 0
    inv[nz] = np.float32(1.0) / np.sqrt(n[nz])
    return inv


def order_topk(score: np.ndarray, idx: np.ndarray, qualifies: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """The best ``k`` of the candidates of every row of ``score`` / ``idx`` ([Q, M]) under the total order, padded with -1 / -inf."""
    Q, M = score.shape
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    for q in range(Q):
        cand = np.flatnonzero(qualifies[q])
        s, i = score[q, cand], idx[q, cand]
        if cand.size > k:   # drop what cannot be among the best k before the full sort (ties of the k-th score all stay)
            kth = np.partition(s, cand.size - k)[cand.size - k]
            keep = s >= kth
            s, i = s[keep], i[keep]
        order = np.lexsort((i, -s.astype(np.float64)))[:k]
        out_i[q, : order.size] = i[order]
        out_s[q, : order.size] = s[order]
    return out_i, out_s


def search_reference(db, queries, k: int = 10, metric: str = "cosine", *, zero_point: int = 0, db_group=None, query_group=None):
    """``(idx [Q, k] int64, score [Q, k] float32)``: the specification of the module docstring."""
    metric = _check_metric(metric)
    db, queries = np.asarray(db), np.asarray(queries)
    if db.ndim != 2 or queries.ndim != 2 or db.shape[1] != queries.shape[1]:
        raise ValueError(f"db {db.shape} and queries {queries.shape} must be [N, D] and [Q, D]")
    if (db.dtype == np.int8) != (queries.dtype == np.int8):
        raise ValueError("queries have the database's dtype")
    if k < 1:
        raise ValueError("k must be >= 1")
    N, Q = db.shape[0], queries.shape[0]
    i8 = db.dtype == np.int8
    if i8:
        x = db.astype(np.int64) - int(zero_point)
    else:
        x = db.astype(np.float32)
    inv_row = inv_norms_reference(db, zero_point)
    inv_q = inv_norms_reference(queries, zero_point)
    rows = np.arange(N, dtype=np.int64)
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    step = max(1, (1 << 24) // max(N, 1))   # queries per block: the score matrix stays near 64 MiB
    for q0 in range(0, Q, step):
        q1 = min(Q, q0 + step)
        if i8:
            dot = ((queries[q0:q1].astype(np.int64) - int(zero_point)) @ x.T).astype(np.float32)
        else:
            dot = queries[q0:q1].astype(np.float32) @ x.T
        if metric == "cosine":
            score = (dot * inv_q[q0:q1, None]).astype(np.float32) * inv_row[None, :]
        else:
            score = dot
        ok = np.ones(score.shape, bool)
        if db_group is not None and query_group is not None:
            ok = np.asarray(db_group)[None, :] != np.asarray(query_group)[q0:q1, None]
        out_i[q0:q1], out_s[q0:q1] = order_topk(score.astype(np.float32), np.broadcast_to(rows, score.shape), ok, k)
    return out_i, out_s


def merge_topk(idx_parts: list, score_parts: list, k: int) -> tuple[np.ndarray, np.ndarray]:
    """Merge per-block results (row numbers already global) under the same total order."""
    idx = np.concatenate(idx_parts, axis=1)
    score = np.concatenate(score_parts, axis=1)
    return order_topk(score, idx, idx >= 0, k)


@dataclass
class SearchResult:
    """``idx`` / ``score`` [Q, k] (-1 / -inf where fewer than k rows qualified) and, per hit, the file and start of the matching row
    (``None`` / NaN in the unused slots)."""

    idx: np.ndarray
    score: np.ndarray
    match_path: list
    match_start_s: np.ndarray
    metric: str


def _load_archive(path: str) -> dict:
    with np.load(path, allow_pickle=False) as z:
        need = ("embeddings", "file_index", "start_s", "paths")
        missing = [key for key in need if key not in z.files]
        if missing:
            raise ValueError(f"{path}: not an archive written by `embed` (no {', '.join(missing)})")
        emb = z["embeddings"]
        out = dict(embeddings=emb, file_index=z["file_index"].astype(np.int64), start_s=z["start_s"].astype(np.float64), paths=[str(p) for p in z["paths"]])
        if emb.dtype == np.int8:
            if "scale" not in z.files or "zero_point" not in z.files:
                raise ValueError(f"{path}: int8 embeddings without scale / zero_point")
            out.update(dtype="int8", scale=float(z["scale"]), zero_point=int(z["zero_point"]))
        elif emb.dtype == np.float32:
            out.update(dtype="float32", scale=1.0, zero_point=0)
        else:
            raise ValueError(f"{path}: embeddings of dtype {emb.dtype}; float32 or int8 expected")
    return out


class EmbeddingIndex:
    """The rows of one or more ``embed`` archives, searchable on the device.

    ``embeddings`` [N, D] float32 or int8, ``file_index`` [N] (index into ``paths``), ``start_s`` [N].  Per-file pooled archives are one
    row per file.  The rows go to the device in blocks of ``budget_bytes``; an index that fits one block stays resident (rows and inverse
    norms) across searches, a larger one is streamed block by block per search and the per-block results are merged on the host."""

    def __init__(self, embeddings, file_index, start_s, paths, dtype: str | None = None, scale: float = 1.0, zero_point: int = 0,
                 budget_bytes: int = 2 << 30):
        emb = np.ascontiguousarray(embeddings)
        if emb.ndim != 2:
            raise ValueError(f"embeddings must be [N, D], got {emb.shape}")
        dtype = dtype or ("int8" if emb.dtype == np.int8 else "float32")
        if dtype not in ("float32", "int8"):
            raise ValueError(f"dtype must be 'float32' or 'int8', not {dtype!r}")
        if emb.dtype != (np.int8 if dtype == "int8" else np.float32):
            raise ValueError(f"embeddings of dtype {emb.dtype} do not match dtype={dtype!r}")
        if not 1 <= emb.shape[1] <= MAX_D:
            raise ValueError(f"embedding width {emb.shape[1]} outside 1..{MAX_D}")
        self.embeddings = emb
        self.file_index = np.asarray(file_index, np.int64)
        self.start_s = np.asarray(start_s, np.float64)
        self.paths = [str(p) for p in paths]
        if self.file_index.shape != (emb.shape[0],) or self.start_s.shape != (emb.shape[0],):
            raise ValueError("file_index and start_s need one entry per row")
        if emb.shape[0] and (self.file_index.min() < 0 or self.file_index.max() >= len(self.paths)):
            raise ValueError("file_index points outside paths")
        if dtype == "float32" and not np.isfinite(emb).all():
            raise ValueError("the embeddings hold values that are not finite")
        self.dtype, self.scale, self.zero_point = dtype, float(scale), int(zero_point) if dtype == "int8" else 0
        self.budget_bytes = int(budget_bytes)
        first: dict = {}   # per path the first path with the same resolved name: the group its rows are excluded by
        self.file_group = np.asarray([first.setdefault(os.path.realpath(p), i) for i, p in enumerate(self.paths)], np.int64)
        self._resident = None   # (device, rows tensor, inverse norms tensor, groups tensor)
        self._ctx = None

    @property
    def dim(self) -> int:
        return int(self.embeddings.shape[1])

    def __len__(self) -> int:
        return int(self.embeddings.shape[0])

    @property
    def dtype_code(self) -> int:
        """``dtype`` as the C ABI's ``BN_DTYPE_*``."""
        from birdnet_stm32 import _hip

        return _hip.DTYPE_I8 if self.dtype == "int8" else _hip.DTYPE_F32

    @classmethod
    def from_npz(cls, *paths: str, budget_bytes: int = 2 << 30) -> "EmbeddingIndex":
        if not paths:
            raise ValueError("no archive given")
        parts = [_load_archive(p) for p in paths]
        first = parts[0]
        for p, a in zip(paths[1:], parts[1:]):
            if a["embeddings"].shape[1] != first["embeddings"].shape[1] or a["dtype"] != first["dtype"]:
                raise ValueError(f"{p}: {a['embeddings'].shape[1]} x {a['dtype']} does not match {paths[0]}: "
                                 f"{first['embeddings'].shape[1]} x {first['dtype']}")
            if first["dtype"] == "int8" and (np.float32(a["scale"]) != np.float32(first["scale"]) or a["zero_point"] != first["zero_point"]):
                raise ValueError(f"{p}: int8 scale / zero point ({a['scale']}, {a['zero_point']}) differ from {paths[0]}'s "
                                 f"({first['scale']}, {first['zero_point']}): the bytes are not comparable")
        all_paths, file_index, off = [], [], 0
        for a in parts:
            file_index.append(a["file_index"] + off)
            all_paths += a["paths"]
            off += len(a["paths"])
        return cls(np.concatenate([a["embeddings"] for a in parts]), np.concatenate(file_index), np.concatenate([a["start_s"] for a in parts]),
                   all_paths, first["dtype"], first["scale"], first["zero_point"], budget_bytes=budget_bytes)

    # -- device side ------------------------------------------------------------------------------------------------------------------
    def block_ranges(self) -> list[tuple[int, int]]:
        """Row ranges that go to the device together: as many rows as fit ``budget_bytes`` (at least one)."""
        row_bytes = self.dim * self.embeddings.dtype.itemsize
        per = max(1, self.budget_bytes // row_bytes)
        return [(lo, min(len(self), lo + per)) for lo in range(0, len(self), per)] or [(0, 0)]

    def close(self) -> None:
        self._resident = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def context(self, ctx=None, device: int = 0):
        """``ctx`` if one is given, else the index's own context on ``device`` (created on first use, replaced when the device changes)."""
        from birdnet_stm32 import _hip

        if ctx is not None:
            return ctx
        if self._ctx is None or self._ctx.device != int(device):
            self.close()
            self._ctx = _hip.Context(int(device), 1)
        return self._ctx

    def device_block(self, ctx, lo: int, hi: int, stream_ptr):
        """Rows ``lo .. hi`` of a block of ``block_ranges()`` on ``ctx``'s device with their inverse norms and file groups (tensors; to be
        called under ``torch.cuda.device``).  The block of an index that fits its budget is kept for the next call."""
        import torch

        from birdnet_stm32 import _hip

        if self._resident is not None and self._resident[0] == (ctx.device, lo, hi):
            return self._resident[1:]
        dev = torch.device("cuda", ctx.device)
        d_db = torch.from_numpy(self.embeddings[lo:hi]).to(dev)
        d_inv = torch.empty(hi - lo, dtype=torch.float32, device=dev)
        d_grp = torch.from_numpy(self.file_group[self.file_index[lo:hi]].astype(np.int32)).to(dev)
        _hip.check(ctx.lib.bn_search_inv_norms(ctx.handle, d_db.data_ptr(), self.dtype_code, hi - lo, self.dim, self.zero_point, d_inv.data_ptr(), stream_ptr))
        self._resident = ((ctx.device, lo, hi), d_db, d_inv, d_grp) if (lo, hi) == (0, len(self)) else None
        return d_db, d_inv, d_grp

    def _check_queries(self, queries):
        """Queries as a contiguous CUDA tensor of the index's dtype (numpy arrays are checked on the host, tensors on the device)."""
        import torch

        want_np = np.int8 if self.dtype == "int8" else np.float32
        if isinstance(queries, torch.Tensor):
            want = torch.int8 if self.dtype == "int8" else torch.float32
            if queries.dtype != want:
                raise ValueError(f"queries of dtype {queries.dtype}; the index holds {self.dtype}")
            if queries.dim() != 2 or queries.shape[1] != self.dim:
                raise ValueError(f"queries must be [Q, {self.dim}], got {tuple(queries.shape)}")
            if self.dtype == "float32" and not bool(torch.isfinite(queries).all()):
                raise ValueError("the queries hold values that are not finite")
            return queries.contiguous()
        q = np.asarray(queries)
        if q.dtype != want_np:
            if self.dtype == "int8":
                raise ValueError(f"queries of dtype {q.dtype}; the index holds int8 bytes")
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [Q, {self.dim}], got {q.shape}")
        if self.dtype == "float32" and not np.isfinite(q).all():
            raise ValueError("the queries hold values that are not finite")
        return np.ascontiguousarray(q)

    def search(self, queries, k: int = 10, metric: str = "cosine", query_file_index=None, exclude_same_file: bool = False, ctx=None,
               device: int = 0) -> SearchResult:
        """The ``k`` best rows per query.  ``query_file_index`` [Q]: index into ``self.paths`` of the file each query came from (-1: none
        of them); with ``exclude_same_file`` the rows of that file do not qualify."""
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        metric = _check_metric(metric)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k={k} outside 1..{MAX_K}")
        q = self._check_queries(queries)
        if exclude_same_file:
            if query_file_index is None:
                raise ValueError("exclude_same_file needs query_file_index")
            qgrp = np.asarray(query_file_index, np.int64)
            if qgrp.shape != (q.shape[0],) or (qgrp.size and qgrp.max() >= len(self.paths)):
                raise ValueError("query_file_index needs one entry per query, each -1 or an index into paths")
            qgrp = np.where(qgrp >= 0, self.file_group[np.maximum(qgrp, 0)] if len(self.paths) else -1, -1)
        ctx = self.context(ctx, device)
        dev = torch.device("cuda", ctx.device)
        Q = int(q.shape[0])
        code = self.dtype_code
        idx_parts, score_parts = [], []
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            sp = ctypes.c_void_p(stream.cuda_stream)
            d_q = q.to(dev) if isinstance(q, torch.Tensor) else torch.from_numpy(q).to(dev)
            d_qinv = torch.empty(max(Q, 1), dtype=torch.float32, device=dev)
            d_qgrp = torch.from_numpy(qgrp.astype(np.int32)).to(dev) if exclude_same_file else None
            if Q:
                _hip.check(ctx.lib.bn_search_inv_norms(ctx.handle, d_q.data_ptr(), code, Q, self.dim, self.zero_point, d_qinv.data_ptr(), sp))
            blocks = self.block_ranges()
            for lo, hi in blocks:
                if hi == lo or Q == 0:
                    continue
                d_db, d_inv, d_grp = self.device_block(ctx, lo, hi, sp)
                d_idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
                d_score = torch.empty((Q, k), dtype=torch.float32, device=dev)
                _hip.check(ctx.lib.bn_search_topk(ctx.handle, d_db.data_ptr(), code, hi - lo, self.dim, self.zero_point, d_inv.data_ptr(), d_q.data_ptr(), Q,
                                                  d_qinv.data_ptr(), _hip.SEARCH_METRICS[metric], d_grp.data_ptr() if exclude_same_file else None,
                                                  d_qgrp.data_ptr() if exclude_same_file else None, k, d_idx.data_ptr(), d_score.data_ptr(), sp))
                bi = d_idx.cpu().numpy().astype(np.int64)
                bi[bi >= 0] += lo
                idx_parts.append(bi)
                score_parts.append(d_score.cpu().numpy())
            stream.synchronize()
        if not idx_parts:
            idx, score = np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf, np.float32)
        elif len(idx_parts) == 1:
            idx, score = idx_parts[0], score_parts[0]
        else:
            idx, score = merge_topk(idx_parts, score_parts, k)
        if metric == "dot" and self.dtype == "int8":
            score = score * (np.float32(self.scale) * np.float32(self.scale))
        return self._result(idx, score, metric)

    def _result(self, idx: np.ndarray, score: np.ndarray, metric: str) -> SearchResult:
        hit = idx >= 0
        safe = np.where(hit, idx, 0)
        start = np.where(hit, self.start_s[safe] if len(self) else 0.0, np.nan)
        files = self.file_index[safe] if len(self) else safe
        match_path = [[self.paths[int(f)] if h else None for f, h in zip(fr, hr)] for fr, hr in zip(files, hit)]
        return SearchResult(idx, score.astype(np.float32), match_path, start, metric)


def search_files(runner, index: EmbeddingIndex, query_paths: list[str], k: int = 10, metric: str = "cosine", query_pooling: str = "none",
                 exclude_same_file: bool = False, chunk_overlap: float = 0.0, max_duration=60, sample_rate: int = 22050, chunk_duration: float = 3.0):
    """Embed ``query_paths`` with ``runner`` (``embed_files``) and search ``index``: ``(SearchResult, FileEmbeddings of the queries)``.

    Queries are per chunk, or one per file with ``query_pooling`` "avg" / "max" (float32 only).  The model's embedding width and dtype
    are checked against the index before anything is read.  ``exclude_same_file`` compares resolved paths."""
    from birdnet_stm32.evaluation.embeddings import embed_files

    query_pooling = str(query_pooling).lower()
    if query_pooling not in QUERY_POOLINGS:
        raise ValueError(f"query_pooling must be one of {QUERY_POOLINGS}, not {query_pooling!r}")
    if query_pooling != "none" and index.dtype == "int8":
        raise ValueError("per-file pooling of the queries works on float32 embeddings; the index holds int8 bytes")
    info = runner.embedding_info()
    if int(info["dim"]) != index.dim:
        raise ValueError(f"the model's embeddings are {info['dim']} wide, the index holds {index.dim}")
    if index.dtype == "int8":
        if info["dtype"] != "int8":
            raise ValueError("the index holds int8 bytes; a float32 model cannot produce them")
        if np.float32(info["scale"]) != np.float32(index.scale) or int(info["zero_point"]) != index.zero_point:
            raise ValueError("the model's int8 scale / zero point differ from the index's: the bytes are not comparable")
    res = embed_files(runner, list(query_paths), chunk_overlap=chunk_overlap, max_duration=max_duration, pooling=query_pooling, dtype=index.dtype,
                      sample_rate=sample_rate, chunk_duration=chunk_duration)
    qfile = same_file_index(index.paths, res.paths)[res.file_index] if exclude_same_file else None
    hits = index.search(res.embeddings, k=k, metric=metric, query_file_index=qfile, exclude_same_file=exclude_same_file, ctx=runner.ctx)
    return hits, res


def same_file_index(db_paths: list[str], query_paths: list[str]) -> np.ndarray:
    """Per query path the index of the database file with the same resolved path, -1 where there is none."""
    where = {}
    for i, p in enumerate(db_paths):
        where.setdefault(os.path.realpath(p), i)
    return np.asarray([where.get(os.path.realpath(p), -1) for p in query_paths], np.int64)
