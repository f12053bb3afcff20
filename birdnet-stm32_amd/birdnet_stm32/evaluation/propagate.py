"""Propagation: a few labelled rows of archives written by ``embed`` spread over all the others along the nearest-neighbour graph.

``propagate_reference`` is the specification in numpy (for small N); ``propagate_index`` runs the same iteration on the device
(``csrc/bn_propagate.hip``, C ABI ``bn_propagate_step`` / ``bn_propagate_decide``; neighbours from ``bn_search_topk``).  Both share every
host-side step: the argument checks, the graph (``build_graph``), the stopping rule (``_spread``) and the hold-out split.  It is label
spreading (Zhou et al. 2004) with the iteration and the stopping rule of scikit-learn 1.7's ``sklearn.semi_supervised.LabelSpreading`` over
a k-nearest-neighbour graph with cosine weights.

1. Rows.  ``[N, D]`` float32, or int8 bytes with a zero point, with ``search``'s meaning.  Zero rows (``inv_norms_reference`` gives 0) take
   no part and come back as label -1, score NaN; ``n`` is the number of the others, and fewer than 2 is refused.
2. Seeds.  ``seed_label [N]`` int32 holds a class ``0..C-1`` for a labelled row and -1 for the others.  Refused: ``C < 1``,
   ``C > 4096`` (``BN_PROPAGATE_MAX_CLASSES``), a label ``>= C`` or ``< -1``, no labelled non-zero row, ``n > 2^21`` (``project``'s limit).  A
   class without seeds is allowed; the label of a zero row is ignored.
3. Neighbours.  ``k = neighbours``; ``k < 1``, ``k >= n`` and ``k > 128`` (``BN_SEARCH_MAX_K``) are refused.  The neighbours of a row are its
   ``k`` best cosine scores ``s`` among the other non-zero rows (``search`` of the rows against themselves, every row its own group).
4. Weights (host, float64).  ``w = exp((s - 1) / tau)`` from the float32 score; ``tau`` finite and > 0.  ``W`` is symmetric over the union of
   the two directions' patterns; where both directions report a pair the larger ``w`` stands; the diagonal is dropped (``symmetrize_max``).
5. Normalisation (host, float64).  ``d_i`` is the sum of row i of ``W`` in ascending column order; ``S_ij = w_ij / sqrt(d_i d_j)`` (0 where
   ``d_i d_j`` is 0: weights that underflowed), stored as float32 CSR ``(rowptr int64, col int32 ascending, val float32)``.
6. Iteration, float32, every operation rounded on its own, nothing fused.  ``F_0[i, c] = 1`` if ``seed_label[i] == c`` else 0.  With
   ``acc = 0`` and, for the entries of row i in ascending column order, ``acc = fl(acc + fl(S_ij F_t[j, c]))``:
   ``F_{t+1}[i, c] = fl(fl(alpha acc) + y)``, ``y = fl(1 - alpha)`` for the seed class and 0 otherwise; ``alpha`` in (0, 1).  The order is
   fixed, so the result is a function of the inputs alone: numpy and the device give the same bits.
7. Stopping (scikit-learn's rule).  ``delta_t = sum_{i,c} |F_t - F_{t-1}|``, every difference exact in float64, the sum float64 in the
   implementation's fixed order; ``delta_0 = sum F_0``.  Before update t + 1: stop if ``delta_t < tol``; stop after ``max_iter`` updates
   at the latest.  ``tol = 0`` never stops early.  ``n_iter`` is the number of updates done.
8. Decision.  ``best`` is the first class with the largest ``F[i, .]`` (float32 comparison), ``score = F[i, best] / sum_c F[i, c]``.  A row
   whose sum is 0 (no labelled row in its component) gets label -1 and score 0 (scikit-learn would call it class 0).  ``min_score`` turns
   the rows below it into -1 in what is written, and nowhere else (``apply_min_score``).
9. Hold-out.  ``holdout = h`` in (0, 1) hides ``round(h * seeds)`` of the labelled non-zero rows (Python's ``round``; at least one, not
   all), the first of ``default_rng([seed]).permutation(seeds)``, runs, and reports accuracy and per-class recall on the hidden rows (a
   hidden row that comes back -1 is wrong).  The labels returned are those of a second run with all seeds; the graph is built once.

The defaults of ``alpha``, ``max_iter`` and ``tol`` are scikit-learn's; ``tau`` and ``neighbours`` are this module's own, and none of them
has been measured on real archives.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from birdnet_stm32.evaluation.project import MAX_N, _rows_and_nonzero, neighbours_reference
from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K
from birdnet_stm32.evaluation.search import inv_norms_reference

MAX_CLASSES = 4096   # BN_PROPAGATE_MAX_CLASSES (include/birdnet_hip.h)
DEFAULT_NEIGHBOURS, DEFAULT_TAU, DEFAULT_ALPHA, DEFAULT_MAX_ITER, DEFAULT_TOL = 15, 0.1, 0.2, 30, 1e-3


def check_propagate_args(n: int, classes: int, neighbours, tau, alpha, max_iter, tol, holdout=0.0) -> None:
    """Everything a run over ``n`` non-zero rows refuses before it looks at the seeds."""
    if n < 2:
        raise ValueError(f"propagation needs at least 2 non-zero rows, the archive holds {n}")
    if n > MAX_N:
        raise ValueError(f"{n} non-zero rows: a run holds at most {MAX_N}")
    if not 1 <= int(classes) <= MAX_CLASSES:
        raise ValueError(f"{classes} classes outside 1..{MAX_CLASSES}")
    k = int(neighbours)
    if k < 1:
        raise ValueError(f"neighbours {neighbours} must be >= 1")
    if k >= n:
        raise ValueError(f"neighbours {neighbours} must be below the number of non-zero rows ({n})")
    if k > SEARCH_MAX_K:
        raise ValueError(f"neighbours {neighbours} above the {SEARCH_MAX_K} `search` returns")
    if not (math.isfinite(float(tau)) and float(tau) > 0.0):
        raise ValueError(f"tau {tau} must be finite and > 0")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"alpha {alpha} must lie in (0, 1)")
    if int(max_iter) < 0:
        raise ValueError("max_iter must be >= 0")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol {tol} must be >= 0")
    if not (float(holdout) == 0.0 or 0.0 < float(holdout) < 1.0):
        raise ValueError(f"holdout {holdout} must be 0 or lie in (0, 1)")


def check_seeds(seed_label, N: int, classes: int, nonzero) -> np.ndarray:
    """``seed_label`` as int32 ``[N]``, refused where item 2 says so."""
    lab = np.asarray(seed_label)
    if lab.shape != (N,) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"seed_label must be {N} integers, one per row")
    if lab.size and (lab.max() >= int(classes) or lab.min() < -1):
        raise ValueError(f"seed_label holds values outside -1..{int(classes) - 1}")
    lab = lab.astype(np.int32)
    if not (lab[nonzero] >= 0).any():
        raise ValueError("no labelled non-zero row: there is nothing to spread")
    return lab


def edge_weights(score, tau: float) -> np.ndarray:
    """``w = exp((s - 1) / tau)`` in float64 from the float32 scores (item 4)."""
    return np.exp((np.asarray(score, np.float32).astype(np.float64) - 1.0) / float(tau))


def symmetrize_max(idx, w, n: int):
    """``(rowptr [n + 1] int64, col int32, w float64)``: the symmetric matrix over the union of the patterns of ``idx [n, k]`` and its
    transpose, in CSR with ascending columns.  Where both directions report a pair the larger weight stands; an entry < 0, >= n or on the
    diagonal is dropped.  (``project.symmetrize`` is its sibling: that one adds the two directions.)"""
    idx = np.asarray(idx, np.int64)
    w = np.asarray(w, np.float64)
    if idx.shape != w.shape or idx.ndim != 2 or idx.shape[0] != n:
        raise ValueError(f"idx {idx.shape} and w {w.shape} must both be [{n}, k]")
    i = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    j = idx.ravel()
    keep = (j >= 0) & (j < n) & (j != i)
    i, j, v = i[keep], j[keep], w.ravel()[keep]
    keys = np.concatenate([i * n + j, j * n + i])
    vals = np.concatenate([v, v])
    if keys.size == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    uniq, first = np.unique(keys, return_index=True)
    top = np.maximum.reduceat(vals, first)
    rowptr = np.searchsorted(uniq // n, np.arange(n + 1)).astype(np.int64)
    return rowptr, (uniq % n).astype(np.int32), top


def normalize(rowptr, col, w):
    """``S_ij = w_ij / sqrt(d_i d_j)`` in float64 (item 5): the entries of ``(rowptr, col, w)`` in place.  ``d_i`` adds row i in ascending
    column order (``np.bincount`` adds in the order of its input); an entry whose ``d_i d_j`` is 0 is 0."""
    rowptr, col, w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.float64)
    n = rowptr.size - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    d = np.bincount(row, w, n)
    den = np.sqrt(d[row] * d[col])
    out = np.zeros(w.shape)
    np.divide(w, den, out=out, where=den > 0)
    return out


def build_graph(idx, score, n: int, tau: float):
    """Items 4 and 5 from the neighbours' ``idx`` / ``score`` ``[n, k]``: ``(rowptr int64, col int32, val float32, val64 float64)``."""
    rowptr, col, w = symmetrize_max(idx, edge_weights(score, tau), n)
    s = normalize(rowptr, col, w)
    return rowptr, col, s.astype(np.float32), s


def initial_labels(seed_label, classes: int) -> np.ndarray:
    """``F_0 [n, C]`` float32 of item 6."""
    lab = np.asarray(seed_label, np.int64)
    F = np.zeros((lab.size, int(classes)), np.float32)
    rows = np.flatnonzero((lab >= 0) & (lab < int(classes)))
    F[rows, lab[rows]] = 1.0
    return F


def step_reference(rowptr, col, val, F, seed_label, alpha: float):
    """One update of item 6 in float32, every operation rounded: ``F_next [n, C]``.  Entry p of every row that has one is added in turn, so
    each ``(i, c)`` sees its row's entries in stored order.  An entry whose column lies outside ``0..n-1`` contributes nothing."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    val, F = np.asarray(val, np.float32), np.asarray(F, np.float32)
    n, C = F.shape
    a = np.float32(alpha)
    lengths = np.diff(rowptr)
    acc = np.zeros((n, C), np.float32)
    for p in range(int(lengths.max()) if n else 0):
        rows = np.flatnonzero(lengths > p)
        at = rowptr[rows] + p
        j = col[at]
        ok = (j >= 0) & (j < n)
        rows, at, j = rows[ok], at[ok], j[ok]
        acc[rows] = acc[rows] + val[at, None] * F[j]
    lab = np.asarray(seed_label, np.int64)
    y = np.zeros((n, C), np.float32)
    seeded = np.flatnonzero((lab >= 0) & (lab < C))
    y[seeded, lab[seeded]] = np.float32(1) - a
    return (a * acc + y).astype(np.float32)


def delta_reference(F_next, F) -> float:
    """``sum |F_next - F|`` of item 7: differences exact in float64, one float64 sum."""
    return float(np.abs(np.asarray(F_next, np.float64) - np.asarray(F, np.float64)).sum())


def decide_reference(F):
    """Item 8: ``(label [n] int32, score [n] float32)``; the sum and the division in float64, rounded once."""
    F = np.asarray(F, np.float32)
    best = F.argmax(axis=1)
    total = F.astype(np.float64).sum(axis=1)
    top = F[np.arange(F.shape[0]), best].astype(np.float64)
    none = total == 0
    score = np.where(none, 0.0, top / np.where(none, 1.0, total)).astype(np.float32)
    return np.where(none, -1, best).astype(np.int32), score


def apply_min_score(labels, scores, min_score: float) -> np.ndarray:
    """The labels as they are written: -1 where the score is below ``min_score`` (NaN scores are -1 already)."""
    labels = np.array(labels, np.int32)
    labels[np.asarray(scores) < float(min_score)] = -1
    return labels


def _spread(step, delta0: float, max_iter: int, tol: float):
    """Item 7 over ``step() -> delta``: ``(n_iter, [delta_0, delta_1, ...])``."""
    history = [float(delta0)]
    n_iter = 0
    while n_iter < int(max_iter) and not history[-1] < float(tol):
        history.append(float(step()))
        n_iter += 1
    return n_iter, history


def spread_float64(rowptr, col, val64, seed_label, classes: int, alpha: float, max_iter: int, tol: float):
    """The recurrence ``F <- alpha S F + (1 - alpha) Y`` in float64 with item 7's rule: ``(F [n, C] float64, n_iter, history)``."""
    rowptr, col, s = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(val64, np.float64)
    n = rowptr.size - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    Y = initial_labels(seed_label, classes).astype(np.float64)
    state = {"F": Y.copy()}

    def step():
        F = state["F"]
        SF = np.stack([np.bincount(row, s * F[col, c], n) for c in range(F.shape[1])], axis=1)
        state["F"] = float(alpha) * SF + (1.0 - float(alpha)) * Y
        return np.abs(state["F"] - F).sum()

    n_iter, history = _spread(step, Y.sum(), max_iter, tol)
    return state["F"], n_iter, history


def normalized_rows(F) -> np.ndarray:
    """Every row of ``F`` over its sum in float64 (a row of zeros stays)."""
    F = np.asarray(F, np.float64)
    total = F.sum(axis=1, keepdims=True)
    return F / np.where(total == 0, 1.0, total)


@dataclass
class HoldoutReport:
    """The hidden rows (indices into the archive), their true and predicted classes, ``accuracy`` and per-class ``recall`` [C] (NaN for a
    class without hidden rows)."""

    rows: np.ndarray
    true: np.ndarray
    predicted: np.ndarray
    accuracy: float
    recall: np.ndarray


def holdout_split(seed_label, nonzero, holdout: float, seed: int) -> np.ndarray:
    """The rows item 9 hides: indices into the archive, in the permutation's order."""
    lab = np.asarray(seed_label)
    live = np.zeros(lab.size, bool)
    live[nonzero] = True
    seeds = np.flatnonzero((lab >= 0) & live)
    m = int(round(float(holdout) * seeds.size))
    if m < 1 or m >= seeds.size:
        raise ValueError(f"holdout {holdout} of {seeds.size} labelled rows hides {m}: at least one must be hidden and one must stay")
    return seeds[np.random.default_rng([int(seed)]).permutation(seeds.size)[:m]]


def holdout_report(hidden, seed_label, labels, classes: int) -> HoldoutReport:
    true = np.asarray(seed_label, np.int32)[hidden]
    pred = np.asarray(labels, np.int32)[hidden]
    recall = np.full(int(classes), np.nan)
    for c in np.unique(true):
        recall[c] = float((pred[true == c] == c).mean())
    return HoldoutReport(np.asarray(hidden, np.int64), true, pred, float((pred == true).mean()), recall)


@dataclass
class PropagateResult:
    """``labels`` [N] int32 (-1: a zero row, or a row no seed reaches) and ``scores`` [N] float32 (NaN for a zero row), ``n_iter`` updates,
    ``delta_history`` (``delta_0`` first), the neighbours ``neighbour_idx`` / ``neighbour_score`` [n, k] of the non-zero rows as the search
    returned them (indices into the non-zero rows), ``nonzero`` [n], the hold-out report or None, and with ``keep_scores`` ``F`` [N, C]
    float32 (NaN for a zero row)."""

    labels: np.ndarray
    scores: np.ndarray
    n_iter: int
    delta_history: list
    neighbour_idx: np.ndarray
    neighbour_score: np.ndarray
    nonzero: np.ndarray
    holdout: HoldoutReport | None = None
    F: np.ndarray | None = None
    extra: dict = field(default_factory=dict)


def _scatter(N, nonzero, label, score, F, keep_scores):
    labels = np.full(N, -1, np.int32)
    scores = np.full(N, np.nan, np.float32)
    labels[nonzero], scores[nonzero] = label, score
    full = None
    if keep_scores:
        full = np.full((N, F.shape[1]), np.nan, np.float32)
        full[nonzero] = F
    return labels, scores, full


def _run_with_holdout(run, N, nonzero, seed_label, classes, holdout, seed, keep_scores, idx, score) -> PropagateResult:
    """Item 9 around ``run(seed_live) -> (F, label, score, n_iter, history)`` over the non-zero rows."""
    report = None
    if float(holdout) > 0.0:
        hidden = holdout_split(seed_label, nonzero, holdout, seed)
        shown = seed_label.copy()
        shown[hidden] = -1
        _, label, _, _, _ = run(shown[nonzero])
        guess = np.full(N, -1, np.int32)
        guess[nonzero] = label
        report = holdout_report(hidden, seed_label, guess, classes)
    F, label, sc, n_iter, history = run(seed_label[nonzero])
    labels, scores, full = _scatter(N, nonzero, label, sc, F, keep_scores)
    return PropagateResult(labels, scores, int(n_iter), history, idx, score, nonzero, report, full)


def propagate_reference(rows, seed_label, classes: int, neighbours: int = DEFAULT_NEIGHBOURS, tau: float = DEFAULT_TAU, alpha: float = DEFAULT_ALPHA,
                        max_iter: int = DEFAULT_MAX_ITER, tol: float = DEFAULT_TOL, holdout: float = 0.0, seed: int = 0, zero_point: int = 0,
                        graph=None, float64: bool = False) -> PropagateResult:
    """Items 1-9 in numpy, for small N; ``F`` is always kept.  ``graph = (idx, score)`` takes the place of the search of item 3 (a device's
    own neighbours, for a teacher-forced comparison).  With ``float64`` the result's ``extra`` also holds the float64 recurrence over the
    unrounded ``S`` with all seeds: ``F64`` [n, C] of the non-zero rows, ``n_iter64`` and ``labels64`` [n]."""
    rows, nonzero = _rows_and_nonzero(rows, zero_point)
    n = int(nonzero.size)
    check_propagate_args(n, classes, neighbours, tau, alpha, max_iter, tol, holdout)
    seed_label = check_seeds(seed_label, rows.shape[0], classes, nonzero)
    if graph is None:
        idx, score = neighbours_reference(np.ascontiguousarray(rows[nonzero]), int(neighbours), zero_point)
    else:
        idx, score = np.asarray(graph[0], np.int64), np.asarray(graph[1], np.float32)
    rowptr, col, val, val64 = build_graph(idx, score, n, tau)

    def run(seed_live):
        state = {"F": initial_labels(seed_live, classes)}

        def step():
            nxt = step_reference(rowptr, col, val, state["F"], seed_live, alpha)
            d = delta_reference(nxt, state["F"])
            state["F"] = nxt
            return d

        n_iter, history = _spread(step, float(state["F"].sum(dtype=np.float64)), max_iter, tol)
        label, sc = decide_reference(state["F"])
        return state["F"], label, sc, n_iter, history

    res = _run_with_holdout(run, rows.shape[0], nonzero, seed_label, classes, holdout, seed, True, idx, score)
    res.extra["csr"] = (rowptr, col, val)
    if float64:
        F64, n64, _ = spread_float64(rowptr, col, val64, seed_label[nonzero], classes, alpha, max_iter, tol)
        res.extra.update(F64=F64, n_iter64=n64, labels64=np.where(F64.sum(axis=1) == 0, -1, F64.argmax(axis=1)))
    return res


# ---------------------------------------------------------------------------------------------------------------------- device
def device_bytes_needed(n: int, D: int, itemsize: int, k: int, classes: int) -> int:
    """What a run keeps on the device at its largest: rows and their scores, then the matrix S, the two label matrices and the outputs."""
    search = n * D * itemsize + n * 12 + 2 * n * k * 4 + n * 8 + (128 << 20)
    spread = 2 * n * k * 8 + (n + 1) * 8 + 2 * n * int(classes) * 4 + n * 4 + n * 8 + n * 8 + 8
    return max(search, spread)


class _DeviceSpread:
    """S, the two label matrices (they ping-pong), the change and the decision stay on the device; the host reads 8 bytes per update."""

    def __init__(self, ctx, csr, n: int, classes: int):
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        self.torch, self.hip, self.ctx = torch, _hip, ctx
        self.dev = torch.device("cuda", ctx.device)
        self.n, self.C = int(n), int(classes)
        rowptr, col, val = csr
        with torch.cuda.device(self.dev):
            self.sp = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            self.d_rowptr = torch.from_numpy(np.ascontiguousarray(rowptr, np.int64)).to(self.dev)
            self.d_col = torch.from_numpy(np.ascontiguousarray(col, np.int32)).to(self.dev)
            self.d_val = torch.from_numpy(np.ascontiguousarray(val, np.float32)).to(self.dev)
            if self.d_col.numel() == 0:   # (an empty tensor has no address; the kernel reads no entry)
                self.d_col, self.d_val = torch.zeros(1, dtype=torch.int32, device=self.dev), torch.zeros(1, dtype=torch.float32, device=self.dev)
            self.d_f = [torch.zeros((self.n, self.C), dtype=torch.float32, device=self.dev) for _ in range(2)]
            self.d_delta = torch.zeros(1, dtype=torch.float64, device=self.dev)
            self.d_label = torch.empty(self.n, dtype=torch.int32, device=self.dev)
            self.d_score = torch.empty(self.n, dtype=torch.float32, device=self.dev)

    def run(self, seed_live, alpha: float, max_iter: int, tol: float, keep_scores: bool):
        torch, lib, h = self.torch, self.ctx.lib, self.ctx.handle
        seed_live = np.ascontiguousarray(seed_live, np.int32)
        seeded = np.flatnonzero(seed_live >= 0)
        with torch.cuda.device(self.dev):
            d_seed = torch.from_numpy(seed_live).to(self.dev)
            self.d_f[0].zero_()
            self.d_f[0][torch.from_numpy(seeded).to(self.dev), torch.from_numpy(seed_live[seeded].astype(np.int64)).to(self.dev)] = 1.0
            state = {"cur": 0}

            def step():
                a, b = self.d_f[state["cur"]], self.d_f[1 - state["cur"]]
                self.hip.check(lib.bn_propagate_step(h, self.d_rowptr.data_ptr(), self.d_col.data_ptr(), self.d_val.data_ptr(), a.data_ptr(), d_seed.data_ptr(),
                                                     self.n, self.C, self.hip.c_float(alpha), b.data_ptr(), self.d_delta.data_ptr(), self.sp))
                state["cur"] = 1 - state["cur"]
                return float(self.d_delta.item())

            n_iter, history = _spread(step, float(seeded.size), max_iter, tol)
            F = self.d_f[state["cur"]]
            self.hip.check(lib.bn_propagate_decide(h, F.data_ptr(), self.n, self.C, self.d_label.data_ptr(), self.d_score.data_ptr(), self.sp))
            return F.cpu().numpy() if keep_scores else None, self.d_label.cpu().numpy(), self.d_score.cpu().numpy(), n_iter, history


def propagate_index(index, seed_label, classes: int, neighbours: int = DEFAULT_NEIGHBOURS, tau: float = DEFAULT_TAU, alpha: float = DEFAULT_ALPHA,
                    max_iter: int = DEFAULT_MAX_ITER, tol: float = DEFAULT_TOL, holdout: float = 0.0, seed: int = 0, device: int = 0, ctx=None,
                    keep_scores: bool = False) -> PropagateResult:
    """The labels of ``seed_label`` spread over the rows of an ``EmbeddingIndex`` on the device.  The non-zero rows go to the device in one
    piece, whatever the index's block budget: an archive that does not fit is refused."""
    import torch

    from birdnet_stm32.evaluation.project import device_neighbours

    rows, zp = index.embeddings, index.zero_point
    nonzero = np.flatnonzero(inv_norms_reference(rows, zp) != 0)
    n, k = int(nonzero.size), int(neighbours)
    check_propagate_args(n, classes, neighbours, tau, alpha, max_iter, tol, holdout)
    seed_label = check_seeds(seed_label, len(index), classes, nonzero)
    ctx = index.context(ctx, device)
    need = device_bytes_needed(n, index.dim, rows.dtype.itemsize, k, classes)
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if need > free:
        raise ValueError(f"the archive does not fit on the device in one piece: {n} rows x {index.dim} and {int(classes)} classes need about "
                         f"{need >> 20} MiB, {free >> 20} MiB are free (archives larger than device memory are out of scope)")
    live = rows if n == len(index) else np.ascontiguousarray(rows[nonzero])
    d_idx, d_score = device_neighbours(ctx, live, zp, k)
    idx, score = d_idx.cpu().numpy().astype(np.int64), d_score.cpu().numpy()
    del d_idx, d_score
    rowptr, col, val, _ = build_graph(idx, score, n, tau)
    backend = _DeviceSpread(ctx, (rowptr, col, val), n, classes)
    return _run_with_holdout(lambda seed_live: backend.run(seed_live, float(alpha), int(max_iter), float(tol), keep_scores), len(index), nonzero,
                             seed_label, classes, holdout, seed, keep_scores, idx, score)
