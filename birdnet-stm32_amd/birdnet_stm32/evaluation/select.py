"""Selection: which rows of archives written by ``embed`` to label next — farthest-first traversal, optionally weighted by uncertainty.

``select_reference`` is the specification in numpy (for small N); ``select_index`` runs the same traversal on the device
(``csrc/bn_select.hip``, C ABI ``bn_select_run``: one fused launch per pick, nothing read back between picks).  Both share every host-side
step: the argument checks (``_prepare``), the mapping between live rows and archive rows and the ``min_key`` cut (``_select``).  It is
k-centre greedy, the core-set selection of Sener & Savarese 2018.  On unit vectors the cosine pick is the pick under the chord distance
``sqrt(2 - 2 cos)``, a metric, so the unweighted traversal is the classical 2-approximation of k-centre on the normalised rows.

1. Rows.  ``[N, D]`` float32, or int8 bytes with a zero point, with ``search``'s meaning.  ``inv = inv_norms_reference(rows, zero_point)``.
   Zero rows (``inv == 0``) take no part: they are never picked and come back with nearest -1 and similarity NaN; ``n`` is the number of
   the others, the live rows.
2. Score.  ``score(i, c) = fl(fl(dot(x_i, x_c) * inv_i) * inv_c)``: ``search``'s cosine of row i as the query against row c.  For float32
   ``dot`` is the float32 inner product and its summation order is the implementation's; for int8 it is the exact int32 inner product of
   ``(byte - zero_point)`` rounded once to float32, one value whatever the order.
3. State per row.  ``m_i`` is the highest score to any row taken so far, -inf for none yet; ``nearest_i`` the row that gave it.  A taken
   row has ``m = +inf`` and ``nearest`` equal to itself.
4. Key.  ``key_i = fl(u_i * fl(1 - m_i))`` with the weight ``u_i`` float32, finite and >= 0, all 1 when no weights are given;
   ``key_i = -inf`` for a zero row and for a taken row, and a NaN key counts as -inf.
5. A pick is the row with the highest key, the lowest index among equal keys (float comparison, so -0 equals 0).  When no row has a key
   above -inf the pick is -1 with key -inf and nothing changes.
6. Taking ``c``.  For every live, untaken row ``i != c``: ``s = score(i, c)``; ``s > m_i`` sets ``m_i = s`` and ``nearest_i = c`` (strict:
   the earlier centre stands on a tie).  Then ``m_c = +inf`` and ``nearest_c = c``.
7. A run is the already-chosen rows taken in the given order, then greedy picks.  The already-chosen rows are the seeds (labelled rows),
   then a caller's ``first``; a seed naming a zero row is ignored, and a row named twice is taken once.  With neither live seeds nor
   ``first``, ``first`` is the most central row: the live row with the highest cosine to the sum of the normalised rows, the lowest index
   among equals (``cluster``'s update and assignment with one cluster).  A computed ``first`` counts as the first of the ``budget`` picks,
   with key +inf: nothing was taken before it.
8. Refused: ``budget < 1``; ``budget`` above the number of live rows that are not already chosen; ``n < 2``; weights of the wrong shape,
   non-finite (as float32) or negative; a seed or ``first`` outside ``0..N-1``; a ``first`` naming a zero row; ``D > 2048``;
   ``n > 2^21`` (``project``'s ``MAX_N``).
9. ``min_key = R`` cuts the result before the first pick whose key is below ``R``: applied to the finished sequence, on the host.  The
   state returned (``nearest``, ``similarity``) is that of the picks that remain: the run is repeated with the shorter budget, which
   gives the same picks, a traversal being a prefix of every longer one.
10. Property.  The key sequence of one run never increases, weighted or not: ``m_i`` only grows, ``fl`` is monotone, so every row's key
    only falls, and the highest key of a later step is at most the highest key of an earlier one.

``uncertainty_reference`` turns the label matrix ``F [N, C]`` that ``propagate --scores_out`` writes into weights.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from birdnet_stm32.evaluation.cluster import assign_reference, centroids_from_sums, update_reference
from birdnet_stm32.evaluation.project import MAX_N, _rows_and_nonzero
from birdnet_stm32.evaluation.propagate import normalized_rows
from birdnet_stm32.evaluation.search import MAX_D, inv_norms_reference

UNCERTAINTY_MODES = ("margin", "entropy", "least_confidence")
F32_INF = np.float32(np.inf)


# ------------------------------------------------------------------------------------------------------------------- specification
def scores_reference(rows, inv, c: int, zero_point: int = 0) -> np.ndarray:
    """``score(i, c)`` of item 2 for every row i: float32 ``[n]``."""
    rows = np.asarray(rows)
    if rows.dtype == np.int8:
        x = rows.astype(np.int64) - int(zero_point)
        dot = (x @ x[c]).astype(np.float32)
    else:
        x = rows.astype(np.float32)
        dot = (x @ x[c]).astype(np.float32)
    return ((dot * inv).astype(np.float32) * inv[c]).astype(np.float32)


def keys_reference(m, inv, weights=None) -> np.ndarray:
    """The keys of item 4 from the state ``m``: float32 ``[n]``, -inf for zero rows, taken rows and NaN."""
    m = np.asarray(m, np.float32)
    u = np.ones(m.shape, np.float32) if weights is None else np.asarray(weights, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        key = (u * (np.float32(1) - m).astype(np.float32)).astype(np.float32)
    key[(np.asarray(inv) == 0) | (m == F32_INF) | np.isnan(key)] = -F32_INF
    return key


def pick_reference(key) -> tuple[int, np.float32]:
    """Item 5: ``(row, key)``, or ``(-1, -inf)``."""
    if key.size == 0:
        return -1, -F32_INF
    best = int(np.argmax(key))   # (the first of equal maxima: the lowest index)
    return (best, key[best]) if key[best] > -F32_INF else (-1, -F32_INF)


def take_reference(rows, inv, m, nearest, c: int, zero_point: int = 0) -> None:
    """Item 6 on the state ``m`` / ``nearest``, in place."""
    s = scores_reference(rows, inv, c, zero_point)
    better = (inv != 0) & (m != F32_INF) & (s > m)
    better[c] = False
    m[better], nearest[better] = s[better], c
    m[c], nearest[c] = F32_INF, c


def run_reference(rows, inv, m, nearest, picked, forced: int, steps: int, weights=None, zero_point: int = 0):
    """``bn_select_run`` in numpy over the state ``m [n]`` float32 / ``nearest [n]`` (both changed in place): ``(picked [steps] int32,
    key [steps] float32)``.  The first ``forced`` entries of ``picked`` are taken in order (one outside ``0..n-1`` or naming a zero row is
    skipped) and their keys come back NaN, standing for "left alone"; the others are chosen by items 4-6."""
    n = np.asarray(rows).shape[0]
    out = np.full(steps, -1, np.int32)
    out[:forced] = np.asarray(picked, np.int32)[:forced]
    key = np.full(steps, np.nan, np.float32)
    for t in range(steps):
        if t < forced:
            c = int(out[t])
            if 0 <= c < n and inv[c] != 0:
                take_reference(rows, inv, m, nearest, c, zero_point)
            continue
        c, k = pick_reference(keys_reference(m, inv, weights))
        out[t], key[t] = c, k
        if c >= 0:
            take_reference(rows, inv, m, nearest, c, zero_point)
    return out, key


def central_reference(live_rows, zero_point: int = 0) -> int:
    """The most central of the (non-zero) rows of item 7, an index into them."""
    S, counts = update_reference(live_rows, np.zeros(live_rows.shape[0], np.int64), 1, zero_point)
    C = centroids_from_sums(S, counts, np.zeros_like(S))
    _, score = assign_reference(live_rows, C, zero_point)
    return int(np.argmax(score))


def uncertainty_reference(F, mode: str = "margin") -> np.ndarray:
    """Weights ``[N]`` float32 from a label matrix ``F [N, C]``, computed in float64 from ``normalized_rows(F)`` and rounded once:
    ``least_confidence`` ``1 - p1``; ``margin`` ``1 - (p1 - p2)`` with ``p2 = 0`` when C = 1; ``entropy`` ``H(p) / log C``, 0 when C = 1
    (``p1 >= p2`` the two largest shares of a row).  A row whose sum is 0 (no seed reaches it) gets 1, a NaN row (a zero row) gets 0."""
    if mode not in UNCERTAINTY_MODES:
        raise ValueError(f"uncertainty must be one of {UNCERTAINTY_MODES}, not {mode!r}")
    F = np.asarray(F, np.float64)
    if F.ndim != 2 or F.shape[1] < 1:
        raise ValueError(f"F must be [N, C] with C >= 1, got {F.shape}")
    C = F.shape[1]
    nan = np.isnan(F).any(axis=1)
    P = normalized_rows(np.where(nan[:, None], 0.0, F))
    unreached = P.sum(axis=1) == 0
    top = -np.sort(-P, axis=1)
    p1 = top[:, 0]
    p2 = top[:, 1] if C > 1 else np.zeros_like(p1)
    if mode == "least_confidence":
        u = 1.0 - p1
    elif mode == "margin":
        u = 1.0 - (p1 - p2)
    elif C == 1:
        u = np.zeros_like(p1)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            u = -np.where(P > 0, P * np.log(P), 0.0).sum(axis=1) / math.log(C)
    u = np.maximum(u, 0.0)
    u[unreached] = 1.0
    u[nan] = 0.0
    return u.astype(np.float32)


@dataclass
class SelectResult:
    """``picked`` [B] int64 archive rows in pick order and their ``key`` [B] float32; ``nearest`` [N] int64 (the taken row closest to every
    row, itself for a taken row, -1 for a zero row) and ``similarity`` [N] float32 (``m``, 1 for a taken row, NaN for a zero row);
    ``seeds`` the already-chosen archive rows that were taken (a caller's ``first`` last), ``first`` the caller's or the computed first
    row, -1 without one, and ``nonzero`` [n]."""

    picked: np.ndarray
    key: np.ndarray
    nearest: np.ndarray
    similarity: np.ndarray
    seeds: np.ndarray
    first: int
    nonzero: np.ndarray


def check_budget(budget) -> int:
    if int(budget) < 1:
        raise ValueError(f"budget {budget} must be >= 1")
    return int(budget)


def check_weights(weights, N: int):
    """``weights`` as float32 ``[N]`` (None stays None), refused where item 8 says so."""
    if weights is None:
        return None
    w = np.asarray(weights)
    if w.shape != (N,) or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
        raise ValueError(f"weights must be {N} numbers, one per row")
    with np.errstate(over="ignore"):
        w = w.astype(np.float32)
    if not np.isfinite(w).all():
        raise ValueError("the weights hold values that are not finite")
    if (w < 0).any():
        raise ValueError("the weights hold negative values")
    return w


def _prepare(N: int, D: int, nonzero, budget, seeds, weights, first):
    """Item 8, and item 7's already-chosen rows: ``(budget, weights [N] or None, chosen archive rows in order, first or None)``."""
    n = int(nonzero.size)
    budget = check_budget(budget)
    if D > MAX_D:
        raise ValueError(f"embedding width {D} above {MAX_D}")
    if n < 2:
        raise ValueError(f"selection needs at least 2 non-zero rows, the archive holds {n}")
    if n > MAX_N:
        raise ValueError(f"{n} non-zero rows: a run holds at most {MAX_N}")
    weights = check_weights(weights, N)
    live = np.zeros(N, bool)
    live[nonzero] = True
    chosen: list[int] = []
    if seeds is not None:
        s = np.asarray(seeds)
        if s.ndim != 1 or (s.size and not np.issubdtype(s.dtype, np.integer)):
            raise ValueError("seeds must be a list of row numbers")
        if s.size and (s.min() < 0 or s.max() >= N):
            raise ValueError(f"seeds hold rows outside 0..{N - 1}")
        chosen = [int(r) for r in dict.fromkeys(s.tolist()) if live[r]]
    if first is not None:
        first = int(first)
        if not 0 <= first < N:
            raise ValueError(f"first {first} outside 0..{N - 1}")
        if not live[first]:
            raise ValueError(f"first {first} is a zero row")
        if first not in chosen:
            chosen.append(first)
    if budget > n - len(chosen):
        raise ValueError(f"budget {budget} above the {n - len(chosen)} non-zero rows that are not chosen already")
    return budget, weights, chosen, first


def _select(N: int, nonzero, chosen, first, forced, computed: bool, budget: int, min_key, run) -> SelectResult:
    """Items 7 and 9 around ``run(forced, steps) -> (picked [steps], key [steps], m [n], nearest [n])`` over the live rows, which starts
    from the empty state every time; then live rows back to archive rows."""
    lead = len(forced) - int(computed)   # entries of a run that are no picks
    picked, key, m, near = run(forced, lead + budget)
    picked, key = np.asarray(picked, np.int64)[lead:], np.array(key, np.float32)[lead:]
    if computed:
        key[0] = F32_INF
    stop = np.flatnonzero((picked < 0) | (key < np.float32(min_key)))
    if stop.size:
        picked, key = picked[:stop[0]], key[:stop[0]]
        _, _, m, near = run(forced, lead + int(stop[0]))
    nearest = np.full(N, -1, np.int64)
    similarity = np.full(N, np.nan, np.float32)
    near = np.asarray(near, np.int64)
    nearest[nonzero] = np.where(near >= 0, nonzero[np.maximum(near, 0)], -1)
    m = np.asarray(m, np.float32)
    similarity[nonzero] = np.where(m == F32_INF, np.float32(1), m)
    return SelectResult(nonzero[picked], key, nearest, similarity, np.asarray(chosen, np.int64), -1 if first is None else int(first), nonzero)


def select_reference(rows, budget: int, seeds=None, weights=None, first=None, min_key: float = 0.0, zero_point: int = 0) -> SelectResult:
    """Items 1-9 in numpy, for small N."""
    rows, nonzero = _rows_and_nonzero(rows, zero_point)
    N, n = rows.shape[0], int(nonzero.size)
    budget, weights, chosen, first = _prepare(N, rows.shape[1], nonzero, budget, seeds, weights, first)
    live = np.ascontiguousarray(rows[nonzero])
    inv = inv_norms_reference(live, zero_point)
    pos = np.full(N, -1, np.int64)
    pos[nonzero] = np.arange(n)
    computed = not chosen
    forced = [central_reference(live, zero_point)] if computed else [int(pos[r]) for r in chosen]
    if computed:
        first = int(nonzero[forced[0]])
    w_live = None if weights is None else weights[nonzero]

    def run(forced, steps):
        m, nearest = np.full(n, -F32_INF, np.float32), np.full(n, -1, np.int32)
        picked, key = run_reference(live, inv, m, nearest, forced, len(forced), steps, w_live, zero_point)
        return picked, key, m, nearest

    return _select(N, nonzero, chosen, first, forced, computed, budget, min_key, run)


# ---------------------------------------------------------------------------------------------------------------------- device
def device_bytes_needed(n: int, D: int, itemsize: int) -> int:
    """What a run keeps on the device: the rows, inverse norms, weights, the state, and the most central row's temporaries."""
    return n * D * itemsize + n * 28 + 3 * D * 4 + (1 << 20)


def device_central(ctx, d_rows, code: int, n: int, D: int, zero_point: int, d_inv, sp) -> int:
    """The most central of the rows on the device (item 7): ``bn_kmeans_accumulate``, ``bn_kmeans_centroids`` and ``bn_kmeans_assign`` with
    one cluster; the host reads the n scores once and takes the first maximum."""
    import torch

    from birdnet_stm32 import _hip

    dev, lib, h = d_rows.device, ctx.lib, ctx.handle
    d_label = torch.zeros(n, dtype=torch.int32, device=dev)
    d_sums = torch.zeros((1, D), dtype=torch.float32, device=dev)
    d_counts = torch.zeros(1, dtype=torch.int64, device=dev)
    d_cent = torch.zeros((1, D), dtype=torch.float32, device=dev)
    d_cinv = torch.zeros(1, dtype=torch.float32, device=dev)
    d_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_score = torch.empty(n, dtype=torch.float32, device=dev)
    d_changed = torch.zeros(1, dtype=torch.int64, device=dev)
    _hip.check(lib.bn_kmeans_accumulate(h, d_rows.data_ptr(), code, n, D, zero_point, d_inv.data_ptr(), d_label.data_ptr(), 1, 0, d_sums.data_ptr(),
                                        d_counts.data_ptr(), sp))
    _hip.check(lib.bn_kmeans_centroids(h, d_sums.data_ptr(), d_counts.data_ptr(), 1, D, d_cent.data_ptr(), d_cinv.data_ptr(), sp))
    _hip.check(lib.bn_kmeans_assign(h, d_rows.data_ptr(), code, n, D, zero_point, d_inv.data_ptr(), d_cent.data_ptr(), d_cinv.data_ptr(), 1, None,
                                    d_out.data_ptr(), d_score.data_ptr(), d_changed.data_ptr(), sp))
    return int(np.argmax(d_score.cpu().numpy()))


def select_index(index, budget: int, seeds=None, weights=None, first=None, min_key: float = 0.0, device: int = 0, ctx=None) -> SelectResult:
    """``budget`` rows of an ``EmbeddingIndex`` chosen on the device.  The non-zero rows go to the device in one piece, whatever the index's
    block budget: an archive that does not fit is refused.  Seeds and ``first`` are the forced prefix of one ``bn_select_run``."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    rows, zp = index.embeddings, index.zero_point
    N, D = len(index), index.dim
    nonzero = np.flatnonzero(inv_norms_reference(rows, zp) != 0)
    n = int(nonzero.size)
    budget, weights, chosen, first = _prepare(N, D, nonzero, budget, seeds, weights, first)
    ctx = index.context(ctx, device)
    need = device_bytes_needed(n, D, rows.dtype.itemsize)
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if need > free:
        raise ValueError(f"the archive does not fit on the device in one piece: {n} rows x {D} need about {need >> 20} MiB, {free >> 20} MiB are "
                         f"free (archives larger than device memory are out of scope)")
    live = rows if n == N else np.ascontiguousarray(rows[nonzero])
    pos = np.full(N, -1, np.int64)
    pos[nonzero] = np.arange(n)
    dev = torch.device("cuda", ctx.device)
    code, lib, h = index.dtype_code, ctx.lib, ctx.handle
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_rows = torch.from_numpy(live).to(dev)
        d_inv = torch.empty(n, dtype=torch.float32, device=dev)
        _hip.check(lib.bn_search_inv_norms(h, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), sp))
        d_w = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights[nonzero])).to(dev)
        computed = not chosen
        forced = [device_central(ctx, d_rows, code, n, D, zp, d_inv, sp)] if computed else [int(pos[r]) for r in chosen]
        if computed:
            first = int(nonzero[forced[0]])

        def run(forced, steps):
            with torch.cuda.device(dev):
                d_m = torch.full((n,), -math.inf, dtype=torch.float32, device=dev)
                d_nearest = torch.full((n,), -1, dtype=torch.int32, device=dev)
                host_picked = np.full(max(steps, 1), -1, np.int32)
                host_picked[:len(forced)] = forced
                d_picked = torch.from_numpy(host_picked).to(dev)
                d_key = torch.full((max(steps, 1),), math.nan, dtype=torch.float32, device=dev)
                _hip.check(lib.bn_select_run(h, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                             d_m.data_ptr(), d_nearest.data_ptr(), d_picked.data_ptr(), len(forced), steps, d_key.data_ptr(), sp))
                return d_picked.cpu().numpy()[:steps], d_key.cpu().numpy()[:steps], d_m.cpu().numpy(), d_nearest.cpu().numpy()

        return _select(N, nonzero, chosen, first, forced, computed, budget, min_key, run)
