"""Density clustering: HDBSCAN over the rows of archives written by ``embed`` — no K, clusters of any size, an explicit noise label.

``hdbscan_reference`` is the specification in numpy (dense pairs, for small N); ``density_index`` runs the same fit with the all-pairs
work on the device (``csrc/bn_density.hip``, C ABI ``bn_density_nearest``; core scores from ``bn_search_topk``).  Both share every
host-side step: the argument checks, the Borůvka loop (``boruvka``) and the hierarchy (``hierarchy``).  The metric is the cosine, and
everything up to the spanning tree is worked out in score space; distances are formed on the host afterwards.

1. Rows.  ``[N, D]`` float32, or int8 bytes with a zero point, with ``search``'s meaning.  Zero rows (``inv_norms_reference`` gives 0) take
   no part and come back with label -1 and score 0; ``n`` is the number of the others, and fewer than 2 is refused.
2. Pair score.  ``s_ij = fl(dot_ij * fl(inv_i * inv_j))``, ``dot`` and ``inv`` as in ``search``: the float32 dot product has a free
   summation order, the int8 one is exact int32 over ``byte - zero_point`` rounded once to float32.  One value per pair, whichever end it
   is looked at from.
3. Core score.  ``c_i`` is the ``(min_samples - 1)``-th best cosine score of ``search`` with row i as the query against the other non-zero
   rows (``search_reference`` / ``bn_search_topk`` unchanged, every row its own group); ``+inf`` for ``min_samples = 1``.  The count
   includes the point itself, as scikit-learn's ``min_samples`` does.
4. Mutual reachability.  ``m_ij = min(s_ij, c_i, c_j)``, a negative zero counting as the positive one.
5. Total order on edges.  ``m`` descending, then ``min(i, j)`` ascending, then ``max(i, j)`` ascending.  The spanning tree is the unique
   maximum spanning tree under this order.  ``mst_reference`` is Kruskal over all pairs.  ``boruvka`` is the loop both backends share: each
   round ``backend.nearest(comp)`` gives for every row its best ``(m, j)`` over the rows of other components — ``m`` descending, then ``j``
   ascending, which agrees with the edge order for the edges at one vertex; the host takes each component's best edge under the edge
   order, drops the duplicate of a pair chosen from both ends, unites, and relabels every component by its smallest row.
6. Distances (host, float64).  ``d = sqrt(max(0, 2 - 2 m))``, the chord between unit vectors; ``lambda = 1 / max(d, 2^-12)``.  Every
   non-zero ``d`` a float32 ``m`` gives is above ``2^-12`` (the smallest is ``sqrt(2 * 2^-24)``), so only duplicates are capped.
7. Hierarchy (host; ``hierarchy``).  The single-linkage tree is built from the tree's edges in the total order.  It is condensed from the
   root downwards with ``min_cluster_size``: at a split at ``lambda`` a side with fewer rows than that falls out of its cluster, every
   row of it with this ``lambda``; two sides that both reach it become two new clusters born at ``lambda``; with one such side the
   cluster goes on.  ``stability(C) = sum over the rows that fell out of C of (lambda_p - birth(C)) + sum over the child clusters of
   (birth(child) - birth(C)) * size(child)``, the root born at 0.  Selection is excess of mass: from the leaves upwards a cluster is kept
   when its stability is at least the sum of its children's (kept or passed up), which are then dropped; the root is never selected.
   A row belongs to the nearest selected cluster at or above the one it fell out of, or to none (label -1).
8. Membership.  ``score_p = min(lambda_p, L) / L`` with ``L`` the largest ``lambda`` among the selected cluster's own condensed-tree
   entries: the rows that fell out of it directly and the births of its children (scikit-learn 1.7's ``_get_probabilities``; with
   the cap of item 6 no ``lambda`` is infinite).  Noise has score 0.
9. Clusters are numbered by the smallest row they hold.  Exemplars are a cluster's members with the largest ``lambda_p``, the lowest row
   among equal ones.

Not built: leaf selection, ``cluster_selection_epsilon``, a single cluster, approximate trees from k-nearest-neighbour graphs, rows
sharded over GPUs.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K
from birdnet_stm32.evaluation.search import inv_norms_reference, search_reference

MAX_N = 1 << 20   # BN_DENSITY_MAX_N (include/birdnet_hip.h)
MIN_DISTANCE = 2.0 ** -12


# ------------------------------------------------------------------------------------------------------------------------- keys
def ordered_image(m) -> np.ndarray:
    """float32 -> uint32 whose unsigned order is the order of the floats (after ``+ 0``: no negative zero)."""
    u = (np.asarray(m, np.float32) + np.float32(0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def image_to_float(image) -> np.ndarray:
    u = np.asarray(image, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def make_keys(m, j) -> np.ndarray:
    """``(image of m) << 32 | (0xFFFFFFFF - j)`` as uint64: a larger key is a better pair."""
    return (ordered_image(m).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(j).astype(np.uint64))


def split_keys(keys):
    """``(m float32, j int64)`` of keys; ``(-inf, -1)`` for the key 0."""
    keys = np.asarray(keys, np.uint64)
    none = keys == 0
    m = image_to_float((keys >> np.uint64(32)).astype(np.uint32)).copy()
    j = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    m[none], j[none] = -np.inf, -1
    return m, j


# ----------------------------------------------------------------------------------------------------------------------- scores
def pair_scores(rows, zero_point: int = 0, dtype=np.float32) -> np.ndarray:
    """``s [n, n]`` of item 2, symmetric bit for bit (the upper triangle of the dot products, mirrored).  ``dtype=np.float64``: the reference
    of the bound tests, products and norms in float64."""
    rows = np.asarray(rows)
    if rows.dtype == np.int8:
        x = rows.astype(np.float64) - int(zero_point)   # (exact: the products stay far below 2^53)
        dot = (x @ x.T).astype(dtype)
    else:
        x = rows.astype(dtype)
        dot = x @ x.T
    dot = np.triu(dot) + np.triu(dot, 1).T
    if dtype == np.float32:
        inv = inv_norms_reference(rows, zero_point)
    else:
        xf = x.astype(np.float64)
        nrm = np.sqrt((xf * xf).sum(axis=1))
        inv = np.divide(1.0, nrm, out=np.zeros_like(nrm), where=nrm > 0)
    return (dot * (inv[:, None] * inv[None, :]).astype(dtype)).astype(dtype)


def core_scores_reference(rows, min_samples: int, zero_point: int = 0) -> np.ndarray:
    """``c [n]`` of item 3 for rows without a zero row."""
    n = rows.shape[0]
    if int(min_samples) == 1:
        return np.full(n, np.inf, np.float32)
    groups = np.arange(n)
    _, score = search_reference(rows, rows, int(min_samples) - 1, "cosine", zero_point=zero_point, db_group=groups, query_group=groups)
    return score[:, -1].astype(np.float32)


def mutual_reachability(s, core) -> np.ndarray:
    """``m [n, n]`` of item 4 (the diagonal means nothing)."""
    core = np.asarray(core, s.dtype)
    return np.minimum(np.minimum(s, core[:, None]), core[None, :]) + s.dtype.type(0)


def nearest_from_scores(m, comp) -> np.ndarray:
    """Keys [n] of ``bn_density_nearest`` from the dense ``m``: per row the best ``(m, j)`` over the rows j with ``comp[j] >= 0`` and
    ``comp[j] != comp[i]``; 0 where there is none or ``comp[i] < 0``."""
    comp = np.asarray(comp, np.int64)
    n = comp.shape[0]
    ok = (comp[None, :] >= 0) & (comp[:, None] >= 0) & (comp[None, :] != comp[:, None])
    masked = np.where(ok, m + m.dtype.type(0), -np.inf)
    j = np.argmax(masked, axis=1)   # (the first of equal maxima: the lowest row)
    return np.where(ok.any(axis=1), make_keys(masked[np.arange(n), j], j), np.uint64(0))


def nearest_reference(rows, core, comp, zero_point: int = 0) -> np.ndarray:
    """The specification of ``bn_density_nearest``: keys [n] uint64."""
    return nearest_from_scores(mutual_reachability(pair_scores(rows, zero_point), core), comp)


# ------------------------------------------------------------------------------------------------------------------------- tree
def _edge_order(m, lo, hi) -> np.ndarray:
    """Positions that sort edges by the total order of item 5."""
    return np.lexsort((hi, lo, -np.asarray(m, np.float64)))


def mst_reference(m):
    """Kruskal over all pairs of the dense ``m``: ``(edges [n - 1, 2] (min, max), weight [n - 1] float32)`` in the total order."""
    n = m.shape[0]
    lo, hi = np.triu_indices(n, 1)
    w = m[lo, hi]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    edges, weight = [], []
    for e in _edge_order(w, lo, hi):
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            edges.append((int(lo[e]), int(hi[e])))
            weight.append(w[e])
            if len(edges) == n - 1:
                break
    return np.asarray(edges, np.int64).reshape(-1, 2), np.asarray(weight, np.float32)


def boruvka(backend, n: int):
    """The spanning tree over a backend with ``nearest(comp int32 [n]) -> keys uint64 [n]``: ``(edges, weight, rounds)``, edges in the
    total order."""
    comp = np.arange(n, dtype=np.int32)
    rows = np.arange(n, dtype=np.int64)
    e_lo, e_hi, e_w = [], [], []
    count, rounds = 0, 0
    while count < n - 1:
        m, j = split_keys(backend.nearest(comp))
        rounds += 1
        have = np.flatnonzero(j >= 0)
        if have.size == 0:
            raise RuntimeError("a round found no edge between components")
        lo, hi, w, c = np.minimum(rows[have], j[have]), np.maximum(rows[have], j[have]), m[have], comp[have]
        order = np.lexsort((hi, lo, -w.astype(np.float64), c))   # per component: its edges in the edge order
        first = np.ones(order.size, bool)
        first[1:] = c[order][1:] != c[order][:-1]
        pick = order[first]
        pick = pick[np.unique(np.stack([lo[pick], hi[pick]], axis=1), axis=0, return_index=True)[1]]   # a pair chosen from both ends once
        # unite: the chosen edges join components, the smaller label is the root, so a set's root is its smallest row
        parent = {}

        def find(a):
            root = a
            while parent.get(root, root) != root:
                root = parent[root]
            while parent.get(a, a) != root:
                parent[a], a = root, parent[a]
            return root

        for e in pick:
            a, b = find(int(comp[lo[e]])), find(int(comp[hi[e]]))
            if a == b:
                raise RuntimeError("a round's edges close a cycle: the backend's order is not the edge order")
            parent[max(a, b)] = min(a, b)
        e_lo.append(lo[pick])
        e_hi.append(hi[pick])
        e_w.append(w[pick])
        count += pick.size
        new = np.arange(n, dtype=np.int32)
        for a in list(parent):
            new[a] = find(a)
        comp = new[comp]
    lo, hi, w = np.concatenate(e_lo), np.concatenate(e_hi), np.concatenate(e_w).astype(np.float32)
    order = _edge_order(w, lo, hi)
    return np.stack([lo[order], hi[order]], axis=1).astype(np.int64), w[order], rounds


# -------------------------------------------------------------------------------------------------------------------- hierarchy
def score_to_lambda(m) -> np.ndarray:
    """Item 6, float64."""
    d = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * np.asarray(m, np.float64)))
    return 1.0 / np.maximum(d, MIN_DISTANCE)


@dataclass
class Hierarchy:
    """The condensed tree and what was selected from it.  Clusters are numbered from the root (0) downwards, a parent before its children.
    ``parent`` / ``birth`` / ``size`` / ``stability`` / ``max_lambda`` / ``selected`` per cluster; ``point_cluster`` / ``point_lambda`` per
    row: the cluster it fell out of and when."""

    parent: np.ndarray
    birth: np.ndarray
    size: np.ndarray
    stability: np.ndarray
    max_lambda: np.ndarray
    selected: np.ndarray
    point_cluster: np.ndarray
    point_lambda: np.ndarray
    labels: np.ndarray
    score: np.ndarray
    cluster_stability: np.ndarray


def hierarchy(edges, weight, n: int, min_cluster_size: int) -> Hierarchy:
    """Items 6 to 9 from the tree's edges in the total order."""
    mcs = int(min_cluster_size)
    lam_edge = score_to_lambda(weight)
    # ---- single linkage: node n + e joins the sets of edge e's two ends
    left, right = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64)
    size = np.ones(2 * n - 1, np.int64)
    uf, top = list(range(n)), list(range(n))   # union-find over rows; per root the tree node of its set

    def find(a):
        while uf[a] != a:
            uf[a] = uf[uf[a]]
            a = uf[a]
        return a

    for e in range(n - 1):
        a, b = find(int(edges[e, 0])), find(int(edges[e, 1]))
        left[e], right[e] = top[a], top[b]
        size[n + e] = size[top[a]] + size[top[b]]
        uf[b] = a
        top[a] = n + e
    # ---- the rows below every node as a range of one ordering
    start = np.zeros(2 * n - 1, np.int64)
    for node in range(2 * n - 2, n - 1, -1):
        start[left[node - n]] = start[node]
        start[right[node - n]] = start[node] + size[left[node - n]]
    leaves = np.empty(n, np.int64)
    leaves[start[:n]] = np.arange(n)

    def below(node):
        return leaves[start[node]:start[node] + size[node]]

    # ---- condense, from the root downwards
    node_cluster = np.full(2 * n - 1, -1, np.int64)
    node_cluster[2 * n - 2] = 0
    parent, birth, csize = [-1], [0.0], [n]
    point_cluster, point_lambda = np.zeros(n, np.int64), np.zeros(n, np.float64)
    for node in range(2 * n - 2, n - 1, -1):
        c = node_cluster[node]
        if c < 0:
            continue
        lam = lam_edge[node - n]
        for child, other in ((left[node - n], right[node - n]), (right[node - n], left[node - n])):
            if size[child] < mcs:
                pts = below(child)
                point_cluster[pts], point_lambda[pts] = c, lam
            elif size[other] >= mcs:
                node_cluster[child] = len(parent)
                parent.append(c)
                birth.append(lam)
                csize.append(int(size[child]))
            else:
                node_cluster[child] = c
    parent, birth, csize = np.asarray(parent, np.int64), np.asarray(birth, np.float64), np.asarray(csize, np.int64)
    K = parent.shape[0]
    # ---- stability and the largest lambda of every cluster's own entries
    stability = np.zeros(K)
    np.add.at(stability, point_cluster, point_lambda - birth[point_cluster])
    max_lambda = np.zeros(K)
    np.maximum.at(max_lambda, point_cluster, point_lambda)
    if K > 1:
        np.add.at(stability, parent[1:], (birth[1:] - birth[parent[1:]]) * csize[1:])
        np.maximum.at(max_lambda, parent[1:], birth[1:])
    # ---- excess of mass, children before parents
    passed = stability.copy()
    below_sum = np.zeros(K)
    selected = np.ones(K, bool)
    selected[0] = False
    for c in range(K - 1, 0, -1):
        if stability[c] < below_sum[c]:
            selected[c] = False
            passed[c] = below_sum[c]
        below_sum[parent[c]] += passed[c]
    rep = np.full(K, -1, np.int64)   # the selected cluster at or above each cluster
    for c in range(1, K):
        rep[c] = rep[parent[c]] if rep[parent[c]] >= 0 else (c if selected[c] else -1)
    selected = rep == np.arange(K)
    # ---- labels by the smallest row, membership
    of = rep[point_cluster]
    labels = np.full(n, -1, np.int64)
    score = np.zeros(n, np.float64)
    member = of >= 0
    ids, first = np.unique(of[member], return_index=True)
    ids = ids[np.argsort(np.flatnonzero(member)[first], kind="stable")]
    number = np.full(K, -1, np.int64)
    number[ids] = np.arange(ids.size)
    labels[member] = number[of[member]]
    L = max_lambda[of[member]]
    score[member] = np.minimum(point_lambda[member], L) / L
    return Hierarchy(parent, birth, csize, stability, max_lambda, selected, point_cluster, point_lambda, labels, score, stability[ids])


def exemplars_of(labels, point_lambda, n_clusters: int, exemplars: int) -> np.ndarray:
    """``[K, exemplars]`` rows of item 9, -1 where a cluster has fewer members."""
    out = np.full((n_clusters, int(exemplars)), -1, np.int64)
    for c in range(n_clusters):
        members = np.flatnonzero(labels == c)
        best = members[np.lexsort((members, -point_lambda[members]))][:int(exemplars)]
        out[c, :best.size] = best
    return out


# -------------------------------------------------------------------------------------------------------------------------- fit
@dataclass
class DensityResult:
    """``labels`` [N] (-1: noise or a zero row), ``score`` [N] float64 membership, ``n_clusters``, ``stability`` [K], ``core`` [N] float32
    (NaN for a zero row), the tree as ``mst_edges`` [n - 1, 2] (rows of the input, ``(min, max)``) and ``mst_weight`` [n - 1] float32 in the
    total order, ``exemplar_idx`` [K, exemplars] (-1 where a cluster has fewer members) and the ``rounds`` the tree took."""

    labels: np.ndarray
    score: np.ndarray
    n_clusters: int
    stability: np.ndarray
    core: np.ndarray
    mst_edges: np.ndarray
    mst_weight: np.ndarray
    exemplar_idx: np.ndarray
    rounds: int


def check_density_args(n: int, min_cluster_size, min_samples, exemplars=0) -> tuple[int, int]:
    """Everything a fit over ``n`` non-zero rows refuses; returns ``(min_cluster_size, min_samples)`` with the default filled in."""
    check_density_flags(min_cluster_size, min_samples, exemplars)
    mcs = int(min_cluster_size)
    ms = mcs if min_samples is None else int(min_samples)
    if n < 2:
        raise ValueError(f"a fit needs at least 2 non-zero rows, the archive holds {n}")
    if n > MAX_N:
        raise ValueError(f"{n} non-zero rows: a tree holds at most {MAX_N}")
    if not 2 <= mcs <= n:
        raise ValueError(f"min_cluster_size={mcs} outside 2..{n} (the number of non-zero rows)")
    if not 1 <= ms <= min(n, SEARCH_MAX_K + 1):
        raise ValueError(f"min_samples={ms} outside 1..{min(n, SEARCH_MAX_K + 1)}: the point and the {SEARCH_MAX_K} neighbours `search` returns, "
                         f"and no more than the {n} non-zero rows")
    return mcs, ms


def check_density_flags(min_cluster_size, min_samples, exemplars=0) -> None:
    """What can be refused before the rows are known."""
    if int(min_cluster_size) < 2:
        raise ValueError(f"min_cluster_size={min_cluster_size} must be >= 2")
    if min_samples is not None and not 1 <= int(min_samples) <= SEARCH_MAX_K + 1:
        raise ValueError(f"min_samples={min_samples} outside 1..{SEARCH_MAX_K + 1}")
    if min_samples is None and int(min_cluster_size) > SEARCH_MAX_K + 1:
        raise ValueError(f"min_samples defaults to min_cluster_size={min_cluster_size}, above {SEARCH_MAX_K + 1}: pass min_samples")
    if int(exemplars) < 0:
        raise ValueError(f"exemplars={exemplars} must be >= 0")


def _rows_and_nonzero(rows, zero_point):
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be [N, D], got {rows.shape}")
    if rows.dtype != np.int8:
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError("the rows hold values that are not finite")
    return rows, np.flatnonzero(inv_norms_reference(rows, zero_point) != 0)


def _finish(N, nonzero, core, edges, weight, rounds, mcs, exemplars) -> DensityResult:
    n = nonzero.size
    h = hierarchy(edges, weight, n, mcs)
    labels, score = np.full(N, -1, np.int64), np.zeros(N, np.float64)
    labels[nonzero], score[nonzero] = h.labels, h.score
    K = int(h.cluster_stability.size)
    lam = np.zeros(N)
    lam[nonzero] = h.point_lambda
    full_core = np.full(N, np.nan, np.float32)
    full_core[nonzero] = core
    return DensityResult(labels, score, K, h.cluster_stability, full_core, nonzero[edges], np.asarray(weight, np.float32),
                         exemplars_of(labels, lam, K, exemplars), int(rounds))


class _NumpyBackend:
    """Dense: the mutual-reachability scores of all pairs, once."""

    def __init__(self, rows, zero_point, core):
        self.m = mutual_reachability(pair_scores(rows, zero_point), core)

    def nearest(self, comp):
        return nearest_from_scores(self.m, comp)


def hdbscan_reference(rows, min_cluster_size: int = 15, min_samples=None, zero_point: int = 0, exemplars: int = 5) -> DensityResult:
    """The fit of the module docstring in numpy over dense pairs: for small N."""
    rows, nonzero = _rows_and_nonzero(rows, zero_point)
    mcs, ms = check_density_args(int(nonzero.size), min_cluster_size, min_samples, exemplars)
    live = np.ascontiguousarray(rows[nonzero])
    core = core_scores_reference(live, ms, zero_point)
    edges, weight, rounds = boruvka(_NumpyBackend(live, zero_point, core), live.shape[0])
    return _finish(rows.shape[0], nonzero, core, edges, weight, rounds, mcs, exemplars)


# ---------------------------------------------------------------------------------------------------------------------- device
class _DeviceBackend:
    """Rows, inverse norms and cores stay on the device; per round the components go up and n keys come back."""

    def __init__(self, ctx, d_rows, d_inv, d_core, code, n, D, zero_point, sp):
        import torch

        from birdnet_stm32 import _hip

        self.torch, self.hip, self.ctx = torch, _hip, ctx
        self.d_rows, self.d_inv, self.d_core, self.code, self.n, self.D, self.zp, self.sp = d_rows, d_inv, d_core, code, n, D, zero_point, sp
        self.dev = torch.device("cuda", ctx.device)
        self.d_comp = torch.empty(n, dtype=torch.int32, device=self.dev)
        self.d_best = torch.empty(n, dtype=torch.int64, device=self.dev)

        self.round_s = []   # device time of every round's call, between two events

    def nearest(self, comp):
        torch = self.torch
        with torch.cuda.device(self.dev):
            self.d_comp.copy_(torch.from_numpy(np.ascontiguousarray(comp, np.int32)))
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            self.hip.check(self.ctx.lib.bn_density_nearest(self.ctx.handle, self.d_rows.data_ptr(), self.code, self.n, self.D, self.zp, self.d_inv.data_ptr(),
                                                           self.d_core.data_ptr(), self.d_comp.data_ptr(), self.d_best.data_ptr(), self.sp))
            t1.record()
            keys = self.d_best.cpu().numpy().view(np.uint64)
            self.round_s.append(t0.elapsed_time(t1) * 1e-3)
            return keys


def device_bytes_needed(n: int, D: int, itemsize: int, k: int) -> int:
    """What a fit keeps on the device at its largest: the rows, per row the inverse norm, core, group, component and key, the neighbour
    lists of the core scores, and ``search``'s workspace."""
    return n * D * itemsize + n * 24 + 2 * n * max(k, 1) * 4 + (128 << 20)


def device_cores(ctx, d_rows, d_inv, code, n: int, D: int, zero_point: int, min_samples: int, sp):
    """``c`` of item 3 as a device tensor: ``bn_search_topk`` of the rows against themselves, every row its own group."""
    import torch

    from birdnet_stm32 import _hip

    dev = torch.device("cuda", ctx.device)
    if min_samples == 1:
        return torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    k = min_samples - 1
    d_grp = torch.arange(n, dtype=torch.int32, device=dev)
    d_idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    d_score = torch.empty((n, k), dtype=torch.float32, device=dev)
    _hip.check(ctx.lib.bn_search_topk(ctx.handle, d_rows.data_ptr(), code, n, D, zero_point, d_inv.data_ptr(), d_rows.data_ptr(), n, d_inv.data_ptr(),
                                      _hip.SEARCH_METRICS["cosine"], d_grp.data_ptr(), d_grp.data_ptr(), k, d_idx.data_ptr(), d_score.data_ptr(), sp))
    return d_score[:, k - 1].contiguous()


def density_index(index, min_cluster_size: int = 15, min_samples=None, exemplars: int = 5, device: int = 0, ctx=None, timings=None) -> DensityResult:
    """The fit of the module docstring over the rows of an ``EmbeddingIndex``, the all-pairs work on the device.  The non-zero rows are
    resident in one piece, whatever the index's block budget (an index without zero rows that fits its budget shares the block ``search``
    keeps): an archive that does not fit is refused.  A dict given as ``timings`` comes back with ``cores_s`` and ``tree_s`` (host clock,
    ending in a device synchronise), ``round_s`` (per round, device events around the kernel) and ``hierarchy_s`` (host)."""
    import ctypes
    import time

    import torch

    from birdnet_stm32 import _hip

    rows, zp = index.embeddings, index.zero_point
    nonzero = np.flatnonzero(inv_norms_reference(rows, zp) != 0)
    n, D = int(nonzero.size), index.dim
    mcs, ms = check_density_args(n, min_cluster_size, min_samples, exemplars)
    ctx = index.context(ctx, device)
    need = device_bytes_needed(n, D, rows.dtype.itemsize, ms - 1)
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if need > free:
        raise ValueError(f"the archive does not fit on the device in one piece: {n} rows x {D} need about {need >> 20} MiB, "
                         f"{free >> 20} MiB are free (archives larger than device memory are out of scope)")
    dev = torch.device("cuda", ctx.device)
    code = index.dtype_code
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if n == len(index) and index.block_ranges() == [(0, n)]:
            d_rows, d_inv = index.device_block(ctx, 0, n, sp)[:2]
        else:
            d_rows = torch.from_numpy(np.ascontiguousarray(rows[nonzero])).to(dev)
            d_inv = torch.empty(n, dtype=torch.float32, device=dev)
            _hip.check(ctx.lib.bn_search_inv_norms(ctx.handle, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), sp))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        d_core = device_cores(ctx, d_rows, d_inv, code, n, D, zp, ms, sp)
        core = d_core.cpu().numpy()
        t1 = time.perf_counter()
        backend = _DeviceBackend(ctx, d_rows, d_inv, d_core, code, n, D, zp, sp)
        edges, weight, rounds = boruvka(backend, n)
        t2 = time.perf_counter()
    res = _finish(len(index), nonzero, core, edges, weight, rounds, mcs, exemplars)
    if timings is not None:
        timings.update(cores_s=t1 - t0, tree_s=t2 - t1, round_s=list(backend.round_s), hierarchy_s=time.perf_counter() - t2)
    return res
