"""Bootstrap intervals of the per-class average precision on the device (``bn_bootstrap_*``, csrc/bn_bootstrap.hip).

``metrics.bootstrap_ap_ci`` (reference: birdnet_stm32/evaluation/metrics.py:239-318) is the specification: one
``np.random.default_rng(seed)`` consumed class by class, ``rng.integers(0, n, size=n)`` per resample, one scikit-learn
``average_precision_score`` per resample.  On 4096 files x 100 classes x 1000 resamples that is 100 000 library calls.  Here the same
draws are reproduced on the device and a resample becomes a vector of multiplicities over the rows, applied to ONE descending
order per class.

The stream, restated (numpy 2.x; ``tests/test_bootstrap_host.py`` holds every line against the generator itself):

* PCG64: ``state = state * PCG64_MULT + inc (mod 2^128)``, output XSL-RR of the NEW state: ``x = hi ^ lo`` rotated right by
  ``state >> 122``.  ``rng.bit_generator.state`` gives ``state`` and ``inc``.
* ``integers`` with a bound <= 2^32 - 1 takes 32-bit values: of each 64-bit output the low half first, then the high half; the spare
  half carries over between calls, so consecutive calls read one continuous stream of *raw positions* 0, 1, 2, ...
* Lemire's bounding: ``m = x * n``, rejected when ``(m & 0xFFFFFFFF) < thr`` with ``thr = (2^32 - n) mod n``, else ``m >> 32``.
  Rejection depends on the raw value alone: the accepted draws are the raw stream with the rejected entries removed.

The functions ``*_reference`` are numpy / Python-integer specifications of what the kernels compute; ``bootstrap_ap_ci_device`` is the
public entry point.
"""

from __future__ import annotations

import warnings

import numpy as np

PCG64_MULT = 0x2360ED051FC65DA44385DF649FCCF645
MAX_N = 32768  # BN_BOOTSTRAP_MAX_N (include/birdnet_hip.h): rows per class the resample kernel's LDS counters hold
_M128 = (1 << 128) - 1
_M64 = (1 << 64) - 1


def ap_tolerance(n: int) -> float:
    """Bound on |device AP - average_precision_score|: the terms are bit-equal, only the order of the sum differs; a sum of at most n
    non-negative terms totalling <= 1 carries at most (n - 1) * 2^-53 error whatever its order, and there are two such sums."""
    return 2.0 * n * 2.0 ** -53


def lemire_threshold(n: int) -> int:
    return ((1 << 32) - n) % n


def generator_state(seed) -> tuple[int, int]:
    """``(state, inc)`` of a fresh ``np.random.default_rng(seed)``; refuses a generator that is not PCG64 or holds a spare half."""
    st = np.random.default_rng(seed).bit_generator.state
    if st.get("bit_generator") != "PCG64" or st.get("has_uint32", 0) != 0:
        raise RuntimeError("np.random.default_rng is not a fresh PCG64")
    return int(st["state"]["state"]), int(st["state"]["inc"])


def pcg64_advance(state: int, inc: int, delta: int) -> int:
    """The state after ``delta`` steps, in O(log delta) (the LCG jump-ahead: square the multiplier, fold the increment)."""
    acc_mult, acc_plus, cur_mult, cur_plus = 1, 0, PCG64_MULT, inc
    while delta > 0:
        if delta & 1:
            acc_mult = (acc_mult * cur_mult) & _M128
            acc_plus = (acc_plus * cur_mult + cur_plus) & _M128
        cur_plus = ((cur_mult + 1) * cur_plus) & _M128
        cur_mult = (cur_mult * cur_mult) & _M128
        delta >>= 1
    return (acc_mult * state + acc_plus) & _M128


def pcg64_raw32_reference(state: int, inc: int, start: int, count: int) -> np.ndarray:
    """uint32 [count]: raw positions ``start .. start + count`` of the 32-bit stream of a PCG64 at ``(state, inc)`` with no spare half:
    position 2 q is the low half of the generator's q-th next 64-bit output, 2 q + 1 its high half."""
    if count <= 0:
        return np.zeros(0, np.uint32)
    q0, q1 = start >> 1, (start + count + 1) >> 1
    s = pcg64_advance(state, inc, q0)
    out = np.empty(2 * (q1 - q0), np.uint32)
    for i in range(q1 - q0):
        s = (s * PCG64_MULT + inc) & _M128
        hi, lo = s >> 64, s & _M64
        x, rot = hi ^ lo, s >> 122
        v = ((x >> rot) | (x << ((-rot) & 63))) & _M64
        out[2 * i] = v & 0xFFFFFFFF
        out[2 * i + 1] = v >> 32
    return out[start - 2 * q0: start - 2 * q0 + count]


def _raw32_fast(state: int, inc: int, start: int, count: int) -> np.ndarray:
    """``pcg64_raw32_reference`` through numpy's own generator placed at the same state (the same stream, tested equal; fast)."""
    if count <= 0:
        return np.zeros(0, np.uint32)
    q0, q1 = start >> 1, (start + count + 1) >> 1
    bg = np.random.PCG64()
    bg.state = {"bit_generator": "PCG64", "state": {"state": pcg64_advance(state, inc, q0), "inc": inc}, "has_uint32": 0, "uinteger": 0}
    raw = bg.random_raw(q1 - q0)
    out = np.empty(2 * (q1 - q0), np.uint32)
    out[0::2] = raw & np.uint64(0xFFFFFFFF)
    out[1::2] = raw >> np.uint64(32)
    return out[start - 2 * q0: start - 2 * q0 + count]


def rejected_positions_reference(state: int, inc: int, bound: int, p_begin: int, p_end: int) -> np.ndarray:
    """int64, ascending: the raw positions in ``[p_begin, p_end)`` whose value Lemire's method rejects for ``bound`` (the rejection scan)."""
    thr = lemire_threshold(bound)
    if thr == 0 or p_end <= p_begin:
        return np.zeros(0, np.int64)
    m = _raw32_fast(state, inc, p_begin, p_end - p_begin).astype(np.uint64) * np.uint64(bound)
    return p_begin + np.flatnonzero((m & np.uint64(0xFFFFFFFF)) < np.uint64(thr)).astype(np.int64)


def bounded_draws_reference(state: int, inc: int, bound: int, count: int, start: int = 0) -> tuple[np.ndarray, int]:
    """``(draws int64 [count], raw positions consumed)``: what ``rng.integers(0, bound, size=count)`` returns for a PCG64 at
    ``(state, inc)`` whose next unread raw position is ``start``.  A bound of 1 consumes nothing, as in numpy."""
    if not 1 <= bound <= 0xFFFFFFFF:
        raise ValueError("bound outside 1 .. 2^32 - 1")
    if bound == 1 or count <= 0:
        return np.zeros(max(count, 0), np.int64), 0
    thr = np.uint64(lemire_threshold(bound))
    got, pos = [], start
    need = count
    while need > 0:
        take = need + need // 2 + 64 if thr else need
        m = _raw32_fast(state, inc, pos, take).astype(np.uint64) * np.uint64(bound)
        ok = np.flatnonzero((m & np.uint64(0xFFFFFFFF)) >= thr)
        if ok.size >= need:
            ok = ok[:need]
            pos += int(ok[-1]) + 1
        else:
            pos += take
        got.append((m[ok] >> np.uint64(32)).astype(np.int64))
        need -= ok.size
    return np.concatenate(got), pos - start


def resample_ranges(rejected, n: int, n_resamples: int, start: int = 0) -> np.ndarray:
    """int64 [n_resamples, 2]: the raw range ``[p0, p1)`` that holds resample b's ``n`` accepted draws, for consecutive resamples read
    from raw position ``start`` on.  ``rejected`` are the rejected raw positions >= start (any order); they must cover every position below
    the last ``p1`` (``ranges[-1, 1]``: the caller extends its scan and calls again when that passes what it scanned).  A range starts at
    its first accepted position and ends behind its last, so the ranges are disjoint and rejected positions between them belong to none."""
    r = np.sort(np.asarray(rejected, np.int64))
    r = r[r >= start]
    before = r - start - np.arange(r.size, dtype=np.int64)  # accepted positions in front of each rejected one (non-decreasing)
    first = np.arange(n_resamples, dtype=np.int64) * n
    last = first + (n - 1)
    out = np.empty((n_resamples, 2), np.int64)
    out[:, 0] = start + first + np.searchsorted(before, first, side="right")
    out[:, 1] = start + last + np.searchsorted(before, last, side="right") + 1
    return out


def ap_from_counts_reference(counts, truth_desc, score_desc) -> float:
    """Average precision of the resample that takes row k of a class's descending order ``counts[k]`` times — the kernel's arithmetic:
    integer prefix sums ``seen`` and ``tps`` of the multiplicities, and at the end of every run of equal scores with ``seen > 0`` the term
    ``(fl(tps / K) - fl(tps_prev / K)) * fl(tps / seen)`` in float64, summed left to right.  NaN when the resample has no positive or no
    negative (``K in {0, n}``): the reference drops it."""
    w = np.asarray(counts, np.int64)
    t = np.asarray(truth_desc).astype(bool)
    s = np.asarray(score_desc)
    seen = np.cumsum(w)
    tps = np.cumsum(w * t)
    total, K = int(seen[-1]), int(tps[-1])
    if K == 0 or K == total:
        return float("nan")
    last = np.r_[np.flatnonzero(np.diff(s)), s.size - 1]
    last = last[seen[last] > 0]
    tp = tps[last].astype(np.float64)
    recall = tp / np.float64(K)
    precision = tp / seen[last].astype(np.float64)
    ap = 0.0
    for term in (recall - np.r_[0.0, recall[:-1]]) * precision:
        ap += float(term)
    return ap


# ---------------------------------------------------------------------------------------------------------------------- device
def _gen_args(state: int, inc: int):
    from ctypes import c_uint64

    return c_uint64(state >> 64), c_uint64(state & _M64), c_uint64(inc >> 64), c_uint64(inc & _M64)


def rejected_positions_device(ctx, state: int, inc: int, bound: int, p_begin: int, p_end: int, capacity: int | None = None) -> np.ndarray:
    """``bn_bootstrap_rejections``: the rejected raw positions in ``[p_begin, p_end)``, ascending (the device appends in any order)."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    thr = lemire_threshold(bound)
    if thr == 0 or p_end <= p_begin:
        return np.zeros(0, np.int64)
    if capacity is None:  # mean + 8 sigma of a binomial, and room for short scans
        mean = (p_end - p_begin) * thr / 2.0 ** 32
        capacity = int(mean + 8.0 * mean ** 0.5) + 64
    with torch.cuda.device(ctx.device):
        stream = torch.cuda.current_stream()
        out = np.empty(capacity, np.int64)
        count = ctypes.c_int64(0)
        _hip.check(ctx.lib.bn_bootstrap_rejections(ctx.handle, *_gen_args(state, inc), ctypes.c_uint32(bound), p_begin, p_end, out.ctypes.data, capacity,
                                                   ctypes.byref(count), ctypes.c_void_p(stream.cuda_stream)))
    return np.sort(out[: count.value])


def device_ranges(ctx, state: int, inc: int, n: int, n_resamples: int, start: int = 0) -> np.ndarray:
    """``resample_ranges`` with the rejection scan on the device: scan a little more than the accepted draws need, extend while the last
    range passes what was scanned."""
    thr = lemire_threshold(n)
    if thr == 0:
        return resample_ranges(np.zeros(0, np.int64), n, n_resamples, start)
    total = n * n_resamples
    rate = thr / 2.0 ** 32
    scanned = start
    rejected = np.zeros(0, np.int64)
    goal = start + total + int(total * rate * 1.25) + 16
    while True:
        rejected = np.concatenate([rejected, rejected_positions_device(ctx, state, inc, n, scanned, goal)])
        scanned = goal
        ranges = resample_ranges(rejected, n, n_resamples, start)
        if int(ranges[-1, 1]) <= scanned:
            return ranges
        goal = int(ranges[-1, 1]) + max(16, (int(ranges[-1, 1]) - scanned) // 4)


def bootstrap_counts_device(ctx, state: int, inc: int, n: int, ranges: np.ndarray, out=None):
    """``bn_bootstrap_counts``: uint32 [B, n] multiplicities of the resamples whose raw ranges are ``ranges`` [B, 2].  ``out`` (an int32
    CUDA tensor [B, n]) is written in place when given."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    ranges = np.ascontiguousarray(ranges, np.int64)
    B = ranges.shape[0]
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        d_ranges = torch.from_numpy(ranges).to(dev)
        d_counts = out if out is not None else torch.empty((B, n), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        _hip.check(ctx.lib.bn_bootstrap_counts(ctx.handle, *_gen_args(state, inc), n, B, d_ranges.data_ptr(), d_counts.data_ptr(),
                                               ctypes.c_void_p(stream.cuda_stream)))
        return d_counts.cpu().numpy().view(np.uint32)


def bootstrap_ap_device(ctx, state: int, inc: int, scores: np.ndarray, truth: np.ndarray, class_ids, n_resamples: int, ranges: np.ndarray,
                        out=None):
    """``bn_bootstrap_ap``: float64 [len(class_ids), n_resamples] APs (NaN: dropped resample) and the per-class descending orders
    int32 [C, n].  ``scores`` float32 [n, C], ``truth`` uint8 [n, C] of 0/1, ``ranges`` int64 [len(class_ids) * n_resamples, 2] in class
    order.  ``out`` (a float64 CUDA tensor of the result's shape) is written in place when given."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    s = np.ascontiguousarray(scores, np.float32)
    t = np.ascontiguousarray(truth, np.uint8)
    n, C = s.shape
    ids = np.ascontiguousarray(class_ids, np.int32)
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        sp = ctypes.c_void_p(stream.cuda_stream)
        d_s = torch.from_numpy(s).to(dev)
        d_t = torch.from_numpy(t).to(dev)
        d_cols = torch.empty((C, n), dtype=torch.int32, device=dev)
        d_flat = torch.empty(n * C, dtype=torch.int32, device=dev)
        _hip.check(ctx.lib.bn_rank_orders(ctx.handle, d_s.data_ptr(), n, C, d_cols.data_ptr(), d_flat.data_ptr(), sp))
        d_ap = out if out is not None else torch.empty((ids.size, n_resamples), dtype=torch.float64, device=dev)
        if ids.size and n_resamples:
            d_ids = torch.from_numpy(ids).to(dev)
            d_ranges = torch.from_numpy(np.ascontiguousarray(ranges, np.int64)).to(dev)
            _hip.check(ctx.lib.bn_bootstrap_ap(ctx.handle, *_gen_args(state, inc), n, C, d_s.data_ptr(), d_t.data_ptr(), d_cols.data_ptr(), d_ids.data_ptr(),
                                               int(ids.size), int(n_resamples), d_ranges.data_ptr(), d_ap.data_ptr(), sp))
        return d_ap.cpu().numpy(), d_cols.cpu().numpy()


_guard_passed: bool | None = None  # the numpy guard's verdict, taken once per process


def _counts_match(device_counts: np.ndarray, numpy_counts: np.ndarray) -> bool:
    return bool(np.array_equal(device_counts, numpy_counts))


def numpy_stream_guard(ctx, n: int, seed) -> bool:
    """numpy does not promise the stream of ``Generator.integers`` across versions: the first use in a process compares the device's first
    resample with numpy's own (``n`` draws below ``n`` from a fresh generator)."""
    global _guard_passed
    if _guard_passed is None:
        try:
            state, inc = generator_state(seed)
            got = bootstrap_counts_device(ctx, state, inc, n, device_ranges(ctx, state, inc, n, 1))[0]
        except RuntimeError as e:
            if "PCG64" not in str(e):
                raise
            got = None
        want = np.bincount(np.random.default_rng(seed).integers(0, n, size=n), minlength=n)
        _guard_passed = got is not None and _counts_match(got, want)
    return _guard_passed


def bootstrap_ap_ci_device(y_true: np.ndarray, y_scores: np.ndarray, classes: list[str], n_bootstrap: int = 1000, confidence: float = 0.95,
                           seed: int = 42, ctx=None) -> list[dict]:
    """``metrics.bootstrap_ap_ci`` with the resamples on the device of ``ctx`` (a ``_hip.Context``): the same list of dicts, ``ap`` equal,
    ``ci_lower`` / ``ci_upper`` within ``ap_tolerance(n)``.  Falls back to the host function, with a ``RuntimeWarning``, when the input is
    outside what the kernels take (more than ``MAX_N`` rows, scores that are not finite float32, labels that are not 0/1) or when numpy's
    stream is not the one restated here."""
    from birdnet_stm32.evaluation._ranking import average_precision_desc
    from birdnet_stm32.evaluation.metrics import bootstrap_ap_ci

    def host(why: str):
        warnings.warn(f"bootstrap_ap_ci_device: {why}; computing the intervals on the host", RuntimeWarning, stacklevel=3)
        return bootstrap_ap_ci(y_true, y_scores, classes, n_bootstrap=n_bootstrap, confidence=confidence, seed=seed)

    if ctx is None:
        raise ValueError("bootstrap_ap_ci_device needs the runner's context (ctx)")
    yt, ys = np.asarray(y_true), np.asarray(y_scores)
    if yt.ndim != 2 or ys.shape != yt.shape or len(classes) > yt.shape[1]:
        raise ValueError("y_true and y_scores must be [files, classes] matrices of one shape")
    n = yt.shape[0]
    if n > MAX_N:
        return host(f"{n} rows exceed the device limit of {MAX_N}")
    if ys.dtype != np.float32 or not np.isfinite(ys).all():
        return host("the scores are not finite float32")
    truth = yt == 1
    if not np.logical_or(truth, yt == 0).all():
        return host("y_true is not a 0/1 indicator matrix")
    n_cls = len(classes)
    pos = truth[:, :n_cls].sum(axis=0).astype(np.int64)
    ids = [c for c in range(n_cls) if 0 < pos[c] < n]
    B = int(n_bootstrap) if ids else 0
    if n == 0:
        return host("no rows")
    if not numpy_stream_guard(ctx, n, seed):
        return host("numpy's integers() stream is not the one the kernels reproduce")
    state, inc = generator_state(seed)
    ranges = device_ranges(ctx, state, inc, n, len(ids) * B) if B > 0 else np.zeros((0, 2), np.int64)
    aps, cols = bootstrap_ap_device(ctx, state, inc, ys, truth.astype(np.uint8), ids, max(B, 0), ranges)
    tail = (1.0 - confidence) / 2.0
    row_of = {c: i for i, c in enumerate(ids)}
    rows = []
    lacking = 0
    for c, name in enumerate(classes):
        o = cols[c]
        lacking += pos[c] == 0
        ap = average_precision_desc(truth[o, c], ys[o, c])
        lo = hi = ap
        if c in row_of and B > 0:
            draws = aps[row_of[c]]
            draws = draws[~np.isnan(draws)]
            if draws.size:
                lo, hi = float(np.percentile(draws, 100 * tail)), float(np.percentile(draws, 100 * (1 - tail)))
        rows.append({"class": name, "ap": ap, "ci_lower": lo, "ci_upper": hi, "n_positive": int(pos[c]), "n_total": n})
    if lacking:  # (the library's warning, once instead of per class)
        warnings.warn(f"No positive class found in y_true for {lacking} of {n_cls} classes, recall is set to one for all thresholds.", UserWarning, stacklevel=2)
    return rows
