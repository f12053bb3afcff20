"""Float64 reference of the float32 device plan, operator by operator, with a per-element rounding bound.

A helper, not a test: numpy only, no torch, no GPU.  It reads what the device gets — ``plan.ops``, ``PlanOp.get(...)`` and the float32
constants in ``plan.tensors`` — and evaluates ONE operator on given float32 inputs: :func:`eval_op` returns the float64 value of the
operator and a bound on ``|device - value|`` for every element.  :func:`walk_plan` takes a whole plan through it, feeding every operator the
arrays a caller-supplied ``fetch`` returns for the operator that produced its inputs (the device's own outputs, or the oracle's layer
outputs: teacher forcing); where ``fetch`` has nothing (a map a fused kernel kept on chip, an operator that is overwritten in place) the
reference value AND its bound are carried into the next operator, so the pair is held as one composite from the last readable input.

The bound (derived here, never fitted to device output)
-------------------------------------------------------
``u = 2^-24`` (unit round-off of float32, round to nearest).  Every float32 operation returns ``exact (1 + d)``, ``|d| <= u``.

*Linear stage* ``y = act(sum_{i<K} w_i x_i + b [+ r])``.  Write ``A = sum |w_i x_i| + |b| [+ |r|]`` (float64).  A term that passes through
``n`` roundings carries a factor ``prod (1 + d_j)``, off from 1 by at most ``n u`` to first order (``gamma_n`` exactly; the difference
``n^2 u^2`` is below ``1e-9`` of the bound for every K here and is covered by counting ``n`` generously).  Hence ``|dy| <= n u A``.
Counting ``n`` from the kernels (csrc/bn_f32.hip, bn_f32_fused.hip, bn_f32_strip.hip, bn_f32_pw.hip): ``n`` is the number of roundings ONE term
``w_i x_i`` passes through — its own product when that is not fused (1; the roundings of the other products do not touch it) and every
addition its partial sum takes part in.  The K terms and the bias are K + 1 values, joined by K additions in whatever grouping; one value
passes through at most K of them.  The baseline kernels are chains of ``fmaf`` started at the bias (the first term: K roundings, no separate
product); the fused kernels run the same sums as ``v_mfma_f32_16x16x4_f32`` steps — the stem and the pointwise stage of every fused and
strip kernel, split-K partial sums in the workgroup-split pointwise kernel.  The order inside such a step is not documented, so it is
counted as four separate products and four additions: a term then has its product and at most 4 additions in its own step and 4 in
every later one, K in all.  One operator may run as either form (that is what the launcher options switch), so every stage takes the larger:

    1 product + K additions (bias included)                        n = K + 1
    + 1 when a gate multiplies the input channels (one more rounding on every term)
    + 1 when a residual is added

i.e. ``n = K + 1 + has_gate + has_res <= K + 3``, inside the cap ``2 K + 4``.  ReLU and ReLU6 are exact and 1-Lipschitz: nothing added.
Per kind: STEM, DW: K = 9, n = 10.  PW, the pointwise stage of DWPW / FRONT: K = Cin, n = Cin + 1 (+1 gate, +1 residual).  MEL: K = the
band length of the mel row, n = len + 1.  RAWFE: K = 16, n = 17.  DENSE / GAPDENSE classifier: K = Cin, n = Cin + 1.  SEGATE dense layers:
K = C and K = Cr without bias, n = K + 1 kept.  ATTNPOOL scores: K = C; its weighted sum: K = P with weights that carry their own error.

*Input error.*  An input known only within ``e_i`` (the inner stage of a fused operator, the unreadable map of a composite) reaches the
stage as ``sum |w_i| e_i`` (plus ``|x| e_g + |g| e_x + e_x e_g`` through a gate, ``e_r`` through a residual), added to the stage's own term.
DWPW, FRONT, GAPDENSE, SEGATE chain their stages this way.

*Mean over P positions* (GAP, the pooling of SEGATE / GAPDENSE): P - 1 additions in any grouping (per-strip partial sums included: still
additions, at most P - 1 on one term) and one division: ``(P - 1 + D) u sum |x| / P``, D the division's error in u (below).

*Products and quotients of two computed values* (SCALE, MAG's ``y / (max + 1e-6)``): first-order propagation plus the operation's own
rounding, ``|a| e_b + |b| e_a + e_a e_b + u |a b|`` and ``(e_a + |q| e_b) / (|b| - e_b) + D u |q|``.  A maximum is exact and moves by at most
the largest input error.  The magnitude scalings (``pwl``, ``pcen``) are linear stages of K = 1, 2 and 4 per element, chained.

*Library functions.*  The build has no fast-math flag, so ``expf``, ``logf`` and ``/`` are the precise device-library functions.  No copy of
the HIP math documentation with its ULP table was found under the ROCm tree used to write this file, so the OpenCL full-profile figures
are used: 3 ulp for exp and log, 2.5 ulp for division; one ulp is at most ``2 u`` relative, so E = L = 6 u and D = 5 u.
Sigmoid ``1 / (1 + exp(-s))``: 1/4-Lipschitz in s; its own arithmetic moves it by at most ``(E + 1 + D) u = 12 u`` relative (the exponential's
relative error enters the denominator with weight ``e / (1 + e) < 1``).  Softmax over C logits with input error ``e_z`` (restating
``softmax_bound`` of tests/test_gpu_head_export.py with the figures above): the argument ``z - max`` is off by ``2 e_z`` and one rounding
``u |z - max| <= 2 u a`` (a = the row's largest |z|), so every exponential by the factor ``t = 2 e_z + 2 u a + E u``, their sum of C terms by
``t + (C - 1) u``, the quotient by ``D u`` more: ``|dP| <= P (2 t + (C - 1 + D) u)``.  Attention pooling uses the same weights over P positions,
then a K = P sum whose weights carry that error.

*Floor.*  ``2^-126`` per element is added (results that underflow to subnormals).  Nothing else is.

*Audio entry.*  ``F32_STFTMEL`` is ``stft512_mag_kernel`` with its ``MEL_OUT`` switch: the operations up to the magnitudes are the ones
docs/exactness.md walks through, so the per-frame bound proven there, ``|S' - S| <= 1148 u ||x_t||_2 + 14 u S'``, is taken as the input error of
the mixer, which in this instantiation is an ``fmaf`` chain over the band started at zero (len roundings on the first term; n = len + 1 is
kept).  ``F32_MELFIN`` and the finalising ``F32_FRONT`` compute ``relu((raw - mn wsum) / rng)`` from the chunk's minimum and maximum of S'.
Those are exact reductions of the device's own magnitudes, so the tests OBSERVE them (``bn_stft_mag`` returns them from the same kernel's
arithmetic on the same audio) and hand them over with error 0, like every other operator input; the finalisation's bound is then a few u:
``rng = (float)((double)(mx - mn) + 1e-10)`` two roundings; ``mn wsum`` one; the subtraction one more (a fused multiply-subtract has fewer) —
in terms of ``|raw|`` and ``|mn wsum|``, not of the (possibly cancelled) result; then a division per element (MELFIN) or one reciprocal and a
product (FRONT).  Without observed extremes (a caller that has none) the reference's own are used, and the largest element bound of the
chunk is carried through ``mn wsum`` and ``rng``: hundreds of times looser, for want of the input.
"""

from __future__ import annotations

import numpy as np

from birdnet_stm32.models import _pack as pk

U = 2.0 ** -24
FLOOR = 2.0 ** -126
ULP_EXP, ULP_LOG, ULP_DIV = 3.0, 3.0, 2.5  # OpenCL full profile (see the docstring); one ulp <= 2 u relative
E_U, L_U, D_U = 2 * ULP_EXP, 2 * ULP_LOG, 2 * ULP_DIV  # in units of u


class V:
    """A value and a bound on how far the device's float32 value may lie from it (``err``: array or the scalar 0.0)."""

    __slots__ = ("val", "err")

    def __init__(self, val, err=0.0):
        self.val = val
        self.err = err

    def reshape(self, *shape):
        return V(self.val.reshape(*shape), self.err.reshape(*shape) if isinstance(self.err, np.ndarray) else self.err)

    def transpose(self, *axes):
        return V(self.val.transpose(*axes), self.err.transpose(*axes) if isinstance(self.err, np.ndarray) else self.err)


def exact(a) -> V:
    return V(np.asarray(a, np.float64), 0.0)


def _has_err(v: V) -> bool:
    return isinstance(v.err, np.ndarray)


# ------------------------------------------------------------------------------------------------------------------ packing inverses
def unpack_pw_fragments(frag: np.ndarray, cin: int) -> np.ndarray:
    """Inverse of ``_lower_f32.pack_pw_fragments``: ``[ceil(Cin/16)][Cout/16][64][4]`` -> ``[Cin][Cout]``; the rows past ``cin`` that the
    packer added must be zero."""
    J, CT = frag.shape[0], frag.shape[1]
    assert frag.shape[2:] == (64, 4) and J == -(-cin // 16)
    w = frag.reshape(J, CT, 4, 16, 4).transpose(0, 2, 4, 1, 3).reshape(J * 16, CT * 16)  # [j][ct][q][c][e] -> [j][q][e][ct][c]
    assert not np.any(w[cin:]), "non-zero weights in the padded rows of the last k-step"
    return np.ascontiguousarray(w[:cin])


def unpack_mel_bands(vals: np.ndarray, bands: np.ndarray, n_bins: int) -> np.ndarray:
    """Inverse of ``_lower_f32.mel_bands``: (values, int32 [3, M] = start, len, offset) -> dense ``[n_bins, M]``."""
    M = bands.shape[1]
    mel = np.zeros((n_bins, M), vals.dtype)
    for m in range(M):
        start, length, off = (int(v) for v in bands[:, m])
        assert 0 <= start and start + length <= n_bins
        mel[start : start + length, m] = vals[off : off + length]
    return mel


def truncate_bf16(w: np.ndarray) -> np.ndarray:
    """float32 values with the low 16 mantissa bits cleared (bfloat16 by truncation), as float32."""
    return (np.ascontiguousarray(w, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ arithmetic
def _clip(v, code):
    if code == 1:
        return np.maximum(v, 0)
    if code == 2:
        return np.minimum(np.maximum(v, 0), 6)
    return v


class Ref:
    """Float64 values with bounds.  ``Ref()`` bounds the device: every counted rounding is worth ``u = 2^-24``.  ``Ref(fold=True)`` bounds the
    distance between two FLOAT64 evaluations that differ only in the float32 rounding of the constants (the oracle's unfused layers against
    the plan's folded ones): a linear stage gets ``1 u A`` (one u per folded weight and bias), a float32 constant of the kernels one u of
    its own, and every counted rounding is worth ``2^-51`` (float64 arithmetic on both sides, in different orders)."""

    name = "float64"

    def __init__(self, fold: bool = False):
        self.u = 2.0 ** -51 if fold else U
        self.fold_u = U if fold else 0.0

    def w(self, w):
        return np.asarray(w, np.float64)

    def act(self, x: V, code: int) -> V:
        return V(_clip(x.val, code), x.err)

    def mm(self, x: V, w, bias=None, res: V | None = None, gate: V | None = None, k_count=None) -> V:
        """``x [..., K] @ w [K, N] + bias [+ res]``; ``gate`` [B, K] multiplies x over the middle axes.  ``k_count``: the number of terms per
        output column when the rest of the column is structurally zero (band-sparse mixer)."""
        w = self.w(w)
        xv, xe = x.val, x.err
        if gate is not None:
            g = gate.val.reshape(gate.val.shape[0], *([1] * (xv.ndim - 2)), -1)
            ge = gate.err.reshape(g.shape) if _has_err(gate) else 0.0
            xe_new = np.abs(g) * xe + np.abs(xv) * ge + xe * ge
            xv, xe = xv * g, xe_new
        val = xv @ w
        a = np.abs(xv) @ np.abs(w)
        err = (xe @ np.abs(w)) if isinstance(xe, np.ndarray) else 0.0
        K = w.shape[0] if k_count is None else np.asarray(k_count, np.float64)
        n = K + 1 + (gate is not None) + (res is not None)
        if bias is not None:
            b = self.w(bias)
            val = val + b
            a = a + np.abs(b)
        if res is not None:
            val = val + res.val
            a = a + np.abs(res.val)
            err = err + res.err
        return V(val, err + (n * self.u + self.fold_u) * a)

    def ew(self, taps: list, etaps: list | None, w, bias) -> V:
        """``sum_k taps[k] * w[k] + bias`` (depthwise: every tap ``[..., C]``, ``w [K, C]``)."""
        w = self.w(w)
        K = len(taps)
        val = np.zeros(taps[0].shape, np.float64)
        a = np.zeros_like(val)
        err = np.zeros_like(val) if etaps is not None else 0.0
        for k in range(K):
            val += taps[k] * w[k]
            a += np.abs(taps[k]) * np.abs(w[k])
            if etaps is not None:
                err += etaps[k] * np.abs(w[k])
        b = self.w(bias)
        return V(val + b, err + ((K + 1) * self.u + self.fold_u) * (a + np.abs(b)))

    def affine(self, coefs: list, vals: list, bias=None) -> V:
        """Elementwise ``sum_k coefs[k] * vals[k] + bias`` with exact coefficients (K = 1 .. 4: the magnitude scalings)."""
        K = len(vals)
        val, a, err = 0.0, 0.0, 0.0
        for c, v in zip(coefs, vals):
            c = self.w(c)
            val = val + c * v.val
            a = a + np.abs(c * v.val)
            err = err + np.abs(c) * v.err
        if bias is not None:
            b = self.w(bias)
            val, a = val + b, a + np.abs(b)
        return V(val, err + ((K + 1) * self.u + self.fold_u) * a)

    def dot(self, x: V, w: V) -> V:
        """``sum over the last axis of x * w`` where both carry errors (attention pooling's weighted sum)."""
        K = x.val.shape[-1]
        val = (x.val * w.val).sum(-1)
        a = np.abs(x.val * w.val).sum(-1)
        err = (np.abs(x.val) * w.err + np.abs(w.val) * x.err + x.err * w.err)
        err = err.sum(-1) if isinstance(err, np.ndarray) else 0.0
        return V(val, err + ((K + 1) * self.u + self.fold_u) * a)

    def mean(self, x: V, axis: int) -> V:
        P = x.val.shape[axis]
        val = x.val.mean(axis)
        a = np.abs(x.val).mean(axis)
        err = x.err.mean(axis) if _has_err(x) else 0.0
        return V(val, err + (P - 1 + D_U) * self.u * a)

    def mul(self, a: V, b: V) -> V:
        val = a.val * b.val
        return V(val, np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err + self.u * np.abs(val))

    def div(self, a: V, b: V) -> V:
        val = a.val / b.val
        den = np.abs(b.val) - b.err
        assert np.all(den > 0)
        return V(val, (a.err + np.abs(val) * b.err) / den + D_U * self.u * np.abs(val))

    def addc(self, a: V, c: float) -> V:
        val = a.val + np.float64(np.float32(c))
        return V(val, a.err + self.u * np.abs(val) + self.fold_u * abs(c))

    def sub(self, a: V, b: V) -> V:
        val = a.val - b.val
        return V(val, a.err + b.err + self.u * np.abs(val))

    def span(self, mn: V, mx: V) -> V:
        """``(float)((double)(mx - mn) + 1e-10)``: a float32 subtraction, the sum in double, one rounding back."""
        val = (mx.val - mn.val) + 1e-10
        return V(val, mx.err + mn.err + 2 * self.u * np.abs(val))

    def amax(self, x: V, axes) -> V:
        return V(x.val.max(axis=axes, keepdims=True), x.err.max(axis=axes, keepdims=True) if _has_err(x) else 0.0)

    def sigmoid(self, s: V) -> V:
        val = 1.0 / (1.0 + np.exp(-s.val))
        return V(val, s.err / 4 + (E_U + 1 + D_U) * self.u * val)

    def softmax(self, z: V) -> V:
        """Over the last axis."""
        C = z.val.shape[-1]
        zv = z.val
        a = np.abs(zv).max(-1, keepdims=True)
        ez = z.err.max(-1, keepdims=True) if _has_err(z) else 0.0
        e = np.exp(zv - zv.max(-1, keepdims=True))
        P = e / e.sum(-1, keepdims=True)
        t = np.expm1(2 * ez + 2 * self.u * a) + E_U * self.u
        return V(P, P * (2 * t + (C - 1 + D_U) * self.u))

    def log_db(self, y: V) -> V:
        yc = np.maximum(y.val, np.float64(np.float32(1e-6)))
        val = 10.0 * np.log(yc) / np.log(10.0)
        lo = np.maximum(yc - y.err, np.float64(np.float32(1e-6)))
        return V(val, 10.0 / np.log(10.0) * np.log(yc / lo) + (L_U + 1 + L_U + D_U) * self.u * np.abs(val) + 10 * L_U * self.u / np.log(10.0))


class Emu:
    """The same formulas in numpy float32 (every product and every sum rounded), in one summation order: 'forward', 'reverse' or 'pairwise'.
    ``trunc``: linear-stage weights cut to bfloat16 first (the mutation the bound must see)."""

    def __init__(self, order: str = "forward", trunc: bool = False):
        self.order, self.trunc = order, trunc
        self.name = f"float32 {order}" + (" bf16 weights" if trunc else "")

    def w(self, w):
        w = np.asarray(w, np.float32)
        return truncate_bf16(w) if self.trunc else w

    def _sum(self, term, K: int):
        if self.order == "pairwise":
            def rec(lo, hi):
                if hi - lo == 1:
                    return term(lo)
                mid = (lo + hi) // 2
                return rec(lo, mid) + rec(mid, hi)
            return rec(0, K)
        ks = range(K) if self.order == "forward" else range(K - 1, -1, -1)
        acc = None
        for k in ks:
            t = term(k)
            acc = t if acc is None else acc + t
        return acc

    @staticmethod
    def _f(v: V):
        return np.asarray(v.val, np.float32)

    def act(self, x: V, code: int) -> V:
        return V(_clip(self._f(x), code))

    def mm(self, x: V, w, bias=None, res=None, gate=None, k_count=None) -> V:
        w = self.w(w)
        xv = self._f(x)
        if gate is not None:
            g = self._f(gate)
            xv = xv * g.reshape(g.shape[0], *([1] * (xv.ndim - 2)), -1)
        acc = self._sum(lambda k: xv[..., k, None] * w[k], w.shape[0])
        if bias is not None:
            acc = acc + np.asarray(bias, np.float32)
        if res is not None:
            acc = acc + self._f(res)
        return V(acc)

    def ew(self, taps, etaps, w, bias) -> V:
        w = self.w(w)
        acc = self._sum(lambda k: np.asarray(taps[k], np.float32) * w[k], len(taps))
        return V(acc + np.asarray(bias, np.float32))

    def affine(self, coefs, vals, bias=None) -> V:
        acc = self._sum(lambda k: np.asarray(coefs[k], np.float32) * self._f(vals[k]), len(vals))
        return V(acc if bias is None else acc + np.asarray(bias, np.float32))

    def dot(self, x: V, w: V) -> V:
        xv, wv = self._f(x), self._f(w)
        return V(self._sum(lambda k: xv[..., k] * wv[..., k], xv.shape[-1]))

    def mean(self, x: V, axis: int) -> V:
        xv = np.moveaxis(self._f(x), axis, 0)
        return V(self._sum(lambda k: xv[k], xv.shape[0]) / np.float32(xv.shape[0]))

    def mul(self, a: V, b: V) -> V:
        return V(self._f(a) * self._f(b))

    def div(self, a: V, b: V) -> V:
        return V(self._f(a) / self._f(b))

    def addc(self, a: V, c: float) -> V:
        return V(self._f(a) + np.float32(c))

    def sub(self, a: V, b: V) -> V:
        return V(self._f(a) - self._f(b))

    def span(self, mn: V, mx: V) -> V:
        return V(((self._f(mx) - self._f(mn)).astype(np.float64) + 1e-10).astype(np.float32))

    def amax(self, x: V, axes) -> V:
        return V(self._f(x).max(axis=axes, keepdims=True))

    def sigmoid(self, s: V) -> V:
        one = np.float32(1)
        return V(one / (one + np.exp(-self._f(s))))

    def softmax(self, z: V) -> V:
        zv = np.moveaxis(self._f(z), -1, 0)
        e = np.exp(zv - zv.max(0, keepdims=True))
        den = self._sum(lambda k: e[k], e.shape[0])
        return V(np.moveaxis(e / den, 0, -1))

    def log_db(self, y: V) -> V:
        return V(np.float32(10) * np.log(np.maximum(self._f(y), np.float32(1e-6))) / np.log(np.float32(10)))


REF = Ref()


# --------------------------------------------------------------------------------------------------------------------------- stages
def _same_taps(a: np.ndarray, H, W, sh, sw, OH, OW, pt, pl):
    """The nine SAME-padded 3x3 tap views of ``a [B, H, W, C]``, each ``[B, OH, OW, C]``, in (row, column) order."""
    pb = max((OH - 1) * sh + 3 - H - pt, 0)
    pr = max((OW - 1) * sw + 3 - W - pl, 0)
    ap = np.pad(a, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    return [ap[:, i : i + (OH - 1) * sh + 1 : sh, j : j + (OW - 1) * sw + 1 : sw, :] for i in range(3) for j in range(3)]


def _geom(op, names=("H", "W", "sh", "sw", "OH", "OW", "pt", "pl")):
    return tuple(int(op.get(n)) for n in names)


def stem_stage(ar, x: V, geom, w, bias, act) -> V:
    """x [B, H, W] (one channel), w [3, 3, Cout] -> [B, OH, OW, Cout]."""
    taps = np.concatenate(_same_taps(x.val[..., None], *geom), axis=-1)  # [B, OH, OW, 9]
    etaps = np.concatenate(_same_taps(x.err[..., None], *geom), axis=-1) if _has_err(x) else 0.0
    return ar.act(ar.mm(V(taps, etaps), np.asarray(w).reshape(9, -1), bias), act)


def dw_stage(ar, x: V, geom, w, bias, act) -> V:
    """x [B, H, W, C], w [3, 3, C] -> [B, OH, OW, C]."""
    taps = _same_taps(x.val, *geom)
    etaps = _same_taps(x.err, *geom) if _has_err(x) else None
    return ar.act(ar.ew(taps, etaps, np.asarray(w).reshape(9, -1), bias), act)


def mag_scale(ar, y: V, magp: np.ndarray, mag: int, axis_shape) -> V:
    """Channel-wise magnitude scaling; ``magp [NP, M]`` rows as ``_lower_f32.mag_params`` packs them, broadcast through ``axis_shape``."""
    r = lambda i: np.asarray(magp[i]).reshape(axis_shape)  # noqa: E731
    if mag == 1:  # pwl: k0 y + sum_i k_i relu(w_i y + b_i)
        inner = [ar.act(ar.affine([r(4 + i)], [y], r(7 + i)), 1) for i in range(3)]
        return ar.affine([r(0), r(1), r(2), r(3)], [y, *inner])
    if mag == 2:  # pcen: rows agc, k1, sw, sb, k2
        y0 = ar.act(ar.affine([np.ones(1, np.float32), -r(0)], [y, y]), 1)
        inner = ar.act(ar.affine([r(2)], [y0], r(3)), 1)
        return ar.act(ar.affine([r(1), r(4)], [y0, inner]), 1)
    if mag == 3:
        return ar.log_db(y)
    return y


def stft_reference(audio: np.ndarray, W: int) -> V:
    """Float64 magnitudes ``[B, W, 257]`` of the evaluate path's STFT (n_fft 512, hop ``T // W``, centred, periodic Hann: oracle/stft.py) with
    the per-frame bound docs/exactness.md proves for ``stft512_mag_kernel``: ``|S' - S| <= 1148 u ||x_t||_2 + 14 u S'`` (x_t: the frame's
    512 samples).  The fused STFT + mixer kernel is that kernel's ``MEL_OUT`` instantiation: the same operations up to the magnitudes."""
    B, T = audio.shape
    hop = T // W
    assert 1 + T // hop >= W
    yp = np.pad(np.asarray(audio, np.float64), ((0, 0), (256, 256)))
    idx = np.arange(512)[None, :] + hop * np.arange(W)[:, None]
    frames = yp[:, idx]  # [B, W, 512]
    k = np.arange(512, dtype=np.float64)
    S = np.abs(np.fft.rfft(frames * (0.5 - 0.5 * np.cos(2.0 * np.pi * k / 512)), axis=2))
    norm = np.sqrt((frames ** 2).sum(axis=2, keepdims=True))
    return V(S, (1148 * U * norm + 14 * U * S) / (1 - 14 * U))


def finalise(ar, raw: V, mn: V, mx: V, wsum, recip: bool) -> V:
    """``relu((raw - mn * wsum[m]) / rng)`` on ``[B, M, W]`` (MELFIN: a division per element; the front block: one reciprocal, a product per
    element).  The subtraction's bound is in terms of ``|raw|`` and ``|mn wsum|`` (the product's rounding, the error of mn), not of the result."""
    rng = ar.span(mn, mx)
    d = ar.sub(raw, ar.mul(mn, V(ar.w(wsum).reshape(1, -1, 1))))
    one = exact(np.ones((1, 1, 1)))
    return ar.act(ar.mul(d, ar.div(one, rng)) if recip else ar.div(d, rng), 1)


def head_stage(ar, x: V, w, bias, act: int):
    """Dense + activation: (scores, logits)."""
    z = ar.mm(x, w, bias)
    if act == 1:
        return ar.sigmoid(z), z
    if act == 2:
        return ar.softmax(z), z
    return z, z


# ------------------------------------------------------------------------------------------------------------------------ operators
def _t(plan, op, name):
    i = op.get(name)
    return plan.tensors[i] if i >= 0 else None


def eval_op(plan, op, in0: V | None, in1: V | None = None, gate: V | None = None, ar=REF, minmax=None) -> dict:
    """Evaluate one plan operator.  Inputs are per-chunk arrays ``[B, ...]`` in the layout the producing operator's ``out_shape`` names (any
    shape with the right element count).  Returns ``{"out": V [B, *out_shape]}``; head operators add ``"logits"`` and, for GAPDENSE, ``"emb"``.
    The audio entry: STFTMEL takes the audio ``[B, T]`` as ``in0`` and adds ``"minmax"`` = (min, max) of the chunk's magnitudes, each a
    ``V [B, 1, 1]``; MELFIN and FRONT with ``raw_mel`` read it as ``minmax`` (the device keeps the pair in a buffer of its own)."""
    k = op.kind
    B = in0.val.shape[0]
    g = op.get
    if k == pk.F32_MEL:
        F, W, M = g("F"), g("W"), g("M")
        mel = unpack_mel_bands(_t(plan, op, "wvals"), _t(plan, op, "bands"), F)
        x = in0.reshape(B, F, W).transpose(0, 2, 1)  # [B, W, F]
        y = ar.act(ar.mm(x, mel, k_count=_t(plan, op, "bands")[1]), 1).transpose(0, 2, 1)  # [B, M, W]
        if not g("norm"):
            y = mag_scale(ar, y, _t(plan, op, "magp"), g("mag"), (1, M, 1))
        return {"out": y.reshape(B, M, W, 1)}
    if k == pk.F32_MAG:
        M, W = g("M"), g("W")
        x = in0.reshape(B, M, W)
        y = ar.div(x, ar.addc(ar.amax(x, (1, 2)), 1e-6))
        return {"out": mag_scale(ar, y, _t(plan, op, "magp"), g("mag"), (1, M, 1)).reshape(B, M, W, 1)}
    if k == pk.F32_RAWFE:
        T, W, M, stride, left = g("T"), g("W"), g("M"), g("stride"), g("pad_left")
        need = stride * (W - 1) + 16
        idx = np.arange(16)[None, :] + stride * np.arange(W)[:, None]

        def frames(a):
            a = np.pad(a.reshape(B, T), ((0, 0), (left, max(0, need - T - left))))
            return a[:, idx]  # [B, W, 16]

        x = V(frames(in0.val), frames(in0.err) if _has_err(in0) else 0.0)
        y = ar.act(ar.mm(x, _t(plan, op, "fb"), _t(plan, op, "bias")), 2)  # [B, W, M]
        y = mag_scale(ar, y, _t(plan, op, "magp"), g("mag"), (1, 1, M))
        return {"out": y.transpose(0, 2, 1).reshape(B, M, W, 1)}
    if k == pk.F32_STEM:
        geom = _geom(op)
        return {"out": stem_stage(ar, in0.reshape(B, geom[0], geom[1]), geom, _t(plan, op, "w"), _t(plan, op, "bias"), g("act"))}
    if k == pk.F32_DW:
        geom = _geom(op)
        return {"out": dw_stage(ar, in0.reshape(B, geom[0], geom[1], g("C")), geom, _t(plan, op, "w"), _t(plan, op, "bias"), g("act"))}
    if k == pk.F32_PW:
        P, Cin, Cout = g("P"), g("Cin"), g("Cout")
        y = ar.mm(in0.reshape(B, P, Cin), _t(plan, op, "w"), _t(plan, op, "bias"), in1.reshape(B, P, Cout) if g("has_res") else None,
                  gate.reshape(B, Cin) if g("has_gate") else None)
        return {"out": ar.act(y, g("act")).reshape(B, *op.out_shape)}
    if k == pk.F32_DWPW:
        geom = _geom(op)
        Cin, Cout, OH, OW = g("Cin"), g("Cout"), g("OH"), g("OW")
        x = in0.reshape(B, geom[0], geom[1], Cin)
        if g("has_dw"):
            x = dw_stage(ar, x, geom, _t(plan, op, "dw_w"), _t(plan, op, "dw_b"), g("dw_act"))
        w = unpack_pw_fragments(_t(plan, op, "pw_w"), Cin)
        y = ar.mm(x.reshape(B, OH * OW, Cin), w, _t(plan, op, "pw_b"), in1.reshape(B, OH * OW, Cout) if g("has_res") else None,
                  gate.reshape(B, Cin) if g("has_gate") else None)
        return {"out": ar.act(y, g("pw_act")).reshape(B, OH, OW, Cout)}
    if k == pk.F32_STFTMEL:
        W, M = g("W"), g("M")
        S = stft_reference(in0.val.reshape(B, -1), W)
        mel = unpack_mel_bands(_t(plan, op, "wvals"), _t(plan, op, "bands"), 257)
        raw = REF.mm(S, mel, k_count=_t(plan, op, "bands")[1]).transpose(0, 2, 1)  # (float64 only: the FFT has no float32 emulation here)
        e_top = S.err.max(axis=(1, 2), keepdims=True)  # an extreme of S' lies within the largest element bound of the extreme of S
        mm = (V(S.val.min(axis=(1, 2), keepdims=True), e_top), V(S.val.max(axis=(1, 2), keepdims=True), e_top))
        return {"out": raw.reshape(B, M, W, 1), "minmax": mm}
    if k == pk.F32_MELFIN:
        M, W = g("M"), g("W")
        y = finalise(ar, in0.reshape(B, M, W), *minmax, _t(plan, op, "wsum"), recip=False)
        if g("norm"):
            y = ar.div(y, ar.addc(ar.amax(y, (1, 2)), 1e-6))
        return {"out": mag_scale(ar, y, _t(plan, op, "magp"), g("mag"), (1, M, 1)).reshape(B, M, W, 1)}
    if k == pk.F32_FRONT:
        H0, W0, C, N, OH, OW = (g(n) for n in ("H0", "W0", "C", "N", "OH", "OW"))
        fin = None
        if g("raw_mel"):  # the audio entry's variant finalises the un-normalised mel energies while it loads them
            in0 = mag_scale(ar, finalise(ar, in0.reshape(B, H0, W0), *minmax, _t(plan, op, "wsum"), recip=True), _t(plan, op, "magp"), g("mag"), (1, H0, 1))
            fin = in0
        from birdnet_stm32.models._netspec import same_pad

        SW, pl0, _ = same_pad(W0, 3, 2)
        _, pt0, _ = same_pad(H0, 3, 1)
        s = stem_stage(ar, in0.reshape(B, H0, W0), (H0, W0, 1, 2, H0, SW, pt0, pl0), _t(plan, op, "stem_w"), _t(plan, op, "stem_b"), g("stem_act"))
        oh, pt1, _ = same_pad(H0, 3, 2)
        ow, pl1, _ = same_pad(SW, 3, 2)
        assert (oh, ow) == (OH, OW)
        d = dw_stage(ar, s, (H0, SW, 2, 2, OH, OW, pt1, pl1), _t(plan, op, "dw_w"), _t(plan, op, "dw_b"), g("dw_act"))
        y = ar.mm(d.reshape(B, OH * OW, C), unpack_pw_fragments(_t(plan, op, "pw_w"), C), _t(plan, op, "pw_b"))
        out = {"out": ar.act(y, g("pw_act")).reshape(B, OH, OW, N)}
        if fin is not None:
            out["stage_fin"] = fin  # the finalised map the stem reads (a stage of its own for the not-slack test)
        return out
    if k == pk.F32_SEGATE:
        P, C = g("P"), g("C")
        m = ar.mean(in0.reshape(B, P, C), 1)
        h = ar.act(ar.mm(m, _t(plan, op, "w1")), 1)
        return {"out": ar.sigmoid(ar.mm(h, _t(plan, op, "w2")))}
    if k == pk.F32_SCALE:
        P, C = g("P"), g("C")
        return {"out": ar.mul(in0.reshape(B, P, C), in1.reshape(B, 1, C)).reshape(B, *op.out_shape)}
    if k == pk.F32_GAP:
        return {"out": ar.mean(in0.reshape(B, g("P"), g("C")), 1)}
    if k == pk.F32_ATTNPOOL:
        P, C = g("P"), g("C")
        x = in0.reshape(B, P, C)
        s = ar.mm(x, np.asarray(_t(plan, op, "score")).reshape(C, 1)).reshape(B, P)
        a = ar.softmax(s)
        return {"out": ar.dot(x.transpose(0, 2, 1), a.reshape(B, 1, P)), "stage_scores": s}
    if k == pk.F32_DENSE:
        scores, logits = head_stage(ar, in0.reshape(B, g("Cin")), _t(plan, op, "w"), _t(plan, op, "bias"), g("act"))
        return {"out": scores, "logits": logits}
    if k == pk.F32_GAPDENSE:
        emb = ar.mean(in0.reshape(B, g("P"), g("Cin")), 1)
        scores, logits = head_stage(ar, emb, _t(plan, op, "w"), _t(plan, op, "bias"), g("act"))
        return {"out": scores, "logits": logits, "emb": emb}
    raise NotImplementedError(f"{pk.KIND_NAMES.get(k, k)} is not covered by the float32 plan reference")


WEIGHT_FIELDS = {  # the tensors Emu(trunc=True) cuts to bfloat16, per kind (kinds without weights have no entry)
    pk.F32_MEL: ("wvals",), pk.F32_RAWFE: ("fb",), pk.F32_STEM: ("w",), pk.F32_DW: ("w",), pk.F32_PW: ("w",), pk.F32_DWPW: ("dw_w", "pw_w"),
    pk.F32_FRONT: ("stem_w", "dw_w", "pw_w"), pk.F32_MELFIN: ("wsum",), pk.F32_SEGATE: ("w1", "w2"), pk.F32_DENSE: ("w",), pk.F32_GAPDENSE: ("w",), pk.F32_ATTNPOOL: ("score",),
}  # fmt: skip


def path_ops(plan, mode: int = pk.PATH_INPUT) -> list[int]:
    return [oi for oi, o in enumerate(plan.ops) if o.p[pk.OP_PATH] in (pk.PATH_BOTH, mode)]


def walk_plan(plan, x: np.ndarray, fetch, mode: int = pk.PATH_INPUT, ar=REF, forced: bool = True, own: bool = False, minmax=None):
    """Take ``plan`` through :func:`eval_op` on the model inputs ``x [B, ...]``; yields ``(oi, op, result dict, got)`` per operator on the
    entry path ``mode``.  ``fetch(oi)`` returns what was observed for operator ``oi`` (``[B, *out_shape]``) or None.  With ``forced`` the
    next operator reads that observation (bound 0); where there is none — or the operator's slot is written again later, in place — it
    reads the reference value with its bound, which makes the two a composite.  ``own``: an operator without an observation hands on its
    reference value as if it had been observed (bound 0; in-place pairs stay composites), so that every bound is one operator's own.
    On ``PATH_AUDIO`` ``x`` is the audio ``[B, T]`` and ``minmax`` the observed ``[B, 2]`` minimum and maximum of the chunk's magnitudes
    (MELFIN and the finalising FRONT then read them with bound 0; None: the reference's own, with the STFT's bound).  An operator :func:`eval_op` does not cover, or one whose input is unknown, yields
    ``None`` as its result; the operators behind the next observed map are evaluated as usual."""
    ops = path_ops(plan, mode)
    slots: dict[int, V] = {}

    aux = {}
    if minmax is not None:
        mm = np.asarray(minmax, np.float64).reshape(-1, 2)
        aux["minmax"] = (exact(mm[:, 0].reshape(-1, 1, 1)), exact(mm[:, 1].reshape(-1, 1, 1)))

    def src(sid):
        if sid in (pk.SLOT_INPUT, pk.SLOT_AUDIO):  # (``x`` is the audio on the audio entry path)
            return exact(x) if (sid == pk.SLOT_AUDIO) == (mode == pk.PATH_AUDIO) else None
        return slots.get(sid)

    for pos, oi in enumerate(ops):
        op = plan.ops[oi]
        has_gate = op.kind in (pk.F32_PW, pk.F32_DWPW) and op.get("has_gate")
        has_in1 = op.kind == pk.F32_SCALE or (op.kind in (pk.F32_PW, pk.F32_DWPW) and op.get("has_res"))
        in0, in1, gate = src(op.in0), src(op.in1) if has_in1 else None, src(op.get("gate_slot")) if has_gate else None
        in_place = op.out >= 0 and any(plan.ops[oj].out == op.out for oj in ops[pos + 1 :])
        got = fetch(oi) if op.out >= 0 and not in_place else None
        known = in0 is not None and (in1 is not None or not has_in1) and (gate is not None or not has_gate)
        try:
            r = eval_op(plan, op, in0, in1, gate, ar, aux.get("minmax")) if known else None
        except NotImplementedError:
            r = None
        if r is None:
            yield oi, op, None, got
            if op.out >= 0:
                slots[op.out] = exact(got) if got is not None else None
            continue
        r["in0"], r["in1"], r["gate"] = in0, in1, gate
        if "minmax" in r and minmax is None:
            aux["minmax"] = r["minmax"]
        r["minmax"] = aux.get("minmax")
        yield oi, op, r, got
        if op.out >= 0:
            if got is not None and forced:
                slots[op.out] = exact(np.asarray(got).reshape(r["out"].val.shape))
            else:
                slots[op.out] = exact(r["out"].val) if (own and not in_place) else r["out"]


def check(got: np.ndarray, ref: V):
    """(all elements within the bound, worst |got - value| / bound, index of the worst element)."""
    err = np.abs(np.asarray(got, np.float64).reshape(ref.val.shape) - ref.val)
    bound = ref.err + FLOOR
    ratio = err / bound
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return bool(np.all(err <= bound)), float(ratio[worst]), tuple(int(i) for i in worst)
