// bn_probe_step.h — the kernels of one training step of a classifier head, written once with a compile-time switch:
// SWEEP = false are the kernels of a single fit (bn_probe.hip), SWEEP = true the same kernels with one more grid axis, the trial of a
// hyperparameter sweep (bn_probe_sweep.hip).  A sweep's workgroup first finds its trial, leaves at once when that trial is inactive, and
// takes what differs per trial — its slices of the per-trial buffers, its row of the device table (ProbeSweepTrial) — where a single
// fit takes kernel arguments; from there on both run the same statements on the same tile-to-workgroup map in the same order, so a trial
// without label smoothing has the bits of a single fit (tests/test_gpu_probe_sweep.py compares them; `make probe-asm-check`
// reports where the two instantiations' floating-point instructions differ: tools/probe_sweep_asm_check.py).
//
// Label smoothing (sweep only, training loss and G only; the validation loss takes the targets as they are), in float32 with a
// rounding after every operation (no fused multiply-add):
//     keep = fl(1 - eps);  add = fl(0.5 * eps) (sigmoid) or fl(eps / fl(C)) (softmax)      on the host
//     y'   = fl(fl(y * keep) + add)                                                          per element, in the forward kernel
// training/linear_probe.py: smooth_targets is the same in numpy.  eps == 0 skips the two operations: y' is y, bit for bit.
//
// Long-tailed training sets (EXT = 1 of the forward kernel; single fit and sweep alike, shared by a sweep's trials): the focal loss of
// the sigmoid head and one weight per row.  With y the target (after smoothing, if any), p the sigmoid and pc = clip(p, 1e-7, 1 - 1e-7):
//     bce  = -(y log pc + (1 - y) log(1 - pc))
//     q    = 1 - (y pc + (1 - y)(1 - pc))                 (> 0: pc is clipped)
//     f    = expf(gamma * logf(q))
//     loss = f bce;    dloss/dz = f (p - y) - gamma (f / q) (2 y - 1) pc (1 - pc) bce
// and row i's elements times w_i, in the loss and in G; the means still divide by B C (or B).  The validation loss (MODE 1) takes the
// loss kind and no weights.  Written in probe_loss_elem with a rounding after every operation, so no instantiation fuses what another
// does not.  EXT = 0 is the kernel without any of this: the statements, and the bits, of a fit that asks for neither.
// training/linear_probe.py: probe_loss / probe_loss_gradient are the same in numpy.
//
// Quantisation-aware fine-tuning (EXT = 2 of the forward kernel; single fit only): the logits on the grid the exported
// logit tensor will have, between the bias add and the activation, in float32 with a rounding after every operation and an IEEE division:
//     t  = z / s_out;   k = rintf(t) + z_out;   kc = min(max(k, -128), 127);   zq = (kc - z_out) * s_out;   pass = (k == kc)
// The activation, softmax's max / sum passes and the loss take zq; the loss statements are EXT = 1's, so the focal loss and row weights
// compose.  Mode 0 writes G where `pass` holds and 0 elsewhere (the straight-through estimator with TensorFlow's clamp mask); mode 2 also
// writes kc.  training/probe_qat.py: fake_quantize_logits is the same in numpy.  The weights such a forward reads are made by the two
// kernels at the end of bn_probe.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/birdnet_hip.h"
#include "bn_device.h"
#include "bn_kernels.h"

namespace bn {

struct ProbeNoSweep {};
template <bool SWEEP>
using ProbeSweepOf = std::conditional_t<SWEEP, ProbeSweepArgs, ProbeNoSweep>;   // the second kernel argument
// ... of the forward kernel: EXT = 2 (single fit only) takes the logit grid there, so every other instantiation keeps its signature
template <bool SWEEP, int EXT>
using ProbeFwdExtraOf = std::conditional_t<EXT == 2, ProbeQatArgs, ProbeSweepOf<SWEEP>>;


constexpr int kRows = 16;       // batch rows per forward workgroup (one MFMA tile)
constexpr int kFwdWaves = 16;   // at most: 16 waves x 16 column tiles x 16 columns = C <= 4096
constexpr int kLdsPad = 4;      // floats behind every staged row: the 16 rows of an A fragment fall into 16 different bank groups

__device__ __forceinline__ uint32_t probe_fmix(uint32_t h) {   // the murmur3 finaliser
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// The dropout draw of element (row in batch, column) of global step `step`: 24 bits, kept iff >= ceil(p * 2^24).
// training/linear_probe.py: dropout_hash is the same function in numpy.
__device__ __forceinline__ uint32_t probe_drop_hash(uint32_t seed, uint32_t step, uint32_t row, uint32_t col) {
    uint32_t h = probe_fmix(seed ^ (step * 0x9E3779B1u));
    h = probe_fmix(h ^ (row * 0x85EBCA77u));
    h = probe_fmix(h ^ (col * 0xC2B2AE3Du));
    return h >> 8;
}

__device__ __forceinline__ float group16_max(float v) {   // over the 16 lanes that share lane >> 4
    for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float group16_sum(float v) {
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// sum of one value per thread of a 256-thread workgroup, the same tree every time; every thread gets the result
__device__ __forceinline__ float block256_sum(float v, float* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}


__device__ __forceinline__ float probe_smooth(float y, float keep, float add) {
#pragma clang fp contract(off)
    const float t = y * keep;
    return t + add;
}

// EXT = 1: the loss of one element and its derivative by the logit, before the mean's scale (see the head of the file)
__device__ __forceinline__ void probe_loss_elem(float p, float pc, float y, bool softmax, bool focal, float gamma, bool weighted, float w, float& le,
                                                float& g) {
#pragma clang fp contract(off)
    g = p - y;
    if (softmax) {
        le = -(y * logf(pc));
    } else {
        const float bce = -(y * logf(pc) + (1.0f - y) * logf(1.0f - pc));
        le = bce;
        if (focal) {
            const float q = 1.0f - (y * pc + (1.0f - y) * (1.0f - pc));
            const float f = expf(gamma * logf(q));
            le = f * bce;
            g = f * g - gamma * (f / q) * (2.0f * y - 1.0f) * pc * (1.0f - pc) * bce;
        }
    }
    if (weighted) {
        le = le * w;
        g = g * w;
    }
}

// EXT = 2: the logit on the int8 grid (s_out, z_out), in two halves (see the head of the file).  The accumulators keep k, the code
// before the clamps, which is all three results in one register: kc = probe_clamp_code(k), zq = probe_dequant(kc), pass = (k == kc).
__device__ __forceinline__ float probe_quant_code(float z, float s_out, float z_out) {
#pragma clang fp contract(off)
    const float t = z / s_out;
    return rintf(t) + z_out;
}
__device__ __forceinline__ float probe_clamp_code(float k) { return fminf(fmaxf(k, -128.0f), 127.0f); }
__device__ __forceinline__ float probe_dequant(float kc, float s_out, float z_out) {
#pragma clang fp contract(off)
    const float d = kc - z_out;
    return d * s_out;
}

// host: does this launch need the EXT = 1 kernel?  Row weights count in mode 0 only, the focal loss in modes 0 and 1.
inline bool probe_fwd_ext(const ProbeFwdArgs& a, int mode) {
    return mode != 2 && (a.loss_kind == BN_PROBE_LOSS_FOCAL || (mode == 0 && a.row_weight != nullptr));
}

__device__ __forceinline__ bool sweep_idle(const ProbeSweepArgs& w, int t) { return w.active && !w.active[t]; }


// ------------------------------------------------------------------------------------------------------------------------- forward
// MODE 0: training (G and the loss partial), 1: loss partial only, 2: scores.  NT: column tiles per wave (tile t of wave w is w + t * waves).
// SWEEP: blockIdx.y is the trial; mode 0 takes its dropout threshold and label smoothing from the table, mode 1 has neither.
// EXT 1 (modes 0 and 1): the loss kind and, in mode 0, the row weights of ProbeFwdArgs; 0: neither, the plain cross-entropy statements.
// EXT 2 (all modes, no sweep): EXT 1 on fake-quantised logits; `w` is then the logit grid.
template <int NT, int MODE, int EXT, bool SWEEP>
__global__ __launch_bounds__(1024) void probe_fwd_kernel(ProbeFwdArgs a, ProbeFwdExtraOf<SWEEP, EXT> w) {
    static_assert(!(SWEEP && EXT == 2), "a sweep has no QAT instantiation");
    const float *W = a.W, *bias = a.b;
    float *out = a.out, *loss_part = a.loss_part;
    uint32_t drop_thresh = a.drop_thresh;
    float drop_scale = a.drop_scale;
    [[maybe_unused]] bool smooth = false;
    [[maybe_unused]] float smooth_keep = 1.0f, smooth_add = 0.0f;
    if constexpr (SWEEP) {
        const int t = blockIdx.y;
        if (sweep_idle(w, t)) return;
        W = w.state + (size_t)t * 4 * w.E;
        bias = W + (size_t)a.D * a.C;
        loss_part = w.loss_part + (size_t)t * w.loss_stride;
        if constexpr (MODE == 0) {
            const ProbeSweepTrial& tr = w.trials[t];
            out = w.G + (size_t)t * w.G_stride;
            drop_thresh = tr.drop_thresh;
            drop_scale = tr.drop_scale;
            smooth = tr.smooth != 0;
            smooth_keep = tr.smooth_keep;
            smooth_add = tr.smooth_add;
        }
    }
    extern __shared__ float xs[];                 // [16][Dp + kLdsPad], rows beyond the batch and columns beyond D are zero
    __shared__ float red[kFwdWaves][kRows];
    __shared__ float red_loss[kFwdWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int D = a.D, C = a.C, Dp = (D + 3) & ~3, ld = Dp + kLdsPad;
    const long row0 = (long)blockIdx.x * kRows;

    for (int e = tid; e < kRows * Dp; e += blockDim.x) {
        const int r = e / Dp, d = e - r * Dp;
        const long row = row0 + r;
        float v = 0.0f;
        if (row < a.n && d < D) {
            const long src = a.idx ? (long)a.idx[row] : row;
            v = a.X[src * D + d];
            if (drop_thresh) v = probe_drop_hash(a.seed, a.step, (uint32_t)row, (uint32_t)d) >= drop_thresh ? v * drop_scale : 0.0f;
        }
        xs[r * ld + d] = v;
    }
    __syncthreads();

    const int ntiles = (C + 15) >> 4;
    const int li = lane & 15, lk = lane >> 4;
    const int per_pass = nw * NT;                          // column tiles the workgroup holds in registers at once
    const int npass = (ntiles + per_pass - 1) / per_pass;  // 1 unless C > 2048
    f32x4 acc[NT];
    bool okc[NT];
    const float* xrow = xs + li * ld + lk;

    // logits of the column tiles of one pass: lane holds rows 4 * lk + r (r = 0..3) of column tile * 16 + li
    auto logits = [&](int pass) {
        const int tile0 = pass * per_pass + wave;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < Dp; k0 += 4) {
            const float av = xrow[k0];
            const int k = k0 + lk;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int tile = tile0 + t * nw;      // wave-uniform
                if (tile < ntiles) {
                    const int c = tile * 16 + li;
                    const float bv = (k < D && c < C) ? W[(size_t)k * C + c] : 0.0f;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = (tile0 + t * nw) * 16 + li;
            okc[t] = (tile0 + t * nw) < ntiles && c < C;
            const float bv = okc[t] ? bias[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += bv;
        }
        if constexpr (EXT == 2) {   // from here on acc holds the codes k; `logit` below turns one into zq
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][r] = probe_quant_code(acc[t][r], w.s_out, w.z_out);
        }
    };
    // the logit the activation takes: the accumulator itself, or (EXT 2) the quantised logit of the code it holds
    auto logit = [&](float v) {
        if constexpr (EXT == 2) return probe_dequant(probe_clamp_code(v), w.s_out, w.z_out);
        else return v;
    };

    // softmax: row maximum m and sum s of exp(z - m) over all columns first — pass by pass in the online form (with one pass that is
    // the plain max / sum); a head wider than one pass computes its logits a second time below, once m and s are known
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool have = false;
    if (a.softmax) {
        for (int pass = 0; pass < npass; ++pass) {
            logits(pass);
            float mn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = -INFINITY;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (okc[t]) v = fmaxf(v, logit(acc[t][r]));
                mn[r] = group16_max(v);
            }
            __syncthreads();
            if (li == 0)
                for (int r = 0; r < 4; ++r) red[wave][4 * lk + r] = mn[r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = m[r];
                for (int w = 0; w < nw; ++w) v = fmaxf(v, red[w][4 * lk + r]);
                mn[r] = v;
            }
            float sn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = 0.0f;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (okc[t]) v += expf(logit(acc[t][r]) - mn[r]);
                sn[r] = group16_sum(v);
            }
            __syncthreads();
            if (li == 0)
                for (int r = 0; r < 4; ++r) red[wave][4 * lk + r] = sn[r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = red[0][4 * lk + r];
                for (int w = 1; w < nw; ++w) v += red[w][4 * lk + r];
                s[r] = pass == 0 ? v : s[r] * expf(m[r] - mn[r]) + v;
                m[r] = mn[r];
            }
        }
        have = npass == 1;
    }

    [[maybe_unused]] float rw[4] = {1.0f, 1.0f, 1.0f, 1.0f};   // the weights of the lane's four rows, loaded once
    [[maybe_unused]] bool weighted = false;
    [[maybe_unused]] const bool focal = EXT && a.loss_kind == BN_PROBE_LOSS_FOCAL;
    if constexpr (EXT && MODE == 0) {
        weighted = a.row_weight != nullptr;
        if (weighted) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = row0 + 4 * lk + r;
                if (row < a.n) rw[r] = a.row_weight[a.idx ? (long)a.idx[row] : row];
            }
        }
    }
    float loss = 0.0f;
    for (int pass = 0; pass < npass; ++pass) {
        if (!have) logits(pass);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = (pass * per_pass + wave + t * nw) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = row0 + 4 * lk + r;
                if (!okc[t] || row >= a.n) continue;
                const float z = logit(acc[t][r]);
                const float p = a.softmax ? expf(z - m[r]) / s[r] : 1.0f / (1.0f + expf(-z));
                if constexpr (MODE == 2) {
                    out[(size_t)row * C + c] = p;
                    if constexpr (EXT == 2)
                        if (w.codes) w.codes[(size_t)row * C + c] = (int8_t)probe_clamp_code(acc[t][r]);
                } else {
                    const long src = (MODE == 0 && a.idx) ? (long)a.idx[row] : row;
                    float y = a.Y[(size_t)src * C + c];
                    if constexpr (SWEEP && MODE == 0)
                        if (smooth) y = probe_smooth(y, smooth_keep, smooth_add);
                    const float pc = fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f);
                    if constexpr (EXT) {
                        float le, g;
                        probe_loss_elem(p, pc, y, a.softmax, focal, a.focal_gamma, weighted, rw[r], le, g);
                        loss += le;
                        if constexpr (MODE == 0 && EXT == 2) out[(size_t)row * C + c] = acc[t][r] == probe_clamp_code(acc[t][r]) ? g * a.g_scale : 0.0f;
                        else if constexpr (MODE == 0) out[(size_t)row * C + c] = g * a.g_scale;
                    } else {
                        if (a.softmax)
                            loss -= y * logf(pc);
                        else
                            loss -= y * logf(pc) + (1.0f - y) * logf(1.0f - pc);
                        if constexpr (MODE == 0) out[(size_t)row * C + c] = (p - y) * a.g_scale;
                    }
                }
            }
        }
    }
    if constexpr (MODE != 2) {
        loss = wave_sum(loss);
        if (lane == 0) red_loss[wave] = loss;
        __syncthreads();
        if (tid == 0) {
            float v = red_loss[0];
            for (int w = 1; w < nw; ++w) v += red_loss[w];
            loss_part[blockIdx.x] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ gradient
// Workgroup (bx, by, bz): rows [16 * (4 by + wave), +16) of dParams (row D is the bias), columns [64 bx, +64), batch rows of group bz.
// SWEEP: blockIdx.z = trial * groups + group.
template <bool SWEEP>
__global__ __launch_bounds__(256) void probe_dw_kernel(ProbeDwArgs a, ProbeSweepOf<SWEEP> w, int sweep_groups) {
    const float* G = a.G;
    float *partial = a.partial, *ss_part = a.ss_part;
    uint32_t drop_thresh = a.drop_thresh;
    float drop_scale = a.drop_scale;
    int group = blockIdx.z, groups = gridDim.z;
    if constexpr (SWEEP) {
        const int t = blockIdx.z / sweep_groups;
        if (sweep_idle(w, t)) return;
        const ProbeSweepTrial& tr = w.trials[t];
        group = blockIdx.z - t * sweep_groups;
        groups = sweep_groups;
        G = w.G + (size_t)t * w.G_stride;
        partial = w.partial + (size_t)t * w.partial_stride;
        ss_part = w.ss_part + (size_t)t * w.ss_stride;
        drop_thresh = tr.drop_thresh;
        drop_scale = tr.drop_scale;
    }
    __shared__ float red[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, C = a.C;
    const int d0 = (blockIdx.y * 4 + wave) * 16, c0 = blockIdx.x * 64;
    const int b_begin = group * a.rows_per_group;
    const int b_end = min(a.B, b_begin + a.rows_per_group);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int d = d0 + li;
    if (d0 <= D) {
        for (int k0 = b_begin; k0 < b_end; k0 += 4) {
            const int bb = k0 + lk;
            float av = 0.0f;
            if (bb < b_end) {
                if (d < D) {
                    av = a.X[(size_t)a.idx[bb] * D + d];
                    if (drop_thresh) av = probe_drop_hash(a.seed, a.step, (uint32_t)bb, (uint32_t)d) >= drop_thresh ? av * drop_scale : 0.0f;
                } else if (d == D) {
                    av = 1.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c0 + 16 * j < C) {   // wave-uniform
                    const int c = c0 + 16 * j + li;
                    const float bv = (bb < b_end && c < C) ? G[(size_t)bb * C + c] : 0.0f;
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
    }
    float ss = 0.0f;
    float* part = partial + (size_t)group * a.E;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + 16 * j + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int dr = d0 + 4 * lk + r;
            if (dr <= D && c < C) {
                part[(size_t)dr * C + c] = acc[j][r];
                ss += acc[j][r] * acc[j][r];
            }
        }
    }
    if (groups == 1) {   // one row group: the partial is the gradient, its squares count for the norm
        ss = block256_sum(ss, red);
        if (threadIdx.x == 0) ss_part[blockIdx.y * gridDim.x + blockIdx.x] = ss;
    }
}

// partial[0] += partial[1] + ... in group order; 1024 elements and one sum of squares per workgroup
template <bool SWEEP>
__global__ __launch_bounds__(256) void probe_reduce_kernel(float* __restrict__ partial, int E, int groups, float* __restrict__ ss_part, ProbeSweepOf<SWEEP> w) {
    if constexpr (SWEEP) {   // blockIdx.y is the trial
        if (sweep_idle(w, blockIdx.y)) return;
        partial += (size_t)blockIdx.y * w.partial_stride;
        ss_part += (size_t)blockIdx.y * w.ss_stride;
    }
    __shared__ float red[256];
    float ss = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = blockIdx.x * 1024 + q * 256 + threadIdx.x;
        if (i < E) {
            float v = partial[i];
            for (int g = 1; g < groups; ++g) v += partial[(size_t)g * E + i];
            partial[i] = v;
            ss += v * v;
        }
    }
    ss = block256_sum(ss, red);
    if (threadIdx.x == 0) ss_part[blockIdx.x] = ss;
}

// -------------------------------------------------------------------------------------------------------------------------- update
// SWEEP: blockIdx.y is the trial; its step sizes are step_sizes[2 t], [2 t + 1], its loss goes to a.step_loss[t].
template <bool SWEEP>
__global__ __launch_bounds__(256) void probe_update_kernel(ProbeUpdateArgs a, ProbeSweepOf<SWEEP> sw, const float* __restrict__ step_sizes) {
    float *params = a.params, *pm = a.m, *pv = a.v, *step_loss = a.step_loss;
    const float *grad = a.grad, *ss_part = a.ss_part, *loss_part = a.loss_part;
    int optimizer = a.optimizer;
    float lr = a.lr, alpha = a.alpha, weight_decay = a.weight_decay, clip = a.clip;
    if constexpr (SWEEP) {
        const int t = blockIdx.y;
        if (sweep_idle(sw, t)) return;
        const ProbeSweepTrial& tr = sw.trials[t];
        params = sw.state + (size_t)t * 4 * sw.E;
        pm = params + sw.E;
        pv = pm + sw.E;
        grad = sw.partial + (size_t)t * sw.partial_stride;
        ss_part = sw.ss_part + (size_t)t * sw.ss_stride;
        loss_part = sw.loss_part + (size_t)t * sw.loss_stride;
        step_loss = a.step_loss + t;
        optimizer = tr.optimizer;
        lr = step_sizes[2 * t];
        alpha = step_sizes[2 * t + 1];
        weight_decay = tr.weight_decay;
        clip = tr.clip;
    }
    __shared__ float red[256];
    const int t = threadIdx.x;
    float scale = 1.0f;
    if (clip > 0.0f) {   // every workgroup adds the same values in the same order: one scale, bit for bit
        float v = 0.0f;
        for (int i = t; i < a.n_ss; i += 256) v += ss_part[i];
        const float norm = sqrtf(block256_sum(v, red));
        if (norm > clip) scale = clip / norm;
    }
    if (blockIdx.x == 0 && step_loss) {
        float v = 0.0f;
        for (int i = t; i < a.n_loss; i += 256) v += loss_part[i];
        v = block256_sum(v, red);
        if (t == 0) *step_loss = v * a.loss_scale;
    }
    const int i = blockIdx.x * 256 + t;
    if (i >= a.E) return;
    const float g = grad[i] * scale;
    float w = params[i];
    if (optimizer == BN_PROBE_OPT_SGD) {   // Keras SGD with momentum: v = 0.9 v - lr g; w += v
        const float v = 0.9f * pm[i] - lr * g;
        pm[i] = v;
        w += v;
    } else {
        if (optimizer == BN_PROBE_OPT_ADAMW) w -= lr * weight_decay * w;   // decoupled, before the Adam step (Keras)
        const float m = pm[i] + (g - pm[i]) * 0.1f;        // 1 - beta as the float32 nearest to 0.1 / 0.001 (1.0f - 0.999f is 1.3e-5 off)
        const float v = pv[i] + (g * g - pv[i]) * 0.001f;
        pm[i] = m;
        pv[i] = v;
        w -= m * alpha / (sqrtf(v) + 1e-7f);   // alpha = lr_t sqrt(1 - b2^t) / (1 - b1^t): the bias correction folded into the step size
    }
    params[i] = w;
}

// out[0] = scale * (part[0] + part[1] + ...), one workgroup, fixed order (bn_probe_loss)
template <bool SWEEP>
__global__ __launch_bounds__(256) void probe_loss_sum_kernel(const float* __restrict__ part, long n, float scale, float* __restrict__ out, ProbeSweepOf<SWEEP> w) {
    if constexpr (SWEEP) {   // blockIdx.x is the trial
        if (sweep_idle(w, blockIdx.x)) return;
        part += (size_t)blockIdx.x * w.loss_stride;
        out += blockIdx.x;
    }
    __shared__ float red[256];
    float v = 0.0f;
    for (long i = threadIdx.x; i < n; i += 256) v += part[i];
    v = block256_sum(v, red);
    if (threadIdx.x == 0) *out = v * scale;
}

// ----------------------------------------------------------------------------------------------------------------------- launchers
// Host code, written once like the kernels: bn_probe.hip calls them with SWEEP = false and ProbeNoSweep{}, bn_probe_sweep.hip with
// SWEEP = true and the sweep's arguments, whose trials are one more grid axis.  A file holds the kernels its calls instantiate.
template <bool SWEEP>
inline unsigned probe_trials(const ProbeSweepOf<SWEEP>& w) {
    if constexpr (SWEEP) return (unsigned)w.T;
    else return 1u;
}

template <int NT, int MODE, int EXT, bool SWEEP>
bool probe_launch_fwd_one(const ProbeFwdArgs& a, const ProbeFwdExtraOf<SWEEP, EXT>& w, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024 && !ensure_dynamic_lds((const void*)&probe_fwd_kernel<NT, MODE, EXT, SWEEP>, lds)) return false;
    hipLaunchKernelGGL((probe_fwd_kernel<NT, MODE, EXT, SWEEP>), grid, block, lds, s, a, w);
    return true;
}

// EXT = 1 only when the call asks for row weights (mode 0) or the focal loss (modes 0 and 1): every other call runs the kernel without
// them.  Mode 2 (scores: bn_head_forward) is a single head's: a sweep has modes 0 and 1 only.
template <int NT, bool SWEEP>
bool probe_launch_fwd_nt(const ProbeFwdArgs& a, const ProbeSweepOf<SWEEP>& w, int mode, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    const bool ext = probe_fwd_ext(a, mode);
    if (mode == 0)
        return ext ? probe_launch_fwd_one<NT, 0, 1, SWEEP>(a, w, grid, block, lds, s) : probe_launch_fwd_one<NT, 0, 0, SWEEP>(a, w, grid, block, lds, s);
    if (SWEEP || mode == 1)
        return ext ? probe_launch_fwd_one<NT, 1, 1, SWEEP>(a, w, grid, block, lds, s) : probe_launch_fwd_one<NT, 1, 0, SWEEP>(a, w, grid, block, lds, s);
    if constexpr (!SWEEP) return probe_launch_fwd_one<NT, 2, 0, SWEEP>(a, w, grid, block, lds, s);   // (last: the order of the kernels in the code object)
    else return false;   // (not reached)
}

// The forward kernel's launch from the shapes: grid (row tiles, trials), one wave per column tile up to kFwdWaves, NT from per_wave
struct ProbeFwdGeom {
    dim3 grid, block;
    size_t lds;
    int per_wave;
};
inline ProbeFwdGeom probe_fwd_geom(const ProbeFwdArgs& a, unsigned trials) {
    const int ntiles = (a.C + 15) / 16;
    const int nw = ntiles < kFwdWaves ? ntiles : kFwdWaves;
    return {dim3((unsigned)((a.n + kRows - 1) / kRows), trials), dim3(64 * nw), (size_t)kRows * (((a.D + 3) & ~3) + kLdsPad) * sizeof(float),
            (ntiles + nw - 1) / nw};
}

// false: the runtime refused the LDS request
template <bool SWEEP>
bool probe_launch_fwd(const ProbeFwdArgs& a, const ProbeSweepOf<SWEEP>& w, int mode, hipStream_t s) {
    const ProbeFwdGeom g = probe_fwd_geom(a, probe_trials<SWEEP>(w));
    if (g.per_wave <= 1) return probe_launch_fwd_nt<1, SWEEP>(a, w, mode, g.grid, g.block, g.lds, s);
    if (g.per_wave <= 2) return probe_launch_fwd_nt<2, SWEEP>(a, w, mode, g.grid, g.block, g.lds, s);
    if (g.per_wave <= 4) return probe_launch_fwd_nt<4, SWEEP>(a, w, mode, g.grid, g.block, g.lds, s);
    return probe_launch_fwd_nt<8, SWEEP>(a, w, mode, g.grid, g.block, g.lds, s);   // C > 2048: two passes over the columns
}

// The EXT = 2 family (bn_probe_set_qat with quantize_logits): all three modes, single fit (bn_probe.hip: launch_probe_fwd_qat)
template <int NT>
bool probe_launch_fwd_qat_nt(const ProbeFwdArgs& a, const ProbeQatArgs& q, int mode, const ProbeFwdGeom& g, hipStream_t s) {
    if (mode == 0) return probe_launch_fwd_one<NT, 0, 2, false>(a, q, g.grid, g.block, g.lds, s);
    if (mode == 1) return probe_launch_fwd_one<NT, 1, 2, false>(a, q, g.grid, g.block, g.lds, s);
    return probe_launch_fwd_one<NT, 2, 2, false>(a, q, g.grid, g.block, g.lds, s);
}

// grid z: trial * row_groups + group
template <bool SWEEP>
void probe_launch_dw(const ProbeDwArgs& a, const ProbeSweepOf<SWEEP>& w, int row_groups, hipStream_t s) {
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)((a.D + 1 + 63) / 64), probe_trials<SWEEP>(w) * (unsigned)row_groups);
    hipLaunchKernelGGL(probe_dw_kernel<SWEEP>, grid, dim3(256), 0, s, a, w, SWEEP ? row_groups : 0);
}

template <bool SWEEP>
void probe_launch_reduce(float* partial, int E, int groups, float* ss_part, const ProbeSweepOf<SWEEP>& w, hipStream_t s) {
    hipLaunchKernelGGL(probe_reduce_kernel<SWEEP>, dim3((unsigned)((E + 1023) / 1024), probe_trials<SWEEP>(w)), dim3(256), 0, s, partial, E, groups, ss_part, w);
}

// a sweep: `a.lr` / `a.alpha` of trial t are step_sizes[2 t], [2 t + 1]; its loss goes to a.step_loss[t]
template <bool SWEEP>
void probe_launch_update(const ProbeUpdateArgs& a, const ProbeSweepOf<SWEEP>& w, const float* step_sizes, hipStream_t s) {
    hipLaunchKernelGGL(probe_update_kernel<SWEEP>, dim3((unsigned)((a.E + 255) / 256), probe_trials<SWEEP>(w)), dim3(256), 0, s, a, w, step_sizes);
}

// one workgroup per head
template <bool SWEEP>
void probe_launch_loss_sum(const float* part, long n, float scale, float* out, const ProbeSweepOf<SWEEP>& w, hipStream_t s) {
    hipLaunchKernelGGL(probe_loss_sum_kernel<SWEEP>, dim3(probe_trials<SWEEP>(w)), dim3(256), 0, s, part, n, scale, out, w);
}

}  // namespace bn
