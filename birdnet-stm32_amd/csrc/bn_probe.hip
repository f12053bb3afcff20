// bn_probe.hip — a classifier head on frozen embeddings: scores = act(dropout(x) W + b), trained on the device.
//
// One training step is three launches (four when the batch is split into row groups):
//   probe_fwd_kernel    a workgroup owns 16 batch rows and ALL C columns: gathers the rows, applies the dropout mask, logits on the matrix
//                       cores (v_mfma_f32_16x16x4_f32: exact f32), activation, the loss partial of its rows, G = dLoss/dlogits.  The logits
//                       of a row tile stay in registers (up to 8 column tiles per wave, 2048 columns per workgroup), so softmax sees whole
//                       rows without a round trip; a wider head takes two passes over the columns.
//   probe_dw_kernel     grid (C tiles, D tiles, row groups): dW = x_dropped^T G over the rows of one group, accumulated in registers, one
//                       partial per group.  The bias is row D of the parameter matrix (a feature that is always 1): db falls out of the same product.
//   probe_reduce_kernel (only with more than one row group) adds the partials in group order.
//   probe_update_kernel adds the per-workgroup sums of squares and loss partials in a fixed order, clips by global norm, applies the optimiser.
// No floating-point atomics anywhere: the map from tiles to workgroups depends on the shapes only and every sum has a fixed order, so the
// same inputs and seed give the same bits.
//
// Device functions: expf and logf (ocml, <= 1 ulp), IEEE division and sqrtf (correctly rounded: the file is built without fast-math).
#include <hip/hip_runtime.h>

#include "../../include/birdnet_hip.h"
#include "bn_device.h"
#include "bn_kernels.h"

namespace bn {


namespace {

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

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------- forward
// MODE 0: training (G and the loss partial), 1: loss partial only, 2: scores.  NT: column tiles per wave (tile t of wave w is w + t * waves).
template <int NT, int MODE>
__global__ __launch_bounds__(1024) void probe_fwd_kernel(ProbeFwdArgs a) {
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
            if (a.drop_thresh) v = probe_drop_hash(a.seed, a.step, (uint32_t)row, (uint32_t)d) >= a.drop_thresh ? v * a.drop_scale : 0.0f;
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
                    const float bv = (k < D && c < C) ? a.W[(size_t)k * C + c] : 0.0f;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = (tile0 + t * nw) * 16 + li;
            okc[t] = (tile0 + t * nw) < ntiles && c < C;
            const float bias = okc[t] ? a.b[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += bias;
        }
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
                    if (okc[t]) v = fmaxf(v, acc[t][r]);
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
                    if (okc[t]) v += expf(acc[t][r] - mn[r]);
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
                const float p = a.softmax ? expf(acc[t][r] - m[r]) / s[r] : 1.0f / (1.0f + expf(-acc[t][r]));
                if constexpr (MODE == 2) {
                    a.out[(size_t)row * C + c] = p;
                } else {
                    const long src = (MODE == 0 && a.idx) ? (long)a.idx[row] : row;
                    const float y = a.Y[(size_t)src * C + c];
                    const float pc = fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f);
                    if (a.softmax)
                        loss -= y * logf(pc);
                    else
                        loss -= y * logf(pc) + (1.0f - y) * logf(1.0f - pc);
                    if constexpr (MODE == 0) a.out[(size_t)row * C + c] = (p - y) * a.g_scale;
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
            a.loss_part[blockIdx.x] = v;
        }
    }
}

template <int NT>
static bool launch_fwd_nt(const ProbeFwdArgs& a, int mode, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    const void* k = mode == 0 ? (const void*)&probe_fwd_kernel<NT, 0> : mode == 1 ? (const void*)&probe_fwd_kernel<NT, 1> : (const void*)&probe_fwd_kernel<NT, 2>;
    if (lds > 64 * 1024 && !ensure_dynamic_lds(k, lds)) return false;
    if (mode == 0)
        hipLaunchKernelGGL((probe_fwd_kernel<NT, 0>), grid, block, lds, s, a);
    else if (mode == 1)
        hipLaunchKernelGGL((probe_fwd_kernel<NT, 1>), grid, block, lds, s, a);
    else
        hipLaunchKernelGGL((probe_fwd_kernel<NT, 2>), grid, block, lds, s, a);
    return true;
}

bool launch_probe_fwd(const ProbeFwdArgs& a, int mode, hipStream_t s) {
    const int ntiles = (a.C + 15) / 16;
    const int nw = ntiles < kFwdWaves ? ntiles : kFwdWaves;
    const int per_wave = (ntiles + nw - 1) / nw;
    const dim3 grid((unsigned)((a.n + kRows - 1) / kRows)), block(64 * nw);
    const size_t lds = (size_t)kRows * (((a.D + 3) & ~3) + kLdsPad) * sizeof(float);
    if (per_wave <= 1) return launch_fwd_nt<1>(a, mode, grid, block, lds, s);
    if (per_wave <= 2) return launch_fwd_nt<2>(a, mode, grid, block, lds, s);
    if (per_wave <= 4) return launch_fwd_nt<4>(a, mode, grid, block, lds, s);
    return launch_fwd_nt<8>(a, mode, grid, block, lds, s);   // C > 2048: two passes over the columns
}

// ------------------------------------------------------------------------------------------------------------------------ gradient
// Workgroup (bx, by, bz): rows [16 * (4 by + wave), +16) of dParams (row D is the bias), columns [64 bx, +64), batch rows of group bz.
__global__ __launch_bounds__(256) void probe_dw_kernel(ProbeDwArgs a) {
    __shared__ float red[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, C = a.C;
    const int d0 = (blockIdx.y * 4 + wave) * 16, c0 = blockIdx.x * 64;
    const int b_begin = blockIdx.z * a.rows_per_group;
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
                    if (a.drop_thresh) av = probe_drop_hash(a.seed, a.step, (uint32_t)bb, (uint32_t)d) >= a.drop_thresh ? av * a.drop_scale : 0.0f;
                } else if (d == D) {
                    av = 1.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c0 + 16 * j < C) {   // wave-uniform
                    const int c = c0 + 16 * j + li;
                    const float bv = (bb < b_end && c < C) ? a.G[(size_t)bb * C + c] : 0.0f;
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
    }
    float ss = 0.0f;
    float* part = a.partial + (size_t)blockIdx.z * a.E;
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
    if (gridDim.z == 1) {   // one row group: the partial is the gradient, its squares count for the norm
        ss = block256_sum(ss, red);
        if (threadIdx.x == 0) a.ss_part[blockIdx.y * gridDim.x + blockIdx.x] = ss;
    }
}

void launch_probe_dw(const ProbeDwArgs& a, int row_groups, hipStream_t s) {
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)((a.D + 1 + 63) / 64), (unsigned)row_groups);
    hipLaunchKernelGGL(probe_dw_kernel, grid, dim3(256), 0, s, a);
}

// partial[0] += partial[1] + ... in group order; 1024 elements and one sum of squares per workgroup
__global__ __launch_bounds__(256) void probe_reduce_kernel(float* __restrict__ partial, int E, int groups, float* __restrict__ ss_part) {
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

void launch_probe_reduce(float* partial, int E, int groups, float* ss_part, hipStream_t s) {
    hipLaunchKernelGGL(probe_reduce_kernel, dim3((unsigned)((E + 1023) / 1024)), dim3(256), 0, s, partial, E, groups, ss_part);
}

// -------------------------------------------------------------------------------------------------------------------------- update
__global__ __launch_bounds__(256) void probe_update_kernel(ProbeUpdateArgs a) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    float scale = 1.0f;
    if (a.clip > 0.0f) {   // every workgroup adds the same values in the same order: one scale, bit for bit
        float v = 0.0f;
        for (int i = t; i < a.n_ss; i += 256) v += a.ss_part[i];
        const float norm = sqrtf(block256_sum(v, red));
        if (norm > a.clip) scale = a.clip / norm;
    }
    if (blockIdx.x == 0 && a.step_loss) {
        float v = 0.0f;
        for (int i = t; i < a.n_loss; i += 256) v += a.loss_part[i];
        v = block256_sum(v, red);
        if (t == 0) *a.step_loss = v * a.loss_scale;
    }
    const int i = blockIdx.x * 256 + t;
    if (i >= a.E) return;
    const float g = a.grad[i] * scale;
    float w = a.params[i];
    if (a.optimizer == BN_PROBE_OPT_SGD) {   // Keras SGD with momentum: v = 0.9 v - lr g; w += v
        const float v = 0.9f * a.m[i] - a.lr * g;
        a.m[i] = v;
        w += v;
    } else {
        if (a.optimizer == BN_PROBE_OPT_ADAMW) w -= a.lr * a.weight_decay * w;   // decoupled, before the Adam step (Keras)
        const float m = a.m[i] + (g - a.m[i]) * 0.1f;        // 1 - beta as the float32 nearest to 0.1 / 0.001 (1.0f - 0.999f is 1.3e-5 off)
        const float v = a.v[i] + (g * g - a.v[i]) * 0.001f;
        a.m[i] = m;
        a.v[i] = v;
        w -= m * a.alpha / (sqrtf(v) + 1e-7f);   // alpha = lr_t sqrt(1 - b2^t) / (1 - b1^t): the bias correction folded into the step size
    }
    a.params[i] = w;
}

void launch_probe_update(const ProbeUpdateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(probe_update_kernel, dim3((unsigned)((a.E + 255) / 256)), dim3(256), 0, s, a);
}

// out[0] = scale * (part[0] + part[1] + ...), one workgroup, fixed order (bn_probe_loss)
__global__ __launch_bounds__(256) void probe_loss_sum_kernel(const float* __restrict__ part, long n, float scale, float* __restrict__ out) {
    __shared__ float red[256];
    float v = 0.0f;
    for (long i = threadIdx.x; i < n; i += 256) v += part[i];
    v = block256_sum(v, red);
    if (threadIdx.x == 0) *out = v * scale;
}

void launch_probe_loss_sum(const float* part, long n, float scale, float* out, hipStream_t s) {
    hipLaunchKernelGGL(probe_loss_sum_kernel, dim3(1), dim3(256), 0, s, part, n, scale, out);
}

void preload_probe() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&probe_update_kernel));
}

}  // namespace bn
