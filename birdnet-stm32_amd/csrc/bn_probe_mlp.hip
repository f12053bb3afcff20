// bn_probe_mlp.hip — the hidden layer of a classifier head with one:
//     a = drop1(x) W1 + b1;  h = relu(a);  z = drop2(h) W2 + b2;  p = sigmoid(z) | softmax(z)
// trained on the device like the linear head of bn_probe.hip.  The parameters are one vector [(D + 1) * H | (H + 1) * C] (each bias the
// last row of its matrix), so the norm, the clip and the optimiser act on it as a whole.  A training step:
//   probe_mlp_hidden_kernel<true>   a workgroup owns 16 batch rows: gathers them through idx with drop1 applied in LDS (as probe_fwd_kernel
//                                   stages them), a on the matrix cores (v_mfma_f32_16x16x4_f32: exact f32), bias, ReLU, drop2, and writes
//                                   hd = relu(a) * m2 [B, H] in batch order.  It also copies the batch's targets (and row weights) into batch
//                                   order, because the kernels behind it index X and Y through one idx and hd has none.
//   probe_fwd_kernel                bn_probe.hip's, on (hd, Yb) without idx and without dropout: logits, activation, loss partials, G
//   probe_dw_kernel                 bn_probe.hip's, on (hd through the identity, G): dW2 and db2
//   probe_mlp_bwd_kernel            dA[b, j] = (sum_c G[b, c] W2[j, c]) * scale2 where hd[b, j] > 0, else 0.  The ReLU gate and drop2's mask
//                                   are both read off hd: hd > 0 exactly where a > 0 and the element was kept.
//   probe_dw_kernel                 bn_probe.hip's, on (X through idx with drop1, dA): dW1 and db1
//   probe_reduce_kernel             (only with more than one row group) and probe_update_kernel, over the whole vector
// The launches of bn_probe.hip are that file's own instantiations, called through its launchers: nothing of them is compiled here.
// No floating-point atomics; every sum has a fixed order that depends on the shapes only, so the same inputs and seed give the same bits.
// <false> is the hidden layer without dropout or gather, over rows as they lie: validation loss and scoring (bn_head_mlp_forward).
#include <hip/hip_runtime.h>

#include "bn_probe_step.h"

namespace bn {

constexpr int kMlpTiles = 4;   // column tiles of H a wave accumulates at once

template <bool TRAIN>
__global__ __launch_bounds__(1024) void probe_mlp_hidden_kernel(ProbeMlpFwdArgs a) {
    extern __shared__ float xs[];                 // [16][Dp + kLdsPad], rows beyond the batch and columns beyond D are zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int D = a.D, H = a.H, Dp = (D + 3) & ~3, ld = Dp + kLdsPad;
    const long row0 = (long)blockIdx.x * kRows;

    for (int e = tid; e < kRows * Dp; e += blockDim.x) {
        const int r = e / Dp, d = e - r * Dp;
        const long row = row0 + r;
        float v = 0.0f;
        if (row < a.n && d < D) {
            const long src = a.idx ? (long)a.idx[row] : row;
            v = a.X[src * D + d];
            if constexpr (TRAIN)
                if (a.drop_thresh) v = probe_drop_hash(a.seed, a.step, (uint32_t)row, (uint32_t)d) >= a.drop_thresh ? v * a.drop_scale : 0.0f;
        }
        xs[r * ld + d] = v;
    }
    if constexpr (TRAIN) {   // the batch's targets and weights in batch order
        const int C = a.C;
        for (int e = tid; e < kRows * C; e += blockDim.x) {
            const int r = e / C, c = e - r * C;
            const long row = row0 + r;
            if (row < a.n) a.Yb[(size_t)row * C + c] = a.Y[(size_t)(a.idx ? (long)a.idx[row] : row) * C + c];
        }
        if (a.row_weight && tid < kRows && row0 + tid < a.n) a.wb[row0 + tid] = a.row_weight[a.idx ? (long)a.idx[row0 + tid] : row0 + tid];
    }
    __syncthreads();

    const int ntiles = (H + 15) >> 4;
    const int li = lane & 15, lk = lane >> 4;
    const float* xrow = xs + li * ld + lk;
    // lane holds rows 4 * lk + r (r = 0..3) of column tile * 16 + li; tile t of a wave's round is tile0 + t * waves
    for (int tile0 = wave; tile0 < ntiles; tile0 += nw * kMlpTiles) {   // wave-uniform
        f32x4 acc[kMlpTiles];
#pragma unroll
        for (int t = 0; t < kMlpTiles; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < Dp; k0 += 4) {
            const float av = xrow[k0];
            const int k = k0 + lk;
#pragma unroll
            for (int t = 0; t < kMlpTiles; ++t) {
                const int tile = tile0 + t * nw;
                if (tile < ntiles) {
                    const int j = tile * 16 + li;
                    const float bv = (k < D && j < H) ? a.W1[(size_t)k * H + j] : 0.0f;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kMlpTiles; ++t) {
            const int tile = tile0 + t * nw;
            const int j = tile * 16 + li;
            if (tile >= ntiles || j >= H) continue;
            const float bv = a.b1[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = row0 + 4 * lk + r;
                if (row >= a.n) continue;
                float v = acc[t][r] + bv;
                v = v > 0.0f ? v : 0.0f;
                if constexpr (TRAIN)
                    if (a.drop_thresh) v = probe_drop_hash(a.seed2, a.step, (uint32_t)row, (uint32_t)j) >= a.drop_thresh ? v * a.drop_scale : 0.0f;
                a.hd[(size_t)row * H + j] = v;
            }
        }
    }
}

// Workgroup (bx, by): batch rows [16 bx, +16), hidden units [16 (4 by + wave), +16); the sum over the classes in steps of 4
__global__ __launch_bounds__(256) void probe_mlp_bwd_kernel(ProbeMlpBwdArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int B = a.B, H = a.H, C = a.C;
    const int row0 = blockIdx.x * 16, j0 = (blockIdx.y * 4 + wave) * 16;
    if (j0 >= H) return;   // wave-uniform; the kernel has no barrier
    const int b = row0 + li, j = j0 + li;
    const float* grow = a.G + (size_t)(b < B ? b : 0) * C;
    const float* wrow = a.W2 + (size_t)(j < H ? j : 0) * C;
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < C; k0 += 4) {
        const int k = k0 + lk;
        const float av = (b < B && k < C) ? grow[k] : 0.0f;
        const float bv = (j < H && k < C) ? wrow[k] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * lk + r;
        if (row < B && j < H) {
            const size_t at = (size_t)row * H + j;
            a.dA[at] = a.hd[at] > 0.0f ? acc[r] * a.scale2 : 0.0f;
        }
    }
}

template <bool TRAIN>
static bool probe_mlp_hidden_launch(const ProbeMlpFwdArgs& a, hipStream_t s) {
    const int ntiles = (a.H + 15) / 16;
    const int nw = ntiles < kFwdWaves ? ntiles : kFwdWaves;
    const size_t lds = (size_t)kRows * (((a.D + 3) & ~3) + kLdsPad) * sizeof(float);
    if (lds > 64 * 1024 && !ensure_dynamic_lds((const void*)&probe_mlp_hidden_kernel<TRAIN>, lds)) return false;
    hipLaunchKernelGGL(probe_mlp_hidden_kernel<TRAIN>, dim3((unsigned)((a.n + kRows - 1) / kRows)), dim3(64 * nw), lds, s, a);
    return true;
}

bool launch_probe_mlp_hidden(const ProbeMlpFwdArgs& a, bool train, hipStream_t s) {
    return train ? probe_mlp_hidden_launch<true>(a, s) : probe_mlp_hidden_launch<false>(a, s);
}

void launch_probe_mlp_bwd(const ProbeMlpBwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(probe_mlp_bwd_kernel, dim3((unsigned)((a.B + 15) / 16), (unsigned)((a.H + 63) / 64)), dim3(256), 0, s, a);
}

void preload_probe_mlp() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&probe_mlp_bwd_kernel));
}

}  // namespace bn
