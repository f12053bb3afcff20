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
// With bn_probe_set_qat two more launches stand in front of the forward, probe_qat_amax_kernel and probe_qat_quant_kernel
// (the weights as the INT8 export will hold them, into a second buffer the forward reads), and the forward is its EXT = 2 instantiation.
// No floating-point atomics anywhere: the map from tiles to workgroups depends on the shapes only and every sum has a fixed order, so the
// same inputs and seed give the same bits.
//
// The kernels are written in bn_probe_step.h, shared with the sweep of bn_probe_sweep.hip: these are the SWEEP = false instantiations.
// Device functions: expf and logf (ocml, <= 1 ulp), IEEE division and sqrtf (correctly rounded: the file is built without fast-math).
#include <hip/hip_runtime.h>

#include "bn_probe_step.h"

// The launchers are bn_probe_step.h's, instantiated here.  The compiler emits a kernel where the file first names it, so preload stands
// between the update and the loss sum: the kernels keep their order in the code object.
namespace bn {

bool launch_probe_fwd(const ProbeFwdArgs& a, int mode, hipStream_t s) { return probe_launch_fwd<false>(a, ProbeNoSweep{}, mode, s); }

void launch_probe_dw(const ProbeDwArgs& a, int row_groups, hipStream_t s) { probe_launch_dw<false>(a, ProbeNoSweep{}, row_groups, s); }

void launch_probe_reduce(float* partial, int E, int groups, float* ss_part, hipStream_t s) {
    probe_launch_reduce<false>(partial, E, groups, ss_part, ProbeNoSweep{}, s);
}

void launch_probe_update(const ProbeUpdateArgs& a, hipStream_t s) { probe_launch_update<false>(a, ProbeNoSweep{}, nullptr, s); }

void preload_probe() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&probe_update_kernel<false>));
}

void launch_probe_loss_sum(const float* part, long n, float scale, float* out, hipStream_t s) {
    probe_launch_loss_sum<false>(part, n, scale, out, ProbeNoSweep{}, s);
}

// ---------------------------------------------------------------------------------- quantisation-aware fine-tuning
// Behind the kernels above in the code object, which keep their places: the forward kernel's EXT = 2 family, and the two kernels that turn
// the shadow parameters into the weights such a forward reads (templates, because the compiler emits a plain kernel in front of every
// instantiation of the file).
bool launch_probe_fwd_qat(const ProbeFwdArgs& a, const ProbeQatArgs& q, int mode, hipStream_t s) {
    const ProbeFwdGeom g = probe_fwd_geom(a, 1u);
    if (g.per_wave <= 1) return probe_launch_fwd_qat_nt<1>(a, q, mode, g, s);
    if (g.per_wave <= 2) return probe_launch_fwd_qat_nt<2>(a, q, mode, g, s);
    if (g.per_wave <= 4) return probe_launch_fwd_qat_nt<4>(a, q, mode, g, s);
    return probe_launch_fwd_qat_nt<8>(a, q, mode, g, s);
}

constexpr int kAmaxCols = 64;                     // a workgroup of the first kernel: 64 columns x 16 row slices, one wave per slice
constexpr int kQuantCols = 256, kQuantRows = 8;   // ... of the second: 256 columns x 8 rows, one thread per column

// amax[c] = max_k |P[k, c]| over the D weight rows; a wave reads 64 consecutive floats of one row
template <int SLICES>   // row slices = waves
__global__ __launch_bounds__(kAmaxCols * SLICES) void probe_qat_amax_kernel(const float* __restrict__ P, int D, int C, float* __restrict__ amax) {
    __shared__ float red[SLICES][kAmaxCols];
    const int cx = threadIdx.x, ky = threadIdx.y, c = blockIdx.x * kAmaxCols + cx;
    float m = 0.0f;
    if (c < C)
        for (int k = ky; k < D; k += SLICES) m = fmaxf(m, fabsf(P[(size_t)k * C + c]));
    red[ky][cx] = m;
    __syncthreads();
    if (ky == 0 && c < C) {
        for (int j = 1; j < SLICES; ++j) m = fmaxf(m, red[j][cx]);
        amax[c] = m;
    }
}

// conversion/quantize.py: quantize_weights in float64, element for element: s = max(amax_c, 5e-7) / 127, q = clip(rint(w / s), -127, 127),
// Pq = float(q) * float(s) as a float32 product, which is q.astype(float32) * s_w bit for bit (q goes through an integer: no -0).
// per_tensor: every class takes the largest amax, which every workgroup finds for itself (a maximum has no order).  Row D, the bias, is copied.
template <bool PER_TENSOR>
__global__ __launch_bounds__(kQuantCols) void probe_qat_quant_kernel(const float* __restrict__ P, float* __restrict__ Pq, const float* __restrict__ amax,
                                                                     int D, int C) {
    __shared__ float red[kQuantCols];
    const int t = threadIdx.x, c = blockIdx.x * kQuantCols + t;
    float am = c < C ? amax[c] : 0.0f;
    if constexpr (PER_TENSOR) {
        float v = 0.0f;
        for (int i = t; i < C; i += kQuantCols) v = fmaxf(v, amax[i]);
        red[t] = v;
        __syncthreads();
        for (int h = kQuantCols / 2; h > 0; h >>= 1) {
            if (t < h) red[t] = fmaxf(red[t], red[t + h]);
            __syncthreads();
        }
        am = red[0];
    }
    if (c >= C) return;
    const double s = fmax((double)am, 5e-7) / 127.0;
    const float sf = (float)s;
    const int k0 = blockIdx.y * kQuantRows, k1 = min(k0 + kQuantRows, D + 1);
    for (int k = k0; k < k1; ++k) {
        float v = P[(size_t)k * C + c];
        if (k < D) v = (float)(int)fmin(fmax(rint((double)v / s), -127.0), 127.0) * sf;
        Pq[(size_t)k * C + c] = v;
    }
}

void launch_probe_qat_weights(const float* P, float* Pq, float* amax, int D, int C, bool per_tensor, hipStream_t s) {
    hipLaunchKernelGGL(probe_qat_amax_kernel<16>, dim3((unsigned)((C + kAmaxCols - 1) / kAmaxCols)), dim3(kAmaxCols, 16), 0, s, P, D, C, amax);
    const dim3 grid((unsigned)((C + kQuantCols - 1) / kQuantCols), (unsigned)((D + 1 + kQuantRows - 1) / kQuantRows));
    if (per_tensor) hipLaunchKernelGGL(probe_qat_quant_kernel<true>, grid, dim3(kQuantCols), 0, s, P, Pq, amax, D, C);
    else hipLaunchKernelGGL(probe_qat_quant_kernel<false>, grid, dim3(kQuantCols), 0, s, P, Pq, amax, D, C);
}

}  // namespace bn
