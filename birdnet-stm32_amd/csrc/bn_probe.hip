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
// The kernels are written in bn_probe_step.h, shared with the sweep of bn_probe_sweep.hip: these are the SWEEP = false instantiations.
// Device functions: expf and logf (ocml, <= 1 ulp), IEEE division and sqrtf (correctly rounded: the file is built without fast-math).
#include <hip/hip_runtime.h>

#include "bn_probe_step.h"

namespace bn {

template <int NT, int MODE, int EXT>
static bool launch_fwd_one(const ProbeFwdArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024 && !ensure_dynamic_lds((const void*)&probe_fwd_kernel<NT, MODE, EXT, false>, lds)) return false;
    hipLaunchKernelGGL((probe_fwd_kernel<NT, MODE, EXT, false>), grid, block, lds, s, a, ProbeNoSweep{});
    return true;
}

// EXT = 1 only when the call asks for row weights (mode 0) or the focal loss (modes 0 and 1): every other call runs the kernel without them
template <int NT>
static bool launch_fwd_nt(const ProbeFwdArgs& a, int mode, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    const bool ext = probe_fwd_ext(a, mode);
    if (mode == 0) return ext ? launch_fwd_one<NT, 0, 1>(a, grid, block, lds, s) : launch_fwd_one<NT, 0, 0>(a, grid, block, lds, s);
    if (mode == 1) return ext ? launch_fwd_one<NT, 1, 1>(a, grid, block, lds, s) : launch_fwd_one<NT, 1, 0>(a, grid, block, lds, s);
    return launch_fwd_one<NT, 2, 0>(a, grid, block, lds, s);
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

void launch_probe_dw(const ProbeDwArgs& a, int row_groups, hipStream_t s) {
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)((a.D + 1 + 63) / 64), (unsigned)row_groups);
    hipLaunchKernelGGL(probe_dw_kernel<false>, grid, dim3(256), 0, s, a, ProbeNoSweep{}, 0);
}

void launch_probe_reduce(float* partial, int E, int groups, float* ss_part, hipStream_t s) {
    hipLaunchKernelGGL(probe_reduce_kernel<false>, dim3((unsigned)((E + 1023) / 1024)), dim3(256), 0, s, partial, E, groups, ss_part, ProbeNoSweep{});
}

void launch_probe_update(const ProbeUpdateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(probe_update_kernel<false>, dim3((unsigned)((a.E + 255) / 256)), dim3(256), 0, s, a, ProbeNoSweep{}, nullptr);
}

void launch_probe_loss_sum(const float* part, long n, float scale, float* out, hipStream_t s) {
    hipLaunchKernelGGL(probe_loss_sum_kernel<false>, dim3(1), dim3(256), 0, s, part, n, scale, out, ProbeNoSweep{});
}

void preload_probe() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&probe_update_kernel<false>));
}

}  // namespace bn
