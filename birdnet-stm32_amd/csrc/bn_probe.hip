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

}  // namespace bn
