// bn_probe_sweep.hip — T classifier heads trained in lock-step on the same rows: a hyperparameter sweep.
//
// One training step of a single head is launch-bound at small batches (bn_probe.hip: three launches, four with row groups, of a few
// dozen workgroups each).  The trials of a sweep share D, C, the activation, the batch, the resident X / Y, the permutation, the step
// counter, the dropout draw and the initial weights; they differ in optimiser, step sizes, weight decay, clip norm, dropout rate (a
// threshold on the shared draw) and label smoothing.  So the same launches carry all of them: the trial is one more grid axis —
//   probe_fwd_kernel     grid (row tiles, T)
//   probe_dw_kernel      grid (C tiles, D tiles, T * row groups): z = trial * groups + group
//   probe_reduce_kernel  grid (E / 1024, T)
//   probe_update_kernel  grid (E / 256, T)
// with the kernels of bn_probe_step.h instantiated with SWEEP = true: a workgroup first takes its trial's row of the device table
// (ProbeSweepTrial) and its slices of the per-trial buffers where a single fit takes kernel arguments, then runs the single fit's
// statements.  Within a trial the tile-to-workgroup map, the row groups and every summation order are those of the single fit: a trial
// without label smoothing has the bits of bn_probe_* with the same hyperparameters.  No floating-point atomics.  Workgroups of a trial
// whose `active` byte is 0 return before they read or write anything.
#include <hip/hip_runtime.h>

#include "bn_probe_step.h"

// The launchers are bn_probe_step.h's, instantiated here.  The compiler emits a kernel where the file first names it, so preload stands
// between the update and the loss sum: the kernels keep their order in the code object.
namespace bn {

// mode 0 (training) or 1 (loss)
bool launch_probe_sweep_fwd(const ProbeFwdArgs& a, const ProbeSweepArgs& w, int mode, hipStream_t s) { return probe_launch_fwd<true>(a, w, mode, s); }

void launch_probe_sweep_dw(const ProbeDwArgs& a, const ProbeSweepArgs& w, int row_groups, hipStream_t s) { probe_launch_dw<true>(a, w, row_groups, s); }

void launch_probe_sweep_reduce(const ProbeSweepArgs& w, int groups, hipStream_t s) {
    probe_launch_reduce<true>(w.partial, w.E, groups, w.ss_part, w, s);
}

void launch_probe_sweep_update(const ProbeUpdateArgs& a, const ProbeSweepArgs& w, const float* step_sizes, hipStream_t s) {
    probe_launch_update<true>(a, w, step_sizes, s);
}

void preload_probe_sweep() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&probe_update_kernel<true>));
}

// out[t] = scale * (the n_parts loss partials of trial t in order) (bn_probe_sweep_loss)
void launch_probe_sweep_loss_sum(const ProbeSweepArgs& w, long n_parts, float scale, float* out, hipStream_t s) {
    probe_launch_loss_sum<true>(w.loss_part, n_parts, scale, out, w, s);
}

// the parameters of every trial with mask[t] != 0 -> its best-weights slot (bn_probe_sweep_snapshot)
__global__ __launch_bounds__(256) void probe_sweep_snapshot_kernel(float* __restrict__ state, int E, const uint8_t* __restrict__ mask) {
    const int t = blockIdx.y;
    if (!mask[t]) return;
    float* p = state + (size_t)t * 4 * E;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < E) p[(size_t)3 * E + i] = p[i];
}

void launch_probe_sweep_snapshot(const ProbeSweepArgs& w, const uint8_t* mask, hipStream_t s) {
    hipLaunchKernelGGL(probe_sweep_snapshot_kernel, dim3((unsigned)((w.E + 255) / 256), (unsigned)w.T), dim3(256), 0, s, w.state, w.E, mask);
}

}  // namespace bn
