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

namespace bn {

template <int NT, int MODE, int EXT>
static bool launch_sweep_fwd_one(const ProbeFwdArgs& a, const ProbeSweepArgs& w, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024 && !ensure_dynamic_lds((const void*)&probe_fwd_kernel<NT, MODE, EXT, true>, lds)) return false;
    hipLaunchKernelGGL((probe_fwd_kernel<NT, MODE, EXT, true>), grid, block, lds, s, a, w);
    return true;
}

template <int NT>
static bool launch_sweep_fwd_nt(const ProbeFwdArgs& a, const ProbeSweepArgs& w, int mode, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    const bool ext = probe_fwd_ext(a, mode);   // as launch_fwd_nt (bn_probe.hip)
    if (mode == 0) return ext ? launch_sweep_fwd_one<NT, 0, 1>(a, w, grid, block, lds, s) : launch_sweep_fwd_one<NT, 0, 0>(a, w, grid, block, lds, s);
    return ext ? launch_sweep_fwd_one<NT, 1, 1>(a, w, grid, block, lds, s) : launch_sweep_fwd_one<NT, 1, 0>(a, w, grid, block, lds, s);
}

// The launch shape of launch_probe_fwd (bn_probe.hip) with the trials along y; mode 0 (training) or 1 (loss)
bool launch_probe_sweep_fwd(const ProbeFwdArgs& a, const ProbeSweepArgs& w, int mode, hipStream_t s) {
    const int ntiles = (a.C + 15) / 16;
    const int nw = ntiles < kFwdWaves ? ntiles : kFwdWaves;
    const int per_wave = (ntiles + nw - 1) / nw;
    const dim3 grid((unsigned)((a.n + kRows - 1) / kRows), (unsigned)w.T), block(64 * nw);
    const size_t lds = (size_t)kRows * (((a.D + 3) & ~3) + kLdsPad) * sizeof(float);
    if (per_wave <= 1) return launch_sweep_fwd_nt<1>(a, w, mode, grid, block, lds, s);
    if (per_wave <= 2) return launch_sweep_fwd_nt<2>(a, w, mode, grid, block, lds, s);
    if (per_wave <= 4) return launch_sweep_fwd_nt<4>(a, w, mode, grid, block, lds, s);
    return launch_sweep_fwd_nt<8>(a, w, mode, grid, block, lds, s);
}

void launch_probe_sweep_dw(const ProbeDwArgs& a, const ProbeSweepArgs& w, int row_groups, hipStream_t s) {
    const dim3 grid((unsigned)((a.C + 63) / 64), (unsigned)((a.D + 1 + 63) / 64), (unsigned)(w.T * row_groups));
    hipLaunchKernelGGL(probe_dw_kernel<true>, grid, dim3(256), 0, s, a, w, row_groups);
}

void launch_probe_sweep_reduce(const ProbeSweepArgs& w, int groups, hipStream_t s) {
    hipLaunchKernelGGL(probe_reduce_kernel<true>, dim3((unsigned)((w.E + 1023) / 1024), (unsigned)w.T), dim3(256), 0, s, w.partial, w.E, groups, w.ss_part, w);
}

void launch_probe_sweep_update(const ProbeUpdateArgs& a, const ProbeSweepArgs& w, const float* step_sizes, hipStream_t s) {
    hipLaunchKernelGGL(probe_update_kernel<true>, dim3((unsigned)((a.E + 255) / 256), (unsigned)w.T), dim3(256), 0, s, a, w, step_sizes);
}

// out[t] = scale * (the n_parts loss partials of trial t in order), one workgroup per trial (bn_probe_sweep_loss)
void launch_probe_sweep_loss_sum(const ProbeSweepArgs& w, long n_parts, float scale, float* out, hipStream_t s) {
    hipLaunchKernelGGL(probe_loss_sum_kernel<true>, dim3((unsigned)w.T), dim3(256), 0, s, w.loss_part, n_parts, scale, out, w);
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

void preload_probe_sweep() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&probe_update_kernel<true>));
}

}  // namespace bn
