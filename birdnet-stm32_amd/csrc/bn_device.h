// bn_device.h — the device primitives every kernel file builds on, defined once: vector types, individually rounded float32
// operations, the two light barriers and the float32 activation.  (The INT8 requantisation forms are in bn_requant.h.)
#pragma once
#include <hip/hip_runtime.h>

namespace bn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

// Individually rounded float32 operations: a fused multiply-add rounds once where numpy rounds twice.  The pragma sits in each body, so
// they never fuse whatever the including file sets.  (The __fmul_rn / __fadd_rn intrinsics do not prevent it: they are inline functions
// of a header compiled with contraction allowed, and after inlining the backend fuses their multiply and add; median + k * mad came out
// one ulp low.)
__device__ __forceinline__ float f_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float f_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float f_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float f_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

// The workgroup's barrier for LDS traffic only: it waits for the wave's own LDS operations, global loads and stores stay in flight across
// it.  (__syncthreads() is a workgroup-scope fence as well: it puts `s_waitcnt vmcnt(0)` in front of the barrier, and a wave that has just
// stored arrives late by a store round trip — in f32_pw_ws_kernel the matrix waves waited 5.5 us per tile for the epilogue waves.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// A wave's LDS writes visible to its own lanes.  LDS instructions of a wave execute in issue order, the compiler only has to keep that
// order: no instruction waits, and nothing is ordered between waves (that takes a workgroup barrier).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// float32 activation of an operator record: 0 none, 1 ReLU, 2 ReLU6
__device__ __forceinline__ float act_f(float v, int act) {
    if (act == 1) return fmaxf(v, 0.0f);
    if (act == 2) return fminf(fmaxf(v, 0.0f), 6.0f);
    return v;
}

}  // namespace bn
