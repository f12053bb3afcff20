// bn_augment.hip — an epoch's augmented model inputs from the resident un-augmented ones (bn_augment_inputs).
//
//   augment_kernel : out[r] = sum over the 1..3 sources of row r of gain * masked(x[source]), SpecAugment masks belonging to the SOURCE
//                    row (reference: audio/augmentation.py:10-71 `apply_mixup` after data/generator.py:169-170 masked every sample).
//
// birdnet_stm32/training/augment.py `augment_reference` is the specification and the results are compared with it for equality, so every
// product and sum whose rounding is part of it goes through the f_add / f_mul helpers of bn_device.h
// (a fused multiply-add rounds once where numpy rounds twice).  A row with one source is copied, not multiplied: -0.0 and
// NaN payloads survive.  Gains go down to 1e-27, products are routinely subnormal; the file is compiled in hipcc's default float32 mode,
// which keeps them.
//
// Alignment.  A row is E = F * W floats and starts wherever r * E puts it: 16-byte aligned for the spectrogram shapes, 8 on the odd rows
// of the raw frontend (66 150 floats), 4 in general — and the output row and each of its sources can differ.  The decision: the OUTPUT
// row sets the grid of 16-byte groups (a scalar head of 0..3 elements up to its first 16-byte boundary, aligned 16-byte stores, a scalar
// tail of 0..3), and the sources are read at the same element offsets through a 16-byte type declared 4-byte aligned, which the compiler
// lowers to the widest load the target allows for that alignment.  One code path, no per-source case split.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_device.h"
#include "bn_kernels.h"

#pragma clang fp contract(off)

namespace bn {
namespace {

constexpr int kAugThreads = 256, kAugUnroll = 4;
constexpr int kAugChunk = kAugThreads * kAugUnroll * 4;   // elements of a row per workgroup

struct __attribute__((packed, aligned(4))) F4U { float v[4]; };   // four floats at any 4-byte boundary

struct AugMasks {            // the (start, width) tables of a row's sources; width >= 0
    int f[3][BN_AUGMENT_MAX_MASKS][2];
    int t[3][BN_AUGMENT_MAX_MASKS][2];
};

// p in [start, start + width), in unsigned arithmetic: no overflow whatever the table holds, and a mask past the edge simply matches nothing there
__device__ __forceinline__ bool in_any(const int (*tab)[2], int n, int p) {
    bool hit = false;
    for (int k = 0; k < n; ++k) hit |= (unsigned)p - (unsigned)tab[k][0] < (unsigned)tab[k][1];
    return hit;
}

template <int NS>
__device__ __forceinline__ float mix(const float* v, const float* g) {
    if (NS == 1) return v[0];
    // numpy's reduction starts from +0.0: 0 + p is p except for p = -0.0, so products that are all -0.0 sum to +0.0 as they do there
    float r = f_add(f_add(0.0f, f_mul(g[0], v[0])), f_mul(g[1], v[1]));
    if (NS == 3) r = f_add(r, f_mul(g[2], v[2]));
    return r;
}

template <int NS>
__device__ __forceinline__ void aug_row(const float* const* xs, const float* g, const AugMasks& mk, int nf, int nt, int W, int E, int head, int n4,
                                        float* __restrict__ o) {
    const int tid = threadIdx.x;
    // the scalar head and tail: at most six elements, by the first threads of the row's first workgroup
    if (blockIdx.y == 0) {
        const int tail = E - head - 4 * n4;
        if (tid < head + tail) {
            const int i = tid < head ? tid : head + 4 * n4 + (tid - head);
            const int f = i / W, t = i - f * W;
            float v[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) v[s] = (in_any(mk.f[s], nf, f) || in_any(mk.t[s], nt, t)) ? 0.0f : xs[s][i];
            o[i] = mix<NS>(v, g);
        }
    }
    const int g0 = blockIdx.y * (kAugThreads * kAugUnroll) + tid;
    F4U val[kAugUnroll][NS];
    unsigned masked[kAugUnroll][NS];   // bit e: element e of the group is masked in source s
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        const int grp = g0 + u * kAugThreads;
        if (grp >= n4) continue;
        const int i = head + 4 * grp;
        int f = i / W, t = i - f * W;
#pragma unroll
        for (int s = 0; s < NS; ++s) masked[u][s] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int s = 0; s < NS; ++s) masked[u][s] |= (unsigned)(in_any(mk.f[s], nf, f) || in_any(mk.t[s], nt, t)) << e;
            if (++t == W) { t = 0; ++f; }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (masked[u][s] != 15u) val[u][s] = *reinterpret_cast<const F4U*>(xs[s] + i);   // a fully masked group is not read
            else val[u][s] = F4U{{0.0f, 0.0f, 0.0f, 0.0f}};
        }
    }
#pragma unroll
    for (int u = 0; u < kAugUnroll; ++u) {
        const int grp = g0 + u * kAugThreads;
        if (grp >= n4) continue;
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) v[s] = (masked[u][s] >> e & 1u) ? 0.0f : val[u][s].v[e];
            r[e] = mix<NS>(v, g);
        }
        f32x4 q = {r[0], r[1], r[2], r[3]};
        *reinterpret_cast<f32x4*>(o + head + 4 * grp) = q;
        asm volatile("s_nop 1" : "+v"(q));   // the data registers of a 16-byte store are not rewritten right behind it (bn_f32_strip.hip: store16)
    }
}

// grid (m, ceil(E / kAugChunk)): workgroup (r, c) writes 16-byte groups c * 1024 .. of output row r; c == 0 also its scalar head and tail
__global__ __launch_bounds__(kAugThreads) void augment_kernel(const float* __restrict__ x, long n_rows, int W, int E, const int* __restrict__ nsrc,
                                                              const int* __restrict__ src, const float* __restrict__ gain,
                                                              const int* __restrict__ fmask, int nf, const int* __restrict__ tmask, int nt,
                                                              float* __restrict__ out) {
    __shared__ AugMasks mk;
    const size_t r = blockIdx.x;
    int ns = nsrc[r];
    ns = ns < 1 ? 1 : (ns > 3 ? 3 : ns);   // a bad plan must not turn into a stray read: counts and indices are clamped
    long si[3];
    const float* xs[3];
    float g[3];
    for (int s = 0; s < 3; ++s) {
        long j = s < ns ? src[3 * r + s] : 0;
        si[s] = j < 0 ? 0 : (j >= n_rows ? n_rows - 1 : j);
        xs[s] = x + (size_t)si[s] * E;
        g[s] = gain[3 * r + s];
    }
    const int tid = threadIdx.x;
    if (tid < 3 * (nf + nt)) {
        const int s = tid / (nf + nt), k = tid - s * (nf + nt);
        const int* e = k < nf ? fmask + ((size_t)si[s] * nf + k) * 2 : tmask + ((size_t)si[s] * nt + (k - nf)) * 2;
        int* d = k < nf ? mk.f[s][k] : mk.t[s][k - nf];
        d[0] = e[0];
        d[1] = e[1] < 0 ? 0 : e[1];
    }
    __syncthreads();
    float* o = out + r * (size_t)E;
    int head = (int)(((16 - ((uintptr_t)o & 15)) & 15) >> 2);
    if (head > E) head = E;
    const int n4 = (E - head) >> 2;
    if (ns == 1) aug_row<1>(xs, g, mk, nf, nt, W, E, head, n4, o);
    else if (ns == 2) aug_row<2>(xs, g, mk, nf, nt, W, E, head, n4, o);
    else aug_row<3>(xs, g, mk, nf, nt, W, E, head, n4, o);
}

}  // namespace

void launch_augment(const float* x, long n_rows, int W, int E, const int* nsrc, const int* src, const float* gain, const int* fmask, int nf,
                    const int* tmask, int nt, long m, float* out, hipStream_t s) {
    const unsigned chunks = (unsigned)((E + kAugChunk - 1) / kAugChunk);
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)m, chunks), dim3(kAugThreads), 0, s, x, n_rows, W, E, nsrc, src, gain, fmask, nf, tmask, nt, out);
}

void preload_augment() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&augment_kernel));
}

}  // namespace bn
