// bn_propagate.hip — graph label spreading over a fixed CSR matrix S: F_next = alpha S F + (1 - alpha) Y.
//
//   propagate_step_kernel    lanes own classes, rows are dealt to groups of G lanes (G a power of two, 1..64: the smallest that covers the
//                            row's classes, so a wave holds 64 / G rows when C is small; a lane loops when C exceeds its group).  A lane walks
//                            the row's entries in ascending order and accumulates its classes on its own: acc = fl(acc + fl(S_ij F[j, c])),
//                            every operation rounded, so the order of evaluation/propagate.py holds by construction: no sum across lanes, no
//                            atomics.  col / val of an entry are the same address in every lane of the group (one broadcast fetch);
//                            F[j, c ..] is contiguous across the group.  VEC = 4: a lane owns four neighbouring classes and reads them in one
//                            16-byte load (C % 4 == 0 and both F arrays 16-byte aligned); VEC = 1 otherwise.  Four entries are fetched ahead
//                            of the additions that consume them.  Row bounds are clipped to 0 .. rowptr[n]; an entry whose column lies outside
//                            0 .. n - 1 is read from row 0 and contributes nothing.  On request the row's float64 sum of |F_next - F| (each
//                            lane over its classes in ascending order, then the group's lanes in a fixed tree).
//   propagate_delta_kernel   one workgroup: the float64 sum of the rows' parts in a fixed order; it stays on the device
//   propagate_decide_kernel  per row the first largest class (float32 comparison), its share of the row's float32 sum, -1 / 0 for a sum of 0
//
// No floating-point atomics anywhere: the same inputs give the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_device.h"
#include "bn_kernels.h"

namespace bn {
namespace {

constexpr int kAhead = 4;   // entries of a row fetched before their additions

template <int VEC>
struct Pack;
template <>
struct Pack<1> {
    typedef float type;
};
template <>
struct Pack<4> {
    typedef f32x4 type;
};

template <int VEC>
__device__ __forceinline__ float lane_elem(const typename Pack<VEC>::type& v, int e) {
    if constexpr (VEC == 1)
        return v;
    else
        return v[e];
}

// the sum of v over the g lanes of a group (a power of two), the same bits in every lane (a + b and b + a round alike)
__device__ __forceinline__ double group_sum(double v, int g) {
    for (int mk = g >> 1; mk >= 1; mk >>= 1) v += __shfl_xor(v, mk);
    return v;
}

template <int VEC, bool DELTA>
__global__ __launch_bounds__(256) void propagate_step_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
                                                             const float* __restrict__ f, const int* __restrict__ seed_label, long n, int C, int g_shift,
                                                             float alpha, float* __restrict__ f_next, double* __restrict__ delta_rows) {
    typedef typename Pack<VEC>::type pack_t;
    const int G = 1 << g_shift, tid = threadIdx.x, l = tid & (G - 1);
    const long row = (long)blockIdx.x * (256 >> g_shift) + (tid >> g_shift);
    const bool ok = row < n;
    const long long nnz = rowptr[n];
    long long b = 0, e = 0;
    int seed = -1;
    if (ok) {   // a table that lies about its rows gives wrong numbers, never a read outside the nnz entries
        b = rowptr[row];
        e = rowptr[row + 1];
        b = b < 0 ? 0 : (b > nnz ? nnz : b);
        e = e < b ? b : (e > nnz ? nnz : e);
        seed = seed_label[row];
    }
    const float keep = f_sub(1.0f, alpha);
    const int units = C / VEC;   // (VEC = 4 only with C % 4 == 0)
    double delta = 0.0;
    for (int u = l; u < units; u += G) {
        const size_t c0 = (size_t)u * VEC;
        pack_t acc = {};
        long long t = b;
        for (; t + kAhead <= e; t += kAhead) {
            int j[kAhead];
            float v[kAhead];
            pack_t q[kAhead];
            bool in[kAhead];
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                j[a] = col[t + a];
                v[a] = val[t + a];
                in[a] = j[a] >= 0 && (long)j[a] < n;
            }
#pragma unroll
            for (int a = 0; a < kAhead; ++a) q[a] = *reinterpret_cast<const pack_t*>(f + (size_t)(in[a] ? j[a] : 0) * C + c0);
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                if constexpr (VEC == 1) {
                    acc = in[a] ? f_add(acc, f_mul(v[a], q[a])) : acc;
                } else {
#pragma unroll
                    for (int x = 0; x < VEC; ++x) acc[x] = in[a] ? f_add(acc[x], f_mul(v[a], q[a][x])) : acc[x];
                }
            }
        }
        for (; t < e; ++t) {
            const int j = col[t];
            const float v = val[t];
            const bool in = j >= 0 && (long)j < n;
            const pack_t q = *reinterpret_cast<const pack_t*>(f + (size_t)(in ? j : 0) * C + c0);
            if constexpr (VEC == 1) {
                acc = in ? f_add(acc, f_mul(v, q)) : acc;
            } else {
#pragma unroll
                for (int x = 0; x < VEC; ++x) acc[x] = in ? f_add(acc[x], f_mul(v, q[x])) : acc[x];
            }
        }
        if (!ok) continue;
        const size_t at = (size_t)row * C + c0;
        pack_t out;
        if constexpr (VEC == 1) {
            out = f_add(f_mul(alpha, acc), (int)c0 == seed ? keep : 0.0f);
        } else {
#pragma unroll
            for (int x = 0; x < VEC; ++x) out[x] = f_add(f_mul(alpha, acc[x]), (int)c0 + x == seed ? keep : 0.0f);
        }
        if constexpr (DELTA) {
            const pack_t old = *reinterpret_cast<const pack_t*>(f + at);
#pragma unroll
            for (int x = 0; x < VEC; ++x) delta += fabs((double)lane_elem<VEC>(out, x) - (double)lane_elem<VEC>(old, x));
        }
        *reinterpret_cast<pack_t*>(f_next + at) = out;
    }
    if constexpr (DELTA) {   // (every lane of the wave arrives here: the shuffles see all 64)
        delta = group_sum(delta, G);
        if (ok && l == 0) delta_rows[row] = delta;
    }
}

// One workgroup of 1024 threads: thread t adds the parts t, t + 1024, ... in order, then a tree over the threads
__global__ __launch_bounds__(1024) void propagate_delta_kernel(const double* __restrict__ delta_rows, long n, double* __restrict__ delta) {
    __shared__ double acc[1024];
    const int t = threadIdx.x;
    double a = 0.0;
    for (long i = t; i < n; i += 1024) a += delta_rows[i];
    acc[t] = a;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if (t < h) acc[t] += acc[t + h];
        __syncthreads();
    }
    if (t == 0) *delta = acc[0];
}

__global__ __launch_bounds__(256) void propagate_decide_kernel(const float* __restrict__ f, long n, int C, int g_shift, int* __restrict__ label,
                                                               float* __restrict__ score) {
    const int G = 1 << g_shift, tid = threadIdx.x, l = tid & (G - 1);
    const long row = (long)blockIdx.x * (256 >> g_shift) + (tid >> g_shift);
    const bool ok = row < n;
    float best = -INFINITY, sum = 0.0f;
    int arg = 0x7fffffff;
    if (ok)
        for (int c = l; c < C; c += G) {
            const float v = f[(size_t)row * C + c];
            sum = f_add(sum, v);
            if (v > best) {   // (ascending c: the first of equal values stays)
                best = v;
                arg = c;
            }
        }
    for (int mk = G >> 1; mk >= 1; mk >>= 1) {
        const float ob = __shfl_xor(best, mk), os = __shfl_xor(sum, mk);
        const int oa = __shfl_xor(arg, mk);
        sum = f_add(sum, os);
        if (ob > best || (ob == best && oa < arg)) {
            best = ob;
            arg = oa;
        }
    }
    if (!ok || l != 0) return;
    const bool none = sum == 0.0f || arg >= C;
    label[row] = none ? -1 : arg;
    score[row] = none ? 0.0f : f_div(best, sum);
}

// the lanes of a row: the smallest power of two that covers `units`, 64 at the most
inline int group_shift(int units) {
    int s = 0;
    while (s < 6 && (1 << s) < units) ++s;
    return s;
}

}  // namespace

size_t propagate_workspace(long n) { return (size_t)n * sizeof(double); }

void launch_propagate_step(const long long* rowptr, const int* col, const float* val, const float* f, const int* seed_label, long n, int C, float alpha,
                           float* f_next, double* delta, void* d_work, hipStream_t s) {
    const bool wide = C % 4 == 0 && (uintptr_t)f % 16 == 0 && (uintptr_t)f_next % 16 == 0;
    const int gs = group_shift(wide ? C / 4 : C);
    const dim3 grid((unsigned)((n + (256 >> gs) - 1) / (256 >> gs)));
    double* rows = (double*)d_work;
    if (wide && delta)
        hipLaunchKernelGGL((propagate_step_kernel<4, true>), grid, dim3(256), 0, s, rowptr, col, val, f, seed_label, n, C, gs, alpha, f_next, rows);
    else if (wide)
        hipLaunchKernelGGL((propagate_step_kernel<4, false>), grid, dim3(256), 0, s, rowptr, col, val, f, seed_label, n, C, gs, alpha, f_next, rows);
    else if (delta)
        hipLaunchKernelGGL((propagate_step_kernel<1, true>), grid, dim3(256), 0, s, rowptr, col, val, f, seed_label, n, C, gs, alpha, f_next, rows);
    else
        hipLaunchKernelGGL((propagate_step_kernel<1, false>), grid, dim3(256), 0, s, rowptr, col, val, f, seed_label, n, C, gs, alpha, f_next, rows);
    if (delta) hipLaunchKernelGGL(propagate_delta_kernel, dim3(1), dim3(1024), 0, s, rows, n, delta);
}

void launch_propagate_decide(const float* f, long n, int C, int* label, float* score, hipStream_t s) {
    const int gs = group_shift(C);
    hipLaunchKernelGGL(propagate_decide_kernel, dim3((unsigned)((n + (256 >> gs) - 1) / (256 >> gs))), dim3(256), 0, s, f, n, C, gs, label, score);
}

void preload_propagate() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&propagate_decide_kernel));
}

}  // namespace bn
