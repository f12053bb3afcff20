// bn_tsne.hip — exact t-SNE over a 2-D map: k-nearest-neighbour affinities, all-pairs repulsion.
//
//   tsne_perplexity_kernel   BN_TSNE_ROW_LANES lanes per row of scores, float64: the search for beta of scikit-learn's
//                            _binary_search_perplexity, every lane holding up to eight of the row's k <= 128 distances; sums across the lanes
//                            in a fixed tree.  The lanes of a wave leave the search together (a row that has finished keeps its state).
//   tsne_repulsion_kernel    grid (row tiles, column ranges).  A workgroup owns BN_TSNE_TILE_I rows, one per thread, and stages its column
//                            range through LDS in tiles of BN_TSNE_TILE_J points, ascending; every lane reads the same point (a broadcast), so
//                            the loop is float32 vector work only, two columns per step in packed instructions (the tile holds x and y
//                            apart for that): two differences, two fused multiply-adds for 1 + dx^2 + dy^2, v_rcp_f32, a product and three
//                            accumulations per pair; the even and the odd columns of a tile have accumulators of their own, added at the
//                            end.  j = i is left out by index, and only the tiles that overlap the workgroup's own rows carry that
//                            comparison.  Writes (R_i, z_i) of its range.
//   tsne_fold_kernel         the ranges' partial sums per row, in ascending range order
//   tsne_z_kernel            one workgroup: Z, the float64 sum of the float32 row sums z_i in a fixed order; it stays on the device
//   tsne_attraction_kernel   BN_TSNE_ROW_LANES lanes per CSR row of P (empty rows, one entry, hubs of n - 1 entries alike): lane l takes the
//                            entries l, l + 16, ... in order, then the lanes are added in a fixed tree; grad = 4 (E A - R / Z).  On request
//                            the row's part of the Kullback-Leibler divergence, in float64.
//   tsne_update_kernel       scikit-learn's _gradient_descent step, element-wise, every operation rounded on its own
//
// No floating-point atomics anywhere: every sum's order is a function of n and of the matrix's pattern, so the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_device.h"
#include "bn_kernels.h"

namespace bn {
namespace {

constexpr int kTileI = BN_TSNE_TILE_I, kTileJ = BN_TSNE_TILE_J, kSplitJ = BN_TSNE_SPLIT_J, kRowLanes = BN_TSNE_ROW_LANES;
constexpr int kRowsPerWg = 256 / kRowLanes;
constexpr int kPerLane = BN_TSNE_MAX_K / kRowLanes;
static_assert(kTileI == 256, "a repulsion workgroup is 256 threads, one row each");
static_assert(kRowLanes == 16 && kPerLane == 8, "a lane of the perplexity kernel holds eight distances");
static_assert(kSplitJ % kTileJ == 0, "a column range is whole LDS tiles");

inline size_t slab(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline long tsne_splits(long n) { return (n + kSplitJ - 1) / kSplitJ; }

// the sum of v over the 16 lanes of a row, the same bits in every lane (a + b and b + a round alike)
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int mk = kRowLanes / 2; mk >= 1; mk >>= 1) v += __shfl_xor(v, mk);
    return v;
}
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int mk = kRowLanes / 2; mk >= 1; mk >>= 1) v = f_add(v, __shfl_xor(v, mk));
    return v;
}

// ------------------------------------------------------------------------------------------------------------------ perplexity
__global__ __launch_bounds__(256) void tsne_perplexity_kernel(const float* __restrict__ score, long n, int k, double target, float* __restrict__ p,
                                                              double* __restrict__ beta_out) {
    const int tid = threadIdx.x, l = tid & (kRowLanes - 1);
    const long row = (long)blockIdx.x * kRowsPerWg + (tid >> 4);
    const bool ok = row < n;
    double d[kPerLane];
    double m = INFINITY;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int j = l + kRowLanes * r;
        d[r] = 0.0;
        if (ok && j < k) {
            const float d2 = f_sub(2.0f, f_mul(2.0f, score[(size_t)row * k + j]));
            d[r] = d2 > 0.0f ? (double)d2 : 0.0;
            m = fmin(m, d[r]);
        }
    }
#pragma unroll
    for (int mk = kRowLanes / 2; mk >= 1; mk >>= 1) m = fmin(m, __shfl_xor(m, mk));
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) d[r] = ok ? d[r] - m : 0.0;

    double beta = 1.0, lo = -INFINITY, hi = INFINITY, S = 1.0;
    bool done = !ok;
    for (int step = 0; step < BN_TSNE_MAX_PERPLEXITY_STEPS; ++step) {
        if (!__any(!done)) break;   // (wave-uniform: the shuffles below always see all 64 lanes)
        double s = 0.0, t = 0.0;
#pragma unroll
        for (int r = 0; r < kPerLane; ++r)
            if (l + kRowLanes * r < k) {
                const double e = exp(-beta * d[r]);
                s += e;
                t += d[r] * e;
            }
        s = group_sum(s);
        t = group_sum(t);
        if (done) continue;
        S = s;
        const double diff = log(s) + beta * t / s - target;
        if (fabs(diff) <= 1e-5 || step == BN_TSNE_MAX_PERPLEXITY_STEPS - 1) {
            done = true;
        } else if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    if (!ok) return;
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
        const int j = l + kRowLanes * r;
        if (j < k) p[(size_t)row * k + j] = (float)(exp(-beta * d[r]) / S);
    }
    if (l == 0) beta_out[row] = beta;
}

// ------------------------------------------------------------------------------------------------------------------- repulsion
// cnt points of the staged tile (x at tx, y at ty) against the thread's own point, two columns per step: the even columns of the tile feed
// the first halves of rx, ry and z, the odd ones the second halves, and an odd last column the first.  DIAG: the tile may hold the thread's
// own column, first + jj == i
template <bool DIAG>
__device__ __forceinline__ void repulse_tile(const float* tx, const float* ty, int cnt, long first, long i, float xi, float yi, v2f& rx, v2f& ry, v2f& z) {
#pragma clang fp contract(off)
    const v2f one = {1.0f, 1.0f}, xi2 = {xi, xi}, yi2 = {yi, yi};
    const int even = cnt & ~1;
#pragma unroll 4
    for (int jj = 0; jj < even; jj += 2) {
        const v2f qx = *reinterpret_cast<const v2f*>(tx + jj), qy = *reinterpret_cast<const v2f*>(ty + jj);
        const v2f dx = xi2 - qx, dy = yi2 - qy;
        const v2f d2 = __builtin_elementwise_fma(dy, dy, __builtin_elementwise_fma(dx, dx, one));
        v2f w = {__builtin_amdgcn_rcpf(d2.x), __builtin_amdgcn_rcpf(d2.y)};
        if (DIAG) {
            if (first + jj == i) w.x = 0.0f;
            if (first + jj + 1 == i) w.y = 0.0f;
        }
        const v2f w2 = w * w;
        z = z + w;
        rx = __builtin_elementwise_fma(w2, dx, rx);
        ry = __builtin_elementwise_fma(w2, dy, ry);
    }
    if (cnt & 1) {
        const float dx = xi - tx[even], dy = yi - ty[even];
        float w = __builtin_amdgcn_rcpf(fmaf(dy, dy, fmaf(dx, dx, 1.0f)));
        if (DIAG && first + even == i) w = 0.0f;
        const float w2 = w * w;
        z.x = z.x + w;
        rx.x = fmaf(w2, dx, rx.x);
        ry.x = fmaf(w2, dy, ry.x);
    }
}

__global__ __launch_bounds__(256) void tsne_repulsion_kernel(const float2* __restrict__ y, long n, float4* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float tile[2 * kTileJ];   // x of the tile's points, then y
    const int tid = threadIdx.x;
    const long i0 = (long)blockIdx.x * kTileI, i = i0 + tid;
    const long jb = (long)blockIdx.y * kSplitJ, je = jb + kSplitJ < n ? jb + kSplitJ : n;
    const float2 me = y[i < n ? i : n - 1];   // (threads past the end repeat the last row and store nothing)
    v2f rx = {0.0f, 0.0f}, ry = {0.0f, 0.0f}, z = {0.0f, 0.0f};
    for (long j0 = jb; j0 < je; j0 += kTileJ) {
        const int cnt = (int)(je - j0 < kTileJ ? je - j0 : kTileJ);
        if (j0 != jb) __syncthreads();   // every wave has left the previous tile
        for (int e = tid; e < cnt; e += 256) {
            const float2 q = y[j0 + e];
            tile[e] = q.x;
            tile[kTileJ + e] = q.y;
        }
        __syncthreads();
        if (j0 < i0 + kTileI && i0 < j0 + cnt)
            repulse_tile<true>(tile, tile + kTileJ, cnt, j0, i, me.x, me.y, rx, ry, z);
        else
            repulse_tile<false>(tile, tile + kTileJ, cnt, j0, i, me.x, me.y, rx, ry, z);
    }
    if (i < n) part[(size_t)blockIdx.y * n + i] = make_float4(f_add(rx.x, rx.y), f_add(ry.x, ry.y), f_add(z.x, z.y), 0.0f);
}

__global__ __launch_bounds__(256) void tsne_fold_kernel(const float4* __restrict__ part, long n, int splits, float2* __restrict__ rep, float* __restrict__ zrow) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 acc = part[i];
    for (int s = 1; s < splits; ++s) {
        const float4 v = part[(size_t)s * n + i];
        acc.x = f_add(acc.x, v.x);
        acc.y = f_add(acc.y, v.y);
        acc.z = f_add(acc.z, v.z);
    }
    rep[i] = make_float2(acc.x, acc.y);
    zrow[i] = acc.z;
}

// One workgroup of 1024 threads: thread t adds z_t, z_(t + 1024), ... in order, then a tree over the threads
__global__ __launch_bounds__(1024) void tsne_z_kernel(const float* __restrict__ zrow, long n, double* __restrict__ z) {
    __shared__ double acc[1024];
    const int t = threadIdx.x;
    double a = 0.0;
    for (long i = t; i < n; i += 1024) a += (double)zrow[i];
    acc[t] = a;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if (t < h) acc[t] += acc[t + h];
        __syncthreads();
    }
    if (t == 0) *z = acc[0];
}

// ------------------------------------------------------------------------------------------------------------------ attraction
template <bool KL>
__global__ __launch_bounds__(256) void tsne_attraction_kernel(const float2* __restrict__ y, long n, const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                              const float* __restrict__ val, float E, const float2* __restrict__ rep, const double* __restrict__ z,
                                                              float2* __restrict__ grad, double* __restrict__ kl_rows) {
    const int tid = threadIdx.x, l = tid & (kRowLanes - 1);
    const long row = (long)blockIdx.x * kRowsPerWg + (tid >> 4);
    const bool ok = row < n;
    const long long nnz = rowptr[n];
    long long b = 0, e = 0;
    float2 me = make_float2(0.0f, 0.0f);
    if (ok) {   // a table that lies about its rows gives wrong numbers, never a read outside the nnz entries
        b = rowptr[row];
        e = rowptr[row + 1];
        b = b < 0 ? 0 : (b > nnz ? nnz : b);
        e = e < b ? b : (e > nnz ? nnz : e);
        me = y[row];
    }
    float ax = 0.0f, ay = 0.0f;
    double kl = 0.0;
    for (long long t = b + l; t < e; t += kRowLanes) {
        int j = col[t];
        j = j < 0 ? 0 : ((long)j >= n ? (int)(n - 1) : j);
        const float pij = val[t];
        const float2 q = y[j];
        const float dx = me.x - q.x, dy = me.y - q.y;
        const float d2 = fmaf(dy, dy, fmaf(dx, dx, 1.0f));
        const float pw = f_mul(pij, __builtin_amdgcn_rcpf(d2));
        ax = fmaf(pw, dx, ax);
        ay = fmaf(pw, dy, ay);
        if constexpr (KL) {
            if (pij > 0.0f) {
                const double ex = (double)me.x - (double)q.x, ey = (double)me.y - (double)q.y;
                kl += (double)pij * log((double)pij * fma(ey, ey, fma(ex, ex, 1.0)));
            }
        }
    }
    ax = group_sum(ax);
    ay = group_sum(ay);
    if constexpr (KL) kl = group_sum(kl);
    if (!ok || l != 0) return;
    const float2 r = rep[row];
    const double Z = *z;
    const float gx = f_sub(f_mul(E, ax), (float)((double)r.x / Z)), gy = f_sub(f_mul(E, ay), (float)((double)r.y / Z));
    grad[row] = make_float2(f_mul(4.0f, gx), f_mul(4.0f, gy));
    if constexpr (KL) kl_rows[row] = kl;
}

// ---------------------------------------------------------------------------------------------------------------------- update
__global__ __launch_bounds__(256) void tsne_update_kernel(float* __restrict__ y, const float* __restrict__ grad, float* __restrict__ update,
                                                          float* __restrict__ gains, long elems, float lr, float momentum) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= elems) return;
    const float g = grad[i], u = update[i];
    float gain = gains[i];
    gain = f_mul(u, g) < 0.0f ? f_add(gain, 0.2f) : f_mul(gain, 0.8f);
    gain = gain < 0.01f ? 0.01f : gain;
    const float nu = f_sub(f_mul(momentum, u), f_mul(lr, f_mul(gain, g)));
    gains[i] = gain;
    update[i] = nu;
    y[i] = f_add(y[i], nu);
}

}  // namespace

void launch_tsne_perplexity(const float* score, long n, int k, double perplexity, float* p, double* beta, hipStream_t s) {
    hipLaunchKernelGGL(tsne_perplexity_kernel, dim3((unsigned)((n + kRowsPerWg - 1) / kRowsPerWg)), dim3(256), 0, s, score, n, k, log(perplexity), p, beta);
}

// [partial sums of the column ranges, float4 per row | R, float2 per row | z, float per row]
size_t tsne_gradient_workspace(long n) { return slab((size_t)tsne_splits(n) * n * sizeof(float4)) + slab((size_t)n * sizeof(float2)) + slab((size_t)n * sizeof(float)); }

void launch_tsne_gradient(const float* y, long n, const long long* rowptr, const int* col, const float* val, float exaggeration, float* grad, double* z,
                          double* kl_rows, void* d_work, hipStream_t s) {
    const long splits = tsne_splits(n);
    char* w = (char*)d_work;
    float4* part = (float4*)w;
    float2* rep = (float2*)(w + slab((size_t)splits * n * sizeof(float4)));
    float* zrow = (float*)((char*)rep + slab((size_t)n * sizeof(float2)));
    const float2* y2 = (const float2*)y;
    hipLaunchKernelGGL(tsne_repulsion_kernel, dim3((unsigned)((n + kTileI - 1) / kTileI), (unsigned)splits), dim3(256), 0, s, y2, n, part);
    hipLaunchKernelGGL(tsne_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, n, (int)splits, rep, zrow);
    hipLaunchKernelGGL(tsne_z_kernel, dim3(1), dim3(1024), 0, s, zrow, n, z);
    const dim3 grid((unsigned)((n + kRowsPerWg - 1) / kRowsPerWg));
    if (kl_rows)
        hipLaunchKernelGGL(tsne_attraction_kernel<true>, grid, dim3(256), 0, s, y2, n, rowptr, col, val, exaggeration, rep, z, (float2*)grad, kl_rows);
    else
        hipLaunchKernelGGL(tsne_attraction_kernel<false>, grid, dim3(256), 0, s, y2, n, rowptr, col, val, exaggeration, rep, z, (float2*)grad, kl_rows);
}

void launch_tsne_update(float* y, const float* grad, float* update, float* gains, long n, float lr, float momentum, hipStream_t s) {
    hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, s, y, grad, update, gains, 2 * n, lr, momentum);
}

void preload_tsne() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&tsne_update_kernel));
}

}  // namespace bn
