// bn_activity.hip — the two per-sample reductions behind chunk selection (reference: birdnet_stm32/audio/activity.py).
//
//   ste_kernel             : short-time energy of resampled windows, mean((y / peak)[512 f : 512 f + 1024]^2) per frame
//                            (reference :12-30 `_short_time_energy` as smart_crop :75-77 calls it)
//   activity_count_kernel  : per feature row, median and MAD of 512 evenly spaced |x|, threshold median + k * MAD, and the number of
//                            elements above it (reference :188-209 `get_activity_ratio` up to its count)
//
// Both repeat a float32 operation order that birdnet_stm32/audio/activity.py spells out (short_time_energy, activity_stats), so their
// results are compared with that module for equality.  Every addition and multiplication whose rounding is part of that order is written
// with the f_add / f_mul / f_sub / f_div helpers of bn_device.h (a fused multiply-add rounds once where numpy rounds twice).
// Percentiles, regions, ratios and every ordering decision stay on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn_device.h"
#include "bn_kernels.h"

#pragma clang fp contract(off)

namespace bn {
namespace {

// ------------------------------------------------------------------------------------------------------------ short-time energy
// numpy sums a contiguous float32 run of 1024 as a binary tree over eight blocks of 128; a block is eight strided accumulators (sixteen
// sequential additions each) folded as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)).  Frames hop by 512 = four blocks, so frame f is the tree over
// block sums 4f .. 4f+7 of the window and every block sum serves two frames: a workgroup squares kSteFrames*4+4 blocks into LDS once,
// eight lanes fold each block (lane = accumulator; the three pair steps are lane-xor 1, 2, 4 — addition commutes, so both lanes of a pair
// hold the same bits), then one thread per frame runs the three tree levels over eight block sums.
constexpr int kSteFrameLen = 1024, kSteHop = 512, kSteBlock = 128;
constexpr int kSteFrames = 16;                                   // frames per workgroup pass
constexpr int kSteBlocks = kSteFrames * (kSteHop / kSteBlock) + (kSteFrameLen - kSteHop) / kSteBlock;   // 68 blocks = 8704 samples
constexpr int kSteRow = kSteBlock + 8;                           // LDS row pitch: the eight blocks a wave folds start eight banks apart
constexpr int kSteTilesX = 32;                                   // grid.x: a window's passes are strided over this many workgroups

__global__ __launch_bounds__(256) void ste_kernel(const float* __restrict__ mono, const float* __restrict__ peak, const long* __restrict__ win_off,
                                                  const int* __restrict__ win_index, const long* __restrict__ frame_off, float* __restrict__ ste) {
    __shared__ float sq[kSteBlocks * kSteRow];
    __shared__ float bsum[kSteBlocks];
    const int w = blockIdx.y, tid = threadIdx.x;
    const long base = win_off[w], len = win_off[w + 1] - base;
    const long f_base = frame_off[w];
    long nf = len >= kSteFrameLen ? 1 + (len - kSteFrameLen) / kSteHop : 0;   // full frames only: every read stays inside the window,
    const long room = frame_off[w + 1] - f_base;                               // every write inside the window's slice of ste
    if (room < nf) nf = room;
    const float p = peak[win_index[w]];
    for (long f0 = (long)blockIdx.x * kSteFrames; f0 < nf; f0 += (long)kSteTilesX * kSteFrames) {   // (uniform per workgroup)
        const int nfr = nf - f0 < kSteFrames ? (int)(nf - f0) : kSteFrames;
        const int nblk = nfr * 4 + 4, ns = nblk * kSteBlock;
        const float* src = mono + base + f0 * kSteHop;
        for (int s = tid; s < ns; s += 256) {
            float v = src[s];
            if (p > 0.0f) v = f_div(v, p);   // the expression of ingest_chunks_kernel
            sq[(s >> 7) * kSteRow + (s & 127)] = f_mul(v, v);
        }
        __syncthreads();
        const int acc = tid & 7;
        for (int b0 = 0; b0 < nblk; b0 += 32) {   // 32 blocks per pass of 256 lanes; lanes past nblk fold block 0 again and drop the result
            const int b = b0 + (tid >> 3);
            const float* row = sq + (b < nblk ? b : 0) * kSteRow + acc;
            float r = row[0];
#pragma unroll
            for (int i = 1; i < kSteBlock / 8; ++i) r = f_add(r, row[i * 8]);
            r = f_add(r, __shfl_xor(r, 1));
            r = f_add(r, __shfl_xor(r, 2));
            r = f_add(r, __shfl_xor(r, 4));
            if (acc == 0 && b < nblk) bsum[b] = r;
        }
        __syncthreads();
        if (tid < nfr) {
            const float* q = bsum + tid * 4;
            const float t = f_add(f_add(f_add(q[0], q[1]), f_add(q[2], q[3])), f_add(f_add(q[4], q[5]), f_add(q[6], q[7])));
            ste[f_base + f0 + tid] = f_div(t, (float)kSteFrameLen);
        }
        __syncthreads();   // (the next pass overwrites sq and bsum)
    }
}

// ------------------------------------------------------------------------------------------------------------ activity counts
constexpr int kActMaxM = 512;

// Non-negative finite floats order as their bit patterns.  Rank of element i among m = how many are smaller, ties broken by position:
// ranks are a permutation, so exactly one thread finds each of the two middle ranks and stores its value.  512 x 512 comparisons against
// LDS broadcasts (four values per read) cost less than the 45 barriers of a bitonic network, and odd m needs no padding.
__device__ __forceinline__ void middle_two(const unsigned* vals, int m, int tid, unsigned* mid) {
    const int lo = (m - 1) >> 1, hi = m >> 1;
    const int m4 = m & ~3;
    for (int i = tid; i < m; i += 256) {
        const unsigned v = vals[i];
        int rank = 0;
        for (int j = 0; j < m4; j += 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(vals + j);
            rank += (q.x < v || (q.x == v && j < i)) + (q.y < v || (q.y == v && j + 1 < i)) + (q.z < v || (q.z == v && j + 2 < i)) +
                    (q.w < v || (q.w == v && j + 3 < i));
        }
        for (int j = m4; j < m; ++j) rank += (vals[j] < v || (vals[j] == v && j < i));
        if (rank == lo) mid[0] = v;
        if (rank == hi) mid[1] = v;
    }
}

__device__ __forceinline__ float median_of(const unsigned* mid, int m) {
    const float a = __uint_as_float(mid[0]), b = __uint_as_float(mid[1]);
    return (m & 1) ? a : f_div(f_add(a, b), 2.0f);   // np.median: the mean of the two middle values, in float32
}

__device__ __forceinline__ int above(float v, float thresh) { return __builtin_fabsf(v) > thresh ? 1 : 0; }

// One workgroup per row.  Rows start wherever b * n puts them (66 150 floats: 8-byte aligned on odd rows), so the stream is a scalar head
// up to the first 16-byte boundary, 16-byte loads (four in flight per thread), and a scalar tail.
__global__ __launch_bounds__(256) void activity_count_kernel(const float* __restrict__ x, long n, const int* __restrict__ idx, int m, float k,
                                                             int* __restrict__ active, float* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) unsigned vals[kActMaxM];
    __shared__ unsigned mid[2];
    __shared__ int wave_count[4];
    const int tid = threadIdx.x;
    const float* row = x + (size_t)blockIdx.x * n;
    for (int i = tid; i < m; i += 256) {
        long j = idx[i];
        j = j < 0 ? 0 : (j >= n ? n - 1 : j);   // a bad index table must not read outside the row
        vals[i] = __float_as_uint(row[j]) & 0x7fffffffu;
    }
    __syncthreads();
    middle_two(vals, m, tid, mid);
    __syncthreads();
    const float med = median_of(mid, m);
    __syncthreads();   // (everyone has read mid before the second selection writes it)
    for (int i = tid; i < m; i += 256) vals[i] = __float_as_uint(f_sub(__uint_as_float(vals[i]), med)) & 0x7fffffffu;
    __syncthreads();
    middle_two(vals, m, tid, mid);
    __syncthreads();
    const float mad = f_add(median_of(mid, m), 1e-10f);
    const float thresh = f_add(med, f_mul(k, mad));

    int cnt = 0;
    long head = (long)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (tid < head) cnt += above(row[tid], thresh);
    const long n4 = (n - head) >> 2;
    const float4* body = reinterpret_cast<const float4*>(row + head);
    for (long i0 = tid; i0 < n4; i0 += 4 * 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i0 + 256 * u < n4 ? body[i0 + 256 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 256 * u < n4) cnt += above(v[u].x, thresh) + above(v[u].y, thresh) + above(v[u].z, thresh) + above(v[u].w, thresh);
    }
    for (long i = head + 4 * n4 + tid; i < n; i += 256) cnt += above(row[i], thresh);

#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) wave_count[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        active[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        if (stats) {
            stats[3 * (size_t)blockIdx.x + 0] = med;
            stats[3 * (size_t)blockIdx.x + 1] = mad;
            stats[3 * (size_t)blockIdx.x + 2] = thresh;
        }
    }
}

}  // namespace

void launch_short_time_energy(const float* mono, const float* peak, const long* win_off, const int* win_index, const long* frame_off, int n_windows,
                              float* ste, hipStream_t s) {
    hipLaunchKernelGGL(ste_kernel, dim3(kSteTilesX, (unsigned)n_windows), dim3(256), 0, s, mono, peak, win_off, win_index, frame_off, ste);
}

void launch_activity_counts(const float* x, int B, long n, const int* idx, int m, float k, int* active, float* stats, hipStream_t s) {
    hipLaunchKernelGGL(activity_count_kernel, dim3((unsigned)B), dim3(256), 0, s, x, n, idx, m, k, active, stats);
}

void preload_activity() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&ste_kernel));
}

}  // namespace bn
