// bn_kmeans.hip — spherical k-means over a matrix of embeddings: one Lloyd iteration is an assignment and an update.
//
//   kmeans_assign_kernel     grid (row ranges).  The centroids sit in LDS as the B operand of the matrix cores, a tile of 16 * NT at a
//                            time (NT <= 8; the tile follows from D and BN_KMEANS_LDS_BYTES, kmeans_geometry).  A workgroup streams its
//                            range of rows once per tile, straight into the A operand (bn_rowstream.h owns the row layout, the padding
//                            beyond D and the prefetch depth; v_mfma_f32_16x16x4_f32: exact float32 products; int8 bytes become
//                            float32(byte - zero_point) on the way, which is exact, and read as the zero point beyond D).  Per row it keeps the best (score, centroid) under the total order — score descending,
//                            centroid index ascending — which is one value however the centroids are tiled: no list, no merge.  With
//                            several tiles the best so far is carried in the row's own label / score slot, which only the lane that
//                            wrote it reads again.  Rows whose label differs from the previous one are counted with integer adds.
//   kmeans_keys_kernel       label -> sort key (rows without a cluster go behind the last one), row numbers 0 .. n-1
//   (rocPRIM radix sort)     stable, ascending by key: the members of a cluster in ascending row order
//   kmeans_offsets_kernel    first sorted position of every cluster (binary search)
//   kmeans_segments_kernel   member counts, and an exclusive scan of the segments (of at most BN_KMEANS_SEGMENT_ROWS members) per cluster
//   kmeans_partial_kernel    one workgroup per (cluster, segment): lanes across D, members one after the other in ascending row order
//   kmeans_fold_kernel       one workgroup per cluster: its segments' partial sums in segment order, onto the old sums with `accumulate`
//   kmeans_scale_kernel      centroid = sum * inverse norm of the sum for clusters with members (the norms are search_inv_norms_kernel's)
//
// No floating-point atomics anywhere: every sum's order is a function of (labels, n, D, K), so the same inputs give the same bits.
//
// Rounding: the dot product is an fmaf chain in the matrix cores (the specification leaves its order free); the two factors of the cosine
// and the terms fl(inv * x) of the sums are single float32 operations, defined in bn_rowstream.h under a contraction-off pragma that holds
// for this whole file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

constexpr int kSeg = BN_KMEANS_SEGMENT_ROWS;
constexpr int kMaxNT = BN_KMEANS_MAX_TILE / 16;
static_assert(kMaxNT == 8, "the launcher instantiates 1, 2, 4 and 8 centroid subtiles");
static_assert(BN_KMEANS_MAX_K <= 256 * 16, "kmeans_segments_kernel scans 16 clusters per thread");

// LDS pitch of a staged centroid in floats: the row padded to 64 elements (one 16-byte int8 load per lane and chunk) plus 4, so the 16
// centroids of a B fragment start four banks apart
__host__ __device__ inline int cent_pitch(int D) { return round_up(D, 64) + 4; }

}  // namespace

bool kmeans_geometry(long n, int D, int K, KmeansGeom* g) {
    int nt = 1;
    while (nt < kMaxNT && 16 * nt < K) nt <<= 1;
    while (nt > 1 && (size_t)16 * nt * cent_pitch(D) * 4 > BN_KMEANS_LDS_BYTES) nt >>= 1;
    const size_t lds = (size_t)16 * nt * cent_pitch(D) * 4;
    if (lds > BN_KMEANS_LDS_BYTES) return false;
    const RowSplit split = split_rows(n, BN_KMEANS_MIN_WG_STEPS, BN_KMEANS_MAX_WGS);
    g->nt = nt;
    g->tiles = (K + 16 * nt - 1) / (16 * nt);
    g->steps_per_wg = split.steps_per_wg;
    g->nwg = split.nwg;
    g->lds = lds;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------ assignment
template <bool I8, int NT>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(KmeansAssignArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TK = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, K = a.K;
    const int pitch = cent_pitch(D), Dp = pitch - 4;
    float* cs = reinterpret_cast<float*>(smem);
    const int nc = row_chunks<I8>(D);
    const bool aligned = ((uintptr_t)a.rows % 16 == 0) && (I8 ? D % 16 == 0 : D % 4 == 0);
    const size_t row_bytes = (size_t)D * (I8 ? 1 : 4);
    const int pad = I8 ? (int)(0x01010101u * (unsigned)(a.zp & 0xff)) : 0;   // bytes equal to the zero point are 0.0f after the conversion
    const long steps = ((long)a.n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.x * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;
    const int tiles = (K + TK - 1) / TK;
    int changed = 0;

    for (int tile = 0; tile < tiles; ++tile) {
        const int c0 = tile * TK;
        if (tile) __syncthreads();   // every wave has left the previous tile
        for (int e = tid; e < TK * Dp; e += 256) {   // stage the tile, zero beyond D and beyond K
            const int c = e / Dp, d = e - c * Dp;
            cs[c * pitch + d] = (c0 + c < K && d < D) ? a.cent[(size_t)(c0 + c) * D + d] : 0.0f;
        }
        __syncthreads();
        float cinv[NT];
        bool cok[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = c0 + t * 16 + li;
            cok[t] = c < K;
            cinv[t] = cok[t] ? a.cent_inv[c] : 0.0f;
        }

        for (long st = s0; st < s1; ++st) {
            const long tile_row = st * kStepRows + wave * 16;
            const long lrow = tile_row + li < a.n ? tile_row + li : (long)a.n - 1;   // rows past the end repeat the last one; nothing is written for them
            const RowView<I8> row{(const unsigned char*)a.rows + (size_t)lrow * row_bytes, D, nc, lk, pad, aligned};

            f32x4 facc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) facc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            row_stream(row, [&](int c, v4i av) __attribute__((always_inline)) {
                if constexpr (I8) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int w = av[g];
                        f32x4 af;
#pragma unroll
                        for (int j = 0; j < 4; ++j) af[j] = (float)((int)(int8_t)(w >> (8 * j)) - a.zp);
                        f32x4 b[NT];
#pragma unroll
                        for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(cs + (t * 16 + li) * pitch + c * 64 + lk * 16 + g * 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int t = 0; t < NT; ++t) facc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b[t][j], facc[t], 0, 0, 0);
                    }
                } else {
                    const f32x4 af = __builtin_bit_cast(f32x4, av);
                    f32x4 b[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(cs + (t * 16 + li) * pitch + c * 16 + lk * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int t = 0; t < NT; ++t) facc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b[t][j], facc[t], 0, 0, 0);
                }
            });

            // ---- facc[t][r]: row tile_row + 4 lk + r against centroid c0 + 16 t + li.  Best per row: over t in the lane, then over li.
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = tile_row + 4 * lk + r;
                const bool rok = row < a.n;
                const float rinv = rok ? a.row_inv[row] : 0.0f;
                float bs = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float s = f_mul(f_mul(facc[t][r], rinv), cinv[t]);
                    if (cok[t] && s > bs) {   // (t ascending: the lower index keeps an equal score)
                        bs = s;
                        bi = c0 + t * 16 + li;
                    }
                }
#pragma unroll
                for (int mk = 1; mk < 16; mk <<= 1) {   // (stays inside the 16 lanes of this lk)
                    const float os = __shfl_xor(bs, mk);
                    const int oi = __shfl_xor(bi, mk);
                    if (before(os, oi, bs, bi)) {
                        bs = os;
                        bi = oi;
                    }
                }
                if (li == r && rok) {
                    if (rinv == 0.0f) {   // a zero row belongs to no cluster
                        bs = 0.0f;
                        bi = -1;
                    } else {
                        if (tile > 0) {   // the best of the earlier tiles (lower indices: they keep an equal score), left here by this lane
                            const float ps = a.score[row];
                            const int pl = a.label[row];
                            if (!(bs > ps)) {
                                bs = ps;
                                bi = pl;
                            }
                        }
                        if (tile == tiles - 1) changed += a.prev ? (a.prev[row] != bi) : 1;
                    }
                    a.label[row] = bi;
                    a.score[row] = bs;
                }
            }
        }
    }
    for (int mk = 1; mk < 64; mk <<= 1) changed += __shfl_xor(changed, mk);
    if (lane == 0 && changed) atomicAdd(a.changed, (unsigned long long)changed);
}

template <bool I8, int NT>
static bool launch_assign_nt(const KmeansAssignArgs& a, const KmeansGeom& g, hipStream_t s) {
    const void* kf = (const void*)&kmeans_assign_kernel<I8, NT>;
    if (g.lds > 64 * 1024 && !ensure_dynamic_lds(kf, g.lds)) return false;
    hipLaunchKernelGGL((kmeans_assign_kernel<I8, NT>), dim3((unsigned)g.nwg), dim3(256), g.lds, s, a);
    return true;
}

bool launch_kmeans_assign(const KmeansAssignArgs& a, const KmeansGeom& g, bool i8, hipStream_t s) {
    if (i8)
        return g.nt == 1 ? launch_assign_nt<true, 1>(a, g, s) : g.nt == 2 ? launch_assign_nt<true, 2>(a, g, s) : g.nt == 4 ? launch_assign_nt<true, 4>(a, g, s)
                                                                                                                            : launch_assign_nt<true, 8>(a, g, s);
    return g.nt == 1 ? launch_assign_nt<false, 1>(a, g, s) : g.nt == 2 ? launch_assign_nt<false, 2>(a, g, s) : g.nt == 4 ? launch_assign_nt<false, 4>(a, g, s)
                                                                                                                            : launch_assign_nt<false, 8>(a, g, s);
}

// ---------------------------------------------------------------------------------------------------------------------- update
namespace {

__global__ __launch_bounds__(256) void kmeans_keys_kernel(const int* __restrict__ label, long n, int K, unsigned* __restrict__ keys, int* __restrict__ rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = label[i];
    keys[i] = (l >= 0 && l < K) ? (unsigned)l : (unsigned)K;   // -1 (and anything that is no cluster) sorts behind the last cluster
    rows[i] = (int)i;
}

// off[c], c = 0 .. K: the first sorted position whose key is >= c
__global__ __launch_bounds__(256) void kmeans_offsets_kernel(const unsigned* __restrict__ keys, long n, int K, int* __restrict__ off) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > K) return;
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (keys[mid] < (unsigned)c)
            lo = mid + 1;
        else
            hi = mid;
    }
    off[c] = (int)lo;
}

// One workgroup: counts[c] (+)= members of c; segoff[c], c = 0 .. K: segments of the clusters before c
__global__ __launch_bounds__(256) void kmeans_segments_kernel(const int* __restrict__ off, int K, int accumulate, int* __restrict__ segoff,
                                                              long long* __restrict__ counts) {
    __shared__ int part[257];
    const int t = threadIdx.x;
    int local = 0;
    for (int c = 16 * t; c < 16 * t + 16 && c < K; ++c) {
        const int m = off[c + 1] - off[c];
        counts[c] = (accumulate ? counts[c] : 0) + m;
        local += (m + kSeg - 1) / kSeg;
    }
    part[t + 1] = local;
    __syncthreads();
    if (t == 0) {
        part[0] = 0;
        for (int i = 1; i <= 256; ++i) part[i] += part[i - 1];
    }
    __syncthreads();
    int run = part[t];
    for (int c = 16 * t; c < 16 * t + 16 && c < K; ++c) {
        segoff[c] = run;
        run += (off[c + 1] - off[c] + kSeg - 1) / kSeg;
    }
    if (t == 255) segoff[K] = part[256];
}

template <bool I8>
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const void* __restrict__ rows, int D, int zp, const float* __restrict__ inv,
                                                             const int* __restrict__ sorted_rows, const int* __restrict__ off, const int* __restrict__ segoff,
                                                             int K, float* __restrict__ partial) {
    const int w = blockIdx.x;
    if (w >= segoff[K]) return;   // (the grid is the upper bound n / segment + K)
    int lo = 0, hi = K - 1;       // the cluster c with segoff[c] <= w < segoff[c + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segoff[mid + 1] > w)
            hi = mid;
        else
            lo = mid + 1;
    }
    const int c = lo;
    const int begin = off[c] + (w - segoff[c]) * kSeg;
    const int end = begin + kSeg < off[c + 1] ? begin + kSeg : off[c + 1];
    for (int d = threadIdx.x; d < D; d += 256) {
        float acc = 0.0f;
        for (int m = begin; m < end; m += 8) {   // eight members' loads in flight, added in member order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = 0.0f;
                if (m + u < end) {
                    const size_t r = (size_t)sorted_rows[m + u];
                    float x;
                    if constexpr (I8)
                        x = (float)((int)((const int8_t*)rows)[r * D + d] - zp);
                    else
                        x = ((const float*)rows)[r * D + d];
                    v[u] = f_mul(inv[r], x);
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (m + u < end) acc = f_add(acc, v[u]);
        }
        partial[(size_t)w * D + d] = acc;
    }
}

__global__ __launch_bounds__(256) void kmeans_fold_kernel(const float* __restrict__ partial, const int* __restrict__ segoff, int D, int accumulate,
                                                          float* __restrict__ sums) {
    const int c = blockIdx.x;
    const int s0 = segoff[c], s1 = segoff[c + 1];
    for (int d = threadIdx.x; d < D; d += 256) {
        float acc = accumulate ? sums[(size_t)c * D + d] : 0.0f;
        for (int s = s0; s < s1; ++s) acc = f_add(acc, partial[(size_t)s * D + d]);
        sums[(size_t)c * D + d] = acc;
    }
}

__global__ __launch_bounds__(256) void kmeans_scale_kernel(const float* __restrict__ sums, const long long* __restrict__ counts, const float* __restrict__ inv,
                                                           int K, int D, float* __restrict__ cent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)K * D) return;
    const int c = (int)(i / D);
    if (counts[c] > 0) cent[i] = f_mul(sums[i], inv[c]);   // a cluster without members keeps its centroid
}

inline size_t slab(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline int key_bits(int K) {   // keys are 0 .. K
    int b = 1;
    while ((1u << b) <= (unsigned)K) ++b;
    return b;
}
inline long max_segments(long n, int K) { return (n + kSeg - 1) / kSeg + K; }

}  // namespace

// [keys | sorted keys | rows | sorted rows | off | segoff | partial sums | rocPRIM storage]
size_t kmeans_accumulate_workspace(long n, int D, int K) {
    size_t sort = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort, (const unsigned*)nullptr, (unsigned*)nullptr, (const int*)nullptr, (int*)nullptr, (size_t)n, 0, key_bits(K));
    return 4 * slab((size_t)n * 4) + 2 * slab((size_t)(K + 1) * 4) + slab((size_t)max_segments(n, K) * D * 4) + slab(sort);
}

bool launch_kmeans_accumulate(const void* rows, bool i8, long n, int D, int zp, const float* row_inv, const int* label, int K, int accumulate, float* sums,
                              long long* counts, void* d_work, size_t work_bytes, hipStream_t s) {
    if (work_bytes < kmeans_accumulate_workspace(n, D, K)) return false;
    char* w = (char*)d_work;
    const size_t sl = slab((size_t)n * 4), sk = slab((size_t)(K + 1) * 4), sp = slab((size_t)max_segments(n, K) * D * 4);
    unsigned* keys = (unsigned*)w;
    unsigned* keys_sorted = (unsigned*)(w + sl);
    int* idx = (int*)(w + 2 * sl);
    int* idx_sorted = (int*)(w + 3 * sl);
    int* off = (int*)(w + 4 * sl);
    int* segoff = (int*)(w + 4 * sl + sk);
    float* partial = (float*)(w + 4 * sl + 2 * sk);
    void* tmp = w + 4 * sl + 2 * sk + sp;
    size_t tmp_bytes = work_bytes - (4 * sl + 2 * sk + sp);
    hipLaunchKernelGGL(kmeans_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, label, n, K, keys, idx);
    if (rocprim::radix_sort_pairs(tmp, tmp_bytes, (const unsigned*)keys, keys_sorted, (const int*)idx, idx_sorted, (size_t)n, 0, key_bits(K), s) != hipSuccess)
        return false;
    hipLaunchKernelGGL(kmeans_offsets_kernel, dim3((unsigned)(K / 256 + 1)), dim3(256), 0, s, keys_sorted, n, K, off);
    hipLaunchKernelGGL(kmeans_segments_kernel, dim3(1), dim3(256), 0, s, off, K, accumulate, segoff, counts);
    const dim3 grid((unsigned)max_segments(n, K));
    if (i8)
        hipLaunchKernelGGL(kmeans_partial_kernel<true>, grid, dim3(256), 0, s, rows, D, zp, row_inv, idx_sorted, off, segoff, K, partial);
    else
        hipLaunchKernelGGL(kmeans_partial_kernel<false>, grid, dim3(256), 0, s, rows, D, zp, row_inv, idx_sorted, off, segoff, K, partial);
    hipLaunchKernelGGL(kmeans_fold_kernel, dim3((unsigned)K), dim3(256), 0, s, partial, segoff, D, accumulate, sums);
    return true;
}

void launch_kmeans_centroids(const float* sums, const long long* counts, int K, int D, float* cent, float* cent_inv, hipStream_t s) {
    launch_search_inv_norms(sums, false, K, D, 0, cent_inv, s);   // (cent_inv holds the sums' inverse norms until the last launch)
    hipLaunchKernelGGL(kmeans_scale_kernel, dim3((unsigned)(((long)K * D + 255) / 256)), dim3(256), 0, s, sums, counts, cent_inv, K, D, cent);
    launch_search_inv_norms(cent, false, K, D, 0, cent_inv, s);
}

void preload_kmeans() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&kmeans_fold_kernel));
}

}  // namespace bn
