// bn_silhouette.hip — the mean cosines behind the exact cosine silhouette of a labelling.
//
// With x^_i the normalised row and S_c the sum of the normalised members of cluster c, sum_{j in c} (1 - x^_i . x^_j) = n_c - x^_i . S_c: the
// silhouette of every row needs the rows against the K sums once, not against each other.
//
//   silhouette_means_kernel  grid (row ranges).  The structure of kmeans_assign_kernel (bn_kmeans.hip): the K sums sit in LDS as the B operand
//                            of the matrix cores, a tile of 16 * NT at a time (kmeans_geometry chooses the tile, as it does for the
//                            centroids); a workgroup streams its range of rows once per tile, straight into the A operand (bn_rowstream.h;
//                            v_mfma_f32_16x16x4_f32: exact float32 products; int8 bytes become float32(byte - zero_point) on the way).
//                            m[i, c] = fl(fl(dot(x_i, S_c) * inv[i]) * w[c]).  Per row the epilogue keeps m at the row's own label, and the
//                            best (m, c) over c != label with w[c] != 0 under the total order of before() — m descending, c ascending —
//                            which is one value however the sums are tiled.  With several tiles own and the best so far are carried in the
//                            row's own output slots, which only the lane that wrote them reads again.
//
// No atomics of any kind: the same inputs give the same bits.  The dot product is an fmaf chain in the matrix cores (the specification
// leaves its order free); the two factors are single float32 operations under the contraction-off pragma of bn_rowstream.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

constexpr int kMaxNT = BN_KMEANS_MAX_TILE / 16;
static_assert(kMaxNT == 8, "the launcher instantiates 1, 2, 4 and 8 subtiles of sums");
constexpr int kNone = 0x7fffffff;   // no other cluster seen yet: behind every index under before()

// LDS pitch of a staged sum in floats, a staged centroid's (bn_kmeans.hip; kmeans_geometry sizes the LDS by it)
__host__ __device__ inline int sum_pitch(int D) { return round_up(D, 64) + 4; }

template <bool I8, int NT>
__global__ __launch_bounds__(256) void silhouette_means_kernel(SilhouetteArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TK = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, K = a.K;
    const int pitch = sum_pitch(D), Dp = pitch - 4;
    float* cs = reinterpret_cast<float*>(smem);
    const int nc = row_chunks<I8>(D);
    const bool aligned = ((uintptr_t)a.rows % 16 == 0) && (I8 ? D % 16 == 0 : D % 4 == 0);
    const size_t row_bytes = (size_t)D * (I8 ? 1 : 4);
    const int pad = I8 ? (int)(0x01010101u * (unsigned)(a.zp & 0xff)) : 0;   // bytes equal to the zero point are 0.0f after the conversion
    const long steps = ((long)a.n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.x * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;
    const int tiles = (K + TK - 1) / TK;

    for (int tile = 0; tile < tiles; ++tile) {
        const int c0 = tile * TK;
        if (tile) __syncthreads();   // every wave has left the previous tile
        for (int e = tid; e < TK * Dp; e += 256) {   // stage the tile, zero beyond D and beyond K
            const int c = e / Dp, d = e - c * Dp;
            cs[c * pitch + d] = (c0 + c < K && d < D) ? a.sums[(size_t)(c0 + c) * D + d] : 0.0f;
        }
        __syncthreads();
        float cw[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = c0 + t * 16 + li;
            cw[t] = c < K ? a.weight[c] : 0.0f;   // (a column beyond K is an empty cluster)
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

            // ---- facc[t][r]: row tile_row + 4 lk + r against sum c0 + 16 t + li.  Per row: over t in the lane, then over li.
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = tile_row + 4 * lk + r;
                const bool rok = row < a.n;
                const float rinv = rok ? a.row_inv[row] : 0.0f;
                const int lab = rok ? a.label[row] : -1;
                const bool live = rinv != 0.0f && lab >= 0 && lab < K;
                float bs = -INFINITY, own = 0.0f;
                int bi = kNone;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int c = c0 + t * 16 + li;
                    const float m = f_mul(f_mul(facc[t][r], rinv), cw[t]);
                    if (c == lab) own = m;
                    if (c != lab && cw[t] != 0.0f && (bi == kNone || m > bs)) {   // (t ascending: the lower index keeps an equal mean)
                        bs = m;
                        bi = c;
                    }
                }
#pragma unroll
                for (int mk = 1; mk < 16; mk <<= 1) {   // (stays inside the 16 lanes of this lk)
                    const float os = __shfl_xor(bs, mk);
                    const int oi = __shfl_xor(bi, mk);
                    if (oi != kNone && (bi == kNone || before(os, oi, bs, bi))) {
                        bs = os;
                        bi = oi;
                    }
                }
                const bool has_own = live && lab >= c0 && lab < c0 + TK;
                own = __shfl(own, (lane & 48) | ((lab - c0) & 15));   // the lane of column `lab`, where this tile holds it
                if (li == r && rok) {
                    if (!live) {   // a zero row, noise, a label that is no cluster
                        a.own[row] = 0.0f;
                        a.other[row] = 0.0f;
                        a.nearest[row] = -1;
                    } else {
                        if (tile > 0) {   // the best of the earlier tiles (lower indices: they keep an equal mean), left here by this lane
                            const float ps = a.other[row];
                            const int pn = a.nearest[row];
                            if (pn >= 0 && (bi == kNone || !(bs > ps))) {
                                bs = ps;
                                bi = pn;
                            }
                        }
                        if (has_own || tile == 0) a.own[row] = has_own ? own : 0.0f;
                        a.other[row] = bi == kNone ? 0.0f : bs;
                        a.nearest[row] = bi == kNone ? -1 : bi;
                    }
                }
            }
        }
    }
}

template <bool I8, int NT>
bool launch_means_nt(const SilhouetteArgs& a, const KmeansGeom& g, hipStream_t s) {
    const void* kf = (const void*)&silhouette_means_kernel<I8, NT>;
    if (g.lds > 64 * 1024 && !ensure_dynamic_lds(kf, g.lds)) return false;
    hipLaunchKernelGGL((silhouette_means_kernel<I8, NT>), dim3((unsigned)g.nwg), dim3(256), g.lds, s, a);
    return true;
}

}  // namespace

bool launch_silhouette_means(const SilhouetteArgs& a, const KmeansGeom& g, bool i8, hipStream_t s) {
    if ((size_t)16 * g.nt * sum_pitch(a.D) * 4 != g.lds) return false;   // the geometry is kmeans_geometry's, for this D
    if (i8)
        return g.nt == 1 ? launch_means_nt<true, 1>(a, g, s) : g.nt == 2 ? launch_means_nt<true, 2>(a, g, s) : g.nt == 4 ? launch_means_nt<true, 4>(a, g, s)
                                                                                                                        : launch_means_nt<true, 8>(a, g, s);
    return g.nt == 1 ? launch_means_nt<false, 1>(a, g, s) : g.nt == 2 ? launch_means_nt<false, 2>(a, g, s) : g.nt == 4 ? launch_means_nt<false, 4>(a, g, s)
                                                                                                                        : launch_means_nt<false, 8>(a, g, s);
}

void preload_silhouette() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&silhouette_means_kernel<false, 1>));
}

}  // namespace bn
