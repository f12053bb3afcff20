// bn_density.hip — one Borůvka round of the maximum spanning tree of the mutual-reachability graph over a matrix of embeddings: for every
// row the best row of another component (birdnet_stm32/evaluation/density.py is the specification).
//
//   density_nearest_kernel   grid (tiles of staged rows, row ranges).  A workgroup stages a tile of 16 * NT rows in LDS as the B operand of
//                            the matrix cores, with their inverse norm, core score and component in registers, and streams its range of
//                            all rows once, straight into the A operand (bn_rowstream.h owns the row layout, the padding beyond D and the
//                            prefetch depth; v_mfma_f32_16x16x4_f32: exact float32 products; v_mfma_i32_16x16x64_i8 on the raw bytes, zero
//                            beyond D, the zero point taken out afterwards through the two rows' byte sums).  The epilogue forms
//                            s = fl(dot * fl(inv_i * inv_j)) and m = min(s, core_i, core_j), masks pairs of one component and keeps per
//                            streamed row the best key of the tile; the tiles and the workgroups meet in a 64-bit integer atomicMax.
//
// The key is (order-preserving image of m) << 32 | (0xFFFFFFFF - j): its integer order is "m descending, then j ascending" read upwards, a
// total order, and a maximum under a total order does not depend on the order in which the candidates arrive.  No floating-point atomics;
// the grid follows from (n, D, dtype) alone (density_geometry).
//
// Symmetry: a product of two floats does not depend on their order, the matrix cores add the products of a pair of rows in an order that
// depends on the element index alone, and the epilogue is symmetric in its two rows: the pair (i, j) has one score whichever of the two is
// staged and whichever is streamed.
//
// Rounding: f_mul, one rounding per product, under the contraction-off pragma of bn_rowstream.h that holds for this whole file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

constexpr int kMaxNT = BN_DENSITY_MAX_TILE / 16;
static_assert(kMaxNT == 8, "the launcher instantiates 1, 2, 4 and 8 staged subtiles");
static_assert(BN_DENSITY_STEP_ROWS == kStepRows, "the public header states the step of every kernel");
static_assert(BN_DENSITY_MAX_N <= (1 << 30), "row numbers fit the low half of a key with room to spare");

// LDS pitch of a staged row in bytes: the padded row plus 16 bytes, so the 16 rows of a B fragment start four banks apart
__host__ __device__ inline int staged_pitch(int D, bool i8) { return i8 ? round_up(D, 64) + 16 : (round_up(D, 64) + 4) * 4; }

// float32 -> uint32 whose unsigned order is the order of the floats (-0 sorts below +0: the epilogue adds +0 first)
__device__ __forceinline__ unsigned ordered_image(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace

bool density_geometry(long n, int D, bool i8, DensityGeom* g) {
    int nt = kMaxNT;
    while (nt > 1 && (size_t)16 * nt * staged_pitch(D, i8) > BN_DENSITY_LDS_BYTES) nt >>= 1;
    while (nt > 1 && 16 * (nt >> 1) >= n) nt >>= 1;   // (a small matrix does not stage rows that are not there)
    const size_t lds = (size_t)16 * nt * staged_pitch(D, i8);
    if (lds > BN_DENSITY_LDS_BYTES) return false;
    const RowSplit split = split_rows(n, BN_DENSITY_MIN_WG_STEPS, BN_DENSITY_MAX_ROW_WGS);
    g->nt = nt;
    g->tiles = (int)((n + 16 * nt - 1) / (16 * nt));
    g->steps_per_wg = split.steps_per_wg;
    g->nwg = split.nwg;
    g->lds = lds;
    return true;
}

template <bool I8, int NT>
__global__ __launch_bounds__(256) void density_nearest_kernel(DensityArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TJ = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, n = a.n;
    const int pitch = staged_pitch(D, I8);
    const int j0 = blockIdx.x * TJ;   // first staged row

    // ---- stage the tile (zero beyond D and beyond n)
    if constexpr (I8) {
        const int Dp = pitch - 16;
        const int8_t* src = (const int8_t*)a.rows;
        for (int e = tid; e < TJ * Dp; e += 256) {
            const int q = e / Dp, d = e - q * Dp;
            smem[q * pitch + d] = (j0 + q < n && d < D) ? (unsigned char)src[(size_t)(j0 + q) * D + d] : 0;
        }
    } else {
        const int Dp = pitch / 4 - 4;
        const float* src = (const float*)a.rows;
        for (int e = tid; e < TJ * Dp; e += 256) {
            const int q = e / Dp, d = e - q * Dp;
            reinterpret_cast<float*>(smem + q * pitch)[d] = (j0 + q < n && d < D) ? src[(size_t)(j0 + q) * D + d] : 0.0f;
        }
    }
    __syncthreads();

    // ---- per lane: its staged row of every subtile
    float jinv[NT], jcore[NT];
    int jcomp[NT], jcorr[NT];
    unsigned jlow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = j0 + t * 16 + li;
        const bool ok = j < n;
        jinv[t] = ok ? a.inv[j] : 0.0f;
        jcore[t] = ok ? a.core[j] : 0.0f;
        jcomp[t] = ok ? a.comp[j] : -1;   // (a row that is not there is a row that takes no part)
        jlow[t] = 0xFFFFFFFFu - (unsigned)j;
        jcorr[t] = 0;
    }
    const int nc = row_chunks<I8>(D);
    if constexpr (I8) {   // dot of centred bytes = sum a b - zp (sum a + sum b) + D zp^2: the staged row's share of it, once
        const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v4i acc = {0, 0, 0, 0};
            for (int c = 0; c < nc; ++c)
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, *reinterpret_cast<const v4i*>(smem + (t * 16 + li) * pitch + c * 64 + lk * 16), acc, 0, 0, 0);
            jcorr[t] = D * a.zp * a.zp - a.zp * acc[0];
        }
    }

    const bool aligned = ((uintptr_t)a.rows % 16 == 0) && (I8 ? D % 16 == 0 : D % 4 == 0);
    const size_t row_bytes = (size_t)D * (I8 ? 1 : 4);
    const long steps = ((long)n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.y * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;

    for (long st = s0; st < s1; ++st) {
        const long tile_row = st * kStepRows + wave * 16;
        const long lrow = tile_row + li < n ? tile_row + li : (long)n - 1;   // rows past the end repeat the last one; nothing is written for them
        const RowView<I8> row{(const unsigned char*)a.rows + (size_t)lrow * row_bytes, D, nc, lk, 0, aligned};   // zero beyond D

        f32x4 facc[NT];
        v4i iacc[NT], rsum = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            facc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            iacc[t] = v4i{0, 0, 0, 0};
        }
        row_stream(row, [&](int c, v4i av) __attribute__((always_inline)) {
            if constexpr (I8) {
                const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
                rsum = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, ones, rsum, 0, 0, 0);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    iacc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, *reinterpret_cast<const v4i*>(smem + (t * 16 + li) * pitch + c * 64 + lk * 16), iacc[t], 0, 0, 0);
            } else {
                const f32x4 af = __builtin_bit_cast(f32x4, av);
                f32x4 b[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(smem + (t * 16 + li) * pitch + (c * 16 + lk * 4) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t = 0; t < NT; ++t) facc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b[t][j], facc[t], 0, 0, 0);
            }
        });

        // ---- accumulator [t][r]: row tile_row + 4 lk + r against staged row j0 + 16 t + li.  Best key per row: over t in the lane, then over li.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long i = tile_row + 4 * lk + r;
            const bool rok = i < n;
            const float rinv = rok ? a.inv[i] : 0.0f;
            const float rcore = rok ? a.core[i] : 0.0f;
            const int rcomp = rok ? a.comp[i] : -1;
            unsigned long long key = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float dot;
                if constexpr (I8)
                    dot = (float)(iacc[t][r] - a.zp * rsum[r] + jcorr[t]);
                else
                    dot = facc[t][r];
                const float s = f_mul(dot, f_mul(rinv, jinv[t]));
                const float m = f_add(fminf(fminf(s, rcore), jcore[t]), 0.0f);   // (+0: a negative zero becomes the positive one)
                const bool ok = rcomp >= 0 && jcomp[t] >= 0 && rcomp != jcomp[t];
                const unsigned long long k = ok ? ((unsigned long long)ordered_image(m) << 32) | jlow[t] : 0ull;
                key = k > key ? k : key;
            }
#pragma unroll
            for (int mk = 1; mk < 16; mk <<= 1) {   // (stays inside the 16 lanes of this lk)
                const unsigned long long o = __shfl_xor(key, mk);
                key = o > key ? o : key;
            }
            if (li == r && key) atomicMax(a.best + i, key);   // (key != 0 only for a row that is there)
        }
    }
}

template <bool I8, int NT>
static bool launch_nearest_nt(const DensityArgs& a, const DensityGeom& g, hipStream_t s) {
    const void* kf = (const void*)&density_nearest_kernel<I8, NT>;
    if (g.lds > 64 * 1024 && !ensure_dynamic_lds(kf, g.lds)) return false;
    hipLaunchKernelGGL((density_nearest_kernel<I8, NT>), dim3((unsigned)g.tiles, (unsigned)g.nwg), dim3(256), g.lds, s, a);
    return true;
}

bool launch_density_nearest(const DensityArgs& a, const DensityGeom& g, bool i8, hipStream_t s) {
    if (i8)
        return g.nt == 1 ? launch_nearest_nt<true, 1>(a, g, s) : g.nt == 2 ? launch_nearest_nt<true, 2>(a, g, s) : g.nt == 4 ? launch_nearest_nt<true, 4>(a, g, s)
                                                                                                                              : launch_nearest_nt<true, 8>(a, g, s);
    return g.nt == 1 ? launch_nearest_nt<false, 1>(a, g, s) : g.nt == 2 ? launch_nearest_nt<false, 2>(a, g, s) : g.nt == 4 ? launch_nearest_nt<false, 4>(a, g, s)
                                                                                                                              : launch_nearest_nt<false, 8>(a, g, s);
}

void preload_density() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&density_nearest_kernel<false, 1>));
}

}  // namespace bn
