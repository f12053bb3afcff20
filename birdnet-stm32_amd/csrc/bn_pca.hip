// bn_pca.hip — principal components of a matrix of embeddings: column sums, the scatter matrix and the projection.
//
//   pca_colsum_kernel        grid (row ranges).  Lanes across the columns, BN_PCA_COLSUM_COLS at a time (fewer lanes for a narrow matrix: the
//                            others take every G-th row); float64 sums in ascending row order, the G groups added in ascending order.
//   pca_colsum_fold_kernel   the ranges' partial sums per column, in ascending range order
//   pca_gram_kernel          grid (pairs of macro tiles of the upper triangle, row ranges).  The transposed product G = sum_i c_i c_i^T: the
//                            reduction runs over rows, so a lane's operand element is (feature, row).  A workgroup stages BN_PCA_STAGE_ROWS
//                            rows of the BN_PCA_MACRO features of either side in LDS (whole-row coalesced loads, issued one stage ahead, centred on the way:
//                            fl32(x - mean); int8 bytes become float32(byte - zero_point), which is exact) and both operands of
//                            v_mfma_f32_16x16x4_f32 come from there: lane (li, lk) takes feature li of its tile and row lk of the step.  Wave w
//                            owns feature tile w of the first side against the four tiles of the second; on a diagonal pair only the tiles
//                            at or above its own.  Products stay in the float32 accumulators for BN_PCA_RUN_ROWS rows, then they move into
//                            float64 registers: the float32 error does not grow with n, and an int8 run stays below 2^24 (256 * 255^2), so
//                            the int8 result is the exact integer.
//   pca_gram_fold_kernel     per entry of the upper triangle the ranges' partial sums in ascending range order, written to (a, b) and (b, a):
//                            G == G^T bit for bit
//   pca_transform_kernel     the structure of kmeans_assign_kernel: a tile of 16 * NT rows of W in LDS as the B operand, the rows streamed
//                            into the A operand by bn_rowstream.h, centred at load from a mean held in LDS; the epilogue stores every product.
//
// No floating-point atomics anywhere: every sum's order is a function of (n, D, dtype[, r]), so the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

constexpr int kRun = BN_PCA_RUN_ROWS, kStage = BN_PCA_STAGE_ROWS, kMacro = BN_PCA_MACRO;
constexpr int kPitch = kMacro + 16;   // floats of a staged row: the four rows of an MFMA step start 16 banks apart
constexpr int kMaxNT = BN_PCA_MAX_TILE / 16;
static_assert(kMacro == 64 && kStage == 64, "a workgroup is four waves, one 16-feature tile of the first side each; a stage is 16 MFMA steps of 4 rows");
static_assert(kRun % kStage == 0, "a run is whole stages");
static_assert((long)kRun * 255 * 255 < (1 << 24), "an int8 run of products stays exact in a float32 accumulator");
static_assert(kMaxNT == 8, "the launcher instantiates 1, 2, 4 and 8 subtiles of W");
static_assert(BN_PCA_STEP_ROWS == kStepRows, "the transform streams rows in bn_rowstream.h's steps");

inline size_t slab(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
__host__ __device__ inline int macro_tiles(int D) { return (D + kMacro - 1) / kMacro; }
__host__ __device__ inline int macro_pairs(int D) { return macro_tiles(D) * (macro_tiles(D) + 1) / 2; }
// position of the pair (ma <= mb) in the row-major walk of the upper triangle
__host__ __device__ inline int pair_index(int ma, int mb, int M) { return ma * M - ma * (ma - 1) / 2 + (mb - ma); }

// ------------------------------------------------------------------------------------------------------------------ column sums
template <bool I8>
__device__ __forceinline__ double elem(const void* rows, size_t i, int zp) {
    if constexpr (I8)
        return (double)((int)((const int8_t*)rows)[i] - zp);
    else
        return (double)((const float*)rows)[i];
}

template <bool I8>
__global__ __launch_bounds__(256) void pca_colsum_kernel(const void* __restrict__ rows, long n, int D, int zp, int dc, long rows_per_wg,
                                                         double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x, G = 256 / dc, g = tid / dc, dl = tid - g * dc;
    const long r_begin = (long)blockIdx.x * rows_per_wg;
    const long r_end = r_begin + rows_per_wg < n ? r_begin + rows_per_wg : n;
    for (int d0 = 0; d0 < D; d0 += dc) {
        const int d = d0 + dl;
        double s = 0.0;
        if (d < D)
            for (long r = r_begin + g; r < r_end; r += 8L * G) {   // eight rows' loads in flight, added in row order
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const long rr = r + (long)u * G;
                    v[u] = rr < r_end ? elem<I8>(rows, (size_t)rr * D + d, zp) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (r + (long)u * G < r_end) s += v[u];
            }
        red[tid] = s;
        __syncthreads();
        if (g == 0 && d < D) {
            for (int q = 1; q < G; ++q) s += red[q * dc + dl];
            part[(size_t)blockIdx.x * D + d] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void pca_colsum_fold_kernel(const double* __restrict__ part, int D, int nwg, double* __restrict__ sum) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += part[(size_t)w * D + d];
    sum[d] = s;
}

// ---------------------------------------------------------------------------------------------------------------- scatter matrix
struct GramArgs {
    const void* rows;
    const float* mean;   // or null
    double* part;        // [ranges][macro pairs][kMacro * kMacro]
    long n, rows_per_range;
    int D, zp;
    bool vec;            // every row starts on a 16-byte boundary and holds whole 16-byte pieces
};

// A thread's 16 elements of rows r0 .. r0 + kStage - 1 of the features 64 m .. 64 m + 63, as they lie in memory (zeros from r_end and from
// D on): loaded one stage ahead, so that the loads are in flight while the matrix cores work on the stage before
struct StageRegs {
    v4i w[4];
};

template <bool I8>
__device__ __forceinline__ void gram_load(const GramArgs& a, int m, long r0, long r_end, StageRegs& g) {
    const int tid = threadIdx.x, D = a.D, col0 = m * kMacro;
#pragma unroll
    for (int j = 0; j < 4; ++j) g.w[j] = v4i{0, 0, 0, 0};
    if (a.vec) {
        if constexpr (I8) {
            const int d = col0 + (tid & 3) * 16;
            const long gr = r0 + (tid >> 2);
            if (gr < r_end && d < D) g.w[0] = *reinterpret_cast<const v4i*>((const unsigned char*)a.rows + (size_t)gr * D + d);   // (D % 16 == 0: inside the row)
        } else {
            const int d = col0 + (tid & 15) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long gr = r0 + (tid >> 4) + 16 * j;
                if (gr < r_end && d < D) g.w[j] = *reinterpret_cast<const v4i*>((const float*)a.rows + (size_t)gr * D + d);   // (D % 4 == 0: inside the row)
            }
        }
    } else {
        const int d = col0 + (tid & 63);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long gr = r0 + (tid >> 6) + 4 * j;
            if (gr < r_end && d < D) {
                if constexpr (I8)
                    g.w[j >> 2][j & 3] = (int)((const int8_t*)a.rows)[(size_t)gr * D + d];
                else
                    g.w[j >> 2][j & 3] = ((const int*)a.rows)[(size_t)gr * D + d];
            }
        }
    }
}

// The loaded elements, made float32 and centred, into xs[row * kPitch + col]; what lies beyond r_end or D stays 0 (it is not centred)
template <bool I8>
__device__ __forceinline__ void gram_store(const GramArgs& a, int m, long r0, long r_end, const float* mu, float* xs, const StageRegs& g) {
    const int tid = threadIdx.x, D = a.D, col0 = m * kMacro;
    if (a.vec) {
        if constexpr (I8) {
            const int row = tid >> 2, c = (tid & 3) * 16;
            const bool ok = r0 + row < r_end && col0 + c < D;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ok ? f_sub((float)((int)(int8_t)(g.w[0][q] >> (8 * j)) - a.zp), mu[c + 4 * q + j]) : 0.0f;
                *reinterpret_cast<f32x4*>(xs + row * kPitch + c + 4 * q) = v;
            }
        } else {
            const int c = (tid & 15) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = (tid >> 4) + 16 * j;
                const bool ok = r0 + row < r_end && col0 + c < D;
                const f32x4 x = __builtin_bit_cast(f32x4, g.w[j]);
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = ok ? f_sub(x[q], mu[c + q]) : 0.0f;
                *reinterpret_cast<f32x4*>(xs + row * kPitch + c) = v;
            }
        }
    } else {
        const int c = tid & 63;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (tid >> 6) + 4 * j;
            const bool ok = r0 + row < r_end && col0 + c < D;
            const int w = g.w[j >> 2][j & 3];
            float x;
            if constexpr (I8)
                x = (float)(w - a.zp);
            else
                x = __builtin_bit_cast(float, w);
            xs[row * kPitch + c] = ok ? f_sub(x, mu[c]) : 0.0f;
        }
    }
}

// One staged block: feature tile `wave` of the first side against the tiles T0 .. 3 of the second (T0 > 0: a diagonal pair, upper triangle only)
template <int T0>
__device__ __forceinline__ void gram_multiply(const float* xa, const float* xb, int wave, int li, int lk, f32x4 (&acc)[4]) {
#pragma unroll 4
    for (int k0 = 0; k0 < kStage; k0 += 4) {
        const float av = xa[(k0 + lk) * kPitch + wave * 16 + li];
#pragma unroll
        for (int t = T0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[(k0 + lk) * kPitch + t * 16 + li], acc[t], 0, 0, 0);
    }
}

template <bool I8>
__global__ __launch_bounds__(256) void pca_gram_kernel(GramArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[2][kStage * kPitch];
    __shared__ float mu[2][kMacro];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (in a scalar register: what depends on it branches, it does not mask lanes)
    const int D = a.D, M = macro_tiles(D);
    int p = blockIdx.x, ma = 0;
    while (p >= M - ma) {   // (blockIdx.x < M (M + 1) / 2: ends with ma < M)
        p -= M - ma;
        ++ma;
    }
    const int mb = ma + p;
    const bool diag = ma == mb;
    const long r_begin = (long)blockIdx.y * a.rows_per_range;
    const long r_end = r_begin + a.rows_per_range < a.n ? r_begin + a.rows_per_range : a.n;
    if (tid < 2 * kMacro) {
        const int side = tid >> 6, d = (side ? mb : ma) * kMacro + (tid & 63);
        mu[side][tid & 63] = (a.mean && d < D) ? a.mean[d] : 0.0f;
    }
    __syncthreads();

    f32x4 acc[4];
    double dacc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 4; ++r) dacc[t][r] = 0.0;
    }
    const float* xa = xs[0];
    const float* xb = diag ? xs[0] : xs[1];
    const int t_first = diag ? wave : 0;   // the first tile of the second side this wave multiplies
    StageRegs ga, gb;
    gram_load<I8>(a, ma, r_begin, r_end, ga);
    if (!diag) gram_load<I8>(a, mb, r_begin, r_end, gb);
    for (long r0 = r_begin; r0 < r_end; r0 += kStage) {
        if (r0 != r_begin) __syncthreads();   // every wave has left the previous stage
        gram_store<I8>(a, ma, r0, r_end, mu[0], xs[0], ga);
        if (!diag) gram_store<I8>(a, mb, r0, r_end, mu[1], xs[1], gb);
        __syncthreads();
        if (r0 + kStage < r_end) {   // the next stage's loads fly while this one is multiplied
            gram_load<I8>(a, ma, r0 + kStage, r_end, ga);
            if (!diag) gram_load<I8>(a, mb, r0 + kStage, r_end, gb);
        }
        switch (t_first) {   // (a scalar: a branch, no lane is masked around a matrix instruction)
            case 0: gram_multiply<0>(xa, xb, wave, li, lk, acc); break;
            case 1: gram_multiply<1>(xa, xb, wave, li, lk, acc); break;
            case 2: gram_multiply<2>(xa, xb, wave, li, lk, acc); break;
            default: gram_multiply<3>(xa, xb, wave, li, lk, acc); break;
        }
        if ((r0 + kStage - r_begin) % kRun == 0 || r0 + kStage >= r_end) {   // the run ends: its float32 sums move into float64
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dacc[t][r] += (double)acc[t][r];
                acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
    }
    // dacc[t][r]: feature 16 wave + 4 lk + r of the first side against feature 16 t + li of the second
    double* out = a.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kMacro * kMacro);
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (t >= t_first)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(wave * 16 + 4 * lk + r) * kMacro + t * 16 + li] = dacc[t][r];
}

__global__ __launch_bounds__(256) void pca_gram_fold_kernel(const double* __restrict__ part, int D, int ranges, double* __restrict__ G) {
    const int b = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
    if (b >= D || a > b) return;   // (a <= b: the 16-tile of a is at or before the tile of b, so the entry was written)
    const int M = macro_tiles(D);
    const size_t stride = (size_t)macro_pairs(D) * (kMacro * kMacro);
    const size_t off = (size_t)pair_index(a / kMacro, b / kMacro, M) * (kMacro * kMacro) + (a % kMacro) * kMacro + (b % kMacro);
    double s = 0.0;
    for (int r = 0; r < ranges; ++r) s += part[(size_t)r * stride + off];
    G[(size_t)a * D + b] = s;
    G[(size_t)b * D + a] = s;
}

// LDS pitch of a staged row of W in floats, as a staged centroid's (bn_kmeans.hip)
__host__ __device__ inline int w_pitch(int D) { return round_up(D, 64) + 4; }

}  // namespace

// -------------------------------------------------------------------------------------------------------------------- geometry
void pca_colsum_geometry(long n, int D, PcaColsumGeom* g) {
    int dc = 1;
    while (dc < D && dc < BN_PCA_COLSUM_COLS) dc <<= 1;
    long wgs = (n + BN_PCA_COLSUM_MIN_ROWS - 1) / BN_PCA_COLSUM_MIN_ROWS;
    wgs = wgs < 1 ? 1 : wgs > BN_PCA_COLSUM_MAX_WGS ? BN_PCA_COLSUM_MAX_WGS : wgs;
    const long per = n > 0 ? (n + wgs - 1) / wgs : 1;
    g->dc = dc;
    g->rows_per_wg = per;
    g->nwg = n > 0 ? (int)((n + per - 1) / per) : 1;
}

void pca_gram_geometry(long n, int D, PcaGramGeom* g) {
    const int P = macro_pairs(D);
    const long runs = (n + kRun - 1) / kRun;
    long ranges = (BN_PCA_GRAM_TARGET_WGS + P - 1) / P;
    ranges = ranges > BN_PCA_GRAM_MAX_RANGES ? BN_PCA_GRAM_MAX_RANGES : ranges;
    ranges = ranges > runs ? runs : ranges;
    ranges = ranges < 1 ? 1 : ranges;
    const long per = runs > 0 ? (runs + ranges - 1) / ranges : 1;
    g->pairs = P;
    g->rows_per_range = per * kRun;
    g->ranges = runs > 0 ? (int)((runs + per - 1) / per) : 1;
}

bool pca_transform_geometry(long n, int D, int r, PcaTransformGeom* g) {
    int nt = 1;
    while (nt < kMaxNT && 16 * nt < r) nt <<= 1;
    const size_t mean_bytes = (size_t)round_up(D, 64) * 4;
    while (nt > 1 && (size_t)16 * nt * w_pitch(D) * 4 + mean_bytes > BN_PCA_LDS_BYTES) nt >>= 1;
    const size_t lds = (size_t)16 * nt * w_pitch(D) * 4 + mean_bytes;
    if (lds > BN_PCA_LDS_BYTES) return false;
    const RowSplit split = split_rows(n, BN_PCA_MIN_WG_STEPS, BN_PCA_MAX_WGS);
    g->nt = nt;
    g->tiles = (r + 16 * nt - 1) / (16 * nt);
    g->steps_per_wg = split.steps_per_wg;
    g->nwg = split.nwg;
    g->lds = lds;
    return true;
}

size_t pca_colsum_workspace(long n, int D) {
    PcaColsumGeom g{};
    pca_colsum_geometry(n, D, &g);
    return slab((size_t)g.nwg * D * sizeof(double));
}

size_t pca_gram_workspace(long n, int D) {
    PcaGramGeom g{};
    pca_gram_geometry(n, D, &g);
    return slab((size_t)g.ranges * g.pairs * (kMacro * kMacro) * sizeof(double));
}

// -------------------------------------------------------------------------------------------------------------------- launchers
void launch_pca_colsum(const void* rows, bool i8, long n, int D, int zp, double* sum, void* d_work, hipStream_t s) {
    PcaColsumGeom g{};
    pca_colsum_geometry(n, D, &g);
    double* part = (double*)d_work;
    if (i8)
        hipLaunchKernelGGL(pca_colsum_kernel<true>, dim3((unsigned)g.nwg), dim3(256), 0, s, rows, n, D, zp, g.dc, g.rows_per_wg, part);
    else
        hipLaunchKernelGGL(pca_colsum_kernel<false>, dim3((unsigned)g.nwg), dim3(256), 0, s, rows, n, D, zp, g.dc, g.rows_per_wg, part);
    hipLaunchKernelGGL(pca_colsum_fold_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, part, D, g.nwg, sum);
}

void launch_pca_gram(const void* rows, bool i8, long n, int D, int zp, const float* mean, double* gram, void* d_work, hipStream_t s) {
    PcaGramGeom g{};
    pca_gram_geometry(n, D, &g);
    GramArgs a{};
    a.rows = rows; a.mean = mean; a.part = (double*)d_work; a.n = n; a.rows_per_range = g.rows_per_range; a.D = D; a.zp = i8 ? zp : 0;
    a.vec = (uintptr_t)rows % 16 == 0 && (i8 ? D % 16 == 0 : D % 4 == 0);
    const dim3 grid((unsigned)g.pairs, (unsigned)g.ranges);
    if (i8)
        hipLaunchKernelGGL(pca_gram_kernel<true>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(pca_gram_kernel<false>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(pca_gram_fold_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)D), dim3(256), 0, s, a.part, D, g.ranges, gram);
}

// -------------------------------------------------------------------------------------------------------------------- transform
template <bool I8, int NT>
__global__ __launch_bounds__(256) void pca_transform_kernel(PcaTransformArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TK = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, R = a.r;
    const int pitch = w_pitch(D), Dp = pitch - 4;
    float* ws = reinterpret_cast<float*>(smem);
    float* mu = ws + TK * pitch;   // [Dp], zero beyond D: a padded element stays 0 after the centring
    const int nc = row_chunks<I8>(D);
    const bool aligned = ((uintptr_t)a.rows % 16 == 0) && (I8 ? D % 16 == 0 : D % 4 == 0);
    const size_t row_bytes = (size_t)D * (I8 ? 1 : 4);
    const int pad = I8 ? (int)(0x01010101u * (unsigned)(a.zp & 0xff)) : 0;   // bytes equal to the zero point are 0.0f after the conversion
    const long steps = ((long)a.n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.x * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;
    const int tiles = (R + TK - 1) / TK;
    for (int d = tid; d < Dp; d += 256) mu[d] = (a.mean && d < D) ? a.mean[d] : 0.0f;

    for (int tile = 0; tile < tiles; ++tile) {
        const int c0 = tile * TK;
        if (tile) __syncthreads();   // every wave has left the previous tile
        for (int e = tid; e < TK * Dp; e += 256) {   // stage the tile, zero beyond D and beyond r
            const int c = e / Dp, d = e - c * Dp;
            ws[c * pitch + d] = (c0 + c < R && d < D) ? a.W[(size_t)(c0 + c) * D + d] : 0.0f;
        }
        __syncthreads();

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
                        const int d0 = c * 64 + lk * 16 + g * 4;
                        const f32x4 m = *reinterpret_cast<const f32x4*>(mu + d0);
                        f32x4 af;
#pragma unroll
                        for (int j = 0; j < 4; ++j) af[j] = f_sub((float)((int)(int8_t)(w >> (8 * j)) - a.zp), m[j]);
                        f32x4 b[NT];
#pragma unroll
                        for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(ws + (t * 16 + li) * pitch + d0);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int t = 0; t < NT; ++t) facc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b[t][j], facc[t], 0, 0, 0);
                    }
                } else {
                    const int d0 = c * 16 + lk * 4;
                    const f32x4 x = __builtin_bit_cast(f32x4, av);
                    const f32x4 m = *reinterpret_cast<const f32x4*>(mu + d0);
                    f32x4 af;
#pragma unroll
                    for (int j = 0; j < 4; ++j) af[j] = f_sub(x[j], m[j]);
                    f32x4 b[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(ws + (t * 16 + li) * pitch + d0);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int t = 0; t < NT; ++t) facc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b[t][j], facc[t], 0, 0, 0);
                }
            });

            // ---- facc[t][r]: row tile_row + 4 lk + r against row c0 + 16 t + li of W
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long orow = tile_row + 4 * lk + r;
                if (orow < a.n) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int k = c0 + t * 16 + li;
                        if (k < R) a.out[(size_t)orow * R + k] = facc[t][r];
                    }
                }
            }
        }
    }
}

template <bool I8, int NT>
static bool launch_transform_nt(const PcaTransformArgs& a, const PcaTransformGeom& g, hipStream_t s) {
    const void* kf = (const void*)&pca_transform_kernel<I8, NT>;
    if (g.lds > 64 * 1024 && !ensure_dynamic_lds(kf, g.lds)) return false;
    hipLaunchKernelGGL((pca_transform_kernel<I8, NT>), dim3((unsigned)g.nwg), dim3(256), g.lds, s, a);
    return true;
}

bool launch_pca_transform(const PcaTransformArgs& a, const PcaTransformGeom& g, bool i8, hipStream_t s) {
    if (i8)
        return g.nt == 1 ? launch_transform_nt<true, 1>(a, g, s) : g.nt == 2 ? launch_transform_nt<true, 2>(a, g, s) : g.nt == 4 ? launch_transform_nt<true, 4>(a, g, s)
                                                                                                                                  : launch_transform_nt<true, 8>(a, g, s);
    return g.nt == 1 ? launch_transform_nt<false, 1>(a, g, s) : g.nt == 2 ? launch_transform_nt<false, 2>(a, g, s) : g.nt == 4 ? launch_transform_nt<false, 4>(a, g, s)
                                                                                                                                  : launch_transform_nt<false, 8>(a, g, s);
}

void preload_pca() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&pca_gram_fold_kernel));
}

}  // namespace bn
