// bn_search.hip — query by example over a matrix of embeddings: the k best rows per query by cosine or dot score.
//
//   search_inv_norms_kernel  1 / sqrt(sum of squares) per row (0 for a zero row), 16 lanes per row.  An index computes it once per block of
//                            rows and hands it to every search.
//   search_score_kernel      grid (row ranges, query passes).  A workgroup holds a tile of 16 * NT queries in LDS and streams its range of
//                            database rows once, straight into the A operand of the matrix cores (bn_rowstream.h owns the row layout,
//                            the padding beyond D and the prefetch depth; v_mfma_f32_16x16x4_f32: exact float32; v_mfma_i32_16x16x64_i8
//                            on the raw bytes, zero beyond D, the zero point taken out afterwards through row and query sums).  Per
//                            query it keeps the best k (score, row) pairs it has
//                            seen as a sorted list in LDS; the list's last entry is the running threshold, so after the first few hundred
//                            rows almost no score passes it and the list is rarely touched.  Each workgroup writes one partial list.
//   search_merge_kernel      one workgroup per query folds the partial lists into the result.
//
// The order is total: score descending, row index ascending among equal scores.  The best k under a total order are one set whatever
// the order in which rows are offered, so neither the split into workgroups nor the arrival order inside one shows in the result; there
// are no floating-point atomics, and the grid follows from (N, D, Q, k) alone (search_geometry).
//
// Rounding: the float32 dot product is an fmaf chain in the matrix cores (the specification leaves the summation order free); the norm's
// square root and division are the correctly rounded ones (the file is built without fast-math) and the two factors of the cosine are
// applied by f_mul, one rounding each — defined in bn_rowstream.h under a contraction-off pragma that holds for this whole file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

// LDS pitch of a staged query in bytes: the padded row plus 16 bytes, so the 16 queries of a B fragment start four banks apart
__host__ __device__ inline int query_pitch(int D, bool i8) { return i8 ? round_up(D, 64) + 16 : (round_up(D, 16) + 4) * 4; }

// One wave offers up to 64 candidates (one per lane; a NaN score is "none") to a sorted list of k <= 128 entries in LDS that only this
// wave touches.  Unused entries are (-inf, -1) and sort last.  Lane l owns positions l and l + 64: an insertion is one read of every
// position and its left neighbour, then one write.
__device__ __forceinline__ void topk_offer(volatile float* ls, volatile int* lx, int k, float s, int idx) {
    const int lane = threadIdx.x & 63;
    unsigned long long m = __ballot(s == s && before(s, idx, ls[k - 1], lx[k - 1]));
    while (m) {   // (wave-uniform)
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cs = __shfl(s, src);
        const int ci = __shfl(idx, src);
        if (!before(cs, ci, ls[k - 1], lx[k - 1])) continue;   // an earlier insertion raised the threshold
        float ns[2];
        int ni[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            ns[h] = cs;
            ni[h] = ci;
            if (p < k) {
                const float es = ls[p];
                const int ei = lx[p];
                if (before(es, ei, cs, ci)) {
                    ns[h] = es;
                    ni[h] = ei;
                } else if (p > 0) {
                    const float ps = ls[p - 1];
                    const int pi = lx[p - 1];
                    if (!before(ps, pi, cs, ci)) {
                        ns[h] = ps;
                        ni[h] = pi;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < k) {
                ls[p] = ns[h];
                lx[p] = ni[h];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

// ----------------------------------------------------------------------------------------------------------------------- norms
template <bool I8>
__global__ __launch_bounds__(256) void search_inv_norms_kernel(const void* __restrict__ rows, long n, int D, int zp, float* __restrict__ inv) {
    const int l16 = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const long r = row < n ? row : n - 1;   // lanes past the end repeat the last row and drop the result
    float nf;
    if constexpr (I8) {
        const int8_t* p = (const int8_t*)rows + (size_t)r * D;
        int acc = 0;
        for (int d = l16; d < D; d += 16) {
            const int v = (int)p[d] - zp;
            acc += v * v;
        }
        for (int mk = 1; mk < 16; mk <<= 1) acc += __shfl_xor(acc, mk);
        nf = (float)acc;   // exact int32 (D <= 2048: below 2^28), one rounding to float32
    } else {
        const float* p = (const float*)rows + (size_t)r * D;
        float acc = 0.0f;
        for (int d = l16; d < D; d += 16) acc = f_add(acc, f_mul(p[d], p[d]));
        for (int mk = 1; mk < 16; mk <<= 1) acc = f_add(acc, __shfl_xor(acc, mk));
        nf = acc;
    }
    if (l16 == 0 && row < n) inv[row] = nf == 0.0f ? 0.0f : f_div(1.0f, sqrtf(nf));
}

void launch_search_inv_norms(const void* rows, bool i8, long n, int D, int zp, float* inv, hipStream_t s) {
    const dim3 grid((unsigned)((n + 15) / 16));
    if (i8)
        hipLaunchKernelGGL(search_inv_norms_kernel<true>, grid, dim3(256), 0, s, rows, n, D, zp, inv);
    else
        hipLaunchKernelGGL(search_inv_norms_kernel<false>, grid, dim3(256), 0, s, rows, n, D, zp, inv);
}

// --------------------------------------------------------------------------------------------------------------------- scoring
// LDS: queries [QP][pitch] | list scores [QP][k] | list rows [QP][k] | score tiles [4][16][QP + 1] | flags [2][QP + 4]
size_t search_lds_bytes(int D, int k, bool i8, int nt) {
    const int QP = 16 * nt;
    return (size_t)QP * query_pitch(D, i8) + (size_t)QP * k * 8 + (size_t)kWaves * 16 * (QP + 1) * 4 + 2 * (QP + 4) * 4;
}

bool search_geometry(long n, int D, int Q, int k, bool i8, SearchGeom* g) {
    int nt = Q <= 16 ? 1 : Q <= 32 ? 2 : 4;
    while (nt > 1 && search_lds_bytes(D, k, i8, nt) > BN_SEARCH_LDS_BYTES) nt >>= 1;
    if (search_lds_bytes(D, k, i8, nt) > BN_SEARCH_LDS_BYTES) return false;
    const RowSplit split = split_rows(n, BN_SEARCH_MIN_WG_STEPS, BN_SEARCH_MAX_WGS);
    g->nt = nt;
    g->steps_per_wg = split.steps_per_wg;
    g->nwg = split.nwg;
    g->lds = search_lds_bytes(D, k, i8, nt);
    return true;
}

template <bool I8, int NT>
__global__ __launch_bounds__(256) void search_score_kernel(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int QP = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, k = a.k;
    const int pitch = query_pitch(D, I8);
    unsigned char* qs = smem;
    float* ls = reinterpret_cast<float*>(smem + (size_t)QP * pitch);
    int* lx = reinterpret_cast<int*>(ls + QP * k);
    float* tiles = reinterpret_cast<float*>(lx + QP * k);
    int* flags = reinterpret_cast<int*>(tiles + kWaves * 16 * (QP + 1));   // [2][QP + 4]: per query, then per wave
    const int q0 = blockIdx.y * QP;   // first query of this workgroup within the launch

    // ---- stage the queries (zero beyond D and beyond Q), empty lists, clear flags
    if constexpr (I8) {
        const int Dp = pitch - 16;
        const int8_t* src = (const int8_t*)a.q;
        for (int e = tid; e < QP * Dp; e += 256) {
            const int q = e / Dp, d = e - q * Dp;
            qs[q * pitch + d] = (q0 + q < a.Q && d < D) ? (unsigned char)src[(size_t)(q0 + q) * D + d] : 0;
        }
    } else {
        const int Dp = pitch / 4 - 4;
        const float* src = (const float*)a.q;
        for (int e = tid; e < QP * Dp; e += 256) {
            const int q = e / Dp, d = e - q * Dp;
            reinterpret_cast<float*>(qs + q * pitch)[d] = (q0 + q < a.Q && d < D) ? src[(size_t)(q0 + q) * D + d] : 0.0f;
        }
    }
    for (int e = tid; e < QP * k; e += 256) {
        ls[e] = -INFINITY;
        lx[e] = -1;
    }
    if (tid < 2 * (QP + 4)) flags[tid] = 0;
    __syncthreads();

    // ---- per lane: its query of every tile
    float qinv[NT];
    int qgrp[NT], qcorr[NT];
    bool qok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int q = q0 + t * 16 + li;
        qok[t] = q < a.Q;
        qinv[t] = (a.cosine && qok[t]) ? a.q_inv[q] : 1.0f;
        qgrp[t] = (a.q_group && qok[t]) ? a.q_group[q] : 0;
        qcorr[t] = 0;
    }
    const int nc = row_chunks<I8>(D);
    if constexpr (I8) {   // dot of centred bytes = sum a b - zp (sum a + sum b) + D zp^2: the query's share of it, once
        const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v4i acc = {0, 0, 0, 0};
            for (int c = 0; c < nc; ++c)
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, *reinterpret_cast<const v4i*>(qs + (t * 16 + li) * pitch + c * 64 + lk * 16), acc, 0, 0, 0);
            qcorr[t] = D * a.zp * a.zp - a.zp * acc[0];
        }
    }

    const bool aligned = ((uintptr_t)a.db % 16 == 0) && (I8 ? D % 16 == 0 : D % 4 == 0);
    const size_t row_bytes = (size_t)D * (I8 ? 1 : 4);
    const long steps = ((long)a.n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.x * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;

    for (long st = s0; st < s1; ++st) {
        const long tile_row = st * kStepRows + wave * 16;
        const long lrow = tile_row + li < a.n ? tile_row + li : (long)a.n - 1;   // rows past the end repeat the last one; their scores are dropped below
        const RowView<I8> row{(const unsigned char*)a.db + (size_t)lrow * row_bytes, D, nc, lk, 0, aligned};   // zero beyond D

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
                    iacc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, *reinterpret_cast<const v4i*>(qs + (t * 16 + li) * pitch + c * 64 + lk * 16), iacc[t], 0, 0, 0);
            } else {
                const f32x4 af = __builtin_bit_cast(f32x4, av);
                f32x4 b[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(qs + (t * 16 + li) * pitch + (c * 16 + lk * 4) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t = 0; t < NT; ++t) facc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b[t][j], facc[t], 0, 0, 0);
            }
        });

        // ---- scores of rows tile_row + 4 lk + r against queries t * 16 + li; which of them pass the query's threshold
        int* fl = flags + (int)(st & 1) * (QP + 4);
        float sc[NT][4];
        bool any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = tile_row + 4 * lk + r;
            const bool rok = row < a.n;
            const float rinv = (a.cosine && rok) ? a.db_inv[row] : 1.0f;
            const int rgrp = (a.db_group && rok) ? a.db_group[row] : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float s;
                if constexpr (I8)
                    s = (float)(iacc[t][r] - a.zp * rsum[r] + qcorr[t]);
                else
                    s = facc[t][r];
                if (a.cosine) s = f_mul(f_mul(s, qinv[t]), rinv);
                const bool ok = rok && qok[t] && !(a.db_group && rgrp == qgrp[t]);
                const int q = t * 16 + li;
                const bool c = ok && before(s, (int)row, ls[q * k + k - 1], lx[q * k + k - 1]);
                if (c) fl[q] = 1;
                any |= c;
                sc[t][r] = ok ? s : __builtin_nanf("");
            }
        }
        if (__any(any)) {   // the wave leaves its score tile for the merge below
            float* tl = tiles + wave * 16 * (QP + 1);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < NT; ++t) tl[(4 * lk + r) * (QP + 1) + t * 16 + li] = sc[t][r];
            if (lane == 0) fl[QP + wave] = 1;
        }
        __syncthreads();
        // Flags of step parity p are written before this barrier and read behind it; the next step writes the other parity, and the step
        // after that comes behind the next barrier — so one barrier per step is enough when nothing passed a threshold.
        const bool work = fl[QP] | fl[QP + 1] | fl[QP + 2] | fl[QP + 3];   // (workgroup-uniform)
        if (work) {
            for (int q = wave; q < QP; q += kWaves) {
                if (!fl[q]) continue;
                for (int w = 0; w < kWaves; ++w) {
                    if (!fl[QP + w]) continue;
                    const float s = lane < 16 ? tiles[(w * 16 + lane) * (QP + 1) + q] : __builtin_nanf("");
                    topk_offer(ls + q * k, lx + q * k, k, s, (int)(st * kStepRows + w * 16 + lane));
                }
            }
            __syncthreads();
            if (tid < QP + 4) fl[tid] = 0;
        }
    }

    __syncthreads();
    for (int e = tid; e < QP * k; e += 256) {
        const int q = e / k, j = e - q * k;
        if (q0 + q < a.Q) {
            const size_t o = ((size_t)(q0 + q) * gridDim.x + blockIdx.x) * k + j;
            a.part_score[o] = ls[e];
            a.part_idx[o] = lx[e];
        }
    }
}

template <bool I8, int NT>
static bool launch_score_nt(const SearchArgs& a, const SearchGeom& g, int passes, hipStream_t s) {
    const void* kf = (const void*)&search_score_kernel<I8, NT>;
    if (g.lds > 64 * 1024 && !ensure_dynamic_lds(kf, g.lds)) return false;
    hipLaunchKernelGGL((search_score_kernel<I8, NT>), dim3((unsigned)g.nwg, (unsigned)passes), dim3(256), g.lds, s, a);
    return true;
}

bool launch_search_scores(const SearchArgs& a, const SearchGeom& g, bool i8, hipStream_t s) {
    const int passes = (a.Q + 16 * g.nt - 1) / (16 * g.nt);
    if (i8) return g.nt == 1 ? launch_score_nt<true, 1>(a, g, passes, s) : g.nt == 2 ? launch_score_nt<true, 2>(a, g, passes, s) : launch_score_nt<true, 4>(a, g, passes, s);
    return g.nt == 1 ? launch_score_nt<false, 1>(a, g, passes, s) : g.nt == 2 ? launch_score_nt<false, 2>(a, g, passes, s) : launch_score_nt<false, 4>(a, g, passes, s);
}

// ----------------------------------------------------------------------------------------------------------------------- merge
// Workgroup q: each of its four waves folds a quarter of query q's partial entries into a list of its own (four loads per lane in flight),
// then wave 0 folds the other three lists into its own and writes the result.
__global__ __launch_bounds__(256) void search_merge_kernel(const float* __restrict__ part_score, const int* __restrict__ part_idx, int nwg, int k,
                                                           int* __restrict__ out_idx, float* __restrict__ out_score) {
    __shared__ float ls[kWaves][BN_SEARCH_MAX_K];
    __shared__ int lx[kWaves][BN_SEARCH_MAX_K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t q = blockIdx.x;
    for (int e = lane; e < k; e += 64) {
        ls[wave][e] = -INFINITY;
        lx[wave][e] = -1;
    }
    __builtin_amdgcn_wave_barrier();
    const long total = (long)nwg * k;
    const float* ps = part_score + q * total;
    const int* pi = part_idx + q * total;
    for (long base = (long)wave * 256; base < total; base += kWaves * 256) {   // (wave-uniform)
        float s[4];
        int ix[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long e = base + u * 64 + lane;
            s[u] = e < total ? ps[e] : __builtin_nanf("");
            ix[u] = e < total ? pi[e] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) topk_offer(ls[wave], lx[wave], k, s[u], ix[u]);
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < kWaves; ++w)
            for (int e0 = 0; e0 < k; e0 += 64) {
                const int e = e0 + lane;
                topk_offer(ls[0], lx[0], k, e < k ? ls[w][e] : __builtin_nanf(""), e < k ? lx[w][e] : -1);
            }
        for (int e = lane; e < k; e += 64) {
            out_idx[q * k + e] = lx[0][e];
            out_score[q * k + e] = ls[0][e];
        }
    }
}

void launch_search_merge(const float* part_score, const int* part_idx, int nwg, int Q, int k, int* out_idx, float* out_score, hipStream_t s) {
    hipLaunchKernelGGL(search_merge_kernel, dim3((unsigned)Q), dim3(256), 0, s, part_score, part_idx, nwg, k, out_idx, out_score);
}

void preload_search() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&search_merge_kernel));
}

}  // namespace bn
