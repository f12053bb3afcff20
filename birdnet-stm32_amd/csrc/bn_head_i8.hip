// bn_head_i8.hip — the INT8 classifier head of an exported model over resident int8 embedding rows: what the
// FULLY_CONNECTED [-> LOGISTIC] -> DEQUANTIZE tail of the .tflite computes, without running the backbone again.
//
//   head_i8_kernel   grid (row ranges, class passes).  A workgroup holds the class tiles of its pass in LDS — 16 zero-padded int8 weight
//                    rows per tile, an operand of v_mfma_i32_16x16x64_i8, next to the tiles' bias / multiplier / shift and the LOGISTIC
//                    table — and streams its range of rows once from memory (bn_rowstream.h owns the row layout, the zero beyond D and the
//                    prefetch depth).  The tiles of a pass are taken NT at a time: a step's rows are streamed once per group of NT tiles, from
//                    the cache after the first.  The class tile is the A operand, so a lane holds four neighbouring classes of one row
//                    and stores them at once.  Per element: mbqm(acc + bias) + zp_out, clamp, then the byte and (sigmoid) the table's
//                    byte as (q + 128) / 256.  The bias holds -z_in * sum(w) (the lowering's fold for i8_fc_kernel), so the raw bytes go
//                    into the matrix cores as they are.
//
// A softmax head stops at the logit bytes; the model's own i8_head_softmax_kernel (bn_i8.hip) turns them into scores, so the arithmetic
// is the exported model's by construction.  The requantisation is mbqm of bn_requant.h: the caller proves its domain per class
// (conversion/head_export.py: quantize_head refuses a head whose accumulators can leave it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_requant.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

// LDS bytes of one class tile: 16 weight rows of Kp bytes at a pitch of Kp + 16 (the 16 classes of a fragment start four banks apart,
// as search_score_kernel's queries do), then bias, multiplier and shift of its 16 classes
__host__ __device__ inline int head_pitch(int D) { return round_up(D, 64) + 16; }
__host__ __device__ inline int head_tile_bytes(int D) { return 16 * head_pitch(D) + 3 * 16 * 4; }
constexpr int kLutBytes = 256;

}  // namespace

bool head_i8_geometry(long n, int D, int C, HeadI8Geom* g) {
    const int tiles = (C + 15) / 16;
    const int cap = (BN_HEAD_I8_LDS_BYTES - kLutBytes) / head_tile_bytes(D);
    if (cap < 1) return false;
    int nt = 1;
    while (nt < 8 && nt < tiles && 2 * nt <= cap) nt *= 2;
    const int want = round_up(tiles, nt), fit = cap / nt * nt;
    g->nt = nt;
    g->pass_tiles = want < fit ? want : fit;
    g->passes = (tiles + g->pass_tiles - 1) / g->pass_tiles;
    const RowSplit split = split_rows(n, BN_HEAD_I8_MIN_WG_STEPS, BN_HEAD_I8_MAX_WGS);
    g->steps_per_wg = split.steps_per_wg;
    g->nwg = split.nwg;
    g->lds = (size_t)g->pass_tiles * head_tile_bytes(D) + kLutBytes;
    return true;
}

namespace {

template <int NT>
__global__ __launch_bounds__(256) void head_i8_kernel(HeadI8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, C = a.C;
    const int Kp = round_up(D, 64), pitch = Kp + 16;
    const int PC = a.pass_tiles * 16;   // classes of a pass, the padded ones included
    unsigned char* ws = smem;           // [PC][pitch]
    int* bias = reinterpret_cast<int*>(smem + (size_t)PC * pitch);
    int* mult = bias + PC;
    int* shift = mult + PC;
    const int8_t* lut = reinterpret_cast<const int8_t*>(shift + PC);
    const int c0 = blockIdx.y * PC;     // first class of this pass

    // ---- stage the pass: weights (zero rows beyond C), requantisation constants, table
    {
        const int vr = Kp / 16;   // 16-byte vectors of a weight row
        for (int e = tid; e < PC * vr; e += 256) {
            const int q = e / vr, j = e - q * vr;
            v4i v = {0, 0, 0, 0};
            if (c0 + q < C) v = *reinterpret_cast<const v4i*>(a.w + (size_t)(c0 + q) * Kp + j * 16);
            *reinterpret_cast<v4i*>(ws + q * pitch + j * 16) = v;
        }
        for (int q = tid; q < PC; q += 256) {
            const bool ok = c0 + q < C;
            bias[q] = ok ? a.bias[c0 + q] : 0;
            mult[q] = ok ? a.mult[c0 + q] : 0;
            shift[q] = ok ? a.shift[c0 + q] : 0;
        }
        if (a.lut && tid < kLutBytes / 4) reinterpret_cast<int*>(shift + PC)[tid] = reinterpret_cast<const int*>(a.lut)[tid];
    }
    __syncthreads();

    const int nc = row_chunks<true>(D);
    const bool aligned = ((uintptr_t)a.rows % 16 == 0) && D % 16 == 0;
    const long steps = (a.n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.x * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;
    const int groups = a.pass_tiles / NT;

    for (long st = s0; st < s1; ++st) {
        const long tile_row = st * kStepRows + wave * 16;
        const long lrow = tile_row + li < a.n ? tile_row + li : a.n - 1;   // rows past the end repeat the last one; nothing of them is stored
        const RowView<true> row{(const unsigned char*)a.rows + (size_t)lrow * D, D, nc, lk, 0, aligned};   // zero beyond D
        for (int g = 0; g < groups; ++g) {
            const int q0 = g * NT * 16;          // first class of the group within the pass
            if (c0 + q0 >= C) break;             // (workgroup-uniform) the pass's last groups may be padding only
            const unsigned char* wg = ws + (size_t)(q0 + li) * pitch + lk * 16;
            v4i acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = v4i{0, 0, 0, 0};
            // the class tile is the A operand and the rows the B operand (a lane's 16 bytes are the same either way), so a lane ends up
            // with four neighbouring classes of ONE row: one 16-byte store of scores, one 4-byte store of logit bytes
            row_stream(row, [&](int c, v4i av) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(wg + t * 16 * pitch + c * 64), av, acc[t], 0, 0, 0);
            });
            // ---- row tile_row + li, classes c0 + q0 + 16 t + 4 lk + r
            const long orow = tile_row + li;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int q = q0 + t * 16 + 4 * lk, cls = c0 + q;
                const v4i b = *reinterpret_cast<const v4i*>(bias + q), m = *reinterpret_cast<const v4i*>(mult + q), sh = *reinterpret_cast<const v4i*>(shift + q);
                int qv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) qv[r] = clampi(mbqm(acc[t][r] + b[r], m[r], sh[r]) + a.zp_out, -128, 127);
                if (orow >= a.n || cls >= C) continue;
                const size_t o = (size_t)orow * C + cls;
                if (a.wide) {   // C % 4 == 0: the quad is whole and its stores are aligned
                    if (a.logit) *reinterpret_cast<int*>(a.logit + o) = pack4(qv);
                    if (a.lut) {
                        f32x4 sc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[r] = (float)((int)lut[qv[r] + 128] + 128) * (1.0f / 256.0f);
                        *reinterpret_cast<f32x4*>(a.scores + o) = sc;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (cls + r < C) {
                            if (a.logit) a.logit[o + r] = (int8_t)qv[r];
                            if (a.lut) a.scores[o + r] = (float)((int)lut[qv[r] + 128] + 128) * (1.0f / 256.0f);
                        }
                }
            }
        }
    }
}

template <int NT>
bool launch_nt(const HeadI8Args& a, const HeadI8Geom& g, hipStream_t s) {
    const void* kf = (const void*)&head_i8_kernel<NT>;
    if (g.lds > 64 * 1024 && !ensure_dynamic_lds(kf, g.lds)) return false;
    hipLaunchKernelGGL((head_i8_kernel<NT>), dim3((unsigned)g.nwg, (unsigned)g.passes), dim3(256), g.lds, s, a);
    return true;
}

}  // namespace

bool launch_head_i8(const HeadI8Args& a, const HeadI8Geom& g, hipStream_t s) {
    return g.nt == 1 ? launch_nt<1>(a, g, s) : g.nt == 2 ? launch_nt<2>(a, g, s) : g.nt == 4 ? launch_nt<4>(a, g, s) : launch_nt<8>(a, g, s);
}

void preload_head_i8() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&head_i8_kernel<1>));
}

}  // namespace bn
