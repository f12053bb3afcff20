// bn_select.hip — farthest-first traversal (k-centre greedy) over a matrix of embeddings: which rows to label next.
//
//   select_pass_kernel   one launch per pass over the rows; the kernel boundary is the only barrier between passes.  A pass
//                          1. agrees on its centre c: a forced pass reads d_picked[t]; a greedy pass folds the previous pass's per-workgroup
//                             partials (key, row) — at most BN_SELECT_MAX_WGS pairs — under the total order "key descending, row ascending"
//                             (before() of bn_rowstream.h).  Every workgroup folds the same pairs under the same order, so all agree on c
//                             without talking to each other; workgroup 0 records d_picked[t] and d_key[t].  A pass without a centre (the
//                             first pass of a call without forced rows; a skipped forced entry; no key above -inf) only computes keys.
//                          2. stages row c in LDS (float32 values, or int8 bytes padded with the zero point: at most 8 KiB) and reads inv_c,
//                          3. streams its range of rows (bn_rowstream.h owns the row layout, the padding beyond D, the 16-byte loads and the
//                             slow path for ragged and unaligned rows) against that one centre on the vector ALU.  float32: each of a row's four
//                             lanes runs one fmaf chain over its 16-byte pieces in ascending order, the four chains are added as
//                             (l0 + l1) + (l2 + l3).  int8: v_dot4 sums of byte products and of bytes, exact in int32:
//                             sum (a - z)(b - z) = sum ab - z (sum a + sum b) + Dp z^2 over the Dp padded elements (the padding is z on both sides).
//                          4. s = fl(fl(dot * inv_i) * inv_c); s > m_i replaces (m_i, nearest_i); row c itself becomes (+inf, c).  Then
//                             key_i = fl(u_i * fl(1 - m_i)), -inf for a zero row, a taken row and a NaN.  A running best per lane, then per
//                             wave, then per workgroup: one partial pair per workgroup, the two partial buffers alternating.
//
// A row's state is read and written by the one lane that owns the row; no atomics of any kind: the same inputs give the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_rowstream.h"

namespace bn {
namespace {

static_assert(kStepRows == BN_SELECT_STEP_ROWS, "the public header states the step");
static_assert(BN_SELECT_MAX_WGS % 256 == 0, "a thread folds BN_SELECT_MAX_WGS / 256 partials");
constexpr int kNoRow = 0x7fffffff;
constexpr int kCentreBytes = 8192;   // BN_SEARCH_MAX_D float32 values
static_assert(BN_SEARCH_MAX_D * 4 <= kCentreBytes, "the centre fits its LDS");

enum { kPassKeys = 0, kPassForced = 1, kPassGreedy = 2 };

// the better of (k, i) and the other lanes' pairs, in every lane of the wave
__device__ __forceinline__ void wave_best(float& k, int& i) {
#pragma unroll
    for (int mk = 1; mk < 64; mk <<= 1) {
        const float ok = __shfl_xor(k, mk);
        const int oi = __shfl_xor(i, mk);
        if (before(ok, oi, k, i)) {
            k = ok;
            i = oi;
        }
    }
}

template <bool I8>
__global__ __launch_bounds__(256) void select_pass_kernel(SelectArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char cs[kCentreBytes];
    __shared__ float wk[kWaves];
    __shared__ int wi[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int D = a.D, n = a.n;

    // ---- 1. the centre
    int c = -1;
    if (a.pass == kPassForced) {
        c = a.picked[a.t];
        if (c < 0 || c >= n || a.inv[c] == 0.0f) c = -1;   // (an entry that names no live row is skipped)
    } else if (a.pass == kPassGreedy) {
        float bk = -INFINITY;
        int bi = kNoRow;
#pragma unroll
        for (int j = 0; j < BN_SELECT_MAX_WGS / 256; ++j) {
            const int p = tid + 256 * j;
            if (p < a.nprev) {
                const float k = a.part_key_in[p];
                const int i = a.part_row_in[p];
                if (before(k, i, bk, bi)) {
                    bk = k;
                    bi = i;
                }
            }
        }
        wave_best(bk, bi);
        if (lane == 0) {
            wk[wave] = bk;
            wi[wave] = bi;
        }
        __syncthreads();
        bk = wk[0];
        bi = wi[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (before(wk[w], wi[w], bk, bi)) {
                bk = wk[w];
                bi = wi[w];
            }
        c = (bk > -INFINITY && bi >= 0 && bi < n) ? bi : -1;
        if (blockIdx.x == 0 && tid == 0) {
            a.picked[a.t] = c;
            a.key[a.t] = c >= 0 ? bk : -INFINITY;
        }
        __syncthreads();   // (wk / wi are written again at the end)
    }

    // ---- 2. row c in LDS
    const int nc = row_chunks<I8>(D);
    const int zp = a.zp;
    float cinv = 0.0f;
    int zsum_c = 0;   // int8: z * (the sum of the centre's padded bytes)
    if (c >= 0) {
        cinv = a.inv[c];
        if constexpr (I8) {
            const int8_t* src = (const int8_t*)a.rows + (size_t)c * D;
            for (int e = tid; e < nc * 64; e += 256) cs[e] = (unsigned char)(e < D ? src[e] : (int8_t)zp);
        } else {
            const float* src = (const float*)a.rows + (size_t)c * D;
            for (int e = tid; e < nc * 16; e += 256) reinterpret_cast<float*>(cs)[e] = e < D ? src[e] : 0.0f;
        }
        __syncthreads();
        if constexpr (I8) {
            int sb = 0;
            for (int e = lane; e < nc * 16; e += 64) sb = __builtin_amdgcn_sdot4(reinterpret_cast<const int*>(cs)[e], 0x01010101, sb, false);
#pragma unroll
            for (int mk = 1; mk < 64; mk <<= 1) sb += __shfl_xor(sb, mk);
            zsum_c = zp * sb;
        }
    }

    // ---- 3. and 4. the workgroup's rows
    const bool aligned = ((uintptr_t)a.rows % 16 == 0) && (I8 ? D % 16 == 0 : D % 4 == 0);
    const size_t row_bytes = (size_t)D * (I8 ? 1 : 4);
    const int pad = I8 ? (int)(0x01010101u * (unsigned)(zp & 0xff)) : 0;
    const long steps = ((long)n + kStepRows - 1) / kStepRows;
    const long s0 = (long)blockIdx.x * a.steps_per_wg;
    const long s1 = s0 + a.steps_per_wg < steps ? s0 + a.steps_per_wg : steps;
    float bk = -INFINITY;
    int bi = kNoRow;

    for (long st = s0; st < s1; ++st) {
        const long tile_row = st * kStepRows + wave * 16;
        const long lrow = tile_row + li < n ? tile_row + li : (long)n - 1;   // rows past the end repeat the last one; nothing is written for them
        const bool owner = lk == 0 && tile_row + li < n;
        float m = 0.0f, inv = 0.0f, u = 1.0f;
        if (owner) {
            m = a.m[lrow];
            inv = a.inv[lrow];
            if (a.weight) u = a.weight[lrow];
        }
        float s = 0.0f;
        if (c >= 0) {   // (uniform over the workgroup)
            const RowView<I8> row{(const unsigned char*)a.rows + (size_t)lrow * row_bytes, D, nc, lk, pad, aligned};
            if constexpr (I8) {
                int sab = 0, sa = 0;
                row_stream(row, [&](int ch, v4i av) __attribute__((always_inline)) {
                    const v4i bv = *reinterpret_cast<const v4i*>(cs + ch * 64 + lk * 16);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        sab = __builtin_amdgcn_sdot4(av[g], bv[g], sab, false);
                        sa = __builtin_amdgcn_sdot4(av[g], 0x01010101, sa, false);
                    }
                });
                sab += __shfl_xor(sab, 16);
                sa += __shfl_xor(sa, 16);
                sab += __shfl_xor(sab, 32);
                sa += __shfl_xor(sa, 32);
                const int dot = sab - zp * sa - zsum_c + nc * 64 * zp * zp;
                s = f_mul(f_mul((float)dot, inv), cinv);
            } else {
                float acc = 0.0f;
                row_stream(row, [&](int ch, v4i av) __attribute__((always_inline)) {
                    const f32x4 x = __builtin_bit_cast(f32x4, av);
                    const f32x4 y = *reinterpret_cast<const f32x4*>(cs + ch * 64 + lk * 16);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = fmaf(x[j], y[j], acc);
                });
                acc = f_add(acc, __shfl_xor(acc, 16));   // l0 + l1 | l2 + l3 (a + b and b + a round alike)
                acc = f_add(acc, __shfl_xor(acc, 32));   // (l0 + l1) + (l2 + l3) in all four lanes
                s = f_mul(f_mul(acc, inv), cinv);
            }
        }
        if (owner) {
            const int r = (int)lrow;
            const bool live = inv != 0.0f;
            if (c >= 0 && live) {
                if (r == c) {
                    m = INFINITY;
                    a.m[r] = m;
                    a.nearest[r] = c;
                } else if (m != INFINITY && s > m) {   // (strict: the earlier centre stands on a tie)
                    m = s;
                    a.m[r] = m;
                    a.nearest[r] = c;
                }
            }
            float key = f_mul(u, f_sub(1.0f, m));
            if (!live || m == INFINITY || !(key > -INFINITY)) key = -INFINITY;   // (a NaN key counts as -inf)
            if (before(key, r, bk, bi)) {
                bk = key;
                bi = r;
            }
        }
    }

    wave_best(bk, bi);
    if (lane == 0) {
        wk[wave] = bk;
        wi[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (before(wk[w], wi[w], bk, bi)) {
                bk = wk[w];
                bi = wi[w];
            }
        a.part_key_out[blockIdx.x] = bk;
        a.part_row_out[blockIdx.x] = bi;
    }
}

}  // namespace

// two alternating buffers of BN_SELECT_MAX_WGS (key, row) pairs
size_t select_workspace() { return (size_t)2 * BN_SELECT_MAX_WGS * (sizeof(float) + sizeof(int)); }

void launch_select_run(const void* rows, bool i8, long n, int D, int zp, const float* inv, const float* weight, float* m, int* nearest, int* picked, int forced,
                       int steps, float* key, void* d_work, hipStream_t s) {
    const RowSplit split = split_rows(n, BN_SELECT_MIN_WG_STEPS, BN_SELECT_MAX_WGS);
    float* part_key[2] = {(float*)d_work, (float*)d_work + BN_SELECT_MAX_WGS};
    int* part_row[2] = {(int*)d_work + 2 * BN_SELECT_MAX_WGS, (int*)d_work + 3 * BN_SELECT_MAX_WGS};
    SelectArgs a{};
    a.rows = rows; a.inv = inv; a.weight = weight; a.m = m; a.nearest = nearest; a.picked = picked; a.key = key;
    a.n = (int)n; a.D = D; a.zp = i8 ? zp : 0; a.nprev = split.nwg; a.steps_per_wg = split.steps_per_wg;
    int flip = 0;
    // t = -1: the keys of the given state, for a call whose first pick is a greedy one
    for (int t = forced == 0 ? -1 : 0; t < steps; ++t) {
        a.t = t;
        a.pass = t < 0 ? kPassKeys : t < forced ? kPassForced : kPassGreedy;
        a.part_key_in = part_key[flip]; a.part_row_in = part_row[flip];
        a.part_key_out = part_key[flip ^ 1]; a.part_row_out = part_row[flip ^ 1];
        if (i8)
            hipLaunchKernelGGL(select_pass_kernel<true>, dim3((unsigned)split.nwg), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(select_pass_kernel<false>, dim3((unsigned)split.nwg), dim3(256), 0, s, a);
        flip ^= 1;
    }
}

void preload_select() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&select_pass_kernel<false>));
}

}  // namespace bn
