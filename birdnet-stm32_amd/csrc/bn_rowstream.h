// bn_rowstream.h — streaming the rows of an [n, D] matrix of float32 or int8 embeddings into an operand of the matrix cores, shared by
// the five kernels that do it (search_score_kernel in bn_search.hip, kmeans_assign_kernel in bn_kmeans.hip, silhouette_means_kernel in bn_silhouette.hip, density_nearest_kernel in bn_density.hip, head_i8_kernel in bn_head_i8.hip).  It owns the row layout, the
// padding rule and the prefetch depth; the kernels keep the tile of the other operand, their MFMA body and their
// epilogue (search, k-means, silhouette and density take the rows as the A operand; the head takes them as B, a lane's 16 bytes being the same either way).
//
// Layout: a step is 64 rows, one 16-row MFMA tile per wave; lane (li, lk) of a wave reads row li of the tile.  A row is cut into chunks of
// 64 bytes, of which the lane takes the 16 at 16 lk: elements 64 c + 16 lk .. + 15 (int8) or 16 c + 4 lk .. + 3 (float32) of chunk c.
// Padding: whatever lies beyond D reads as the caller's pad word.  Prefetch: the loads of the next kGroup chunks are in flight while the
// current kGroup are used.
#pragma once
#include "../../include/birdnet_hip.h"
#include "bn_device.h"

// From here to the end of the including translation unit: every float32 operation is rounded on its own.  The includers want that for
// their whole file (the specifications they are tested against count the roundings).
#pragma clang fp contract(off)

namespace bn {
namespace {

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// (s, i) comes before (ts, ti) in the total order: score descending, index ascending among equal scores
__device__ __forceinline__ bool before(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

constexpr int kWaves = 4;       // waves per streaming workgroup, one 16-row tile each per step
constexpr int kStepRows = 64;   // rows of a step
constexpr int kGroup = 4;       // chunks of a row tile whose loads are in flight together
static_assert(kStepRows == 16 * kWaves, "a step is one MFMA row tile per wave");
static_assert(kStepRows == BN_SEARCH_STEP_ROWS && kStepRows == BN_KMEANS_STEP_ROWS && kStepRows == BN_HEAD_I8_STEP_ROWS, "the public header states the step of every kernel");

// chunks of a row: 64 bytes each, the last one padded
template <bool I8>
__host__ __device__ inline int row_chunks(int D) {
    return I8 ? round_up(D, 64) / 64 : round_up(D, 16) / 16;
}

// The deal of the n rows' steps to workgroups: at least min_steps_per_wg steps each (while there are that many), at most max_wgs
// workgroups, none of them without a step.  Workgroup b takes steps [b, b + 1) * steps_per_wg.
struct RowSplit {
    long steps_per_wg;
    int nwg;
};
inline RowSplit split_rows(long n, int min_steps_per_wg, int max_wgs) {
    const long steps = (n + kStepRows - 1) / kStepRows;
    long wgs = (steps + min_steps_per_wg - 1) / min_steps_per_wg;
    wgs = wgs < 1 ? 1 : wgs > max_wgs ? max_wgs : wgs;
    const long per = steps > 0 ? (steps + wgs - 1) / wgs : 1;
    return {per, steps > 0 ? (int)((steps + per - 1) / per) : 1};
}

// One lane's view of its row.  `aligned`: the matrix starts on a 16-byte boundary and so does every row (D % 16 == 0 for int8, D % 4 == 0
// for float32); the float32 rows are 4-byte aligned in any case (the C ABI demands it).
template <bool I8>
struct RowView {
    const unsigned char* rp;   // the lane's row
    int D, nc, lk;             // nc = row_chunks<I8>(D)
    int pad;                   // the word read beyond D: 0, or an int8 zero point in each of its bytes
    bool aligned;

    // chunk c of the row, as the 16 bytes of the lane; the pad word for c >= nc (the prefetch asks one group ahead)
    __device__ __forceinline__ v4i load(int c) const {
        const v4i padded = {pad, pad, pad, pad};
        if (c >= nc) return padded;
        if constexpr (I8) {
            const int d0 = c * 64 + lk * 16;
            if (aligned && d0 + 16 <= D) return *reinterpret_cast<const v4i*>(rp + d0);
            unsigned w[4] = {(unsigned)pad, (unsigned)pad, (unsigned)pad, (unsigned)pad};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (d0 + j < D) w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((unsigned)rp[d0 + j] << (8 * (j & 3)));
            return v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        } else {
            const int d0 = c * 16 + lk * 4;
            if (aligned && d0 + 4 <= D) return *reinterpret_cast<const v4i*>(rp + (size_t)d0 * 4);
            int w[4] = {pad, pad, pad, pad};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (d0 + j < D) w[j] = reinterpret_cast<const int*>(rp)[d0 + j];
            return v4i{w[0], w[1], w[2], w[3]};
        }
    }
};

// use(c, chunk c of the row) for c = 0 .. nc - 1 in order.  `use` is wave-uniform in c (every lane of a wave has the same nc), so it may
// issue MFMAs.  A float32 user casts the whole vector, __builtin_bit_cast(f32x4, v): the cast of one element, v[j], read element 0 for every j.
template <bool I8, class Use>
__device__ __forceinline__ void row_stream(const RowView<I8>& row, Use&& use) {
    v4i cur[kGroup], nxt[kGroup];
#pragma unroll
    for (int u = 0; u < kGroup; ++u) cur[u] = row.load(u);
    for (int c0 = 0; c0 < row.nc; c0 += kGroup) {
#pragma unroll
        for (int u = 0; u < kGroup; ++u) nxt[u] = row.load(c0 + kGroup + u);
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
            if (c0 + u < row.nc) use(c0 + u, cur[u]);   // (wave-uniform)
#pragma unroll
        for (int u = 0; u < kGroup; ++u) cur[u] = nxt[u];
    }
}

}  // namespace
}  // namespace bn
