// bn_indices.hip — acoustic indices of raw STFT magnitudes: one chunk's spectrogram S [257, W] in, eight scalars and three values per bin
// out (birdnet_stm32/evaluation/indices.py is the specification).
//
//   acoustic_indices_kernel   one workgroup of four waves per chunk, one pass over the chunk's 257 x W floats, every element read once.
//
// A wave takes whole bins (bin = wave, wave + 4, ...).  Lane l holds the 16-byte piece [4 l + 256 j, 4 l + 256 j + 4) of the row for
// j = 0 .. ceil(W / 256) - 1: one wide load per piece where every row starts on a 16-byte boundary (the chunk does and W % 4 == 0), four
// guarded scalar loads otherwise, and the same arithmetic in the same order behind either, so both give the same bits.  The neighbour in
// time of a piece's first element is the last element of the lane below; lane 0 takes lane 63's from the previous piece.  Per bin the
// wave folds r_f = sum S, p_f = sum P, sum |dS|, sum P ln P and the integer count of cells above the threshold inside itself
// (lane order, then a xor tree), and 1 - H(P[f, :]) needs no second pass: -sum q ln q = ln p_f - (sum P ln P) / p_f.  Each wave keeps the
// column energies of its own bins in registers (four per piece), so e_t costs no traffic until the end.
//
// Per-bin results and the four waves' column partials meet in LDS; wave 0 then computes the eight scalars (entropies the direct way,
// q = v / sum v, over the values in LDS) and all four waves write the per-bin block.  No atomics: the same input gives the same bits on
// every run.  Counts are integers.  Divisions whose operands are exact for integer-valued magnitudes (ACI_f, CVR_f, NDSI) are single
// correctly rounded float32 divisions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/birdnet_hip.h"
#include "bn_device.h"
#include "bn_kernels.h"

namespace bn {
namespace {

constexpr int kBins = BN_INDICES_BINS;            // 257
constexpr int kWaves = 4;
constexpr int kPiece = 256;                       // floats a wave covers with one piece per lane
constexpr int kMaxPieces = BN_INDICES_MAX_W / kPiece;   // 4
constexpr int kBands = BN_INDICES_MAX_BANDS;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// -sum q ln q over v[0 .. n), q = v / total, by the lanes of one wave; 0 when total is 0
__device__ __forceinline__ float wave_entropy(const float* v, int n, int lane) {
    float s = 0.0f;
    for (int i = lane; i < n; i += 64) s += v[i];
    const float total = wave_sum(s);
    if (!(total > 0.0f)) return 0.0f;
    float h = 0.0f;
    for (int i = lane; i < n; i += 64) {
        const float q = f_div(v[i], total);
        if (q > 0.0f) h -= q * logf(q);
    }
    return wave_sum(h);
}

template <bool kWide>
__device__ __forceinline__ f32x4 load_piece(const float* __restrict__ row, int t0, int W) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kWide) {   // W % 4 == 0: a piece is inside the row or outside it
        if (t0 < W) v = *reinterpret_cast<const f32x4*>(row + t0);
    } else {
        if (t0 < W) v.x = row[t0];
        if (t0 + 1 < W) v.y = row[t0 + 1];
        if (t0 + 2 < W) v.z = row[t0 + 2];
        if (t0 + 3 < W) v.w = row[t0 + 3];
    }
    return v;
}

template <bool kWide>
__global__ __launch_bounds__(256) void acoustic_indices_kernel(const float* __restrict__ spec, const float* __restrict__ minmax, int W,
                                                               bn_indices_params prm, float* __restrict__ out, float* __restrict__ spectral) {
    __shared__ __attribute__((aligned(16))) float ecol[kWaves][BN_INDICES_MAX_W];   // the waves' column energies; row 0 becomes e_t
    __shared__ float s_p[kBins], s_aci[kBins], s_ent[kBins];
    __shared__ int s_cnt[kBins];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const float* chunk = spec + b * (size_t)kBins * W;
    const float smax = minmax[2 * b + 1];
    const float thr = f_mul(smax, prm.cover_ratio);
    const float ln_w = logf((float)W);
    const int pieces = (W + kPiece - 1) / kPiece;

    f32x4 e[kMaxPieces];
#pragma unroll
    for (int j = 0; j < kMaxPieces; ++j) e[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    f32x4 next = load_piece<kWide>(chunk + (size_t)wave * W, 4 * lane, W);
    for (int f = wave; f < kBins; f += kWaves) {
        const float* row = chunk + (size_t)f * W;
        const f32x4 first = next;
        if (f + kWaves < kBins) next = load_piece<kWide>(row + (size_t)kWaves * W, 4 * lane, W);   // the next bin's first piece, in flight meanwhile
        float r = 0.0f, p = 0.0f, d = 0.0f, plnp = 0.0f, last = 0.0f;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kMaxPieces; ++j) {
            if (j < pieces) {   // (uniform)
                const int t0 = kPiece * j + 4 * lane;
                const f32x4 v = j == 0 ? first : load_piece<kWide>(row, t0, W);
                float left = __shfl_up(v.w, 1);
                const float wrap = __shfl(last, 63);
                if (lane == 0) left = wrap;
                last = v.w;
                const bool m0 = t0 < W, m1 = t0 + 1 < W, m2 = t0 + 2 < W, m3 = t0 + 3 < W;   // (elements outside the row were loaded as 0)
                r += v.x; r += v.y; r += v.z; r += v.w;
                const f32x4 q = {f_mul(v.x, v.x), f_mul(v.y, v.y), f_mul(v.z, v.z), f_mul(v.w, v.w)};
                p += q.x; p += q.y; p += q.z; p += q.w;
                if (m0 && t0 > 0) d += __builtin_fabsf(f_sub(v.x, left));
                if (m1) d += __builtin_fabsf(f_sub(v.y, v.x));
                if (m2) d += __builtin_fabsf(f_sub(v.z, v.y));
                if (m3) d += __builtin_fabsf(f_sub(v.w, v.z));
                if (q.x > 0.0f) plnp += q.x * logf(q.x);
                if (q.y > 0.0f) plnp += q.y * logf(q.y);
                if (q.z > 0.0f) plnp += q.z * logf(q.z);
                if (q.w > 0.0f) plnp += q.w * logf(q.w);
                cnt += (m0 && v.x > thr) + (m1 && v.y > thr) + (m2 && v.z > thr) + (m3 && v.w > thr);
                e[j] += q;
            }
        }
        r = wave_sum(r);
        p = wave_sum(p);
        d = wave_sum(d);
        plnp = wave_sum(plnp);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            s_p[f] = p;
            s_cnt[f] = cnt;
            s_aci[f] = r > 0.0f ? f_div(d, r) : 0.0f;
            s_ent[f] = p > 0.0f ? 1.0f - (logf(p) - f_div(plnp, p)) / ln_w : 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxPieces; ++j)
        if (j < pieces) *reinterpret_cast<f32x4*>(&ecol[wave][kPiece * j + 4 * lane]) = e[j];   // (256 j + 4 lane + 3 <= 1023)
    __syncthreads();

    if (spectral) {
        float* sp = spectral + b * (size_t)(3 * kBins);
        const float fw = (float)W;
        for (int f = tid; f < kBins; f += 256) {
            sp[f] = s_aci[f];
            sp[kBins + f] = s_ent[f];
            sp[2 * kBins + f] = f_div((float)s_cnt[f], fw);
        }
    }
    if (wave != 0) return;

    // ---- the eight scalars, by wave 0
    for (int t = lane; t < W; t += 64) ecol[0][t] = ((ecol[0][t] + ecol[1][t]) + ecol[2][t]) + ecol[3][t];
    wave_sync();
    const float ht = f_div(wave_entropy(ecol[0], W, lane), ln_w);
    const float hf = f_div(wave_entropy(s_p, kBins, lane), logf((float)kBins));
    float aci = 0.0f, pa = 0.0f, pb = 0.0f;
    for (int f = lane; f < kBins; f += 64) {
        aci += s_aci[f];
        if (f >= prm.anthro_k0 && f < prm.anthro_k1) pa += s_p[f];
        if (f >= prm.bio_k0 && f < prm.bio_k1) pb += s_p[f];
    }
    aci = wave_sum(aci);
    pa = wave_sum(pa);
    pb = wave_sum(pb);
    const float both = f_add(pa, pb);
    const float ndsi = both > 0.0f ? f_div(f_sub(pb, pa), both) : 0.0f;

    float bi = 0.0f;
    if (smax > 0.0f) {
        const float floor_p = 1e-12f * smax * smax, fw = (float)W;
        float lo = __builtin_inff();
        // (individually rounded: a level fused into its subtraction would differ from the same level inside the minimum)
        for (int f = prm.bio_k0 + lane; f < prm.bio_k1; f += 64) lo = fminf(lo, f_mul(10.0f, log10f(fmaxf(f_div(s_p[f], fw), floor_p))));
        lo = wave_min(lo);
        for (int f = prm.bio_k0 + lane; f < prm.bio_k1; f += 64) bi += f_sub(f_mul(10.0f, log10f(fmaxf(f_div(s_p[f], fw), floor_p))), lo);
        bi = wave_sum(bi) * prm.df_khz;
    }

    // ADI and AEI: lane b < n_bands holds its band's share of cells above the threshold
    const int nb = prm.n_bands;
    float c = 0.0f;
    if (lane < nb) {
        const int k0 = prm.band_edge[lane], k1 = prm.band_edge[lane + 1];
        int n = 0;
        for (int f = k0; f < k1; ++f) n += s_cnt[f];
        if (k1 > k0) c = f_div((float)n, (float)((k1 - k0) * W));
    }
    const float total = wave_sum(c);
    float adi = 0.0f, aei = 0.0f;
    if (total > 0.0f) {
        const float q = f_div(c, total);
        adi = wave_sum(q > 0.0f ? -q * logf(q) : 0.0f);
        int rank = 0;   // position in ascending order, equal values in band order
#pragma unroll
        for (int j = 0; j < kBands; ++j) {
            const float cj = __shfl(c, j);
            if (j < nb && (cj < c || (cj == c && j < lane))) ++rank;
        }
        const float weighted = wave_sum(lane < nb ? (float)(rank + 1) * c : 0.0f);
        const float fn = (float)nb;
        aei = 2.0f * weighted / (fn * total) - (fn + 1.0f) / fn;
    }
    if (lane == 0) {
        float* o = out + b * (size_t)BN_INDICES_SCALARS;
        o[0] = aci;
        o[1] = hf;
        o[2] = ht;
        o[3] = f_mul(hf, ht);
        o[4] = ndsi;
        o[5] = bi;
        o[6] = adi;
        o[7] = aei;
    }
}

}  // namespace

void launch_acoustic_indices(const float* spec, const float* minmax, int B, int W, const bn_indices_params& prm, float* out, float* spectral,
                             hipStream_t s) {
    // every row of every chunk starts on a 16-byte boundary: the wide loads
    const bool wide = (uintptr_t)spec % 16 == 0 && W % 4 == 0;
    if (wide)
        hipLaunchKernelGGL(acoustic_indices_kernel<true>, dim3((unsigned)B), dim3(256), 0, s, spec, minmax, W, prm, out, spectral);
    else
        hipLaunchKernelGGL(acoustic_indices_kernel<false>, dim3((unsigned)B), dim3(256), 0, s, spec, minmax, W, prm, out, spectral);
}

void preload_indices() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&acoustic_indices_kernel<true>));
}

}  // namespace bn
