// bn_tail_common.h — helpers shared by the two fused-tail kernels (bn_i8_tail.hip, bn_i8_tail2.hip): the staging of the high-dword
// requantisation constants (bn_requant.h: rq_hi), and the MEAN -> FULLY_CONNECTED -> head part behind the last block.
#pragma once
#include "bn_kernels.h"
#include "bn_requant.h"

namespace bn {
namespace {

// (multiplier, c1, shift) of the constant block -> (multiplier, C01, C23, packed shifts - 1) in LDS
__device__ __forceinline__ void stage_rq(v4i* dst, v4i m, v4i c1, v4i sh) {
    const long c[4] = {rq64(c1.x), rq64(c1.y), rq64(c1.z), rq64(c1.w)};
    dst[0] = m;
    dst[1] = (v4i){(int)c[0], (int)(c[0] >> 32), (int)c[1], (int)(c[1] >> 32)};
    dst[2] = (v4i){(int)c[2], (int)(c[2] >> 32), (int)c[3], (int)(c[3] >> 32)};
    dst[3] = (v4i){pack_shifts(sh - 1), 0, 0, 0};
}
__device__ __forceinline__ long pair(int lo, int hi) { return __builtin_bit_cast(long, (v2i){lo, hi}); }

// MEAN + FULLY_CONNECTED + head for the workgroup's chunks.  (As a real function call it costs a stack copy of the arguments: 1168 B of
// scratch per lane — it stays inlined.)
// EMB: the pooled bytes also go to the embedding output of the WithEmb<Args> kernel argument (int8 or dequantised float32; i8_tail_emb_kernel).
template <int NTHREADS, int PAD, class Args, bool EMB = false>
__device__ __forceinline__ void tail_head(const Args& a, unsigned char* lds, int chunk0) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // keeps this part's index arithmetic from being hoisted to the top of the kernel and held in registers across
                                   // the blocks, which run at the 128-register cap of a 16-wave workgroup (it was what spilled)
    // The classifier matrix (NC x C bytes: 25.6 KB) comes into LDS for the four chunks of the group: as 64 dependent dword loads per
    // (chunk, class) thread, 256 bytes apart between neighbouring threads, the head took 15 % of a group's time with 60 % of the threads idle.
    // Requested here (coalesced 16-byte loads, one round trip for the whole workgroup), written behind the MEAN; it overlays the last
    // block's pointwise weights, which nobody reads any more (the block's end barrier is behind us).  Rows of C / 4 + 1 dwords: thread j
    // walks row j, so neighbouring threads sit on neighbouring banks.
    const auto& L = a.L[a.n_layers - 1];
    const int c16 = a.C / 16, n_w16 = a.NC * c16, pitchw = a.C / 4 + 1;
    constexpr int NW = 4096 / NTHREADS;   // staging rounds: up to 4096 sixteen-byte pieces of the classifier matrix
    v4i wreg[NW];
    if (a.fcw_off >= 0) {
        const v4i* gw = reinterpret_cast<const v4i*>(a.cst + a.g_fcw);
#pragma unroll
        for (int u = 0; u < NW; ++u) {
            const int i = tid + u * NTHREADS;
            wreg[u] = i < n_w16 ? gw[i] : (v4i){0, 0, 0, 0};
        }
    }
    // ---- MEAN over the positions of the last map: one thread per (chunk slot, channel) ---------------------------------------
    const int pitch = a.C + PAD;
    for (int i = tid; i < kTailG * a.C; i += NTHREADS) {
        const int g = i / a.C, c = i - g * a.C;
        const int8_t* src = reinterpret_cast<const int8_t*>(lds + L.y_off + g * a.P * pitch + c);
        int s = 0;
        for (int k = 0; k < a.P; ++k) s += src[k * pitch];
        reinterpret_cast<int8_t*>(lds + a.mean_off)[i] = (int8_t)mean_q(s, a.P, a.mean_zp_in, a.mean_mult, a.mean_shift, a.mean_zp_out);
    }
    if (a.fcw_off >= 0) {
        int* wl = reinterpret_cast<int*>(lds + a.fcw_off);
#pragma unroll
        for (int u = 0; u < NW; ++u) {
            const int i = tid + u * NTHREADS;
            if (i < n_w16) {
                int* d = wl + (i / c16) * pitchw + 4 * (i % c16);
                d[0] = wreg[u].x; d[1] = wreg[u].y; d[2] = wreg[u].z; d[3] = wreg[u].w;
            }
        }
    }
    __syncthreads();
    if constexpr (EMB) {
        // the pooled bytes of the group ([slot][C] in LDS) to a.emb, four per thread: a dword or a float4 store.  The arguments come through
        // the kernel-argument pointer (held in registers from the top of the kernel they cost this kernel, at its register cap, scratch)
        const WithEmb<Args>* ap = (const WithEmb<Args>*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ap));
        const int c4 = ap->a.C / 4;
        for (int i = tid; i < kTailG * c4; i += NTHREADS) {
            const int g = i / c4;
            if (chunk0 + g >= ap->a.B) break;
            const int q = reinterpret_cast<const int*>(lds + ap->a.mean_off)[i];
            const size_t e = (size_t)chunk0 * ap->a.C + 4 * (size_t)i;   // (slots are consecutive chunks: [slot][C] is [chunk][C])
            if (ap->e.f32) {
                const int zp = ap->e.zp;
                const float sc = ap->e.scale;
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(ap->e.emb) + e) =
                    make_float4((float)((int)(int8_t)q - zp) * sc, (float)((int)(int8_t)(q >> 8) - zp) * sc, (float)((int)(int8_t)(q >> 16) - zp) * sc,
                                (float)((q >> 24) - zp) * sc);
            } else {
                *reinterpret_cast<int*>(reinterpret_cast<int8_t*>(ap->e.emb) + e) = q;
            }
        }
    }
    // ---- FULLY_CONNECTED + head: one thread per (chunk slot, class) ----------------------------------------------------------
    for (int i = tid; i < kTailG * a.NC; i += NTHREADS) {
        const int g = i / a.NC, j = i - g * a.NC;
        const int chunk = chunk0 + g;
        if (chunk >= a.B) continue;
        const int* xr = reinterpret_cast<const int*>(lds + a.mean_off + g * a.C);
        const int* wr = a.fcw_off >= 0 ? reinterpret_cast<const int*>(lds + a.fcw_off) + j * pitchw : a.cst + a.g_fcw + j * (a.C / 4);
        int acc = a.cst[a.g_fcb + j];
        for (int k = 0; k < a.C / 4; ++k) acc = dot4(xr[k], wr[k], acc);
        const int qv = clampi(mbqm(acc, a.cst[a.g_fcm + j], a.cst[a.g_fcs + j]) + a.fc_zp_out, a.fc_lo, a.fc_hi);
        const size_t o = (size_t)chunk * a.NC + j;
        if (a.logits) a.logits[o] = (float)(qv - a.head_zp_fc) * a.s_fc;
        if (a.g_hlut >= 0) {
            const int ov = reinterpret_cast<const int8_t*>(a.cst + a.g_hlut)[qv + 128];
            a.scores[o] = (float)(ov - a.head_zp_out) * a.s_head;
        } else {
            a.scores[o] = (float)(qv - a.head_zp_fc) * a.s_fc;
        }
    }
}


}  // namespace
}  // namespace bn
