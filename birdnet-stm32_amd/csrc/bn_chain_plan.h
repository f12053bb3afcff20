// bn_chain_plan.h — kernel arguments of the fused INT8 chains (i8_tail_kernel, i8_tail2_kernel, i8_mid2_kernel) and the host-side planners
// that fill them from the packer's descriptor tables and place every block's pieces in LDS (bn_chain_plan.cpp).  No HIP in here: the
// planners are plain integer arithmetic, and a plain C++ compiler builds them (tests/host/chain_plan_main.cpp runs them without a device).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BN_HOST_DEVICE __host__ __device__
#else
#define BN_HOST_DEVICE
#endif

namespace bn {

// The back half of the INT8 graph as one kernel with the maps in LDS (bn_i8_tail.hip).
constexpr int kTailG = 4;          // chunks a workgroup holds at a time (models/_lower_i8.py: TAIL_G)
constexpr int kTailWaves = 16;
constexpr int kTailThreads = 64 * kTailWaves;
constexpr int kTailLayerWords = 24;    // descriptor words per block, first form (models/_lower_i8.py: TAIL_LAYER_WORDS)
constexpr int kTailHeadWords = 16;     // descriptor words of the head, both forms (models/_lower_i8.py: TAIL_HEAD_WORDS)
struct Tail8Layer {
    int H, W, Cin, Cout, S, OH, OW, pt, pl, has_add;
    int zp_in, dw_lo, dw_hi, pw_lo, pw_hi;        // clamp bounds (pointwise: + 128 with the ADD)
    int add_m, add_c1, add_e, add_lo, add_hi;     // output rescale of the ADD (zero point folded into c1) and its clamp
    int g_w, g_dwc, g_pwc, g_lut;                 // word offsets of the block's sections in the constant block
    int x_off, y_off, w_off, dwc_off, pwc_off, lut_off, zp_off;  // LDS byte offsets (x_off < 0: the input map is in global memory)
};
struct Tail8Args {
    const int8_t* x;      // [B][H0][W0][C0]: input map of the first block
    float* scores;        // [B][NC]
    float* logits;        // [B][NC] or null
    const int32_t* cst;   // constant block (models/_lower_i8.py: tail_constants)
    int B, n_layers, NC, P, C;
    int mean_zp_in, mean_mult, mean_shift, mean_zp_out, mean_off;
    int fc_zp_out, fc_lo, fc_hi, g_fcw, g_fcb, g_fcm, g_fcs, g_hlut, head_zp_fc, head_zp_out;
    float s_fc, s_head;
    int lds_bytes;
    int fcw_off;          // LDS copy of the classifier matrix for the head, rows of C / 4 + 1 dwords (-1: read it from memory); overlays the last block's weights
    Tail8Layer L[8];};
bool tail_plan(const int32_t* desc, int n_words, int n_layers, Tail8Args& a);  // a.NC must be set; false = not a topology / size the kernel takes
long tail_const_words(const Tail8Args& a);

// The same back half with the DEPTHWISE stage on the matrix cores too (bn_i8_tail2.hip): 8 waves per workgroup, maps in place.
constexpr int kTail2Waves = 8;
constexpr int kTail2Threads = 64 * kTail2Waves;
constexpr int kTail2LayerWords = 32;   // models/_lower_i8.py: TAIL2_LAYER_WORDS
struct Tail2Layer {
    int H, W, Cin, Cout, S, OH, OW, pt, pl, has_add;
    int zp_in, dw_lo, dw_hi, pw_lo, pw_hi;        // clamp bounds (pointwise with the ADD: minus the block's own zero point)
    int add_m, add_c1, add_e, add_lo, add_hi;     // output rescale of the ADD (zero point folded into c1) and its clamp
    int res_m, res_c_lo, res_c_hi, res_k;         // rescale of the residual byte: (((b + 128) << 24) res_m + res_c) >> 32 >> res_k
    int g_cst;                                    // word offset of the block's constants: depthwise part (A fragments | constants), then pointwise part (A fragments | constants)
    int x_off, y_off, dw_off, pw_off, zp_off;     // LDS byte offsets (x_off < 0: the input map is in global memory)
};
constexpr int kMidG = 2;   // chunks a workgroup of i8_mid2_kernel holds at a time
struct Tail2Args {
    const int8_t* x;
    int8_t* y;            // i8_mid2_kernel: where the last map goes, [B][P][C]
    float* scores;
    float* logits;
    const int32_t* cst;   // constant block (models/_lower_i8.py: tail2_constants)
    int B, n_layers, NC, P, C;
    int mean_zp_in, mean_mult, mean_shift, mean_zp_out, mean_off;
    int fc_zp_out, fc_lo, fc_hi, g_fcw, g_fcb, g_fcm, g_fcs, g_hlut, head_zp_fc, head_zp_out;
    float s_fc, s_head;
    int lds_bytes;
    int fcw_off;
    int bar_off;          // LDS byte offset of the chunk barriers' counters (one dword per chunk slot)
    int resident;         // i8_mid2_kernel: every block's constants have LDS of their own (tail2_plan_resident) — staged once, chunk-local barriers
    int satpack;          // the kernels' shift-saturate-pack epilogues (v_ashr_pk_i8_i32): set by tail2_plan from tail2_satpack_ok, cleared by option i8_satpack
    Tail2Layer L[8];};
constexpr int kTail2MaxDw16 = 7 * kTail2Threads;   // sixteen-byte pieces of the largest depthwise part a block may prefetch (256 channels: 3392)
// bytes of a block's depthwise part (expanded weights + constants) and pointwise part (weights + constants) in the constant block and in LDS:
// what the kernels copy and what the planners place
BN_HOST_DEVICE inline int tail2_dw_bytes(const Tail2Layer& L, bool first) { return (L.Cin / 16) * (3 * 1024 + (first ? 8 : 5) * 64); }
BN_HOST_DEVICE inline int tail2_pw_bytes(const Tail2Layer& L) { return (L.Cin + 63) / 64 * 64 * L.Cout + (L.Cout / 16) * 5 * 64; }
bool tail2_plan(const int32_t* desc, int n_words, int n_layers, Tail2Args& a, bool mid = false);  // a.NC must be set (tail); mid: the stage-2 chain, no head
// every clamp in front of a stored byte of the chain is the int8 range itself: (dw_lo, dw_hi) and, without the ADD, (pw_lo, pw_hi), with it
// (add_lo, add_hi), all (-128, 127) in every block — the saturation of v_ashr_pk_i8_i32 then IS the clamp; false: the chain keeps med3
bool tail2_satpack_ok(const Tail2Args& a);
bool tail2_plan_resident(Tail2Args& a);   // a stage-2 plan tail2_plan accepted -> its resident placement; false (a unspecified): it does not fit, keep the staged one
bool tail2_plan_dump(const Tail2Args& a, int* out, int n);   // bn_debug_mid_plan (include/birdnet_hip.h has the layout)
long tail2_const_words(const Tail2Args& a, bool mid = false);

}  // namespace bn
