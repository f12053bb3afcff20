// bn_requant.h — gemmlowp/TFLite fixed-point requantisation on the vector ALU, shared by the INT8 kernels.
//
//   MultiplyByQuantizedMultiplier(x, M0, shift) = RoundingDivideByPOT(SaturatingRoundingDoublingHighMul(x << left, M0), right)
//
// The fast forms below are algebraically identical to the reference definitions for M0 >= 0 whenever |x| * M0 / 2^31 + 2^(e-1) + 1
// stays below 2^31 (e = the right shift) — in particular for |x| < 2^30.  The lowering pass proves that bound per channel from the
// weights and the folded bias before a plan is built (models/_lower_i8.py: _expect_acc_range; (q - zp) << 20 < 2^28 in ADD):
//   SRDHM: trunc((x*M0 + nudge) / 2^31), nudge = 2^30 for x*M0 >= 0 and 1 - 2^30 otherwise, equals the ARITHMETIC shift
//          (x*M0 + 2^30) >> 31 for both signs (for negatives trunc(y/2^31) = floor((y + 2^31 - 1)/2^31) and the nudges differ
//          by exactly 2^31 - 1), i.e. one 32x32+64 -> 64 multiply-add (v_mad_i64_i32) and a funnel shift;
//   RoundingDivideByPOT(v, e): (v >> e) + ((v & mask) > (mask >> 1) + (v < 0)) equals (v + half + (v < 0 ? -1 : 0)) >> e
//          with half = 2^(e-1) (and v itself for e = 0).
// Left shifts (shift > 0) and negative multipliers take the literal reference path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn_device.h"

namespace bn {

__device__ __forceinline__ int32_t srdhm_ref(int32_t a, int32_t b) {
    const bool overflow = (a == b) && (a == INT32_MIN);
    const int64_t ab = (int64_t)a * (int64_t)b;
    const int64_t nudge = ab >= 0 ? (1ll << 30) : (1ll - (1ll << 30));
    const int32_t r = (int32_t)((ab + nudge) / (1ll << 31));
    return overflow ? INT32_MAX : r;
}
__device__ __forceinline__ int32_t rdivpot_ref(int32_t x, int exponent) {
    const int32_t mask = (int32_t)((1u << exponent) - 1u);
    const int32_t remainder = x & mask;
    const int32_t threshold = (mask >> 1) + (x < 0 ? 1 : 0);
    return (x >> exponent) + (remainder > threshold ? 1 : 0);
}
__device__ __forceinline__ int32_t mbqm_ref(int32_t x, int32_t mult, int shift) {
    const int left = shift > 0 ? shift : 0;
    const int right = shift > 0 ? 0 : -shift;
    return rdivpot_ref(srdhm_ref(x * (1 << left), mult), right);
}

__device__ __forceinline__ int32_t srdhm_pos(int32_t x, int32_t m) {  // m >= 0
    // (x*m + 2^30) >> 31 on the 64-bit product: one v_mad_i64_i32 and one v_alignbit_b32
    return (int32_t)(((int64_t)x * (int64_t)m + (1ll << 30)) >> 31);
}
__device__ __forceinline__ int32_t rdivpot_fast(int32_t v, int e) {  // e >= 0
    const int32_t half = e ? (1 << (e - 1)) : 0;  // e up to 31 occurs (dead channels with vanishing scales)
    const int32_t adj = e ? (v >> 31) : 0;
    return (v + half + adj) >> e;
}
__device__ __forceinline__ int32_t mbqm(int32_t x, int32_t mult, int shift) {
    if (shift <= 0 && mult >= 0) return rdivpot_fast(srdhm_pos(x, mult), -shift);
    return mbqm_ref(x, mult, shift);
}

// Every multiplier >= 0 and every shift < 0 (checked on the host over all channels of an operator at load time): the
// workgroup-uniform flag `all_right` selects the branch-free form, with no per-element sign/zero tests on the exponent.
__device__ __forceinline__ int32_t mbqm_right(int32_t x, int32_t mult, int shift) {
    const int e = -shift;  // >= 1
    const int32_t v = srdhm_pos(x, mult);
    return (v + (1 << (e - 1)) + (v >> 31)) >> e;
}
__device__ __forceinline__ int32_t mbqm_u(int32_t x, int32_t mult, int shift, bool all_right) {
    return all_right ? mbqm_right(x, mult, shift) : mbqm(x, mult, shift);
}

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// clamp as ONE instruction; lo <= hi.  (The compiler cannot prove lo <= hi for run-time bounds and emits compare + select + min.)
__device__ __forceinline__ int med3(int v, int lo, int hi) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ int perm(int s0, int s1, uint32_t sel) { return (int)__builtin_amdgcn_perm((uint32_t)s0, (uint32_t)s1, sel); }
// One multiply-accumulate of four packed int8 channels without unpacking: v_dot4_i32_i8
__device__ __forceinline__ int dot4(int a, int b, int c) { return __builtin_amdgcn_sdot4(a, b, c, false); }
// first link of a dot4 chain in the three-address form (no move of the bias into the accumulator)
__device__ __forceinline__ int dot4_first(int a, int b, int c) {
    int r;
    asm("v_dot4_i32_i8 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// the low bytes of four values as one dword (three v_perm_b32)
__device__ __forceinline__ int pack4(const int (&q)[4]) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)q[1], (uint32_t)q[0], 0x0c0c0400u), hi = __builtin_amdgcn_perm((uint32_t)q[3], (uint32_t)q[2], 0x0c0c0400u);
    return (int)__builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// q = ((srdhm(x, m) + c1 + sign) >> e), c1 = 2^(e-1) + (zp << e): RoundingDivideByPOT(SRDHM(x, m), e) + zp with the rounding offset and
// the zero point in one addend
__device__ __forceinline__ int rq(int x, int m, int c1, int e) {
    const int v = srdhm_pos(x, m);
    return (v + c1 + (v >> 31)) >> e;
}

// Where the clamp's lower bound is at or above the zero point (ReLU / ReLU6 outputs: the packer checks it) a negative v gives a result
// <= zero point with or without the sign term (v + 2^(e-1) < 2^e) and both clamp to the same bound: (v + c1) >> e,
// and with the addend folded into the 64-bit multiply-add: ((x*m + 2^30) >> 31 + c1) >> e == (x*m + 2^30 + c1 * 2^31) >> (31 + e)
// (nested floors) == hi32(x*m + C) >> (e - 1) for e >= 1: v_mad_i64_i32 with a per-channel 64-bit constant C = 2^30 + c1 * 2^31, then ONE
// arithmetic shift of the high dword — 2 instructions + clamp instead of 5 + clamp.  rq64(c1) builds C; kernels keep (C, e - 1) per channel.
__device__ __forceinline__ long rq64(int c1) { return ((long)c1 << 31) + 0x40000000L; }
// The four shifts of a channel quad are packed into the bytes of ONE register (SDWA picks byte `e` as the shift
// count: no unpacking instruction, three registers less per quad)
__device__ __forceinline__ int pack_shifts(v4i sh) { return sh.x | (sh.y << 8) | (sh.z << 16) | (sh.w << 24); }
// v >> byte `e` of `packed`
__device__ __forceinline__ int ashr_byte(int packed, int v, int e) {
    int r;
    switch (e) {  // e is a compile-time constant after unrolling
        case 0: asm("v_ashrrev_i32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(r) : "v"(packed), "v"(v)); break;
        case 1: asm("v_ashrrev_i32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(r) : "v"(packed), "v"(v)); break;
        case 2: asm("v_ashrrev_i32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(r) : "v"(packed), "v"(v)); break;
        default: asm("v_ashrrev_i32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(r) : "v"(packed), "v"(v)); break;
    }
    return r;
}
__device__ __forceinline__ int rq_hi(int x, int m, long c, int e1_packed, int e) {
    return ashr_byte(e1_packed, (int)(((long)x * (long)m + c) >> 32), e);
}

// h of rq_hi alone: hi32(x m + C)
__device__ __forceinline__ int rq_h(int x, int m, long c) { return (int)(((long)x * (long)m + c) >> 32); }

// The clamp IN FRONT of the shift: for every int32 h, e1 >= 0 and lo <= hi
//     clamp(h >> e1, lo, hi) == clamp(h, lo << e1, ((hi + 1) << e1) - 1) >> e1
// (the arithmetic shift is monotone and floors: h >> e1 >= lo iff h >= lo << e1, h >> e1 <= hi iff h < (hi + 1) << e1;
// tests/test_front_strip_forms.py).  Shifts are 1 .. 22 (e1 <= 21), so the bounds stay inside +-2^28.  With the clamp done on h
// against per-channel bounds the shift is the LAST instruction of a requantisation, and SDWA lets it write its low byte into
// byte j of the register where the value is read next: no byte-packing permutes.
__device__ __forceinline__ void shifted_bounds(int lo, int hi, int e1, int& blo, int& bhi) {
    blo = lo << e1;
    bhi = ((hi + 1) << e1) - 1;
}
// A partial (dst_sel: BYTE) write must not be followed directly by a vector-ALU instruction that reads the register (gfx940 and
// later forward the wrong bytes; the compiler inserts the wait state for its own instructions but does not look into inline
// assembly), and UNUSED_PRESERVE reads the destination.  So the deposits come in blocks whose neighbouring instructions write
// DIFFERENT registers (or have an independent instruction between them), and a block whose last result a vector-ALU instruction
// may read next ends in s_nop 0.
#define BN_DEP(dst, src, J, E, MODE) \
    "v_ashrrev_i32_sdwa " dst ", %[sh], " src " dst_sel:BYTE_" #J " dst_unused:UNUSED_" MODE " src0_sel:BYTE_" #E " src1_sel:DWORD\n\t"
// column J of a byte-transposed quad: the low byte of (h[e] >> byte e of sh) -> byte J of t[e]; J = 0 starts the dwords (other bytes 0)
#define BN_DEP_COLUMN(J, MODE, CONSTRAINT, TAIL)                                                                                  \
    asm(BN_DEP("%[t0]", "%[h0]", J, 0, MODE) BN_DEP("%[t1]", "%[h1]", J, 1, MODE) BN_DEP("%[t2]", "%[h2]", J, 2, MODE)            \
            BN_DEP("%[t3]", "%[h3]", J, 3, MODE) TAIL                                                                             \
        : [t0] CONSTRAINT(t[0]), [t1] CONSTRAINT(t[1]), [t2] CONSTRAINT(t[2]), [t3] CONSTRAINT(t[3])                              \
        : [sh] "v"(sh), [h0] "v"(h[0]), [h1] "v"(h[1]), [h2] "v"(h[2]), [h3] "v"(h[3]))
__device__ __forceinline__ void deposit_column(int (&t)[4], const int (&h)[4], int sh, int j) {
    switch (j) {  // j is a compile-time constant after unrolling
        case 0: BN_DEP_COLUMN(0, "PAD", "=&v", ""); break;
        case 1: BN_DEP_COLUMN(1, "PRESERVE", "+v", ""); break;
        default: BN_DEP_COLUMN(2, "PRESERVE", "+v", "s_nop 0"); break;  // the window dwords are complete: any reader may follow
    }
}
// the four channels of a quad into the four bytes of ONE dword, clamps included (they are the independent instructions between
// two writes of the same register): byte e of the result = low byte of (med3(h[e], lo[e], hi[e]) >> byte e of sh)
__device__ __forceinline__ int clamp_deposit_quad(int (&h)[4], const int (&lo)[4], const int (&hi)[4], int sh) {
    int d;
    asm("v_med3_i32 %[h0], %[h0], %[l0], %[u0]\n\t"
        "v_med3_i32 %[h1], %[h1], %[l1], %[u1]\n\t"
        BN_DEP("%[d]", "%[h0]", 0, 0, "PAD")
        "v_med3_i32 %[h2], %[h2], %[l2], %[u2]\n\t"
        BN_DEP("%[d]", "%[h1]", 1, 1, "PRESERVE")
        "v_med3_i32 %[h3], %[h3], %[l3], %[u3]\n\t"
        BN_DEP("%[d]", "%[h2]", 2, 2, "PRESERVE")
        "s_nop 0\n\t"
        BN_DEP("%[d]", "%[h3]", 3, 3, "PRESERVE")
        "s_nop 0"
        : [d] "=&v"(d), [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3])
        : [sh] "v"(sh), [l0] "v"(lo[0]), [l1] "v"(lo[1]), [l2] "v"(lo[2]), [l3] "v"(lo[3]), [u0] "v"(hi[0]), [u1] "v"(hi[1]), [u2] "v"(hi[2]),
          [u3] "v"(hi[3]));
    return d;
}
// two quads (already clamped) into two dwords, the writes alternating between them; the dwords go to a store (no vector-ALU reader)
__device__ __forceinline__ void deposit_two_quads(int& d0, int& d1, const int (&a)[4], const int (&b)[4], int sha, int shb) {
    asm("v_ashrrev_i32_sdwa %[d0], %[sa], %[a0] dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d1], %[sb], %[b0] dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d0], %[sa], %[a1] dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d1], %[sb], %[b1] dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d0], %[sa], %[a2] dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d1], %[sb], %[b2] dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d0], %[sa], %[a3] dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3 src1_sel:DWORD\n\t"
        "v_ashrrev_i32_sdwa %[d1], %[sb], %[b3] dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3 src1_sel:DWORD"
        : [d0] "=&v"(d0), [d1] "=&v"(d1)
        : [sa] "v"(sha), [sb] "v"(shb), [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [b0] "v"(b[0]), [b1] "v"(b[1]),
          [b2] "v"(b[2]), [b3] "v"(b[3]));
}

// Shift, clamp and pack as ONE instruction where the clamp is the int8 range: v_ashr_pk_i8_i32 d, a, b, s shifts two int32 right
// arithmetically by s[4:0], saturates each to [-128, 127] and writes the two bytes into one half of d (byte 0 of the half from a, byte 1
// from b); op_sel:[0,0,0,1] picks the high half.  Either form leaves the other half of d as it was (tests/test_gpu_satpack.py holds the
// hardware to all of this).  clamp(h >> e1, -128, 127) == sat_i8(h >> e1) for every int32 h, so where (lo, hi) = (-128, 127) the tail
// med3 + shift + byte packing of a requantisation collapses into it — for two values that share their shift: two positions of one
// channel, or two channels behind a per-layer shift (tests/test_satpack_forms.py has the algebra of every use).
// The high-half write is a partial write under the rule above: a block that a vector-ALU instruction may read next ends in s_nop 0, and
// two writes of the same register have a write of another register (or s_nop 0) between them.
//
// the pair in the low half, the high half zero
__device__ __forceinline__ int sat_pack2(int h0, int h1, int s) { return (int)(uint16_t)__builtin_amdgcn_ashr_pk_i8_i32(h0, h1, s); }
// the pair into the high half of dst, its low half kept
__device__ __forceinline__ void sat_pack2_hi(int& dst, int h0, int h1, int s) {
    asm("v_ashr_pk_i8_i32 %0, %1, %2, %3 op_sel:[0,0,0,1]\n\ts_nop 0" : "+v"(dst) : "v"(h0), "v"(h1), "v"(s));
}
// Two positions (a, b) x four channels behind per-channel shifts s[0..3] (low five bits): ra = bytes (a0 b0 a1 b1), rb = (a2 b2 a3 b3).
// The byte selectors kSatSelA / kSatSelB of perm(rb, ra, .) then give position a's and position b's dword of NHWC bytes.
constexpr uint32_t kSatSelA = 0x06040200u, kSatSelB = 0x07050301u;
__device__ __forceinline__ void sat_pack_2x4(int& ra, int& rb, const int (&a)[4], const int (&b)[4], const int (&s)[4]) {
    asm("v_ashr_pk_i8_i32 %[ra], %[a0], %[b0], %[s0]\n\t"
        "v_ashr_pk_i8_i32 %[rb], %[a2], %[b2], %[s2]\n\t"
        "v_ashr_pk_i8_i32 %[ra], %[a1], %[b1], %[s1] op_sel:[0,0,0,1]\n\t"
        "v_ashr_pk_i8_i32 %[rb], %[a3], %[b3], %[s3] op_sel:[0,0,0,1]\n\t"
        "s_nop 0"
        : [ra] "=&v"(ra), [rb] "=&v"(rb)
        : [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [b0] "v"(b[0]), [b1] "v"(b[1]), [b2] "v"(b[2]), [b3] "v"(b[3]),
          [s0] "v"(s[0]), [s1] "v"(s[1]), [s2] "v"(s[2]), [s3] "v"(s[3]));
}
// The four channels of ONE position behind a shift all four share (wave-uniform: the ADD's output rescale) -> its dword of NHWC bytes.
// Two positions at a time, the writes alternating between the dwords; the dwords go to a store (no vector-ALU reader).
__device__ __forceinline__ void sat_pack_quads(int& d0, int& d1, const int (&a)[4], const int (&b)[4], int s) {
    asm("v_ashr_pk_i8_i32 %[d0], %[a0], %[a1], %[s]\n\t"
        "v_ashr_pk_i8_i32 %[d1], %[b0], %[b1], %[s]\n\t"
        "v_ashr_pk_i8_i32 %[d0], %[a2], %[a3], %[s] op_sel:[0,0,0,1]\n\t"
        "v_ashr_pk_i8_i32 %[d1], %[b2], %[b3], %[s] op_sel:[0,0,0,1]"
        : [d0] "=&v"(d0), [d1] "=&v"(d1)
        : [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [b0] "v"(b[0]), [b1] "v"(b[1]), [b2] "v"(b[2]), [b3] "v"(b[3]), [s] "s"(s));
}
// Three columns (h0, h1, h2) of four channels behind per-channel shifts s[0..3] -> byte j of t[e] = column j of channel e: the depthwise
// window dwords deposit_column builds, in two steps so that a third column may be computed between them.  Byte 3 repeats column 2
// (the window's fourth tap weight is 0).  The second step ends the block for any reader.
__device__ __forceinline__ void sat_window_lo(int (&t)[4], const int (&h0)[4], const int (&h1)[4], const int (&s)[4]) {
    asm("v_ashr_pk_i8_i32 %[t0], %[a0], %[b0], %[s0]\n\t"
        "v_ashr_pk_i8_i32 %[t1], %[a1], %[b1], %[s1]\n\t"
        "v_ashr_pk_i8_i32 %[t2], %[a2], %[b2], %[s2]\n\t"
        "v_ashr_pk_i8_i32 %[t3], %[a3], %[b3], %[s3]"
        : [t0] "=&v"(t[0]), [t1] "=&v"(t[1]), [t2] "=&v"(t[2]), [t3] "=&v"(t[3])
        : [a0] "v"(h0[0]), [a1] "v"(h0[1]), [a2] "v"(h0[2]), [a3] "v"(h0[3]), [b0] "v"(h1[0]), [b1] "v"(h1[1]), [b2] "v"(h1[2]), [b3] "v"(h1[3]),
          [s0] "v"(s[0]), [s1] "v"(s[1]), [s2] "v"(s[2]), [s3] "v"(s[3]));
}
__device__ __forceinline__ void sat_window_hi(int (&t)[4], const int (&h2)[4], const int (&s)[4]) {
    asm("v_ashr_pk_i8_i32 %[t0], %[a0], %[a0], %[s0] op_sel:[0,0,0,1]\n\t"
        "v_ashr_pk_i8_i32 %[t1], %[a1], %[a1], %[s1] op_sel:[0,0,0,1]\n\t"
        "v_ashr_pk_i8_i32 %[t2], %[a2], %[a2], %[s2] op_sel:[0,0,0,1]\n\t"
        "v_ashr_pk_i8_i32 %[t3], %[a3], %[a3], %[s3] op_sel:[0,0,0,1]\n\t"
        "s_nop 0"
        : [t0] "+v"(t[0]), [t1] "+v"(t[1]), [t2] "+v"(t[2]), [t3] "+v"(t[3])
        : [a0] "v"(h2[0]), [a1] "v"(h2[1]), [a2] "v"(h2[2]), [a3] "v"(h2[3]), [s0] "v"(s[0]), [s1] "v"(s[1]), [s2] "v"(s[2]), [s3] "v"(s[3]));
}
__device__ __forceinline__ int sat_pack_quad(const int (&a)[4], int s) {
    int d;
    asm("v_ashr_pk_i8_i32 %[d], %[a0], %[a1], %[s]\n\t"
        "s_nop 0\n\t"
        "v_ashr_pk_i8_i32 %[d], %[a2], %[a3], %[s] op_sel:[0,0,0,1]"
        : [d] "=&v"(d)
        : [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [s] "s"(s));
    return d;
}

// int8 MEAN of `raw_sum` = sum of the P raw bytes of a channel.  Two published forms (oracle/int8_graph.py has both behind mean_form):
//   integer (default): MultiplyByQuantizedMultiplier(raw_sum - zp_in P, mult, shift) with 1 / P folded into the multiplier (reduce.h);
//   float (shift == kMeanFloatForm, mult = the float32 bits of s_in / s_out): TFLite's float-arithmetic QuantizedMeanOrSum —
//       round(raw_sum / P * scale + (-zp_in * scale)) in float32, every operation rounded on its own (no fused multiply-add).
// The lowering pass picks the form (models/_lower_i8.py: lower_i8(mean_form=...)); ~4 % of the pooled bytes of the shipped graph differ by
// one step between the two (tests/test_oracle_pinning.py counts them), so a deployment that must match a given interpreter picks its form.
constexpr int32_t kMeanFloatForm = 0x7fffff00;
__device__ __forceinline__ int32_t mean_q(int32_t raw_sum, int32_t P, int32_t zp_in, int32_t mult, int32_t shift, int32_t zp_out) {
#pragma clang fp contract(off)
    if (shift == kMeanFloatForm) {
        const float scale = __int_as_float(mult);
        const float bias = (float)(-zp_in) * scale;
        const float mean = (float)raw_sum / (float)P;
        const float t = mean * scale;
        const float r = roundf(t + bias) + (float)zp_out;
        return (int32_t)fminf(fmaxf(r, -128.0f), 127.0f);
    }
    return clampi(mbqm(raw_sum - zp_in * P, mult, shift) + zp_out, -128, 127);
}

}  // namespace bn
