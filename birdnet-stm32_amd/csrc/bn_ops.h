// bn_ops.h — the one definition of what OpRec.p[] / t[] / f[] hold for every operator kind (bn_blob.h: BnOpKind).
//
// Per kind a namespace bn::op::<kind> with the enums Pi (indices into p), Ti (into t) and Fi (into f), in index order; a kind's names are
// unique across its three enums.  The writer (birdnet_stm32/models/_pack.py: OP_FIELDS) holds the same names in the same order, and
// tests/test_lowering_and_abi.py compares the two.  The validator (bn_plan_check.hip), the load-time preparation and the executor
// (bn_plan_run.hip) and bn_api.hip address operator records through these names only.  rsvN: an entry the kind leaves at its default.
// act codes: 0 none, 1 relu, 2 relu6.   mag codes: 0 none, 1 pwl, 2 pcen, 3 db.
#pragma once
#include "bn_blob.h"

// the ten conv-geometry fields the 3x3 stages share (F32_STEM, F32_DW, F32_DWPW, I8_STEM, I8_DW, I8_DWPW): input map, strides, the kind's
// own use of entry 5, output map, top / left padding.  c names the channel entry (Cout of a stem, C, Cin of a fused block).
#define BN_FIELDS_GEOM(c, p5) H, W, c, sh, sw, p5, OH, OW, pt, pl
// the residual ADD behind a pointwise stage (I8_PW, I8_DWPW): operand 1 = the residual (zero point, multiplier, shift), operand 2 = the
// convolution's result, then the output's multiplier, shift, zero point and clamp
#define BN_FIELDS_ADD has_add, add_z1, add_m1, add_s1, add_m2, add_s2, add_mo, add_so, add_zo, add_amin, add_amax

namespace bn {
namespace op {

// ---- float32 plan ----------------------------------------------------------------------------------------------------------------
// spec [F][W] -> mel [M][W]   t: wvals(f32) bands(i32 [3][M]: start,len,off) magp(f32 [NP][M])
namespace f32_mel {
enum Pi { F, W, M, mag, norm, P_END };
enum Ti { wvals, bands, magp, T_END };
}
// in place [M][W]: x/(max+1e-6) then magnitude scaling
namespace f32_mag {
enum Pi { M, W, mag, P_END };
enum Ti { rsv0, rsv1, magp, T_END };
}
// wave [T] -> [M][W]   t: fb(f32 [16][M] BN-folded) bias magp
namespace f32_rawfe {
enum Pi { T, W, M, stride, pad_left, mag, P_END };
enum Ti { fb, bias, magp, T_END };
}
// [H][W] (C=1) -> [OH][OW][Cout]   t: w[3][3][Cout] bias[Cout]
namespace f32_stem {
enum Pi { BN_FIELDS_GEOM(Cout, act), P_END };
enum Ti { w, bias, T_END };
}
// [H][W][C] -> [OH][OW][C]   t: w[3][3][C] bias[C]
namespace f32_dw {
enum Pi { BN_FIELDS_GEOM(C, act), P_END };
enum Ti { w, bias, T_END };
}
// [P][Cin] -> [P][Cout]   in1: residual slot, gate_slot: slot of the squeeze-excite gate   t: w[Cin][Cout] bias
namespace f32_pw {
enum Pi { P, Cin, Cout, act, has_res, has_gate, gate_slot, P_END };
enum Ti { w, bias, T_END };
}
// [P][C] -> gate [C]   t: w1[C][Cr] w2[Cr][C]
namespace f32_segate {
enum Pi { P, C, Cr, P_END };
enum Ti { w1, w2, T_END };
}
// [P][C] * gate(in1)[C] -> [P][C]
namespace f32_scale {
enum Pi { P, C, P_END };
}
// [P][C] -> [C]
namespace f32_gap {
enum Pi { P, C, P_END };
}
// [Cin] -> scores [Cout] (+ logits)   act: 0 linear, 1 sigmoid, 2 softmax   t: w[Cin][Cout] bias
namespace f32_dense {
enum Pi { Cin, Cout, act, P_END };
enum Ti { w, bias, T_END };
}
// [P][C] -> [C]   t: score[C]
namespace f32_attnpool {
enum Pi { P, C, P_END };
enum Ti { score, T_END };
}
// fused [depthwise 3x3 ->] pointwise 1x1 on the matrix cores; has_dw = 0: plain 1x1 conv of in0
// in1: residual slot   t: dw_w[3][3][Cin] dw_b[Cin] pw_w(fragment order [Cin/16][Cout/16][64][4]) pw_b[Cout]
namespace f32_dwpw {
enum Pi { BN_FIELDS_GEOM(Cin, dw_act), Cout, pw_act, has_res, has_gate, gate_slot, has_dw, TH, TW, NB, P_END };
enum Ti { dw_w, dw_b, pw_w, pw_b, T_END };
}
// audio [T] -> un-normalised mel energies [M][W] (+ min/max of the magnitudes): STFT with the band-sparse mixer fused   T: 0 = runtime
namespace f32_stftmel {
enum Pi { T, W, M, P_END };
enum Ti { wvals, bands, T_END };
}
// un-normalised mel energies -> frontend output [M][W]   t: wsum[M] - magp
namespace f32_melfin {
enum Pi { M, W, mag, norm, P_END };
enum Ti { wsum, rsv1, magp, T_END };
}
// frontend output [H0][W0] -> stem 3x3 s(1,2) -> depthwise 3x3 s2 -> pointwise, one kernel   t: pw_w in fragment order
// raw_mel = 1 (audio path): in0 holds un-normalised mel energies, finalised while the patch is loaded (wsum, magp)
namespace f32_front {
enum Pi { H0, W0, C, N, OH, OW, stem_act, dw_act, pw_act, raw_mel, mag, P_END };
enum Ti { stem_w, stem_b, dw_w, dw_b, pw_w, pw_b, wsum, magp, T_END };
}
// global average pool + Dense + sigmoid/softmax in one kernel: [P][Cin] -> scores [Cout] (+ logits)   t: w[Cin][Cout] bias
namespace f32_gapdense {
enum Pi { P, Cin, Cout, act, P_END };
enum Ti { w, bias, T_END };
}
// ---- INT8 plan -------------------------------------------------------------------------------------------------------------------
// spec f32 [F][W] -> q int8 [W][Kp]
namespace i8_quant {
enum Pi { F, W, Kp, zp, fill, P_END };
enum Fi { scale, F_END };
}
// [W][Kp] -> [M][W]   t: w[M][Kp] bias(zp-folded) mult shift lut[M][256]
namespace i8_mel {
enum Pi { W, Kp, M, zp_out, act_min, act_max, has_lut, P_END };
enum Ti { w, bias, mult, shift, lut, T_END };
}
// [H][W] -> [OH][OW][Cout]   t: w[3][3][Cout] bias mult shift
namespace i8_stem {
enum Pi { BN_FIELDS_GEOM(Cout, rsv5), zp_in, zp_out, act_min, act_max, P_END };
enum Ti { w, bias, mult, shift, T_END };
}
// [H][W][C] -> [OH][OW][C]   t: w[3][3][C] bias mult shift
namespace i8_dw {
enum Pi { BN_FIELDS_GEOM(C, rsv5), zp_in, zp_out, act_min, act_max, P_END };
enum Ti { w, bias, mult, shift, T_END };
}
// [P][Cin] -> [P][Cout]   in1: residual slot   t: w[Cout][Cin] bias(zp-folded) mult shift
namespace i8_pw {
enum Pi { P, Cin, Cout, zp_out, act_min, act_max, BN_FIELDS_ADD, P_END };
enum Ti { w, bias, mult, shift, T_END };
}
// [P][C] -> [C]
namespace i8_mean {
enum Pi { P, C, zp_in, mult, shift, zp_out, P_END };
}
// [Cin] -> [Cout]   t: w[Cout][Cin rounded up to 4, zero padded] bias(zp-folded) mult shift lut[256]
// (lut: the int8 LOGISTIC behind the layer, squeeze-excite gates)
namespace i8_fc {
enum Pi { Cin, Cout, zp_out, act_min, act_max, has_lut, P_END };
enum Ti { w, bias, mult, shift, lut, T_END };
}
// [C] int8 -> scores f32 (+ logits f32)   t: lut[256]
// softmax = 1: scores = float32 softmax of the dequantised input (DEQUANTIZE -> SOFTMAX graphs of conversion/export.py)
namespace i8_head {
enum Pi { C, zp_fc, zp_out, has_lut, softmax, P_END };
enum Ti { lut, T_END };
enum Fi { s_fc, s_out, beta, F_END };
}
// fused [depthwise 3x3 ->] pointwise 1x1 on the int8 matrix cores (has_dw = 0: plain 1x1; transposed = 1: mel mixer)
// in1: residual slot   t: dw_w dw_b(zp folded) dw_mult dw_shift pw_w(fragment order) pw_b(zp folded) pw_mult pw_shift lut[Cout][256],
// strip_cst: constant block of the strip kernel (strip = 1), add_tab: the whole ADD as a 64 KB table
// q_at_load = 1 (mel mixer): QUANTIZE runs while the mixer loads the float32 spectrogram [qF][W]: qscale, qzp, qfill (byte of the padded bins)
namespace i8_dwpw {
enum Pi { BN_FIELDS_GEOM(Cin, qF), dw_zp_in, dw_zp_out, dw_amin, dw_amax, Cout, pw_zp_out, pw_amin, pw_amax, BN_FIELDS_ADD, has_dw, transposed, TH, TW, NB, has_lut, strip, q_at_load, qzp, qfill, P_END };
enum Ti { dw_w, dw_b, dw_mult, dw_shift, pw_w, pw_b, pw_mult, pw_shift, lut, strip_cst, add_tab, T_END };
enum Fi { qscale, F_END };
}
// frontend output [H0][W0] int8 -> stem 3x3 s(1,2) -> depthwise 3x3 s2 -> pointwise, one kernel
// t: dw_b, pw_b zp folded, pw_w in fragment order; strip_cst: constant block of the strip kernel (strip = 1)
namespace i8_front {
enum Pi { H0, W0, C, N, OH, OW, stem_zp_in, stem_zp_out, stem_amin, stem_amax, dw_zp_out, dw_amin, dw_amax, pw_zp_out, pw_amin, pw_amax, strip, P_END };
enum Ti { stem_w, stem_b, stem_mult, stem_shift, dw_w, dw_b, dw_mult, dw_shift, pw_w, pw_b, pw_mult, pw_shift, strip_cst, T_END };
}
// the back half of the INT8 graph in one kernel: n_layers blocks [DW 3x3 -> PW 1x1 (-> ADD)] with the maps in LDS, then MEAN,
// FULLY_CONNECTED and the head (bn_i8_tail.hip)
// t: constant block (int32 words), descriptor table (24 words per block + 16 head words; models/_lower_i8.py: tail_constants);
// cst2, desc2 (optional): the same for i8_tail2_kernel (32 words per block)
namespace i8_tail {
enum Pi { in_bytes, pw_macs, dw_macs, other_macs, n_classes, n_layers, H0, W0, C0, P_last, C_last, P_END };
enum Ti { cst, desc, cst2, desc2, T_END };
enum Fi { s_fc, s_head, F_END };
}
// int8 MUL of a map with a per-chunk gate vector (squeeze-excite): [P][C] * gate(in1)[C] -> [P][C]
namespace i8_scale {
enum Pi { P, C, zp_x, zp_gate, mult, shift, zp_out, act_min, act_max, P_END };
}
// per-chunk max normalisation of an int8 map (REDUCE_MAX over the whole map -> ADD epsilon -> DIV by that scalar) followed by an
// optional per-channel 256-entry table (the PWL behind it): [C][W] -> [C][W].  Everything after the max is a function of bytes:
// t: denominator byte per max byte (256), DIV table [256 denominators][256 values] (row/column = byte + 128), per-channel table [C][256] (has_lut)
namespace i8_maxnorm {
enum Pi { C, W, has_lut, P_END };
enum Ti { denom, div, lut, T_END };
}
// raw frontend of an exported INT8 graph: QUANTIZE of the float32 waveform [T] -> [PAD] -> CONV_2D 1x16 stride s VALID (ReLU6 clamp)
// -> optional per-channel table (magnitude scaling) -> [M][W] int8
// t: weights [M][16] int8, bias (zero point of the input folded), multipliers, shifts, table [M][256] (has_lut)
namespace i8_rawfe {
enum Pi { T, W, M, stride, pad_left, q_zp, zp_out, act_min, act_max, has_lut, P_END };
enum Ti { w, bias, mult, shift, lut, T_END };
enum Fi { q_scale, F_END };
}
// attention pooling of an exported graph: score FC + int8 SOFTMAX over the positions + MUL + SUM (bn_i8.hip)
// launch_i8_attnpool takes the record's p as it is: the order below is the order of AttnPool8Args
namespace i8_attnpool {
enum Pi { P, C, fc_bias, fc_mult, fc_shift, fc_zo, form, zx, za, mul_mult, mul_shift, mul_zo, mul_lo, mul_hi, sum_mult, sum_shift, sum_zo, P_END };
enum Ti { score, tables, T_END };
}
// the three blocks of stage 2 of the shipped INT8 graph in one kernel (a stride-2 block from memory, two residual blocks in LDS, the last
// map back to memory): bn_i8_tail2.hip, i8_mid2_kernel
// t: constant block (int32 words), descriptor table (32 words per block; models/_lower_i8.py: tail2_constants without head)
namespace i8_mid {
enum Pi { in_bytes, pw_macs, dw_macs, rsv3, rsv4, n_layers, H0, W0, C0, P_last, C_last, P_END };
enum Ti { cst, desc, T_END };
}

// ---- cross-kind entries (bn_blob.h) ---------------------------------------------------------------------------------------------------
// Every record carries p[BN_OP_PATH] and may carry a fusion tag in p[BN_OP_TAIL_TAG]; BN_OP_F32_FRONT also p[BN_OP_FRONT2_DIST]; the kinds
// that can produce the embedding also p[BN_OP_EMB_ZP .. BN_OP_EMB_TAG] and f[BN_OP_EMB_SCALE].  A kind's own fields end below the first of
// these it can carry:
static_assert(f32_mel::P_END <= BN_OP_TAIL_TAG, "f32_mel: fields run into the cross-kind entries");
static_assert(f32_mag::P_END <= BN_OP_TAIL_TAG, "f32_mag: fields run into the cross-kind entries");
static_assert(f32_rawfe::P_END <= BN_OP_TAIL_TAG, "f32_rawfe: fields run into the cross-kind entries");
static_assert(f32_stem::P_END <= BN_OP_TAIL_TAG, "f32_stem: fields run into the cross-kind entries");
static_assert(f32_dw::P_END <= BN_OP_TAIL_TAG, "f32_dw: fields run into the cross-kind entries");
static_assert(f32_pw::P_END <= BN_OP_TAIL_TAG, "f32_pw: fields run into the cross-kind entries");
static_assert(f32_segate::P_END <= BN_OP_TAIL_TAG, "f32_segate: fields run into the cross-kind entries");
static_assert(f32_scale::P_END <= BN_OP_TAIL_TAG, "f32_scale: fields run into the cross-kind entries");
static_assert(f32_gap::P_END <= BN_OP_EMB_ZP, "f32_gap: fields run into the cross-kind entries");
static_assert(f32_dense::P_END <= BN_OP_TAIL_TAG, "f32_dense: fields run into the cross-kind entries");
static_assert(f32_attnpool::P_END <= BN_OP_EMB_ZP, "f32_attnpool: fields run into the cross-kind entries");
static_assert(f32_dwpw::P_END <= BN_OP_TAIL_TAG, "f32_dwpw: fields run into the cross-kind entries");
static_assert(f32_stftmel::P_END <= BN_OP_TAIL_TAG, "f32_stftmel: fields run into the cross-kind entries");
static_assert(f32_melfin::P_END <= BN_OP_TAIL_TAG, "f32_melfin: fields run into the cross-kind entries");
static_assert(f32_front::P_END <= BN_OP_FRONT2_DIST, "f32_front: fields run into the cross-kind entries");
static_assert(f32_gapdense::P_END <= BN_OP_EMB_ZP, "f32_gapdense: fields run into the cross-kind entries");
static_assert(i8_quant::P_END <= BN_OP_TAIL_TAG, "i8_quant: fields run into the cross-kind entries");
static_assert(i8_mel::P_END <= BN_OP_TAIL_TAG, "i8_mel: fields run into the cross-kind entries");
static_assert(i8_stem::P_END <= BN_OP_TAIL_TAG, "i8_stem: fields run into the cross-kind entries");
static_assert(i8_dw::P_END <= BN_OP_TAIL_TAG, "i8_dw: fields run into the cross-kind entries");
static_assert(i8_pw::P_END <= BN_OP_TAIL_TAG, "i8_pw: fields run into the cross-kind entries");
static_assert(i8_mean::P_END <= BN_OP_EMB_ZP, "i8_mean: fields run into the cross-kind entries");
static_assert(i8_fc::P_END <= BN_OP_TAIL_TAG, "i8_fc: fields run into the cross-kind entries");
static_assert(i8_head::P_END <= BN_OP_TAIL_TAG, "i8_head: fields run into the cross-kind entries");
static_assert(i8_front::P_END <= BN_OP_TAIL_TAG, "i8_front: fields run into the cross-kind entries");
static_assert(i8_tail::P_END <= BN_OP_EMB_ZP && (int)i8_tail::F_END <= BN_OP_EMB_SCALE, "i8_tail: fields run into the cross-kind entries");
static_assert(i8_scale::P_END <= BN_OP_TAIL_TAG, "i8_scale: fields run into the cross-kind entries");
static_assert(i8_maxnorm::P_END <= BN_OP_TAIL_TAG, "i8_maxnorm: fields run into the cross-kind entries");
static_assert(i8_rawfe::P_END <= BN_OP_TAIL_TAG, "i8_rawfe: fields run into the cross-kind entries");
static_assert(i8_attnpool::P_END <= BN_OP_EMB_ZP, "i8_attnpool: fields run into the cross-kind entries");
static_assert(i8_mid::P_END <= BN_OP_TAIL_TAG, "i8_mid: fields run into the cross-kind entries");
// The one exception: the mel-mixer fields of BN_OP_I8_DWPW (has_lut .. qfill) lie on p[34..38], the indices of BN_OP_EMB_ZP, BN_OP_EMB_DIM,
// BN_OP_EMB_TAG, BN_OP_FRONT2_DIST and BN_OP_TAIL_TAG.  It is safe because (1) the kind is never the embedding's producer and never a
// front block, so only the tag in p[38] can meet it; (2) qfill is non-zero only on the mel mixer (q_at_load), which the packer never tags
// (its tagging passes skip transposed / q_at_load blocks, and the mixer is no part of a fused chain); (3) qfill is an int8 byte and can
// never equal a tag (0x7A11....).  Blob version 5 fixes the layout, so the fields stay where they are.
static_assert(i8_dwpw::has_lut == BN_OP_EMB_ZP && i8_dwpw::strip == BN_OP_EMB_DIM && i8_dwpw::q_at_load == BN_OP_EMB_TAG &&
                  i8_dwpw::qzp == BN_OP_FRONT2_DIST && i8_dwpw::qfill == BN_OP_TAIL_TAG && i8_dwpw::P_END == BN_OP_PATH,
              "i8_dwpw: the stated overlap with the cross-kind entries");
static_assert(i8_attnpool::P == 0 && i8_attnpool::sum_zo == 16 && i8_attnpool::P_END == 17, "i8_attnpool: launch_i8_attnpool reads p[0..16] in this order");
static_assert((int)i8_stem::P_END == i8_dw::P_END && (int)f32_stem::P_END == f32_dw::P_END && (int)i8_tail::C_last - i8_tail::n_layers == i8_mid::C_last - i8_mid::n_layers, "kinds decoded by one function share their layout");

}  // namespace op
}  // namespace bn
