// bn_plan_check.hip — load-time validation of a packed device plan (host code only).
//
// bn_model_load() hands every operator record of the blob to the kernel launchers unchanged, and the kernels trust the
// geometry in OpRec.p[] for all their addressing.  A truncated, stale or hostile blob must therefore be refused HERE, with
// BN_ERR_FORMAT, instead of becoming an out-of-bounds device access: per operator kind this pass derives the bytes per
// chunk the operator reads from and writes to each slot and the bytes it reads from each constant tensor, and compares
// them with SlotRec.bytes_per_chunk / TensorRec.nbytes.  Slot ids stored in p[] (squeeze-excite gates) are checked like
// in0 / in1 / out.  Fields are addressed by the names of bn_ops.h.  The reference's counterpart is the flatbuffer verifier inside tf.lite.Interpreter
// (reference: birdnet_stm32/models/runners.py:57).
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_ops.h"

namespace bn {

namespace {

struct Checker {
    const BlobHeader& h;
    const std::vector<SlotRec>& slots;
    const std::vector<TensorRec>& tensors;
    std::string& err;
    size_t oi = 0;
    const OpRec* o = nullptr;
    bool ok = true;

    bool bad(const char* fmt, ...) {
        if (!ok) return false;  // keep the first message
        char buf[384];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = "operator " + std::to_string(oi) + " (kind " + std::to_string(o->kind) + "): " + buf;
        ok = false;
        return false;
    }

    // every dimension positive and below 2^24; byte extents are bounded by slot() (the kernels index with 32-bit integers)
    bool dims(std::initializer_list<int> v, const char* what) {
        for (int x : v)
            if (x <= 0 || x >= (1 << 24)) return bad("%s: dimension %d out of range", what, x);
        return true;
    }

    // slot `id` must be able to hold `need` bytes per chunk
    bool slot(int id, long long need, const char* what) {
        if (!ok) return false;
        if (need < 0 || need >= (1LL << 31)) return bad("%s: %lld bytes per chunk overflow 32-bit addressing", what, need);
        long long cap;
        if (id == BN_SLOT_INPUT) cap = (long long)h.input_elems * 4;
        else if (id == BN_SLOT_SCORES || id == BN_SLOT_LOGITS) cap = (long long)h.num_classes * 4;
        else if (id == BN_SLOT_AUDIO) return true;  // the caller's waveform: its length arrives with the call
        else if (id < 0 || id >= (int)slots.size()) return bad("%s: slot id %d is not a slot of this plan (%zu slots)", what, id, slots.size());
        else if (slots[id].bytes_per_chunk == 0) return bad("%s: slot %d has no storage", what, id);
        else cap = (long long)slots[id].bytes_per_chunk;
        if (need > cap) return bad("%s: needs %lld bytes per chunk, slot %d holds %lld", what, need, id, cap);
        return true;
    }

    // constant tensor t[k] must hold at least `need` bytes
    bool tensor(int k, long long need, const char* what) {
        if (!ok) return false;
        const int id = o->t[k];
        if (id < 0 || id >= (int)tensors.size()) return bad("%s: tensor t[%d] = %d is absent", what, k, id);
        if ((long long)tensors[id].nbytes < need) return bad("%s: tensor t[%d] holds %llu bytes, the operator reads %lld", what, k, (unsigned long long)tensors[id].nbytes, need);
        return true;
    }

    // clamp bounds of a value that is used as a table index (value + 128 into 256 entries): must be int8 bounds
    bool clamp8(int lo, int hi, const char* what) {
        if (lo < -128 || hi > 127 || lo > hi) return bad("%s: clamp [%d, %d] is not an int8 range (the clamped value indexes a 256-entry table)", what, lo, hi);
        return true;
    }

    bool conv_geom(int H, int W, int sh, int sw, int OH, int OW, int pt, int pl) {
        if (sh < 1 || sw < 1 || sh > 2 || sw > 2) return bad("stride %dx%d (1 or 2 expected)", sh, sw);
        if (OH != (H + sh - 1) / sh || OW != (W + sw - 1) / sw) return bad("output %dx%d does not follow from input %dx%d at stride %dx%d (SAME)", OH, OW, H, W, sh, sw);
        if (pt < 0 || pt > 1 || pl < 0 || pl > 1) return bad("padding %d/%d outside a 3x3 window", pt, pl);
        return true;
    }
};

long long up(long long v, long long m) { return (v + m - 1) / m * m; }

}  // namespace

int i8_strip_waves(int Cin, int Cout, int stride, int OW, bool add);  // bn_i8_strip.hip

bool check_plan(const BlobHeader& h, const std::vector<SlotRec>& slots, const std::vector<TensorRec>& tensors,
                const std::vector<OpRec>& ops, std::string& err) {
    Checker c{h, slots, tensors, err};
    if (h.num_classes == 0 || h.num_classes > (1u << 20) || h.input_elems == 0 || h.input_elems >= (1u << 29)) {
        err = "header: implausible num_classes / input_elems";
        return false;
    }
    for (size_t oi = 0; oi < ops.size() && c.ok; ++oi) {
        const OpRec& o = ops[oi];
        const int* p = o.p;
        c.oi = oi;
        c.o = &o;
        if (p[BN_OP_PATH] < BN_PATH_BOTH || p[BN_OP_PATH] > BN_PATH_AUDIO) c.bad("path tag %d", p[BN_OP_PATH]);
        switch (o.kind) {
            case BN_OP_F32_MEL: {
                namespace k = op::f32_mel;
                c.dims({p[k::F], p[k::W], p[k::M]}, "mel") && c.slot(o.in0, 4LL * p[k::F] * p[k::W], "input") && c.slot(o.out, 4LL * p[k::M] * p[k::W], "output") &&
                    c.tensor(k::wvals, 4, "band weights") && c.tensor(k::bands, 12LL * p[k::M], "band table") &&
                    (p[k::mag] == 0 || c.tensor(k::magp, 4LL * p[k::M], "magnitude parameters"));
                break;
            }
            case BN_OP_F32_MAG: {
                namespace k = op::f32_mag;
                c.dims({p[k::M], p[k::W]}, "mag") && c.slot(o.out, 4LL * p[k::M] * p[k::W], "map") && (p[k::mag] == 0 || c.tensor(k::magp, 4LL * p[k::M], "magnitude parameters"));
                break;
            }
            case BN_OP_F32_RAWFE: {
                namespace k = op::f32_rawfe;
                c.dims({p[k::T], p[k::W], p[k::M], p[k::stride]}, "raw frontend") && c.slot(o.in0, 4LL * p[k::T], "waveform") && c.slot(o.out, 4LL * p[k::M] * p[k::W], "output") &&
                    c.tensor(k::fb, 64LL * p[k::M], "filterbank") && c.tensor(k::bias, 4LL * p[k::M], "bias") &&
                    (p[k::mag] == 0 || c.tensor(k::magp, 4LL * p[k::M], "magnitude parameters"));
                if (c.ok && p[k::pad_left] < 0) c.bad("negative left padding");
                if (c.ok && p[k::W] % 4) c.bad("raw frontend width %d is not a multiple of 4 (the kernel stores dwords of one filter)", p[k::W]);
                break;
            }
            case BN_OP_F32_STEM:
            case BN_OP_F32_DW: {
                namespace k = op::f32_dw;  // (F32_STEM: the same layout, C = Cout)
                const long long cin = o.kind == BN_OP_F32_STEM ? 1 : p[k::C];
                c.dims({p[k::H], p[k::W], p[k::C], p[k::OH], p[k::OW]}, "conv") && c.conv_geom(p[k::H], p[k::W], p[k::sh], p[k::sw], p[k::OH], p[k::OW], p[k::pt], p[k::pl]) &&
                    c.slot(o.in0, 4LL * p[k::H] * p[k::W] * cin, "input") && c.slot(o.out, 4LL * p[k::OH] * p[k::OW] * p[k::C], "output") &&
                    c.tensor(k::w, 36LL * p[k::C], "weights") && c.tensor(k::bias, 4LL * p[k::C], "bias");
                break;
            }
            case BN_OP_F32_PW: {
                namespace k = op::f32_pw;
                c.dims({p[k::P], p[k::Cin], p[k::Cout]}, "pointwise") && c.slot(o.in0, 4LL * p[k::P] * p[k::Cin], "input") && c.slot(o.out, 4LL * p[k::P] * p[k::Cout], "output") &&
                    (!p[k::has_res] || c.slot(o.in1, 4LL * p[k::P] * p[k::Cout], "residual")) && (!p[k::has_gate] || c.slot(p[k::gate_slot], 4LL * p[k::Cin], "gate")) &&
                    c.tensor(k::w, 4LL * p[k::Cin] * p[k::Cout], "weights") && c.tensor(k::bias, 4LL * p[k::Cout], "bias");
                break;
            }
            case BN_OP_F32_SEGATE: {
                namespace k = op::f32_segate;
                c.dims({p[k::P], p[k::C], p[k::Cr]}, "squeeze-excite") && c.slot(o.in0, 4LL * p[k::P] * p[k::C], "input") && c.slot(o.out, 4LL * p[k::C], "gate") &&
                    c.tensor(k::w1, 4LL * p[k::C] * p[k::Cr], "reduce weights") && c.tensor(k::w2, 4LL * p[k::C] * p[k::Cr], "expand weights");
                break;
            }
            case BN_OP_F32_SCALE: {
                namespace k = op::f32_scale;
                c.dims({p[k::P], p[k::C]}, "scale") && c.slot(o.in0, 4LL * p[k::P] * p[k::C], "input") && c.slot(o.in1, 4LL * p[k::C], "gate") &&
                    c.slot(o.out, 4LL * p[k::P] * p[k::C], "output");
                break;
            }
            case BN_OP_F32_GAP:
            case BN_OP_F32_ATTNPOOL: {
                namespace k = op::f32_attnpool;  // (F32_GAP: the same P, C; no tensor)
                c.dims({p[k::P], p[k::C]}, "pool") && c.slot(o.in0, 4LL * p[k::P] * p[k::C], "input") && c.slot(o.out, 4LL * p[k::C], "output") &&
                    (o.kind == BN_OP_F32_GAP || c.tensor(k::score, 4LL * p[k::C], "score vector"));
                break;
            }
            case BN_OP_F32_DENSE: {
                namespace k = op::f32_dense;
                c.dims({p[k::Cin], p[k::Cout]}, "dense") && c.slot(o.in0, 4LL * p[k::Cin], "input") && c.slot(o.out, 4LL * p[k::Cout], "scores") &&
                    c.tensor(k::w, 4LL * p[k::Cin] * p[k::Cout], "weights") && c.tensor(k::bias, 4LL * p[k::Cout], "bias");
                if (c.ok && p[k::Cout] != (int)h.num_classes) c.bad("classifier width %d, header says %u classes", p[k::Cout], h.num_classes);
                break;
            }
            case BN_OP_F32_GAPDENSE: {
                namespace k = op::f32_gapdense;
                c.dims({p[k::P], p[k::Cin], p[k::Cout]}, "pool+dense") && c.slot(o.in0, 4LL * p[k::P] * p[k::Cin], "input") && c.slot(o.out, 4LL * p[k::Cout], "scores") &&
                    c.tensor(k::w, 4LL * p[k::Cin] * p[k::Cout], "weights") && c.tensor(k::bias, 4LL * p[k::Cout], "bias");
                if (c.ok && p[k::Cout] != (int)h.num_classes) c.bad("classifier width %d, header says %u classes", p[k::Cout], h.num_classes);
                break;
            }
            case BN_OP_F32_DWPW: {
                namespace k = op::f32_dwpw;
                const long long out_b = 4LL * p[k::OH] * p[k::OW] * p[k::Cout];
                c.dims({p[k::H], p[k::W], p[k::Cin], p[k::OH], p[k::OW], p[k::Cout]}, "fused block") && c.slot(o.in0, 4LL * p[k::H] * p[k::W] * p[k::Cin], "input") &&
                    c.slot(o.out, out_b, "output") && (!p[k::has_res] || c.slot(o.in1, out_b, "residual")) &&
                    (!p[k::has_gate] || c.slot(p[k::gate_slot], 4LL * p[k::Cin], "gate")) && c.tensor(k::pw_w, 4LL * up(p[k::Cin], 16) * p[k::Cout], "pointwise weights") &&
                    c.tensor(k::pw_b, 4LL * p[k::Cout], "pointwise bias");
                if (c.ok && p[k::has_dw])
                    c.conv_geom(p[k::H], p[k::W], p[k::sh], p[k::sw], p[k::OH], p[k::OW], p[k::pt], p[k::pl]) && c.tensor(k::dw_w, 36LL * p[k::Cin], "depthwise weights") &&
                        c.tensor(k::dw_b, 4LL * p[k::Cin], "depthwise bias");
                if (c.ok && !p[k::has_dw] && (p[k::H] != p[k::OH] || p[k::W] != p[k::OW])) c.bad("plain 1x1 convolution must keep the map size");
                if (c.ok && (p[k::TH] < 1 || p[k::TW] < 1 || p[k::NB] < 1)) c.bad("tile %dx%dx%d", p[k::TH], p[k::TW], p[k::NB]);
                break;
            }
            case BN_OP_F32_STFTMEL: {
                namespace k = op::f32_stftmel;
                c.dims({p[k::W], p[k::M]}, "stft+mel") && c.slot(o.out, 4LL * p[k::M] * p[k::W], "mel energies") && c.tensor(k::wvals, 4, "band weights") &&
                    c.tensor(k::bands, 12LL * p[k::M], "band table");
                break;
            }
            case BN_OP_F32_MELFIN: {
                namespace k = op::f32_melfin;
                c.dims({p[k::M], p[k::W]}, "mel finish") && c.slot(o.in0, 4LL * p[k::M] * p[k::W], "input") && c.slot(o.out, 4LL * p[k::M] * p[k::W], "output") &&
                    c.tensor(k::wsum, 4LL * p[k::M], "band sums") && (p[k::mag] == 0 || c.tensor(k::magp, 4LL * p[k::M], "magnitude parameters"));
                break;
            }
            case BN_OP_F32_FRONT: {
                namespace k = op::f32_front;
                c.dims({p[k::H0], p[k::W0], p[k::C], p[k::N], p[k::OH], p[k::OW]}, "front block") && c.slot(o.in0, 4LL * p[k::H0] * p[k::W0], "frontend map") &&
                    c.slot(o.out, 4LL * p[k::OH] * p[k::OW] * p[k::N], "output") && c.tensor(k::stem_w, 36LL * p[k::C], "stem weights") &&
                    c.tensor(k::stem_b, 4LL * p[k::C], "stem bias") && c.tensor(k::dw_w, 36LL * p[k::C], "depthwise weights") &&
                    c.tensor(k::dw_b, 4LL * p[k::C], "depthwise bias") && c.tensor(k::pw_w, 4LL * up(p[k::C], 16) * p[k::N], "pointwise weights") &&
                    c.tensor(k::pw_b, 4LL * p[k::N], "pointwise bias") &&
                    (!p[k::raw_mel] || (c.tensor(k::wsum, 4LL * p[k::H0], "band sums") && (p[k::mag] == 0 || c.tensor(k::magp, 4LL * p[k::H0], "magnitude parameters"))));
                if (c.ok && (p[k::OH] != (p[k::H0] + 1) / 2 || p[k::OW] != ((p[k::W0] + 1) / 2 + 1) / 2))
                    c.bad("front block output %dx%d does not follow from %dx%d", p[k::OH], p[k::OW], p[k::H0], p[k::W0]);
                break;
            }
            case BN_OP_I8_QUANT: {
                namespace k = op::i8_quant;
                c.dims({p[k::F], p[k::W], p[k::Kp]}, "quantise") && c.slot(o.in0, 4LL * p[k::F] * p[k::W], "spectrogram") && c.slot(o.out, 1LL * p[k::W] * p[k::Kp], "output");
                if (c.ok && p[k::Kp] < p[k::F]) c.bad("padded bin count %d below %d bins", p[k::Kp], p[k::F]);
                break;
            }
            case BN_OP_I8_MEL: {
                namespace k = op::i8_mel;
                c.dims({p[k::W], p[k::Kp], p[k::M]}, "mel") && c.slot(o.in0, 1LL * p[k::W] * p[k::Kp], "input") && c.slot(o.out, 1LL * p[k::M] * p[k::W], "output") &&
                    c.tensor(k::w, 1LL * p[k::M] * p[k::Kp], "weights") && c.tensor(k::bias, 4LL * p[k::M], "bias") && c.tensor(k::mult, 4LL * p[k::M], "multipliers") &&
                    c.tensor(k::shift, 4LL * p[k::M], "shifts") && (!p[k::has_lut] || c.tensor(k::lut, 256LL * p[k::M], "table"));
                if (c.ok && p[k::has_lut]) c.clamp8(p[k::act_min], p[k::act_max], "mel");  // the clamped value + 128 indexes the 256-entry table
                break;
            }
            case BN_OP_I8_STEM:
            case BN_OP_I8_DW: {
                namespace k = op::i8_dw;  // (I8_STEM: the same layout, C = Cout)
                const long long cin = o.kind == BN_OP_I8_STEM ? 1 : p[k::C];
                c.dims({p[k::H], p[k::W], p[k::C], p[k::OH], p[k::OW]}, "conv") && c.conv_geom(p[k::H], p[k::W], p[k::sh], p[k::sw], p[k::OH], p[k::OW], p[k::pt], p[k::pl]) &&
                    c.slot(o.in0, 1LL * p[k::H] * p[k::W] * cin, "input") && c.slot(o.out, 1LL * p[k::OH] * p[k::OW] * p[k::C], "output") && c.tensor(k::w, 9LL * p[k::C], "weights") &&
                    c.tensor(k::bias, 4LL * p[k::C], "bias") && c.tensor(k::mult, 4LL * p[k::C], "multipliers") && c.tensor(k::shift, 4LL * p[k::C], "shifts");
                break;
            }
            case BN_OP_I8_PW: {
                namespace k = op::i8_pw;
                c.dims({p[k::P], p[k::Cin], p[k::Cout]}, "pointwise") && c.slot(o.in0, 1LL * p[k::P] * p[k::Cin], "input") && c.slot(o.out, 1LL * p[k::P] * p[k::Cout], "output") &&
                    (!p[k::has_add] || c.slot(o.in1, 1LL * p[k::P] * p[k::Cout], "residual")) && c.tensor(k::w, 1LL * p[k::Cin] * p[k::Cout], "weights") &&
                    c.tensor(k::bias, 4LL * p[k::Cout], "bias") && c.tensor(k::mult, 4LL * p[k::Cout], "multipliers") && c.tensor(k::shift, 4LL * p[k::Cout], "shifts");
                break;
            }
            case BN_OP_I8_MEAN: {
                namespace k = op::i8_mean;
                c.dims({p[k::P], p[k::C]}, "mean") && c.slot(o.in0, 1LL * p[k::P] * p[k::C], "input") && c.slot(o.out, 1LL * p[k::C], "output");
                break;
            }
            case BN_OP_I8_FC: {
                namespace k = op::i8_fc;
                c.dims({p[k::Cin], p[k::Cout]}, "fully connected") && c.slot(o.in0, 1LL * p[k::Cin], "input") && c.slot(o.out, 1LL * p[k::Cout], "output") &&
                    c.tensor(k::w, up(p[k::Cin], 4) * p[k::Cout], "weights") && c.tensor(k::bias, 4LL * p[k::Cout], "bias") && c.tensor(k::mult, 4LL * p[k::Cout], "multipliers") &&
                    c.tensor(k::shift, 4LL * p[k::Cout], "shifts") && (!p[k::has_lut] || c.tensor(k::lut, 256, "table"));
                if (c.ok && p[k::has_lut]) c.clamp8(p[k::act_min], p[k::act_max], "fully connected");
                break;
            }
            case BN_OP_I8_SCALE: {
                namespace k = op::i8_scale;
                c.dims({p[k::P], p[k::C]}, "scale") && c.slot(o.in0, 1LL * p[k::P] * p[k::C], "input") && c.slot(o.in1, 1LL * p[k::C], "gate") &&
                    c.slot(o.out, 1LL * p[k::P] * p[k::C], "output");
                if (c.ok && p[k::C] % 4) c.bad("channel count %d is not a multiple of 4", p[k::C]);
                break;
            }
            case BN_OP_I8_MAXNORM: {
                namespace k = op::i8_maxnorm;
                c.dims({p[k::C], p[k::W]}, "max normalisation") && c.slot(o.in0, 1LL * p[k::C] * p[k::W], "input") && c.slot(o.out, 1LL * p[k::C] * p[k::W], "output") &&
                    c.tensor(k::denom, 256, "denominator table") && c.tensor(k::div, 65536, "division table") && (!p[k::has_lut] || c.tensor(k::lut, 256LL * p[k::C], "channel table"));
                if (c.ok && p[k::W] % 4) c.bad("map width %d is not a multiple of 4 (the kernel reads dwords of one channel)", p[k::W]);
                break;
            }
            case BN_OP_I8_RAWFE: {
                namespace k = op::i8_rawfe;
                c.dims({p[k::T], p[k::W], p[k::M], p[k::stride]}, "raw frontend") && c.slot(o.in0, 4LL * p[k::T], "waveform") && c.slot(o.out, 1LL * p[k::M] * p[k::W], "output") &&
                    c.tensor(k::w, 16LL * p[k::M], "filterbank") && c.tensor(k::bias, 4LL * p[k::M], "bias") && c.tensor(k::mult, 4LL * p[k::M], "multipliers") &&
                    c.tensor(k::shift, 4LL * p[k::M], "shifts") && (!p[k::has_lut] || c.tensor(k::lut, 256LL * p[k::M], "table"));
                if (c.ok && p[k::pad_left] < 0) c.bad("negative left padding");
                if (c.ok && p[k::has_lut]) c.clamp8(p[k::act_min], p[k::act_max], "raw frontend");
                if (c.ok && p[k::W] % 4) c.bad("raw frontend width %d is not a multiple of 4 (the kernel stores dwords of one filter)", p[k::W]);
                break;
            }
            case BN_OP_I8_ATTNPOOL: {
                namespace k = op::i8_attnpool;
                c.dims({p[k::P], p[k::C]}, "attention pooling") && c.slot(o.in0, 1LL * p[k::P] * p[k::C], "input map") && c.slot(o.out, 1LL * p[k::C], "output") &&
                    c.tensor(k::score, 1LL * p[k::C], "score vector") && c.tensor(k::tables, p[k::form] == 0 ? 2048 : 1024, "softmax tables");
                if (c.ok && (p[k::C] % 4 || p[k::P] > 4096 || 1LL * p[k::P] * p[k::C] + 2LL * p[k::P] + 32 > 64 * 1024))  // (P <= 4096: the int32 sum of the exponentials)
                    c.bad("attention pooling map %d x %d does not fit the kernel", p[k::P], p[k::C]);
                if (c.ok && (p[k::form] < 0 || p[k::form] > 1)) c.bad("softmax form %d", p[k::form]);
                if (c.ok) c.clamp8(p[k::mul_lo], p[k::mul_hi], "attention pooling MUL");
                break;
            }
            case BN_OP_I8_HEAD: {
                namespace k = op::i8_head;
                c.dims({p[k::C]}, "head") && c.slot(o.in0, 1LL * p[k::C], "input") && c.slot(o.out, 4LL * p[k::C], "scores") && (!p[k::has_lut] || c.tensor(k::lut, 256, "table"));
                if (c.ok && p[k::C] != (int)h.num_classes) c.bad("classifier width %d, header says %u classes", p[k::C], h.num_classes);
                break;
            }
            case BN_OP_I8_DWPW: {
                namespace k = op::i8_dwpw;
                const long long out_b = 1LL * p[k::OH] * p[k::OW] * p[k::Cout];
                c.dims({p[k::H], p[k::W], p[k::Cin], p[k::OH], p[k::OW], p[k::Cout]}, "fused block");
                if (c.ok && p[k::q_at_load]) c.dims({p[k::qF]}, "spectrogram bins") && c.slot(o.in0, 4LL * p[k::qF] * p[k::W], "spectrogram");
                else c.slot(o.in0, 1LL * p[k::H] * p[k::W] * p[k::Cin], "input");
                c.slot(o.out, out_b, "output") && (!p[k::has_add] || c.slot(o.in1, out_b, "residual")) && c.tensor(k::pw_w, up(p[k::Cin], 64) * p[k::Cout], "pointwise weights") &&
                    c.tensor(k::pw_b, 4LL * p[k::Cout], "pointwise bias") && c.tensor(k::pw_mult, 4LL * p[k::Cout], "pointwise multipliers") &&
                    c.tensor(k::pw_shift, 4LL * p[k::Cout], "pointwise shifts") && (!p[k::has_lut] || c.tensor(k::lut, 256LL * p[k::Cout], "table"));
                if (c.ok && p[k::has_dw])
                    c.conv_geom(p[k::H], p[k::W], p[k::sh], p[k::sw], p[k::OH], p[k::OW], p[k::pt], p[k::pl]) && c.tensor(k::dw_w, 9LL * p[k::Cin], "depthwise weights") &&
                        c.tensor(k::dw_b, 4LL * p[k::Cin], "depthwise bias") && c.tensor(k::dw_mult, 4LL * p[k::Cin], "depthwise multipliers") &&
                        c.tensor(k::dw_shift, 4LL * p[k::Cin], "depthwise shifts");
                if (c.ok && !p[k::has_dw] && (p[k::H] != p[k::OH] || p[k::W] != p[k::OW])) c.bad("plain 1x1 convolution must keep the map size");
                if (c.ok && !p[k::has_dw] && p[k::has_add] && o.t[k::add_tab] >= 0) c.tensor(k::add_tab, 65536, "ADD table");
                if (c.ok && (p[k::TH] < 1 || p[k::TW] < 1 || p[k::NB] < 1)) c.bad("tile %dx%dx%d", p[k::TH], p[k::TW], p[k::NB]);
                // the transposed form is the mel mixer: a plain 1x1 over the frames of one chunk, no residual; only it takes a table or float32 input
                if (c.ok && p[k::transposed] && (p[k::has_dw] || p[k::has_add] || p[k::H] != 1 || p[k::OH] != 1 || p[k::NB] != 1))
                    c.bad("transposed output on a block that is not a mel mixer");
                if (c.ok && !p[k::transposed] && (p[k::has_lut] || p[k::q_at_load])) c.bad("table / fused QUANTIZE on a block without transposed output");
                if (c.ok && p[k::has_lut]) c.clamp8(p[k::pw_amin], p[k::pw_amax], "mel mixer");
                if (c.ok && p[k::has_add])  // both index the 256-entry rescale tables
                    c.clamp8(p[k::pw_amin], p[k::pw_amax], "block with ADD") && c.clamp8(p[k::add_amin], p[k::add_amax], "ADD");
                if (c.ok && p[k::strip] && o.t[k::strip_cst] >= 0) {  // constant block of the strip kernel (bn_i8_strip.hip: kPWC + NW * nPWC words)
                    const int nw = p[k::sh] == p[k::sw] ? i8_strip_waves(p[k::Cin], p[k::Cout], p[k::sh], p[k::OW], p[k::has_add] != 0) : 0;
                    if (nw) {
                        const long long ql = p[k::Cin] / nw / 16, nt = p[k::Cout] / nw / 16;
                        const long long words = nw * (4 * ql * 12 + 4 * ql * 4 + 4 * ql * 12 + nt * nw * 64 * ql + 4 * nt * 4 + 4 * nt * 12);
                        c.tensor(k::strip_cst, 4 * words, "strip constants") && (!p[k::has_add] || o.t[k::add_tab] < 0 || c.tensor(k::add_tab, 65536, "ADD table"));
                    }
                }
                break;
            }
            case BN_OP_I8_FRONT: {
                namespace k = op::i8_front;
                c.dims({p[k::H0], p[k::W0], p[k::C], p[k::N], p[k::OH], p[k::OW]}, "front block") && c.slot(o.in0, 1LL * p[k::H0] * p[k::W0], "frontend map") &&
                    c.slot(o.out, 1LL * p[k::OH] * p[k::OW] * p[k::N], "output") && c.tensor(k::stem_w, 9LL * p[k::C], "stem weights") &&
                    c.tensor(k::stem_b, 4LL * p[k::C], "stem bias") && c.tensor(k::stem_mult, 4LL * p[k::C], "stem multipliers") &&
                    c.tensor(k::stem_shift, 4LL * p[k::C], "stem shifts") && c.tensor(k::dw_w, 9LL * p[k::C], "depthwise weights") &&
                    c.tensor(k::dw_b, 4LL * p[k::C], "depthwise bias") && c.tensor(k::dw_mult, 4LL * p[k::C], "depthwise multipliers") &&
                    c.tensor(k::dw_shift, 4LL * p[k::C], "depthwise shifts") && c.tensor(k::pw_w, up(p[k::C], 64) * p[k::N], "pointwise weights") &&
                    c.tensor(k::pw_b, 4LL * p[k::N], "pointwise bias") && c.tensor(k::pw_mult, 4LL * p[k::N], "pointwise multipliers") &&
                    c.tensor(k::pw_shift, 4LL * p[k::N], "pointwise shifts") && (!p[k::strip] || o.t[k::strip_cst] < 0 || c.tensor(k::strip_cst, 496 * 4, "strip constants"));
                if (c.ok && (p[k::OH] != (p[k::H0] + 1) / 2 || p[k::OW] != ((p[k::W0] + 1) / 2 + 1) / 2))
                    c.bad("front block output %dx%d does not follow from %dx%d", p[k::OH], p[k::OW], p[k::H0], p[k::W0]);
                break;
            }
            case BN_OP_I8_TAIL: {
                namespace k = op::i8_tail;
                c.dims({p[k::in_bytes], p[k::n_classes], p[k::n_layers], p[k::H0], p[k::W0], p[k::C0]}, "fused tail") &&
                    c.slot(o.in0, 1LL * p[k::H0] * p[k::W0] * p[k::C0], "input map") && c.slot(o.out, 4LL * p[k::n_classes], "scores") &&
                    c.tensor(k::cst, 16, "constant block") && c.tensor(k::desc, 4LL * (kTailLayerWords * p[k::n_layers] + kTailHeadWords), "descriptor table");
                if (c.ok && (p[k::n_classes] != (int)h.num_classes || p[k::n_layers] > 8 || p[BN_OP_TAIL_TAG] != BN_TAIL_OP)) c.bad("fused tail header");
                break;  // the descriptor table itself is validated by bn::tail_plan (bn_chain_plan.cpp) at load (bn_plan_run.hip: prepare_plan)
            }
            case BN_OP_I8_MID: {
                namespace k = op::i8_mid;
                c.dims({p[k::in_bytes], p[k::n_layers], p[k::H0], p[k::W0], p[k::C0], p[k::P_last], p[k::C_last]}, "fused stage-2 chain") &&
                    c.slot(o.in0, 1LL * p[k::H0] * p[k::W0] * p[k::C0], "input map") && c.slot(o.out, 1LL * p[k::P_last] * p[k::C_last], "output map") &&
                    c.tensor(k::cst, 16, "constant block") && c.tensor(k::desc, 4LL * kTail2LayerWords * p[k::n_layers], "descriptor table");
                if (c.ok && (p[k::n_layers] > 8 || p[BN_OP_TAIL_TAG] != BN_MID_OP)) c.bad("fused stage-2 chain header");
                break;  // (descriptor table: bn::tail2_plan, bn_chain_plan.cpp, at load)
            }
            default:
                c.bad("unknown operator kind");
                break;
        }
    }
    return c.ok;
}

}  // namespace bn
