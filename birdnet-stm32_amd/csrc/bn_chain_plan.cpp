// bn_chain_plan.cpp — the host side of the fused INT8 chains: kernel arguments from the packer's descriptor tables, and where every block's
// maps, weights and constants lie in the 160 KB of LDS a workgroup of i8_tail_kernel (bn_i8_tail.hip), i8_tail2_kernel or i8_mid2_kernel
// (bn_i8_tail2.hip) owns.  These functions decide which offsets the kernels address, whether a chain is fused at all, and whether a stale
// or hostile table is refused before a kernel trusts it.  Plain C++: tests/test_chain_plan_host.py runs them on the CPU under sanitizers.
#include "bn_chain_plan.h"

#include <algorithm>
#include <vector>

namespace bn {
namespace {

constexpr int kLdsCap = 160 * 1024;   // LDS of a CU: what one workgroup of a fused chain may plan with
// (the stamped measurement build, `make stamps`, keeps the top 16 bytes free for the chunk barriers' counters: its staged plans get them too)
#ifdef BN_TAIL_STAMPS
constexpr int kStampBytes = 16;
#else
constexpr int kStampBytes = 0;
#endif

// first-fit allocator over the workgroup's LDS: `used` holds [begin, end) intervals that must stay intact
struct Span {
    int b, e;
};
bool overlap(Span p, Span q) { return p.b < q.e && q.b < p.e; }
int first_fit(std::vector<Span>& used, int bytes, int cap) {
    bytes = (bytes + 15) & ~15;
    int pos = 0;
    for (;;) {
        bool moved = false;
        for (const Span& s : used)
            if (overlap({pos, pos + bytes}, s)) {
                pos = (s.e + 15) & ~15;
                moved = true;
            }
        if (!moved) break;
    }
    if (pos + bytes > cap) return -1;
    used.push_back({pos, pos + bytes});
    return pos;
}

// The block shapes the kernels are instantiated for (the `if (L.Cin == ...)` chains of tail_main / tail2_main and of mid2_main): the first
// entry is the chain's first block, whose taps come from memory; the others may follow it in any order.  Even maps of at most 32 x 64
// positions, stride 1 or 2 (SAME padding: 1 / 1 at stride 1, 0 / 1 at stride 2), output positions a multiple of the 16 of a tile.
struct BlockShape {
    int Cin, Cout, S, H, W, has_add;
};
constexpr BlockShape kTailShapes[] = {{64, 128, 2, 16, 32, 0}, {128, 128, 1, 8, 16, 1}, {128, 256, 2, 8, 16, 0}, {256, 256, 1, 4, 8, 1}};
constexpr BlockShape kMidShapes[] = {{32, 64, 2, 32, 64, 0}, {64, 64, 1, 16, 32, 1}};
// block i of the chain `layers` has one of the shapes, and its input is what block i - 1 stores
template <class Layer, int N>
bool shape_ok(const Layer* layers, int i, const BlockShape (&shapes)[N]) {
    const Layer& L = layers[i];
    if (i > 0 && (L.H != layers[i - 1].OH || L.W != layers[i - 1].OW || L.Cin != layers[i - 1].Cout)) return false;
    for (int k = i == 0 ? 0 : 1; k < (i == 0 ? 1 : N); ++k) {
        const BlockShape& s = shapes[k];
        if (L.Cin == s.Cin && L.Cout == s.Cout && L.S == s.S && L.H == s.H && L.W == s.W && L.has_add == s.has_add && L.pt == (s.S == 1) &&
            L.pl == (s.S == 1) && L.OH == s.H / s.S && L.OW == s.W / s.S)
            return true;
    }
    return false;
}
// a clamp whose result is stored as a byte or indexes a 256-entry table (off: the value is kept + off)
bool int8_range(int lo, int hi, int off = 0) { return lo >= -128 + off && hi <= 127 + off && lo <= hi; }

// the 20 descriptor words both forms' blocks start with, and the 16 head words behind the last block
template <class Layer>
void read_layer(const int32_t* d, Layer& L) {
    L.H = d[0]; L.W = d[1]; L.Cin = d[2]; L.Cout = d[3]; L.S = d[4]; L.OH = d[5]; L.OW = d[6]; L.pt = d[7]; L.pl = d[8]; L.has_add = d[9];
    L.zp_in = d[10]; L.dw_lo = d[11]; L.dw_hi = d[12]; L.pw_lo = d[13]; L.pw_hi = d[14];
    L.add_m = d[15]; L.add_c1 = d[16]; L.add_e = d[17]; L.add_lo = d[18]; L.add_hi = d[19];
}
template <class Args>
void read_head(const int32_t* h, Args& a) {
    a.mean_zp_in = h[0]; a.mean_mult = h[1]; a.mean_shift = h[2]; a.mean_zp_out = h[3];
    a.fc_zp_out = h[4]; a.fc_lo = h[5]; a.fc_hi = h[6]; a.g_fcw = h[7]; a.g_fcb = h[8]; a.g_fcm = h[9]; a.g_fcs = h[10]; a.g_hlut = h[11];
    a.head_zp_fc = h[12]; a.head_zp_out = h[13]; a.P = h[14]; a.C = h[15];
}

}  // namespace

// Build the kernel arguments from the descriptor table the packer wrote (24 words per block + 16 head words) and plan the LDS of
// every block.  Returns false when the topology is not one the kernel takes or a block's maps do not fit 160 KB.
bool tail_plan(const int32_t* desc, int n_words, int n_layers, Tail8Args& a) {
    constexpr int LW = kTailLayerWords, HW = kTailHeadWords, CAP = kLdsCap;
    if (n_layers < 1 || n_layers > 8 || n_words != LW * n_layers + HW) return false;
    a.n_layers = n_layers;
    int cur_off = -1;   // where the current input map lives (-1: global memory)
    int lds_need = 0;
    for (int i = 0; i < n_layers; ++i) {
        const int32_t* d = desc + LW * i;
        Tail8Layer& L = a.L[i];
        read_layer(d, L);
        L.g_w = d[20]; L.g_dwc = d[21]; L.g_pwc = d[22]; L.g_lut = d[23];
        if (!shape_ok(a.L, i, kTailShapes)) return false;
        if (L.has_add && (L.Cin != L.Cout || L.S != 1 || L.g_lut < 0 || L.add_e < 1 || L.add_e > 22 || L.add_m < 0)) return false;
        const int tiles = kTailG * L.OH * L.OW / 16;
        if (tiles < kTailWaves && (kTailWaves % tiles || (L.Cout / 16) % (kTailWaves / tiles))) return false;
        if ((L.g_w | L.g_dwc | L.g_pwc) & 3 || (L.has_add && (L.g_lut & 3))) return false;
        // offsets into the constant block start at 0 (tail_const_words bounds them from above: a stale or hostile blob must not make the
        // kernel read in front of the block), and every clamp whose result indexes a table or is stored as a byte is an int8 range
        // (+ 128 where the pointwise value of a residual block is kept as the index of the second ADD table)
        if (L.g_w < 0 || L.g_dwc < 0 || L.g_pwc < 0 || (L.has_add && L.g_lut < 0)) return false;
        if (!int8_range(L.dw_lo, L.dw_hi) || !int8_range(L.pw_lo, L.pw_hi, L.has_add ? 128 : 0)) return false;
        if (L.has_add && !int8_range(L.add_lo, L.add_hi)) return false;
        std::vector<Span> used;
        L.x_off = cur_off;
        if (cur_off >= 0) used.push_back({cur_off, cur_off + kTailG * L.H * L.W * (L.Cin + 4)});
        L.y_off = first_fit(used, kTailG * L.OH * L.OW * (L.Cout + 4), CAP);
        L.w_off = first_fit(used, L.Cin * L.Cout, CAP);
        L.dwc_off = first_fit(used, L.Cin * 32 + 64, CAP);   // staged in rq_hi form: 8 x 16 bytes per channel quad (+ up to four slots of skew),
        L.pwc_off = first_fit(used, L.Cout * 20, CAP);  // 5 x 16 bytes per four output channels
        L.lut_off = L.has_add ? first_fit(used, 2048, CAP) : 0;
        L.zp_off = first_fit(used, L.Cin + 16, CAP);
        if (L.y_off < 0 || L.w_off < 0 || L.dwc_off < 0 || L.pwc_off < 0 || L.lut_off < 0 || L.zp_off < 0) return false;
        if (i == n_layers - 1) {
            a.mean_off = first_fit(used, kTailG * L.Cout, CAP);
            if (a.mean_off < 0) return false;
        }
        for (const Span& s : used) lds_need = s.e > lds_need ? s.e : lds_need;
        cur_off = L.y_off;
    }
    read_head(desc + LW * n_layers, a);
    if (a.g_fcw < 0 || a.g_fcb < 0 || a.g_fcm < 0 || a.g_fcs < 0 || a.g_hlut < -1 || (a.g_fcw & 3)) return false;
    if (!int8_range(a.fc_lo, a.fc_hi)) return false;  // (the classifier byte + 128 indexes the head's table)
    const Tail8Layer& last = a.L[n_layers - 1];
    if (a.P != last.OH * last.OW || a.C != last.Cout || a.C % 4 || a.NC < 1 || kTailG * a.NC > kTailThreads * 4) return false;
    // the head's LDS copy of the classifier matrix overlays the last block's pointwise weights (4 x 1024 threads x 16 bytes are staged at most)
    const int fc_bytes = a.NC * (a.C / 4 + 1) * 4;
    a.fcw_off = (a.C % 16 == 0 && fc_bytes <= last.Cin * last.Cout && a.NC * (a.C / 16) <= 4 * kTailThreads) ? last.w_off : -1;
    a.lds_bytes = lds_need;
    return true;
}

// words of the constant block the kernel reads (for the load-time check of the tensor's size)
long tail_const_words(const Tail8Args& a) {
    long need = 0;
    auto upto = [&](long off, long words) { need = off + words > need ? off + words : need; };
    for (int i = 0; i < a.n_layers; ++i) {
        const Tail8Layer& L = a.L[i];
        upto(L.g_w, (long)L.Cin * L.Cout / 4);
        upto(L.g_dwc, (long)L.Cin * 7);
        upto(L.g_pwc, (long)L.Cout * 4);
        if (L.has_add) upto(L.g_lut, 512);
    }
    upto(a.g_fcw, (long)a.NC * a.C / 4);
    upto(a.g_fcb, a.NC);
    upto(a.g_fcm, a.NC);
    upto(a.g_fcs, a.NC);
    if (a.g_hlut >= 0) upto(a.g_hlut, 64);
    return need;
}

namespace {

Span dw_span(const Tail2Layer& L, bool first) { return {L.dw_off, L.dw_off + tail2_dw_bytes(L, first)}; }
// the map of a block of the second form sits at LDS offset 0, input and output in place: G chunks, a pitch of C + 16 bytes
int tail2_map_bytes(const Tail2Layer& L, bool first, int G) {
    return std::max(first ? 0 : G * L.H * L.W * (L.Cin + 16), G * L.OH * L.OW * (L.Cout + 16));
}
// the chunk barriers' counters (one dword per chunk slot) above everything else; the staged forms use them in the stamped measurement build
// only, so a staged plan that fills the LDS to the last byte stays valid without them (bar_off = -1: that build then stamps no chunk barrier)
void tail2_place_counters(Tail2Args& a) {
    a.bar_off = (a.lds_bytes + 15) & ~15;
    if (a.bar_off + 16 > kLdsCap) a.bar_off = -1;
    else a.lds_bytes = a.bar_off + 16;
}

}  // namespace

// Kernel arguments and LDS plan from the packer's descriptor table (32 words per block + 16 head words).  A block's map sits at LDS
// offset 0 (input and output in place).  Its depthwise part and zero-point row are written while the PREVIOUS block's pointwise phase
// runs: they avoid that block's output map (= this block's input) and pointwise part; its pointwise part is written while its own
// depthwise phase runs: it avoids the map, the zero-point row and the depthwise part.  The first block's depthwise part is written behind
// the last block of the previous group and stays through the head: it avoids the last map, the last pointwise part, the pooled vector and
// the head's copy of the classifier matrix.  false = not a topology / size the kernel takes (the plan keeps i8_tail_kernel).
bool tail2_plan(const int32_t* desc, int n_words, int n_layers, Tail2Args& a, bool mid) {
    constexpr int LW = kTail2LayerWords, CAP = kLdsCap - kStampBytes;
    const int HW = mid ? 0 : kTailHeadWords, G = mid ? kMidG : kTailG;
    if (n_layers < 1 || n_layers > 8 || n_words != LW * n_layers + HW) return false;
    a.n_layers = n_layers;
    int lds_need = 0;
    Span prev_pw{0, 0}, map_last{0, 0};
    auto grow = [&](int end) { lds_need = end > lds_need ? end : lds_need; };
    // The first block's depthwise part is the one piece whose neighbours in time are at BOTH ends of the chain (it is written behind the last
    // block's pointwise phase): placed by first fit like the others it can collide with the last block's parts, so a second attempt puts it at
    // the top of the LDS.
    for (int attempt = 0; attempt < 2; ++attempt) {
        lds_need = 0;
        prev_pw = {0, 0};
        for (int i = 0; i < n_layers; ++i) {
            const int32_t* d = desc + LW * i;
            Tail2Layer& L = a.L[i];
            read_layer(d, L);
            L.res_m = d[20]; L.res_c_lo = d[21]; L.res_c_hi = d[22]; L.res_k = d[23]; L.g_cst = d[24];
            const bool first = i == 0;
            if (!(mid ? shape_ok(a.L, i, kMidShapes) : shape_ok(a.L, i, kTailShapes))) return false;
            if (L.g_cst < 0 || (L.g_cst & 3)) return false;
            if (first && L.zp_in != -128) return false;   // (zero-filled taps + border biases assume it; the packer checks the same)
            // every clamp whose result is stored as a byte is an int8 range (with the ADD the block's own term is not clamped: pw_lo / pw_hi unused)
            if (!int8_range(L.dw_lo, L.dw_hi) || L.pw_lo > L.pw_hi) return false;
            if (!L.has_add && !int8_range(L.pw_lo, L.pw_hi)) return false;
            if (L.has_add && (!int8_range(L.add_lo, L.add_hi) || L.add_e < 1 || L.add_e > 22 || L.add_m < 0 || L.res_m < 0 || L.res_k < 3 || L.res_k > 19))
                return false;
            if (tail2_dw_bytes(L, first) / 16 > kTail2MaxDw16) return false;
            const Span map{0, tail2_map_bytes(L, first, G)};
            L.x_off = first ? -1 : 0;
            L.y_off = 0;
            std::vector<Span> used{map};
            if (prev_pw.e > prev_pw.b) used.push_back(prev_pw);
            L.zp_off = first ? 0 : first_fit(used, L.Cin + 16, CAP);
            if (L.zp_off < 0) return false;
            L.dw_off = first && attempt ? (CAP - tail2_dw_bytes(L, first)) & ~15 : first_fit(used, tail2_dw_bytes(L, first), CAP);
            if (L.dw_off < 0) return false;
            used = {map, dw_span(L, first)};
            if (!first) used.push_back({L.zp_off, L.zp_off + L.Cin + 16});
            L.pw_off = first_fit(used, tail2_pw_bytes(L), CAP);
            if (L.pw_off < 0) return false;
            prev_pw = {L.pw_off, L.pw_off + tail2_pw_bytes(L)};
            grow(map.e); grow(dw_span(L, first).e); grow(prev_pw.e);
        }
        // the first block's depthwise part of the NEXT group is written behind the last block's pointwise phase and lies there through the head
        const Tail2Layer& last = a.L[n_layers - 1];
        map_last = {0, G * last.OH * last.OW * (last.Cout + 16)};
        if (!overlap(dw_span(a.L[0], true), map_last) && !overlap(dw_span(a.L[0], true), prev_pw)) break;
        if (attempt) return false;
    }
    const Tail2Layer& last = a.L[n_layers - 1];
    a.resident = 0;
    a.satpack = tail2_satpack_ok(a) ? 1 : 0;
    a.bar_off = -1;
    a.fcw_off = -1;   // (tail: the classifier's fragments come straight from memory)
    if (mid) {
        a.P = last.OH * last.OW;
        a.C = last.Cout;
        a.lds_bytes = lds_need;
        tail2_place_counters(a);
        return a.C % 16 == 0;
    }
    read_head(desc + LW * n_layers, a);
    if (a.g_fcw < 0 || a.g_fcb < 0 || a.g_hlut < -1 || (a.g_fcw & 3) || (a.g_fcb & 3)) return false;
    if (!int8_range(a.fc_lo, a.fc_hi)) return false;
    if (a.P != last.OH * last.OW || a.C != last.Cout || a.C % 64 || a.C > 256 || a.NC < 1 || (a.NC + 15) / 16 > kTail2Waves) return false;
    std::vector<Span> used{map_last, dw_span(a.L[0], true)};
    a.mean_off = first_fit(used, kTailG * last.Cout, CAP);
    if (a.mean_off < 0) return false;
    grow(a.mean_off + kTailG * last.Cout);
    a.lds_bytes = lds_need;
    tail2_place_counters(a);
    return true;
}

// Which epilogue form a chain's kernel may run (bn_i8_tail2.hip: SAT).  The packed shift-and-saturate instruction clamps to [-128, 127] and
// to nothing else, so ONE narrower bound anywhere in the chain (a ReLU6 output whose 6 / scale stays below 127, an ADD output whose zero
// point is above -128) keeps the whole launch on the med3 form: the choice is per launch, not per block.
bool tail2_satpack_ok(const Tail2Args& a) {
    if (a.n_layers < 1 || a.n_layers > 8) return false;
    for (int i = 0; i < a.n_layers; ++i) {
        const Tail2Layer& L = a.L[i];
        if (L.dw_lo != -128 || L.dw_hi != 127) return false;
        if (L.has_add ? (L.add_lo != -128 || L.add_hi != 127) : (L.pw_lo != -128 || L.pw_hi != 127)) return false;
    }
    return true;
}

// The resident placement of a stage-2 plan (i8_mid2_kernel, option i8_mid_split): from a plan tail2_plan(..., mid = true) accepted, the same
// blocks with LDS of its own for every block's depthwise part, pointwise part and zero-point row, laid out one behind the other above the
// maps (the largest map of the chain times kMidG: input and output in place at offset 0), then the chunk barriers' counters.  Nothing
// overlaps anything, so nothing is staged twice and nothing orders the two chunk slots.  false = it does not fit the 160 KB of a CU (or a
// part is larger than the one-time staging copies): the caller keeps the staged plan and the kernel its staged form.
bool tail2_plan_resident(Tail2Args& a) {
    if (a.n_layers < 1 || a.n_layers > 8) return false;
    int map_bytes = 0;
    for (int i = 0; i < a.n_layers; ++i) map_bytes = std::max(map_bytes, tail2_map_bytes(a.L[i], i == 0, kMidG));
    std::vector<Span> used{{0, map_bytes}};
    for (int i = 0; i < a.n_layers; ++i) {
        Tail2Layer& L = a.L[i];
        if (tail2_dw_bytes(L, i == 0) / 16 > kTail2MaxDw16 || tail2_pw_bytes(L) / 16 > kTail2MaxDw16) return false;
        if ((L.dw_off = first_fit(used, tail2_dw_bytes(L, i == 0), kLdsCap)) < 0) return false;
        if ((L.pw_off = first_fit(used, tail2_pw_bytes(L), kLdsCap)) < 0) return false;
        L.zp_off = 0;
        if (i > 0 && (L.zp_off = first_fit(used, L.Cin + 16, kLdsCap)) < 0) return false;
    }
    if ((a.bar_off = first_fit(used, 16, kLdsCap)) < 0) return false;
    for (size_t i = 0; i < used.size(); ++i)   // (first fit cannot produce an overlap; a cheap proof at load beats a wrong byte later)
        for (size_t j = i + 1; j < used.size(); ++j)
            if (overlap(used[i], used[j])) return false;
    const Tail2Layer& last = a.L[a.n_layers - 1];
    if (last.OH != 16 || last.OW != 32 || last.Cout != 64 || a.P != 16 * 32 || a.C != 64) return false;   // (the wave-by-wave write-back's geometry)
    int end = 0;
    for (const Span& u : used) end = std::max(end, u.e);
    a.lds_bytes = end;
    a.resident = 1;
    return end <= kLdsCap;
}

bool tail2_plan_dump(const Tail2Args& a, int* out, int n) {
    if (n < 5 + 6 * a.n_layers) return false;
    int map_bytes = 0;
    for (int i = 0; i < a.n_layers; ++i) {
        const Tail2Layer& L = a.L[i];
        map_bytes = std::max(map_bytes, tail2_map_bytes(L, i == 0, kMidG));
        int* o = out + 5 + 6 * i;
        o[0] = L.dw_off; o[1] = tail2_dw_bytes(L, i == 0); o[2] = L.pw_off; o[3] = tail2_pw_bytes(L); o[4] = L.zp_off; o[5] = i == 0 ? 0 : L.Cin + 16;
    }
    out[0] = a.resident; out[1] = a.lds_bytes; out[2] = map_bytes; out[3] = a.bar_off; out[4] = a.n_layers;
    return true;
}

long tail2_const_words(const Tail2Args& a, bool mid) {
    long need = 0;
    auto upto = [&](long off, long words) { need = off + words > need ? off + words : need; };
    for (int i = 0; i < a.n_layers; ++i) upto(a.L[i].g_cst, (tail2_dw_bytes(a.L[i], i == 0) + tail2_pw_bytes(a.L[i])) / 4);
    if (mid) return need;
    const long nct = (a.NC + 15) / 16;
    upto(a.g_fcw, nct * (a.C / 64) * 256);
    upto(a.g_fcb, nct * 48);
    if (a.g_hlut >= 0) upto(a.g_hlut, 64);
    return need;
}

}  // namespace bn
