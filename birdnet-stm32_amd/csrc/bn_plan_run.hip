// bn_plan_run.hip — what happens to a parsed plan between bn_model_load() and the kernels (host code only): the load-time preparation
// (embedding mark, per-operator records, sizes of the pooling scratch) and the executor that turns one launch group of
// bn_forward() / bn_infer_audio() into kernel launches on the caller's stream.  Operator records are addressed through bn_ops.h.
#include <algorithm>
#include <cstring>

#include "bn_model.h"
#include "bn_quant_in.h"

namespace bn {

namespace {

// A fused kernel runs its head operator and the partner(s) the packer tagged as ONE launch: only when the partner runs wherever the head
// does — it belongs to both entry paths (the usual case: one head per path in front of a shared block) or to the head's own.  A partner of
// the OTHER path would not run at all in this mode: separate launches then.
inline bool same_path(const OpRec& head, const OpRec& partner) {
    return partner.p[BN_OP_PATH] == BN_PATH_BOTH || partner.p[BN_OP_PATH] == head.p[BN_OP_PATH];
}
inline bool on_path(const OpRec& o, int mode) { return o.p[BN_OP_PATH] == BN_PATH_BOTH || o.p[BN_OP_PATH] == mode; }
inline int tag(const OpRec& o) { return o.p[BN_OP_TAIL_TAG]; }

// ---- the fusion conditions that both the scratch sizing (at load) and the executor (per call) apply ------------------------------------
// squeeze-excite gate `g` pools exactly the map [OH][OW][C] that the depthwise operator `d` (F32_DW) writes
bool gate_pools_dw(const OpRec& d, const OpRec& g) {
    namespace k = op::f32_dw;
    namespace q = op::f32_segate;
    return g.kind == BN_OP_F32_SEGATE && g.in0 == d.out && g.p[q::C] == d.p[k::C] && g.p[q::P] == d.p[k::OH] * d.p[k::OW];
}
// row blocks of channel sums f32_pwdw_kernel writes for the depthwise operator `d`
int pwdw_row_blocks(const OpRec& d) {
    const int OH = d.p[op::f32_dw::OH], rb = f32_pwdw_rows(OH);
    return (OH + rb - 1) / rb;
}
// the MEAN operator `mo` pools exactly the map the INT8 depthwise operator `d` writes
bool mean_pools_dw8(const OpRec& d, const OpRec& mo) {
    namespace k = op::i8_dw;
    return mo.in0 == d.out && mo.p[op::i8_mean::C] == d.p[k::C];
}

// ---- decoders: the one place where a kind's record turns into launcher arguments ------------------------------------------------------
I8ConvGeom conv_geom8(const OpRec& d) {  // I8_STEM / I8_DW (rq_right: the caller's)
    namespace k = op::i8_dw;
    const int* q = d.p;
    return I8ConvGeom{q[k::H], q[k::W], q[k::C], q[k::sh], q[k::sw], q[k::OH], q[k::OW], q[k::pt], q[k::pl], q[k::zp_in], q[k::zp_out], q[k::act_min], q[k::act_max]};
}

template <class K>
I8AddParams add_params(const int* q, K has_add) {  // the BN_FIELDS_ADD block that starts at `has_add`
    const int* a = q + has_add;
    return I8AddParams{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]};
}

// Prepared record of the fused chain operator `o` (I8_TAIL: Tail8Args from t[cst] / t[desc] and, when present, the second form from
// t[cst2] / t[desc2]; I8_MID: Tail2Args and its resident placement).  Shared steps: the descriptor table's tensor, whole words, the
// planner, the first layer's geometry against the record, the constant block's size.
template <class Args, class Plan, class Words>
bool chain_prep(const bn_model* m, const char* base, const OpRec& o, int t_cst, int t_desc, Args& a, Plan plan, Words const_words) {
    namespace k = op::i8_tail;  // (I8_MID shares n_layers .. C_last: bn_ops.h)
    const TensorRec& td = m->tensors[o.t[t_desc]];
    const TensorRec& tc = m->tensors[o.t[t_cst]];
    return (td.nbytes & 3) == 0 && plan((const int32_t*)(base + td.offset), (int)(td.nbytes / 4), o.p[k::n_layers], a) && a.L[0].H == o.p[k::H0] &&
           a.L[0].W == o.p[k::W0] && a.L[0].Cin == o.p[k::C0] && const_words(a) * 4 <= (long)tc.nbytes;
}

}  // namespace

int prepare_plan(bn_model* m, const void* blob) {
    const char* base = (const char*)blob;
    const size_t n = m->ops.size();
    // the embedding mark: only on the pooling operators in front of a head (and the fused kernels that pool on chip), all of one width / quantisation
    for (size_t oi = 0; oi < n; ++oi) {
        const OpRec& o = m->ops[oi];
        if (o.p[BN_OP_EMB_TAG] != BN_EMB_OP) continue;
        const int* p = o.p;
        const bool i8 = o.kind == BN_OP_I8_TAIL || o.kind == BN_OP_I8_MEAN || o.kind == BN_OP_I8_ATTNPOOL;
        int width = -1;
        switch (o.kind) {
            case BN_OP_I8_TAIL: width = p[op::i8_tail::C_last]; break;
            case BN_OP_I8_MEAN: width = p[op::i8_mean::C]; break;
            case BN_OP_I8_ATTNPOOL: width = p[op::i8_attnpool::C]; break;
            case BN_OP_F32_GAP: width = p[op::f32_gap::C]; break;
            case BN_OP_F32_ATTNPOOL: width = p[op::f32_attnpool::C]; break;
            case BN_OP_F32_GAPDENSE: width = p[op::f32_gapdense::Cin]; break;
            default: break;
        }
        const float sc = i8 ? o.f[BN_OP_EMB_SCALE] : 1.0f;
        const int zp = i8 ? p[BN_OP_EMB_ZP] : 0;
        const bool same = m->emb_dim == 0 || (m->emb_dim == width && m->emb_scale == sc && m->emb_zp == zp);
        if (width <= 0 || width % 4 || width != p[BN_OP_EMB_DIM] || i8 != (m->hdr.dtype == BN_DTYPE_I8) || !same || (i8 && !(sc > 0.0f)) ||
            zp < -128 || zp > 127 || (o.kind != BN_OP_I8_TAIL && o.kind != BN_OP_F32_GAPDENSE && o.out < 0))
            return fail(BN_ERR_FORMAT, "operator %zu (kind %d): malformed embedding mark", oi, o.kind);
        m->emb_dim = width;
        m->emb_scale = sc;
        m->emb_zp = zp;
    }
    // the plan's first operator: may bn_infer_audio hand it the tile-major spectrogram, and is the guarded mixer built for its QUANTIZE?
    for (const OpRec& o : m->ops)
        if (o.in0 == BN_SLOT_INPUT) {
            namespace k = op::i8_dwpw;
            m->spec_tiled_ok = o.kind == BN_OP_I8_DWPW && o.p[k::q_at_load] && o.p[k::transposed] && o.p[k::W] % 64 == 0;
            m->guard_form_ok = m->spec_tiled_ok && o.p[k::qzp] == -128;
        }
    // can every requantisation of (t_mult, t_shift) take the branch-free right-shift form: multipliers >= 0, shifts < 0?
    auto all_right = [&](int t_mult, int t_shift) {
        if (t_mult < 0 || t_shift < 0) return false;
        const TensorRec& tm = m->tensors[t_mult];
        const TensorRec& ts = m->tensors[t_shift];
        const int32_t* pm = (const int32_t*)(base + tm.offset);
        const int32_t* ps = (const int32_t*)(base + ts.offset);
        if ((tm.nbytes | ts.nbytes) & 3) return false;
        for (size_t i = 0; i < tm.nbytes / 4; ++i)
            if (pm[i] < 0) return false;
        for (size_t i = 0; i < ts.nbytes / 4; ++i)
            if (ps[i] >= 0) return false;
        return true;
    };
    // every shift of t_shift >= -20: the 64-bit addend of the one-multiply-add requantisation cannot overflow
    auto all_narrow = [&](int t_shift) {
        if (t_shift < 0) return false;
        const TensorRec& ts = m->tensors[t_shift];
        const int32_t* ps = (const int32_t*)(base + ts.offset);
        bool narrow = true;
        for (size_t i = 0; i < ts.nbytes / 4; ++i) narrow = narrow && ps[i] >= -20;
        return narrow;
    };
    m->prep.clear();
    m->prep.resize(n);
    for (size_t oi = 0; oi < n; ++oi) {
        const OpRec& o = m->ops[oi];
        const int* p = o.p;
        if (o.kind != BN_OP_I8_DWPW && o.kind != BN_OP_I8_DW && o.kind != BN_OP_I8_STEM && o.kind != BN_OP_I8_FRONT && o.kind != BN_OP_I8_TAIL &&
            o.kind != BN_OP_I8_MID)
            continue;
        m->prep[oi].reset(new OpPrep());
        OpPrep& pr = *m->prep[oi];
        if (o.kind == BN_OP_I8_DWPW) {
            namespace k = op::i8_dwpw;
            const bool pw_ok = all_right(o.t[k::pw_mult], o.t[k::pw_shift]);  // (bit 2: the pointwise stage alone, whatever the ADD behind it looks like)
            bool ok = pw_ok && (!p[k::has_dw] || all_right(o.t[k::dw_mult], o.t[k::dw_shift]));
            if (p[k::has_add])
                ok = ok && p[k::add_m1] >= 0 && p[k::add_s1] < 0 && p[k::add_m2] >= 0 && p[k::add_s2] < 0 && p[k::add_mo] >= 0 && p[k::add_so] < 0;
            const bool narrow = pw_ok && all_narrow(o.t[k::pw_shift]);  // (i8_pw_lds_kernel)
            pr.rq_right = (ok ? 1 : 0) | (narrow ? 2 : 0) | (pw_ok ? 4 : 0);
        } else if (o.kind == BN_OP_I8_DW || o.kind == BN_OP_I8_STEM) {
            namespace k = op::i8_dw;
            pr.rq_right = (all_right(o.t[k::mult], o.t[k::shift]) ? 1 : 0) | (all_narrow(o.t[k::shift]) ? 2 : 0);
        } else if (o.kind == BN_OP_I8_FRONT) {
            namespace k = op::i8_front;
            pr.rq_right = all_right(o.t[k::stem_mult], o.t[k::stem_shift]) && all_right(o.t[k::dw_mult], o.t[k::dw_shift]) &&
                          all_right(o.t[k::pw_mult], o.t[k::pw_shift]);
        } else if (o.kind == BN_OP_I8_MID) {
            namespace k = op::i8_mid;
            Tail2Args& ma = pr.chain;
            const int nl = p[k::n_layers];
            pr.ok = chain_prep(m, base, o, k::cst, k::desc, ma, [](const int32_t* d, int nw, int l, Tail2Args& a) { return tail2_plan(d, nw, l, a, true); },
                               [](const Tail2Args& a) { return tail2_const_words(a, true); }) &&
                    ma.L[nl - 1].OH * ma.L[nl - 1].OW == p[k::P_last] && ma.L[nl - 1].Cout == p[k::C_last];
            pr.resident = ma;
            pr.alt_ok = pr.ok && tail2_plan_resident(pr.resident);
            m->has_mid = m->has_mid || pr.ok;
        } else {  // BN_OP_I8_TAIL
            namespace k = op::i8_tail;
            pr.tail.NC = pr.chain.NC = p[k::n_classes];
            pr.tail.s_fc = pr.chain.s_fc = o.f[k::s_fc];
            pr.tail.s_head = pr.chain.s_head = o.f[k::s_head];
            pr.ok = chain_prep(m, base, o, k::cst, k::desc, pr.tail, [](const int32_t* d, int nw, int l, Tail8Args& a) { return tail_plan(d, nw, l, a); },
                               [](const Tail8Args& a) { return tail_const_words(a); });
            m->has_tail = m->has_tail || pr.ok;
            // the second form's constants are optional; it only ever runs where the first form could (same coverage, same fallback)
            if (pr.ok && o.t[k::cst2] >= 0 && o.t[k::desc2] >= 0 && (size_t)o.t[k::cst2] < m->tensors.size() && (size_t)o.t[k::desc2] < m->tensors.size())
                pr.alt_ok = chain_prep(m, base, o, k::cst2, k::desc2, pr.chain, [](const int32_t* d, int nw, int l, Tail2Args& a) { return tail2_plan(d, nw, l, a); },
                                       [](const Tail2Args& a) { return tail2_const_words(a); });
        }
    }
    // sizes of the pooling scratch: the largest use of each fusion the executor may take (the same conditions, see PlanRun)
    for (size_t i = 0; i + 1 < n; ++i) {
        const OpRec& a = m->ops[i];
        const OpRec& b = m->ops[i + 1];
        // row-block channel sums of fused inverted-residual pairs
        if (a.kind == BN_OP_F32_DWPW && tag(a) == BN_PWDW_HEAD && b.kind == BN_OP_F32_DW)
            m->gap_part_elems = std::max(m->gap_part_elems, (size_t)pwdw_row_blocks(b) * (size_t)b.p[op::f32_dw::C]);
        // stand-alone depthwise stage -> gate: one partial sum per strip (at most OH / 4 row blocks)
        if (a.kind == BN_OP_F32_DW && b.kind == BN_OP_F32_SEGATE && b.in0 == a.out) {
            namespace k = op::f32_dw;
            int cq = 16;
            while ((a.p[k::C] / 4) % cq) cq >>= 1;
            const int ncol = 64 / cq;
            m->gap_part_elems = std::max(m->gap_part_elems, (size_t)((a.p[k::OW] + ncol - 1) / ncol) * (size_t)((a.p[k::OH] + 3) / 4) * (size_t)a.p[k::C]);
        }
        // INT8 depthwise stage -> MEAN of a squeeze-excite gate: channel sums taken on the way out
        if (a.kind == BN_OP_I8_DW && b.kind == BN_OP_I8_MEAN && mean_pools_dw8(a, b)) m->pool8_C = std::max(m->pool8_C, (size_t)a.p[op::i8_dw::C]);
    }
    return BN_OK;
}

StftGuard guard_slice(const bn_model* m, size_t b0, const SpecStage& st) {
    StftGuard g = m->guard;
    const size_t W = m->hdr.spec_width;
    g.eps += b0 * W;
    g.rec += b0 * ((W + 15) / 16) * kGuardRec;
    g.count += b0;
    g.dirty += b0;
    g.mn_lo += b0;
    g.min_interval = g_opt.stft_minint;
    // every launch group has its own lists and counters (a batch beyond kMaxGridBatch runs the STFT stage of all groups before the plan of the first)
    const size_t group = b0 / kMaxGridBatch;
    g.work += b0 * ((W + 63) / 64);
    g.n_work += group;
    g.hard += b0;
    g.n_hard += 2 * group;
    g.audio = st.audio;  // (already offset to the launch group's first chunk by bn_infer_audio)
    g.T = st.T;
    g.hop = st.hop;
    g.tabs = m->ctx->tables;
    g.flag_cap = g_opt.stft_flagcap;
    // the frame part of the bound (bn_quant_in.h): empirical, proven, or — tests only — far too small
    const int gm = g_opt.stft_guard;
    g.k_l2 = gm == 1 ? kGuardL2Proven : gm == 2 ? kGuardL2 / 1024.0f : kGuardL2;
    g.k_peak = gm == 1 ? 0.0f : gm == 2 ? kGuardPeak / 1024.0f : kGuardPeak;
    g.audit_scale = gm == 2 ? 1024.0f : 1.0f;
    g.slack_scale = gm == 2 ? 0.0f : 1.0f;
    g.audit = g_opt.stft_audit ? m->d_audit : nullptr;
    return g;
}

namespace {

// The executor of one launch group.  Members: the group's arguments, what one operator leaves behind for a later one (a fused kernel that
// already ran a partner, pooled sums waiting for their gate), and the operator being run.  One member function per kind that decides
// between fused forms; each returns BN_OK once the operator's launches are issued.
struct PlanRun {
    bn_model* const m;
    const RunArgs& a;
    const int B;
    hipStream_t const s;
    const int mode;        // the entry path: BN_PATH_AUDIO / BN_PATH_INPUT
    const size_t n;        // operators in the plan
    const bool tail_on, mid_on;

    // ---- across operators ----
    size_t gap_for = (size_t)-1;   // squeeze-excite gate whose pooling comes as row-block sums from the fused kernel in front of it
    int gap_R = 0, cand_R = 0;
    size_t cand_for = (size_t)-1;  // (candidate: becomes gap_for once the fused kernel has been launched)
    size_t pwdw_head_done = (size_t)-1;  // expand convolution that ran inside the fused kernel of the stem operator in front of it
    size_t pwdw_done = (size_t)-1;       // depthwise stage that ran inside the expand convolution in front of it
    size_t front2_done = (size_t)-1;     // operator that the fused front kernel of this run has already covered
    size_t segate_done[2] = {(size_t)-1, (size_t)-1};  // the two dense layers of a squeeze-excite gate that ran inside the pooling kernel
    size_t pool8_for = (size_t)-1;  // MEAN operator whose channel sums the depthwise kernel in front of it has already put into d_pool8
    size_t scale_done = (size_t)-1; // 1x1 convolution that already ran with the squeeze-excite MUL in front of it applied on load
    int emb_written = 0;            // marked operators that stored the embedding in this call (exactly one runs per path)

    // ---- the operator being run ----
    size_t oi = 0;
    const OpRec* o = nullptr;
    const int* p = nullptr;
    char *in0 = nullptr, *in1 = nullptr, *out = nullptr;
    const float* mm = nullptr;  // per-chunk min / max of the runner-boundary input, when the operator reads it
    ProfScope* prof = nullptr;

    PlanRun(bn_model* m_, const RunArgs& a_)
        : m(m_), a(a_), B(a_.B), s(a_.s), mode(a_.d_audio ? BN_PATH_AUDIO : BN_PATH_INPUT), n(m_->ops.size()), tail_on(m_->has_tail && g_opt.i8_tail),
          mid_on(m_->has_mid && g_opt.i8_mid && g_opt.i8_strip) {}

    char* slot_ptr(int id) const {
        if (id == BN_SLOT_INPUT) return (char*)a.d_input;
        if (id == BN_SLOT_AUDIO) return (char*)a.d_audio;
        if (id == BN_SLOT_SCORES) return (char*)a.d_scores;
        if (id == BN_SLOT_LOGITS) return (char*)a.d_logits;
        if (id < 0 || id >= (int)m->d_slots.size()) return nullptr;
        return m->d_slots[id] + a.slot_b0 * m->slots[id].bytes_per_chunk;
    }
    const float* tf(const OpRec& r, int k) const { return (const float*)m->tensor(r.t[k]); }
    const int8_t* t8(const OpRec& r, int k) const { return (const int8_t*)m->tensor(r.t[k]); }
    const int32_t* t32(const OpRec& r, int k) const { return (const int32_t*)m->tensor(r.t[k]); }
    void* emb_for(const OpRec& r) const { return (a.d_emb && r.p[BN_OP_EMB_TAG] == BN_EMB_OP) ? a.d_emb : nullptr; }

    bool prep_ok() const { return m->prep[oi] && m->prep[oi]->ok; }  // the fused chain operator's maps fit its kernel

    void mark_slot(int sid, int v) {
        if (sid >= 0 && (size_t)sid < m->slot_valid.size()) m->slot_valid[sid] = (uint8_t)v;
    }
    // a fused kernel kept this operator's map on chip and wrote `partner`'s output instead
    void fused_into(size_t partner) {
        m->out_valid[oi] = 0;
        mark_slot(o->out, 0);
        m->out_valid[partner] = 1;
        mark_slot(m->ops[partner].out, 1);
    }

    // ---- decoders that need the group's pointers ----
    DwPwArgs dwpw_args(const OpRec& d) const {
        namespace k = op::f32_dwpw;
        DwPwArgs r{};
        const int* q = d.p;
        r.x = (const float*)slot_ptr(d.in0);
        r.res = q[k::has_res] ? (const float*)slot_ptr(d.in1) : nullptr;
        r.gate = q[k::has_gate] ? (const float*)slot_ptr(q[k::gate_slot]) : nullptr;
        r.y = (float*)slot_ptr(d.out);
        r.dw_w = tf(d, k::dw_w); r.dw_b = tf(d, k::dw_b); r.pw_w = tf(d, k::pw_w); r.pw_b = tf(d, k::pw_b);
        r.B = B; r.H = q[k::H]; r.W = q[k::W]; r.Cin = q[k::Cin]; r.sh = q[k::sh]; r.sw = q[k::sw]; r.dw_act = q[k::dw_act];
        r.OH = q[k::OH]; r.OW = q[k::OW]; r.pt = q[k::pt]; r.pl = q[k::pl]; r.Cout = q[k::Cout]; r.pw_act = q[k::pw_act];
        r.has_dw = q[k::has_dw]; r.TH = q[k::TH]; r.TW = q[k::TW]; r.NB = q[k::NB];
        return r;
    }
    DwPw8Args dwpw8_args(const OpRec& d, size_t di) const {
        namespace k = op::i8_dwpw;
        DwPw8Args r{};
        const int* q = d.p;
        r.x = (const int8_t*)slot_ptr(d.in0);
        r.res = q[k::has_add] ? (const int8_t*)slot_ptr(d.in1) : nullptr;
        r.y = (int8_t*)slot_ptr(d.out);
        r.dw_w = t8(d, k::dw_w); r.dw_b = t32(d, k::dw_b); r.dw_mult = t32(d, k::dw_mult); r.dw_shift = t32(d, k::dw_shift);
        r.pw_w = t8(d, k::pw_w); r.pw_b = t32(d, k::pw_b); r.pw_mult = t32(d, k::pw_mult); r.pw_shift = t32(d, k::pw_shift);
        r.lut = q[k::has_lut] ? t8(d, k::lut) : nullptr;
        r.B = B; r.H = q[k::H]; r.W = q[k::W]; r.Cin = q[k::Cin]; r.sh = q[k::sh]; r.sw = q[k::sw]; r.OH = q[k::OH]; r.OW = q[k::OW];
        r.pt = q[k::pt]; r.pl = q[k::pl]; r.dw_zp_in = q[k::dw_zp_in]; r.dw_zp_out = q[k::dw_zp_out]; r.dw_amin = q[k::dw_amin]; r.dw_amax = q[k::dw_amax];
        r.Cout = q[k::Cout]; r.pw_zp_out = q[k::pw_zp_out]; r.pw_amin = q[k::pw_amin]; r.pw_amax = q[k::pw_amax];
        r.add = add_params(q, k::has_add);
        r.has_dw = q[k::has_dw]; r.transposed = q[k::transposed]; r.TH = q[k::TH]; r.TW = q[k::TW]; r.NB = q[k::NB];
        r.rq_right = m->prep[di]->rq_right;
        r.add_tab = (q[k::has_add] && !q[k::has_dw] && d.t[k::add_tab] >= 0) ? t8(d, k::add_tab) : nullptr;
        return r;
    }

    // the gate right behind a fused (expand, depthwise) pair pools the depthwise map: the fused kernel hands it per-row-block channel sums
    float* gap_target(size_t di) {
        const OpRec& d = m->ops[di];
        cand_for = (size_t)-1;
        if (g_opt.f32_pwdw < 2 || !m->d_gap_part || di + 1 >= n) return nullptr;
        const OpRec& g = m->ops[di + 1];
        const int R = pwdw_row_blocks(d);
        if (!gate_pools_dw(d, g) || (size_t)R * d.p[op::f32_dw::C] > m->gap_part_elems || !on_path(g, mode)) return nullptr;
        cand_for = di + 1;
        cand_R = R;
        return m->d_gap_part;
    }
    // the fused kernel launched with gap_target()'s buffer: the gate behind it reads the sums
    void take_gap() {
        gap_for = cand_for;
        gap_R = cand_R;
    }
    // launch_f32_pwdw for the expand convolution `ea` and the depthwise operator `d` behind it
    bool launch_pwdw(const DwPwArgs& ea, size_t di, const F32StemIn* st) {
        namespace k = op::f32_dw;
        const OpRec& d = m->ops[di];
        const int* q = d.p;
        return f32_pwdw_supported(ea, q[k::H], q[k::W], q[k::C], q[k::sh], q[k::sw], q[k::OH], q[k::OW]) &&
               launch_f32_pwdw(ea, tf(d, k::w), tf(d, k::bias), (float*)slot_ptr(d.out), q[k::sh], q[k::OH], q[k::OW], q[k::pt], q[k::pl], q[k::act], st,
                               gap_target(di), s);
    }

    // does the MEAN operator `mi` run as i8_segate_kernel (MEAN -> FC -> FC in one launch)?
    bool segate_fused(size_t mi) const {
        namespace k = op::i8_mean;
        namespace f = op::i8_fc;
        if (mi + 2 >= n) return false;
        const OpRec& r = m->ops[mi];
        const OpRec& f1 = m->ops[mi + 1];
        const OpRec& f2 = m->ops[mi + 2];
        const int C = r.p[k::C];
        return r.kind == BN_OP_I8_MEAN && tag(r) == BN_SEGATE_HEAD && g_opt.i8_strip && same_path(r, f1) && same_path(r, f2) && f1.kind == BN_OP_I8_FC &&
               f2.kind == BN_OP_I8_FC && tag(f1) == BN_SEGATE_COVERED && tag(f2) == BN_SEGATE_COVERED && f1.in0 == r.out && f2.in0 == f1.out &&
               f1.p[f::Cin] == C && f2.p[f::Cin] == f1.p[f::Cout] && f2.p[f::Cout] == C && C % 4 == 0 && f2.out != r.in0;
    }

    // ---- float32 plan ----
    int f32_stem() {
        namespace k = op::f32_stem;
        if (tag(*o) == BN_PWDW_STEM && g_opt.f32_pwdw && g_opt.f32_strip && oi + 2 < n) {
            // stem -> expand 1x1 -> depthwise 3x3 as ONE kernel: neither the stem map nor the expanded map is written
            namespace e_ = op::f32_dwpw;
            const OpRec& e = m->ops[oi + 1];
            const OpRec& d = m->ops[oi + 2];
            if (same_path(*o, e) && same_path(*o, d) && e.kind == BN_OP_F32_DWPW && tag(e) == BN_PWDW_HEAD && d.kind == BN_OP_F32_DW && tag(d) == BN_PWDW_COVERED &&
                e.in0 == o->out && d.in0 == e.out && d.out != o->in0 && d.out != o->out && d.out != e.out && e.p[e_::H] == p[k::OH] && e.p[e_::W] == p[k::OW] &&
                e.p[e_::Cin] == p[k::Cout]) {
                const DwPwArgs ea = dwpw_args(e);
                const F32StemIn st{(const float*)in0, tf(*o, k::w), tf(*o, k::bias), p[k::H], p[k::W], p[k::sh], p[k::sw], p[k::pt], p[k::pl], p[k::act]};
                if (ea.Cin <= 32 && launch_pwdw(ea, oi + 2, &st)) {  // (the stem on the matrix cores feeds at most two channel tiles)
                    pwdw_head_done = oi + 1;
                    pwdw_done = oi + 2;
                    fused_into(oi + 2);
                    take_gap();
                    return BN_OK;
                }
            }
        }
        launch_f32_stem((const float*)in0, (float*)out, B, p[k::H], p[k::W], p[k::Cout], p[k::sh], p[k::sw], p[k::act], p[k::OH], p[k::OW], p[k::pt], p[k::pl],
                        tf(*o, k::w), tf(*o, k::bias), s);
        return BN_OK;
    }

    int f32_dw() {
        namespace k = op::f32_dw;
        // a squeeze-excite gate right behind the stage pools per-strip channel sums written by the depthwise kernel (as behind fused pairs)
        float* gp = nullptr;
        int R = 0;
        if (g_opt.f32_pwdw >= 2 && m->d_gap_part && oi + 1 < n) {
            const OpRec& g = m->ops[oi + 1];
            R = f32_dw_stream_strips(B, p[k::C], p[k::OH], p[k::OW]);
            if (gate_pools_dw(*o, g) && (size_t)R * p[k::C] <= m->gap_part_elems && on_path(g, mode)) gp = m->d_gap_part;
        }
        if (launch_f32_dw((const float*)in0, (float*)out, B, p[k::H], p[k::W], p[k::C], p[k::sh], p[k::sw], p[k::act], p[k::OH], p[k::OW], p[k::pt], p[k::pl],
                          tf(*o, k::w), tf(*o, k::bias), gp, s) && gp) {
            gap_for = oi + 1;
            gap_R = R;
        }
        return BN_OK;
    }

    int f32_dwpw() {
        const DwPwArgs r = dwpw_args(*o);
        if (tag(*o) == BN_PWDW_HEAD && g_opt.f32_pwdw && g_opt.f32_strip && oi + 1 < n) {
            // inverted-residual block: the expand convolution runs inside the depthwise kernel behind it (the expanded map stays in LDS)
            const OpRec& d = m->ops[oi + 1];
            if (same_path(*o, d) && d.kind == BN_OP_F32_DW && tag(d) == BN_PWDW_COVERED && d.in0 == o->out && d.out != o->in0 && d.out != o->out &&
                launch_pwdw(r, oi + 1, nullptr)) {
                pwdw_done = oi + 1;
                fused_into(oi + 1);
                take_gap();
                return BN_OK;
            }
        }
        if (!f32_dwpw_supported(r.Cin, r.Cout) || (r.has_dw && r.Cin % 16) || r.TH * r.TW * r.NB != 64 || r.OH % r.TH || r.OW % r.TW)
            return fail(BN_ERR_FORMAT, "operator %zu: unsupported fused block geometry", oi);
        launch_f32_dwpw(r, s);
        return BN_OK;
    }

    int f32_front() {
        namespace k = op::f32_front;
        if (!f32_front_supported(p[k::H0], p[k::W0], p[k::C], p[k::N], p[k::OH], p[k::OW]))
            return fail(BN_ERR_FORMAT, "operator %zu: unsupported front-block geometry", oi);
        const float* minmax = p[k::raw_mel] ? m->d_minmax : nullptr;
        const int dist = p[BN_OP_FRONT2_DIST];
        if (tag(*o) == BN_FRONT2_HEAD && g_opt.f32_front2 && g_opt.f32_strip && g_opt.f32_front_staged && dist > 0 && oi + (size_t)dist < n) {
            // front block + the residual block behind it as one kernel: the 32-channel map between them stays in LDS
            const OpRec& d = m->ops[oi + (size_t)dist];
            if (same_path(*o, d) && d.kind == BN_OP_F32_DWPW && tag(d) == BN_FRONT2_COVERED && d.in0 == o->out && d.out != o->in0) {  // (never in place)
                const F32FrontStripArgs f{(const float*)in0, nullptr, tf(*o, k::stem_w), tf(*o, k::stem_b), tf(*o, k::dw_w), tf(*o, k::dw_b), tf(*o, k::pw_w),
                                          tf(*o, k::pw_b), minmax, tf(*o, k::wsum), tf(*o, k::magp), B, p[k::H0], p[k::W0], p[k::OH], p[k::OW], 0,
                                          p[k::stem_act], p[k::dw_act], p[k::pw_act], p[k::mag]};
                const DwPwArgs da = dwpw_args(d);
                if (p[k::C] == 16 && p[k::N] == 32 && f32_front2_supported(f, da) && launch_f32_front2(f, da, s)) {
                    front2_done = oi + (size_t)dist;
                    fused_into(front2_done);
                    return BN_OK;
                }
            }
        }
        launch_f32_front((const float*)in0, (float*)out, B, p[k::H0], p[k::W0], p[k::C], p[k::N], p[k::OH], p[k::OW], p[k::stem_act], p[k::dw_act], p[k::pw_act],
                         tf(*o, k::stem_w), tf(*o, k::stem_b), tf(*o, k::dw_w), tf(*o, k::dw_b), tf(*o, k::pw_w), tf(*o, k::pw_b), minmax, tf(*o, k::wsum),
                         tf(*o, k::magp), p[k::mag], s);
        return BN_OK;
    }

    // ---- INT8 plan ----
    int i8_conv() {  // I8_STEM / I8_DW
        namespace k = op::i8_dw;
        I8ConvGeom g = conv_geom8(*o);
        g.rq_right = m->prep[oi]->rq_right;
        const int8_t* w = t8(*o, k::w);
        const int32_t *bias = t32(*o, k::bias), *mult = t32(*o, k::mult), *shift = t32(*o, k::shift);
        if (o->kind == BN_OP_I8_DW) {  // row-streaming form (three loads per input row instead of nine per output) where the shape allows
            // ... which also adds up what it stores when the squeeze-excite gate's MEAN is the next operator (integer sums: bit-identical)
            int32_t* pool = nullptr;
            if (g_opt.i8_dw_pool && m->d_pool8 && oi + 1 < n && segate_fused(oi + 1)) {
                const OpRec& mo = m->ops[oi + 1];
                if (same_path(*o, mo) && mean_pools_dw8(*o, mo) && mo.p[op::i8_mean::P] == p[k::OH] * p[k::OW] && (size_t)p[k::C] <= m->pool8_C) pool = m->d_pool8;
            }
            if (launch_i8_dw_stream((const int8_t*)in0, (int8_t*)out, B, g, w, bias, mult, shift, s, pool)) {
                if (pool) pool8_for = oi + 1;
                return BN_OK;
            }
        }
        if (o->kind == BN_OP_I8_STEM && launch_i8_stem_stream((const int8_t*)in0, (int8_t*)out, B, g, w, bias, mult, shift, s)) return BN_OK;
        auto fn = o->kind == BN_OP_I8_STEM ? launch_i8_stem : launch_i8_dw;
        fn((const int8_t*)in0, (int8_t*)out, B, g, w, bias, mult, shift, s);
        return BN_OK;
    }

    int i8_dwpw() {
        namespace k = op::i8_dwpw;
        DwPw8Args r = dwpw8_args(*o, oi);
        if (tag(*o) == BN_PWDW8_HEAD && g_opt.i8_pwdw && g_opt.i8_strip && oi + 1 < n) {
            // inverted-residual block of an exported graph: expand convolution + depthwise stage as one kernel (the expanded map stays in LDS)
            namespace dk = op::i8_dw;
            const OpRec& d = m->ops[oi + 1];
            if (same_path(*o, d) && d.kind == BN_OP_I8_DW && tag(d) == BN_PWDW8_COVERED && d.in0 == o->out && d.out != o->in0 && d.out != o->out) {
                const I8ConvGeom g = conv_geom8(d);
                if (i8_pwdw_supported(r, g) &&
                    launch_i8_pwdw(r, g, t8(d, dk::w), t32(d, dk::bias), t32(d, dk::mult), t32(d, dk::shift), (int8_t*)slot_ptr(d.out), s)) {
                    pwdw_done = oi + 1;
                    fused_into(oi + 1);
                    return BN_OK;
                }
            }
        }
        if (r.transposed && p[k::q_at_load]) {  // QUANTIZE fused into the mel mixer: the input slot holds the float32 spectrogram
            r.qx = (const float*)in0;
            r.qminmax = mm;
            r.qscale = o->f[k::qscale];
            r.qzp = p[k::qzp];
            r.qfill = p[k::qfill];
            r.qF = p[k::qF];
            r.qtiled = (a.spec.tiled && o->in0 == BN_SLOT_INPUT) ? 1 : 0;
            r.x = nullptr;
            if (!i8_mel_mfma_supported(r)) return fail(BN_ERR_FORMAT, "operator %zu: fused QUANTIZE needs the mel-mixer kernel's geometry", oi);
            if (a.spec.guard && r.qtiled && mm) {
                // audio path: list the bytes the float32 STFT leaves in doubt, recompute those elements in float64, run the
                // blocks whose bytes changed once more (bn_stft_exact.hip)
                r.qguard = guard_slice(m, a.slot_b0, a.spec);
                r.qmode = 1;
                launch_i8_dwpw(r, s);
                prof->end();  // (the operator's own launch; the float64 pass has its own profiling entry)
                ProfScope fix(m, (int)n + 2, s);
                launch_stft_fix(m->ctx->tables, a.spec.audio, B, a.spec.T, a.spec.hop, r.W, (float*)in0, true, r.qguard, mm, r.qscale, r.qzp, s);
                r.qmode = 2;
                launch_i8_dwpw(r, s);
                return BN_OK;
            }
        }
        // wide early layers: wave-autonomous strip kernel when the packer prepared its constant block
        if (p[k::strip] && o->t[k::strip_cst] >= 0 && g_opt.i8_strip && r.has_dw && !r.transposed && r.sh == r.sw &&
            i8_strip_supported(r.Cin, r.Cout, r.sh, r.OW, r.add.enabled != 0) && (!r.add.enabled || (r.res == r.x && o->t[k::add_tab] >= 0))) {
            const int off = r.add.enabled ? 128 : 0;
            Strip8Args q{r.x, r.y, t32(*o, k::strip_cst), B, r.H, r.W, r.OH, r.OW, 0, r.pt, r.pl, r.dw_zp_in, r.dw_amin, r.dw_amax, r.pw_amin + off,
                         r.pw_amax + off, r.pw_zp_out, r.add, r.add.enabled ? t8(*o, k::add_tab) : nullptr};
            launch_i8_strip(q, r.Cin, r.Cout, r.sh, s);
            return BN_OK;
        }
        if (!i8_dwpw_supported(r.Cin, r.Cout) || r.TH * r.TW * r.NB != 64 || r.OH % r.TH || r.OW % r.TW)
            return fail(BN_ERR_FORMAT, "operator %zu: unsupported fused INT8 block geometry", oi);
        launch_i8_dwpw(r, s);
        return BN_OK;
    }

    int i8_front() {
        namespace k = op::i8_front;
        I8FrontParams q{};
        q.stem_w = t8(*o, k::stem_w); q.stem_b = t32(*o, k::stem_b); q.stem_mult = t32(*o, k::stem_mult); q.stem_shift = t32(*o, k::stem_shift);
        q.dw_w = t8(*o, k::dw_w); q.dw_b = t32(*o, k::dw_b); q.dw_mult = t32(*o, k::dw_mult); q.dw_shift = t32(*o, k::dw_shift);
        q.pw_w = t8(*o, k::pw_w); q.pw_b = t32(*o, k::pw_b); q.pw_mult = t32(*o, k::pw_mult); q.pw_shift = t32(*o, k::pw_shift);
        q.H0 = p[k::H0]; q.W0 = p[k::W0]; q.C = p[k::C]; q.N = p[k::N]; q.OH = p[k::OH]; q.OW = p[k::OW];
        q.stem_zp_in = p[k::stem_zp_in]; q.stem_zp_out = p[k::stem_zp_out]; q.stem_amin = p[k::stem_amin]; q.stem_amax = p[k::stem_amax];
        q.dw_zp_out = p[k::dw_zp_out]; q.dw_amin = p[k::dw_amin]; q.dw_amax = p[k::dw_amax];
        q.pw_zp_out = p[k::pw_zp_out]; q.pw_amin = p[k::pw_amin]; q.pw_amax = p[k::pw_amax];
        q.rq_right = m->prep[oi]->rq_right;
        if (p[k::strip] && o->t[k::strip_cst] >= 0 && g_opt.i8_strip && i8_front_strip_supported(q.H0, q.W0, q.C, q.N, q.OH, q.OW)) {
            FrontStrip8Args fa{(const int8_t*)in0, (int8_t*)out, t32(*o, k::strip_cst), B, q.H0, q.W0, q.OH, q.OW, 0, q.stem_zp_in, q.stem_amin, q.stem_amax,
                               q.stem_zp_out, q.dw_amin, q.dw_amax, q.pw_amin, q.pw_amax, 0};
            fa.satpack = (g_opt.i8_satpack & 2) && front_strip_satpack_ok(q.stem_amin, q.stem_amax);
            launch_i8_front_strip(fa, s);
            return BN_OK;
        }
        if (!i8_front_supported(q.H0, q.W0, q.C, q.N, q.OH, q.OW)) return fail(BN_ERR_FORMAT, "operator %zu: unsupported INT8 front-block geometry", oi);
        launch_i8_front(q, (const int8_t*)in0, (int8_t*)out, B, s);
        return BN_OK;
    }

    int i8_mid() {
        const OpPrep& pr = *m->prep[oi];
        Tail2Args ma = g_opt.i8_mid_split && pr.alt_ok ? pr.resident : pr.chain;
        ma.x = (const int8_t*)in0;
        ma.y = (int8_t*)out;
        ma.cst = t32(*o, op::i8_mid::cst);
        ma.B = B;
        if (!(g_opt.i8_satpack & 1)) ma.satpack = 0;
        if (!launch_i8_mid2(ma, s)) return fail(BN_ERR_DEVICE, "could not raise the LDS limit of the fused stage-2 kernel");
        return BN_OK;
    }

    int i8_tail() {
        namespace k = op::i8_tail;
        const OpPrep& pr = *m->prep[oi];
        const EmbOut eo{a.d_emb, a.emb_dtype == BN_EMB_F32, p[BN_OP_EMB_ZP], o->f[BN_OP_EMB_SCALE]};
        const EmbOut* emb = emb_for(*o) ? &eo : nullptr;
        emb_written += emb != nullptr;
        bool launched;
        if (g_opt.i8_tail_mfdw && pr.alt_ok) {
            Tail2Args t2 = pr.chain;
            t2.x = (const int8_t*)in0;
            t2.scores = a.d_scores;
            t2.logits = a.d_logits;
            t2.cst = t32(*o, k::cst2);
            t2.B = B;
            if (!(g_opt.i8_satpack & 1)) t2.satpack = 0;
            launched = launch_i8_tail2(t2, s, emb);
        } else {
            Tail8Args ta = pr.tail;
            ta.x = (const int8_t*)in0;
            ta.scores = a.d_scores;
            ta.logits = a.d_logits;
            ta.cst = t32(*o, k::cst);
            ta.B = B;
            launched = launch_i8_tail(ta, s, emb);
        }
        if (!launched) return fail(BN_ERR_DEVICE, "could not raise the LDS limit of the fused tail kernel");
        return BN_OK;
    }

    int i8_mean() {
        namespace k = op::i8_mean;
        namespace f = op::i8_fc;
        if (segate_fused(oi)) {
            const OpRec& f1 = m->ops[oi + 1];
            const OpRec& f2 = m->ops[oi + 2];
            launch_i8_segate((const int8_t*)in0, (int8_t*)slot_ptr(f2.out), B, p[k::P], p[k::C], p[k::zp_in], p[k::mult], p[k::shift], p[k::zp_out],
                             f1.p[f::Cout], f1.p[f::zp_out], f1.p[f::act_min], f1.p[f::act_max], t8(f1, f::w), t32(f1, f::bias), t32(f1, f::mult), t32(f1, f::shift),
                             f1.p[f::has_lut] ? t8(f1, f::lut) : nullptr, f2.p[f::zp_out], f2.p[f::act_min], f2.p[f::act_max], t8(f2, f::w), t32(f2, f::bias),
                             t32(f2, f::mult), t32(f2, f::shift), f2.p[f::has_lut] ? t8(f2, f::lut) : nullptr, s, oi == pool8_for ? m->d_pool8 : nullptr);
            segate_done[0] = oi + 1;
            segate_done[1] = oi + 2;
            fused_into(oi + 2);
            return BN_OK;
        }
        launch_i8_mean((const int8_t*)in0, (int8_t*)out, B, p[k::P], p[k::C], p[k::zp_in], p[k::mult], p[k::shift], p[k::zp_out], s);
        return BN_OK;
    }

    int i8_scale() {
        namespace k = op::i8_scale;
        if (tag(*o) == BN_SCALE_HEAD && g_opt.i8_strip && oi + 1 < n) {
            // the projection convolution behind the gate applies it while loading (the scaled map is never written)
            namespace dk = op::i8_dwpw;
            const OpRec& d = m->ops[oi + 1];
            if (same_path(*o, d) && d.kind == BN_OP_I8_DWPW && tag(d) == BN_SCALE_COVERED && d.in0 == o->out && d.out != o->in0 && d.out != o->in1 &&
                d.p[dk::Cin] == p[k::C] && d.p[dk::OH] * d.p[dk::OW] == p[k::P]) {
                DwPw8Args a2 = dwpw8_args(d, oi + 1);
                a2.x = (const int8_t*)in0;
                a2.gate = (const int8_t*)in1;
                a2.g_zx = p[k::zp_x]; a2.g_zg = p[k::zp_gate]; a2.g_mult = p[k::mult]; a2.g_shift = p[k::shift]; a2.g_zo = p[k::zp_out];
                a2.g_amin = p[k::act_min]; a2.g_amax = p[k::act_max];
                if (!a2.has_dw && !a2.transposed && i8_pw_wave_takes(a2)) {
                    launch_i8_dwpw(a2, s);
                    scale_done = oi + 1;
                    fused_into(oi + 1);
                    return BN_OK;
                }
            }
        }
        launch_i8_scale((const int8_t*)in0, (const int8_t*)in1, (int8_t*)out, B, p[k::P], p[k::C], p[k::zp_x], p[k::zp_gate], p[k::mult], p[k::shift],
                        p[k::zp_out], p[k::act_min], p[k::act_max], s);
        return BN_OK;
    }

    // the kinds that are one launch whatever ran before them
    int single_launch() {
        const float* x = (const float*)in0;
        const int8_t* x8 = (const int8_t*)in0;
        float* y = (float*)out;
        int8_t* y8 = (int8_t*)out;
        switch (o->kind) {
            case BN_OP_F32_MEL: {
                namespace k = op::f32_mel;
                if (p[k::norm]) launch_u32_fill((uint32_t*)m->d_smax, 0u, B, s);
                launch_f32_mel(x, mm, y, m->d_smax, B, p[k::F], p[k::W], p[k::M], tf(*o, k::wvals), (const int*)m->tensor(o->t[k::bands]), tf(*o, k::magp),
                               p[k::mag], p[k::norm], s);
                break;
            }
            case BN_OP_F32_STFTMEL: {
                namespace k = op::f32_stftmel;
                launch_minmax_init(m->d_minmax, B, s);
                if (!launch_stft512_mel(m->ctx->tables, a.d_audio, B, a.T, a.hop, p[k::W], y, p[k::M], tf(*o, k::wvals), (const int*)m->tensor(o->t[k::bands]),
                                        m->d_minmax, s))
                    return fail(BN_ERR_UNSUPPORTED, "the fused STFT+mel kernel takes at most 128 mel bins (got %d)", p[k::M]);
                break;
            }
            case BN_OP_F32_MELFIN: {
                namespace k = op::f32_melfin;
                launch_f32_melfin(x, m->d_minmax, y, B, p[k::M], p[k::W], tf(*o, k::wsum), tf(*o, k::magp), p[k::mag], p[k::norm], s);
                break;
            }
            case BN_OP_F32_RAWFE: {
                namespace k = op::f32_rawfe;
                launch_f32_rawfe(x, y, B, p[k::T], p[k::W], p[k::M], p[k::stride], p[k::pad_left], tf(*o, k::fb), tf(*o, k::bias), tf(*o, k::magp), p[k::mag], s);
                break;
            }
            case BN_OP_F32_MAG: {
                namespace k = op::f32_mag;
                launch_f32_mag(y, m->d_smax, B, p[k::M], p[k::W], tf(*o, k::magp), p[k::mag], s);
                break;
            }
            case BN_OP_F32_PW: {
                namespace k = op::f32_pw;
                launch_f32_pw(x, p[k::has_res] ? (const float*)in1 : nullptr, p[k::has_gate] ? (const float*)slot_ptr(p[k::gate_slot]) : nullptr, y, B, p[k::P],
                              p[k::Cin], p[k::Cout], p[k::act], tf(*o, k::w), tf(*o, k::bias), s);
                break;
            }
            case BN_OP_F32_GAPDENSE: {
                namespace k = op::f32_gapdense;
                launch_f32_gap_dense(x, y, a.d_logits, B, p[k::P], p[k::Cin], p[k::Cout], p[k::act], tf(*o, k::w), tf(*o, k::bias), s, (float*)emb_for(*o));
                emb_written += emb_for(*o) != nullptr;
                break;
            }
            case BN_OP_F32_SEGATE: {
                namespace k = op::f32_segate;
                launch_f32_segate(x, y, B, p[k::P], p[k::C], p[k::Cr], tf(*o, k::w1), tf(*o, k::w2), oi == gap_for ? m->d_gap_part : nullptr, gap_R, s);
                break;
            }
            case BN_OP_F32_SCALE:
                launch_f32_scale(x, (const float*)in1, y, B, p[op::f32_scale::P], p[op::f32_scale::C], s);
                break;
            case BN_OP_F32_GAP:
                launch_f32_gap(x, y, B, p[op::f32_gap::P], p[op::f32_gap::C], s);
                break;
            case BN_OP_F32_ATTNPOOL:
                launch_f32_attnpool(x, y, B, p[op::f32_attnpool::P], p[op::f32_attnpool::C], tf(*o, op::f32_attnpool::score), s);
                break;
            case BN_OP_F32_DENSE: {
                namespace k = op::f32_dense;
                launch_f32_dense(x, y, a.d_logits, B, p[k::Cin], p[k::Cout], p[k::act], tf(*o, k::w), tf(*o, k::bias), s);
                break;
            }
            case BN_OP_I8_QUANT: {
                namespace k = op::i8_quant;
                launch_i8_quant(x, mm, y8, B, p[k::F], p[k::W], p[k::Kp], p[k::zp], p[k::fill], o->f[k::scale], s);
                break;
            }
            case BN_OP_I8_MEL: {
                namespace k = op::i8_mel;
                launch_i8_mel(x8, y8, B, p[k::W], p[k::Kp], p[k::M], p[k::zp_out], p[k::act_min], p[k::act_max], t8(*o, k::w), t32(*o, k::bias), t32(*o, k::mult),
                              t32(*o, k::shift), p[k::has_lut] ? t8(*o, k::lut) : nullptr, s);
                break;
            }
            case BN_OP_I8_PW: {
                namespace k = op::i8_pw;
                launch_i8_pw(x8, (const int8_t*)in1, y8, B, p[k::P], p[k::Cin], p[k::Cout], p[k::zp_out], p[k::act_min], p[k::act_max], add_params(p, k::has_add),
                             t8(*o, k::w), t32(*o, k::bias), t32(*o, k::mult), t32(*o, k::shift), s);
                break;
            }
            case BN_OP_I8_FC: {
                namespace k = op::i8_fc;
                launch_i8_fc(x8, y8, B, p[k::Cin], p[k::Cout], p[k::zp_out], p[k::act_min], p[k::act_max], t8(*o, k::w), t32(*o, k::bias), t32(*o, k::mult),
                             t32(*o, k::shift), p[k::has_lut] ? t8(*o, k::lut) : nullptr, s);
                break;
            }
            case BN_OP_I8_ATTNPOOL:  // (the launcher takes the record's p in the order of op::i8_attnpool)
                if (!launch_i8_attnpool(x8, y8, B, p, t8(*o, op::i8_attnpool::score), t32(*o, op::i8_attnpool::tables), s))
                    return fail(BN_ERR_FORMAT, "operator %zu: attention pooling geometry", oi);
                break;
            case BN_OP_I8_MAXNORM: {
                namespace k = op::i8_maxnorm;
                launch_i8_maxnorm(x8, y8, B, p[k::C], p[k::W], t8(*o, k::denom), t8(*o, k::div), p[k::has_lut] ? t8(*o, k::lut) : nullptr, s);
                break;
            }
            case BN_OP_I8_RAWFE: {
                namespace k = op::i8_rawfe;
                launch_i8_rawfe(x, y8, B, p[k::T], p[k::W], p[k::M], p[k::stride], p[k::pad_left], o->f[k::q_scale], p[k::q_zp], p[k::zp_out], p[k::act_min],
                                p[k::act_max], t8(*o, k::w), t32(*o, k::bias), t32(*o, k::mult), t32(*o, k::shift), p[k::has_lut] ? t8(*o, k::lut) : nullptr, s);
                break;
            }
            case BN_OP_I8_HEAD: {
                namespace k = op::i8_head;
                if (p[k::softmax])  // float32 softmax behind DEQUANTIZE
                    launch_i8_head_softmax(x8, a.d_scores, a.d_logits, B, p[k::C], p[k::zp_fc], o->f[k::s_fc], o->f[k::beta], s);
                else
                    launch_i8_head(x8, a.d_scores, a.d_logits, B, p[k::C], p[k::zp_fc], p[k::zp_out], o->f[k::s_fc], o->f[k::s_out],
                                   p[k::has_lut] ? t8(*o, k::lut) : nullptr, s);
                break;
            }
            default:
                return fail(BN_ERR_UNSUPPORTED, "plan operator %zu has unknown kind %d", oi, o->kind);
        }
        return BN_OK;
    }

    int dispatch() {
        switch (o->kind) {
            case BN_OP_F32_STEM: return f32_stem();
            case BN_OP_F32_DW: return f32_dw();
            case BN_OP_F32_DWPW: return f32_dwpw();
            case BN_OP_F32_FRONT: return f32_front();
            case BN_OP_I8_STEM:
            case BN_OP_I8_DW: return i8_conv();
            case BN_OP_I8_DWPW: return i8_dwpw();
            case BN_OP_I8_FRONT: return i8_front();
            case BN_OP_I8_MID: return i8_mid();
            case BN_OP_I8_TAIL: return i8_tail();
            case BN_OP_I8_MEAN: return i8_mean();
            case BN_OP_I8_SCALE: return i8_scale();
            default: return single_launch();
        }
    }

    int run() {
        // the pooling scratch is zero between uses (i8_segate_kernel clears what it reads); cleared here as well, so that a call that failed half-way
        // cannot leave sums behind for the next one
        if (m->d_pool8 && g_opt.i8_dw_pool) HIP_TRY(hipMemsetAsync(m->d_pool8, 0, (size_t)B * m->pool8_C * sizeof(int32_t), s));
        m->out_valid.assign(n, 0);
        m->slot_valid.assign(m->d_slots.size(), 0);
        for (oi = 0; oi < n; ++oi) {
            o = &m->ops[oi];
            p = o->p;
            if (!on_path(*o, mode)) continue;
            if (oi == front2_done || oi == pwdw_done || oi == pwdw_head_done || oi == scale_done || oi == segate_done[0] || oi == segate_done[1])
                continue;  // ran inside a preceding operator's kernel
            if (tag(*o) == BN_MID_COVERED && mid_on) continue;    // the fused stage-2 chain runs these blocks
            if (tag(*o) == BN_MID_OP && !(mid_on && prep_ok())) continue;
            if (tag(*o) == BN_TAIL_COVERED && tail_on) continue;  // the fused tail operator runs these blocks
            if (tag(*o) == BN_TAIL_OP && !(tail_on && prep_ok())) continue;
            ProfScope scope(m, (int)oi, s);
            prof = &scope;
            m->out_valid[oi] = 1;  // (a fused kernel that keeps this operator's map on chip clears it again and marks the partner it wrote)
            mark_slot(o->out, 1);
            in0 = slot_ptr(o->in0);
            in1 = slot_ptr(o->in1);
            out = slot_ptr(o->out);
            mm = (o->in0 == BN_SLOT_INPUT) ? a.d_minmax : nullptr;
            if (int rc = dispatch()) return rc;
            // unfused pooling in front of the head: its output slot holds the embedding — copy / dequantise it behind the operator
            if (emb_for(*o) && m->out_valid[oi] &&
                (o->kind == BN_OP_I8_MEAN || o->kind == BN_OP_I8_ATTNPOOL || o->kind == BN_OP_F32_GAP || o->kind == BN_OP_F32_ATTNPOOL)) {
                const bool src_i8 = o->kind == BN_OP_I8_MEAN || o->kind == BN_OP_I8_ATTNPOOL;
                launch_emb_store(out, src_i8, a.d_emb, a.emb_dtype == BN_EMB_F32, B, m->emb_dim, m->emb_scale, m->emb_zp, s);
                ++emb_written;
            }
        }
        HIP_TRY(hipGetLastError());
        if (a.d_emb && emb_written != 1)
            return fail(BN_ERR_UNSUPPORTED, "%d marked operators stored the embedding on this path (expected exactly one)", emb_written);
        return BN_OK;
    }
};

}  // namespace

int run_plan(bn_model* m, const RunArgs& a) { return PlanRun(m, a).run(); }

}  // namespace bn
