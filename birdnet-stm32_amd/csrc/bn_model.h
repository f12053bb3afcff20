// bn_model.h — the context and model objects behind the C ABI, shared by bn_api.hip (lifetime, entry points), bn_plan_run.hip
// (load-time preparation of a plan and its executor) and bn_probe_api.hip (the probe's entry points).  Internal: nothing here is part of
// include/birdnet_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/birdnet_hip.h"
#include "bn_kernels.h"
#include "bn_ops.h"

namespace bn {

int fail(int code, const char* fmt, ...);  // records the message bn_last_error() returns, passes `code` through (bn_api.hip)
int check_device(bn_ctx* ctx);             // what an entry point does first: the context's device and option switches (bn_api.hip)
int grow_device_buffer(void** p, size_t* have, size_t need, size_t alloc, hipStream_t s, int code, const char* what);   // (bn_api.hip)

constexpr int kMaxGridBatch = 32768;  // chunks per launch group (gridDim.y/z limit is 65535)

// What the load-time preparation derives for one operator.  Only the kinds named here have a record.
struct OpPrep {
    // I8_STEM, I8_DW, I8_DWPW, I8_FRONT — bit 0: every requantisation of the operator has a multiplier >= 0 and a right shift; bit 1: every
    // (pointwise) shift lies in [-20, -1]; bit 2 (I8_DWPW): the pointwise stage alone passes bit 0's test
    uint8_t rq_right = 0;
    // I8_TAIL, I8_MID — kernel arguments and LDS plan built from the operator's descriptor table
    bool ok = false;       // the maps fit: I8_TAIL runs from `tail` (i8_tail_kernel), I8_MID from `chain` (i8_mid2_kernel)
    bool alt_ok = false;   // I8_TAIL: the plan carries the second form's constants and `chain` fits (i8_tail2_kernel);
                           // I8_MID: `resident` fits (the resident LDS placement, option i8_mid_split)
    Tail8Args tail{};
    Tail2Args chain{};
    Tail2Args resident{};
};

// The per-call facts of bn_infer_audio's spectrogram stage that the plan's first operator and the exactness pass need.
struct SpecStage {
    bool tiled = false;            // d_input holds the tile-major spectrogram the STFT wrote
    bool guard = false;            // the first operator lists doubtful bytes, the float64 pass follows it
    const float* audio = nullptr;  // the launch group's waveforms and their geometry
    int T = 0, hop = 0;
};

}  // namespace bn

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return bn::fail(BN_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct bn_ctx {
    std::vector<std::pair<int bn::Options::*, int>> opt_override;   // switches this context sets for itself (bn_ctx_set_option)
    int device = 0;
    int max_batch = 0;
    float* d_window = nullptr;
    float4* d_tw256 = nullptr;
    float4* d_tw512 = nullptr;
    double* d_f64tab = nullptr;      // hann64[512], cs64[512] (bn_stft_exact.hip)
    bn::StftTables tables{};
    float* d_block_peaks = nullptr;  // bn_ingest_resample: per-workgroup maxima, grown on demand
    size_t block_peaks_elems = 0;
    void* d_rank_work = nullptr;     // bn_rank_orders: transposed keys, index arrays, rocPRIM storage; grown on demand
    size_t rank_work_bytes = 0;
    void* d_search_work = nullptr;   // bn_search_topk: the workgroups' partial lists; grown on demand
    size_t search_work_bytes = 0;
    void* d_kmeans_work = nullptr;   // bn_kmeans_accumulate: sort keys, row orders, segment partial sums, rocPRIM storage; grown on demand
    size_t kmeans_work_bytes = 0;
    void* d_tsne_work = nullptr;     // bn_tsne_gradient: the column ranges' partial sums, the folded repulsion and row sums; grown on demand
    size_t tsne_work_bytes = 0;
    void* d_pca_work = nullptr;      // bn_pca_colsum / bn_pca_gram: the row ranges' float64 partial sums; grown on demand
    size_t pca_work_bytes = 0;
    void* d_propagate_work = nullptr;   // bn_propagate_step: the rows' float64 parts of the change; grown on demand
    size_t propagate_work_bytes = 0;
    void* d_select_work = nullptr;      // bn_select_run: the two alternating buffers of per-workgroup partial picks; allocated on first use
    size_t select_work_bytes = 0;
    void* d_boot_work = nullptr;     // bn_bootstrap_*: jump-ahead table, rejection counter and list, prepared class orders; grown on demand
    size_t boot_work_bytes = 0;
    void* d_mlp_work = nullptr;      // bn_head_mlp_forward: the hidden activations of one step of rows; grown on demand
    size_t mlp_work_bytes = 0;
};

struct bn_model {
    bn_ctx* ctx = nullptr;
    BlobHeader hdr{};
    std::vector<OpRec> ops;
    std::vector<TensorRec> tensors;
    std::vector<SlotRec> slots;
    char* d_consts = nullptr;            // one allocation, tensors at their blob offsets
    size_t consts_base = 0;              // blob offset of the first payload byte
    size_t consts_bytes = 0;
    std::vector<std::unique_ptr<bn::OpPrep>> prep;   // per operator: what bn::prepare_plan derived for it; null for the kinds that need nothing
    bool has_mid = false;                // the plan holds a usable fused stage-2 operator
    std::vector<uint8_t> out_valid;      // per operator: it wrote its output slot in the last forward call (not when a fused kernel covered it)
    std::vector<uint8_t> slot_valid;     // per slot: some operator wrote it in the last forward call
    bool has_tail = false;               // the plan holds a usable fused tail operator
    bool guard_form_ok = false;          // ... and its QUANTIZE has zero point -128 (the only form the guarded mixer is built for)
    bool spec_tiled_ok = false;          // the plan's first operator reads the spectrogram through i8_mel_mfma_kernel<QIN>: bn_infer_audio
                                         // may hand it the tile-major layout the STFT writes fastest
    std::vector<char*> d_slots;          // max_batch * bytes_per_chunk each
    float* d_spec = nullptr;             // [max_batch][F][W] for bn_infer_audio
    float* d_minmax = nullptr;           // [max_batch][2]
    char* d_guard = nullptr;             // buffers of the exactness pass (INT8 plans whose first operator quantises the spectrogram)
    bn::StftGuard guard{};
    bool last_tiled = false;             // layout of d_spec after the last bn_infer_audio call (bn_debug_input_bytes)
    int last_B = 0;
    int* d_audit = nullptr;              // [2] exactness audit: elements audited, violations (option stft_audit; zeroed per bn_infer_audio call)
    float* d_smax = nullptr;             // [max_batch] per-sample maxima of the frontend
    float* d_gap_part = nullptr;         // [max_batch][gap_part_elems] channel sums per row block from f32_pwdw_kernel for the squeeze-excite gate behind it
    size_t gap_part_elems = 0;
    int32_t* d_pool8 = nullptr;          // [max_batch][pool8_C] int32 channel sums from i8_dw_stream_kernel for the squeeze-excite gate behind it (zero between uses)
    size_t pool8_C = 0;
    size_t workspace_bytes = 0;
    int emb_dim = 0;                     // the plan's embedding (operators tagged BN_EMB_OP): width, int8 quantisation; 0 = none marked
    float emb_scale = 1.0f;
    int emb_zp = 0;
    // per-operator HIP-event timing (bn_profile_*): one (start, stop) pair per launch group
    bool profiling = false;
    int prof_only = -1;                  // >= 0: bracket only this operator (index n_ops = the STFT stage)
    struct EvRec {
        int op;
        hipEvent_t start, stop;
    };
    std::vector<EvRec> ev_used;
    std::vector<hipEvent_t> ev_free;

    hipEvent_t take_event() {
        if (!ev_free.empty()) {
            hipEvent_t e = ev_free.back();
            ev_free.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }

    const void* tensor(int id) const {
        if (id < 0) return nullptr;
        return d_consts + (tensors[id].offset - consts_base);
    }
};

namespace bn {

// Brackets the launches of one plan operator with HIP events on the launch stream when profiling.
struct ProfScope {
    bn_model* m;
    hipStream_t s;
    hipEvent_t stop = nullptr;
    ProfScope(bn_model* m_, int op, hipStream_t s_) : m(m_), s(s_) {
        if (!m->profiling || (m->prof_only >= 0 && m->prof_only != op)) return;
        hipEvent_t start = m->take_event();
        stop = m->take_event();
        (void)hipEventRecord(start, s);
        m->ev_used.push_back({op, start, stop});
    }
    void end() {
        if (stop) (void)hipEventRecord(stop, s);
        stop = nullptr;
    }
    ~ProfScope() { end(); }
};

// ---- bn_plan_run.hip ----
// Host-side preparation of a parsed plan (`blob`: the bytes its TensorRecs point into): the embedding mark, the per-operator records and
// the sizes of the pooling scratch.  No device call.  BN_OK, or BN_ERR_FORMAT with the message set.
int prepare_plan(bn_model* m, const void* blob);
// The exactness pass's buffers for the chunks from b0 on.
StftGuard guard_slice(const bn_model* m, size_t b0, const SpecStage& st);
// One launch group of a forward call.
struct RunArgs {
    const float* d_input;   // runner-boundary input of the group (null on audio-path plans)
    const float* d_minmax;  // its per-chunk min / max, or null
    int B;
    float* d_scores;
    float* d_logits;        // or null
    void* d_emb;            // or null: where the group's embeddings go, in the form emb_dtype (BN_EMB_*)
    int emb_dtype;
    hipStream_t s;
    const float* d_audio = nullptr;  // audio-path plans: the group's waveforms and their geometry
    int T = 0, hop = 0;
    size_t slot_b0 = 0;     // chunk index the group starts at inside the workspace slots
    SpecStage spec{};       // bn_infer_audio with a spectrogram stage in front of the plan
};
int run_plan(bn_model* m, const RunArgs& a);

}  // namespace bn
