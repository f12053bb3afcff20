// bn_probe_api.hip — the C ABI of a classifier head on frozen embeddings and of its training (host code only):
// bn_head_forward, bn_probe_* (one head; kernels in bn_probe.hip), bn_probe_sweep_* (T heads in lock-step; bn_probe_sweep.hip) and
// bn_head_i8_forward (the head as exported into an INT8 model; bn_head_i8.hip).
//
// A single fit and a sweep are one procedure: their handles share ProbeHandle, and the checks, the workspace growth and the step loop
// are written once (probe_epoch<SWEEP>, probe_loss<SWEEP>).  They differ in where the step sizes come from (computed here, or the
// caller's table), in the strides of the workspaces (a sweep's hold T heads) and in which launcher runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "bn_model.h"

using bn::check_device;
using bn::fail;
using bn::grow_device_buffer;

namespace bn {

struct ProbeHandle {
    bn_ctx* ctx = nullptr;
    int D = 0, C = 0, act = 0, T = 1;                       // T: heads trained at once: 1, or the trials of a sweep
    int loss = BN_PROBE_LOSS_CE;                            // bn_probe_set_loss / bn_probe_sweep_set_loss (shared by a sweep's trials)
    float gamma = 0;
    uint32_t seed = 0;
    int64_t total = 1, t = 0;                               // steps of the cosine schedule (a sweep: for the record), steps taken
    // one step's workspaces of one head; a sweep holds T of each, one behind the other
    float* d_G = nullptr;         size_t G_bytes = 0;       // [batch, C] dLoss/dlogits
    float* d_partial = nullptr;   size_t partial_bytes = 0; // [row groups][(D + 1) * C]
    float* d_loss_part = nullptr; size_t loss_bytes = 0;    // one per 16 rows
    float* d_ss = nullptr;                                  // [probe_n_ss] sums of squares per workgroup of the gradient / reduce kernel
};

}  // namespace bn

struct bn_probe : bn::ProbeHandle {
    int opt = 0;
    float lr = 0, wd = 0, clip = 0, drop = 0;
    float *d_params = nullptr, *d_m = nullptr, *d_v = nullptr;   // [(D + 1) * C] each: W, then the bias as row D
    // bn_probe_set_qat: the forward reads d_wq, made from d_params in front of it, and / or puts the logits on a grid
    int qat_weights = 0, qat_logits = 0;                         // 0 off, 1 per class, 2 per tensor; 0 / 1
    float qat_s_out = 0; int qat_z_out = 0;
    float* d_wq = nullptr;                                       // [(D + 1) * C] the fake-quantised parameters, then amax [C]
};

struct bn_probe_sweep : bn::ProbeHandle {
    int n_ss = 0;
    bn::ProbeSweepTrial* d_trials = nullptr;                // [T]
    float* d_state = nullptr;                               // [T][4][(D + 1) * C]: parameters, m, v, snapshot
};

// A head with one hidden layer (bn_probe_mlp.hip).  D and C are the handle's; the shared workspaces hold G [batch, C],
// the row-group partials of the whole parameter vector and the output layer's loss partials.
struct bn_probe_mlp : bn::ProbeHandle {
    int H = 0, opt = 0;
    float lr = 0, wd = 0, clip = 0, drop = 0;
    float *d_params = nullptr, *d_m = nullptr, *d_v = nullptr;   // [(D + 1) * H | (H + 1) * C] each
    float* d_hd = nullptr;   size_t hd_bytes = 0;                // [rows, H] the hidden activations of a batch, or of a step of bn_probe_mlp_loss
    float* d_dA = nullptr;   size_t dA_bytes = 0;                // [batch, H]
    float* d_Yb = nullptr;   size_t Yb_bytes = 0;                // [batch, C] the batch's targets in batch order
    float* d_wb = nullptr;   size_t wb_bytes = 0;                // [batch] ... and its row weights
    void* d_iota = nullptr;  size_t iota_bytes = 0;              // [batch] int32 0, 1, ...: hd's rows as the gradient kernel indexes them
};

namespace {

template <bool SWEEP>
using ProbeOf = std::conditional_t<SWEEP, bn_probe_sweep, bn_probe>;

int probe_shape_check(int D, int C, int activation) {
    if (D < 1 || D > BN_PROBE_MAX_D) return fail(BN_ERR_ARG, "embedding width D=%d outside 1..%d", D, BN_PROBE_MAX_D);
    if (C < 1 || C > BN_PROBE_MAX_C) return fail(BN_ERR_ARG, "class count C=%d outside 1..%d", C, BN_PROBE_MAX_C);
    if (activation != BN_PROBE_ACT_SIGMOID && activation != BN_PROBE_ACT_SOFTMAX) return fail(BN_ERR_ARG, "unknown activation %d", activation);
    return BN_OK;
}

// The hyperparameters of bn_probe_create (trial < 0) or of row `trial` of a sweep's table, whose refusals begin "trial %d: "
int probe_hyper_check(int trial, int optimizer, float lr, float weight_decay, float clipnorm, float dropout) {
    char pre[24] = "";
    if (trial >= 0) snprintf(pre, sizeof pre, "trial %d: ", trial);
    if (optimizer < BN_PROBE_OPT_ADAM || optimizer > BN_PROBE_OPT_SGD) return fail(BN_ERR_ARG, "%sunknown optimizer %d", pre, optimizer);
    if (!(lr >= 0.0f) || !(weight_decay >= 0.0f) || !(clipnorm >= 0.0f)) return fail(BN_ERR_ARG, "%slr, weight_decay and clipnorm must be >= 0", pre);
    if (!(dropout >= 0.0f && dropout < 1.0f)) return fail(BN_ERR_ARG, "%sdropout %g outside [0, 1)", pre, (double)dropout);
    return BN_OK;
}

// What a call on a handle checks first, in this order; `what`: "probe" or "sweep", `pointers`: every device pointer it needs is there
int probe_call_check(const bn::ProbeHandle* p, const char* what, bool pointers) {
    if (!p) return fail(BN_ERR_ARG, "null %s", what);
    if (int rc = check_device(p->ctx)) return rc;
    if (!pointers) return fail(BN_ERR_ARG, "null device pointer");
    return BN_OK;
}

int probe_rows_check(int64_t n) {
    if (n < 1 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    return BN_OK;
}

int probe_set_loss(bn::ProbeHandle* p, const char* what, int loss, float focal_gamma) {
    if (!p) return fail(BN_ERR_ARG, "null %s", what);
    if (loss != BN_PROBE_LOSS_CE && loss != BN_PROBE_LOSS_FOCAL) return fail(BN_ERR_ARG, "unknown loss %d", loss);
    if (loss == BN_PROBE_LOSS_FOCAL && p->act != BN_PROBE_ACT_SIGMOID) return fail(BN_ERR_ARG, "the focal loss is the sigmoid head's: not with softmax");
    if (!(focal_gamma >= 0.0f) || !std::isfinite(focal_gamma)) return fail(BN_ERR_ARG, "focal_gamma %g must be finite and >= 0", (double)focal_gamma);
    p->loss = loss; p->gamma = focal_gamma;
    return BN_OK;
}

// Most row groups the gradient kernel uses for any batch of up to B rows: enough workgroups for two per CU, at least 16 rows per
// group, and the partials inside BN_PROBE_WORKSPACE_BYTES.  Monotone in B.
int64_t probe_group_cap(int B, int D, int C) {
    const size_t E = (size_t)(D + 1) * C;
    const int tiles = ((D + 1 + 63) / 64) * ((C + 63) / 64);
    int64_t g = std::max<int64_t>(1, 512 / tiles);
    g = std::min<int64_t>(g, std::max<int64_t>(1, (int64_t)(BN_PROBE_WORKSPACE_BYTES / (E * sizeof(float)))));
    return std::min<int64_t>(g, (B + 15) / 16);
}

// Row groups of the gradient kernel for a batch of B rows: from the shapes only.  The rows per group are a multiple of 4 (one MFMA
// k-step), so groups <= probe_group_cap(B) — but NOT monotone in B: a short last batch can have more groups than the full one,
// which is why the workspace is sized by the cap of the full batch.
void probe_groups(int B, int D, int C, int* groups, int* rows_per_group) {
    const int64_t g = probe_group_cap(B, D, C);
    const int rpg = (int)((((B + g - 1) / g) + 3) & ~(int64_t)3);
    *rows_per_group = rpg;
    *groups = (B + rpg - 1) / rpg;
}

// Norm partials of one head: one per workgroup of the gradient kernel, or of the reduce kernel when the batch is split into row groups
int probe_n_ss_tiles(int D, int C) { return ((D + 1 + 63) / 64) * ((C + 63) / 64); }
int probe_n_ss_reduce(int E) { return (E + 1023) / 1024; }
int probe_n_ss(int D, int C) { return std::max(probe_n_ss_tiles(D, C), probe_n_ss_reduce((D + 1) * C)); }

// Dropout at rate p: an element is kept iff its 24-bit draw is >= thresh (0: no dropout), and then scaled
void probe_dropout(float p, uint32_t* thresh, float* scale) {
    *thresh = p > 0.0f ? (uint32_t)std::ceil((double)p * 16777216.0) : 0u;
    *scale = (float)(1.0 / (1.0 - (double)p));
}

// The scale of the loss's mean over n rows: over rows x classes (sigmoid) or over rows (softmax)
float probe_mean_scale(bool softmax, int64_t n, int C) { return softmax ? (float)(1.0 / (double)n) : (float)(1.0 / ((double)n * C)); }

// W [D, C] and b [C] from one head to another.  A (D + 1) x C parameter block is the head (block, block + D * C): its row D is the bias
hipError_t probe_copy_head(float* dst_W, float* dst_b, const float* src_W, const float* src_b, int D, int C, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(dst_W, src_W, (size_t)D * C * sizeof(float), hipMemcpyDeviceToDevice, s);
    return e != hipSuccess ? e : hipMemcpyAsync(dst_b, src_b, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, s);
}

int probe_grow(float** p, size_t* bytes, size_t floats, hipStream_t s) {
    return grow_device_buffer((void**)p, bytes, floats * sizeof(float), floats * sizeof(float), s, BN_ERR_NOMEM, "probe");
}

// the handle's own buffers (`own`) and the shared workspaces; the caller deletes the handle
void probe_free(bn::ProbeHandle* p, std::initializer_list<void*> own) {
    if (p->ctx) (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();   // steps still in flight read and write the buffers freed below
    for (void* q : own)
        if (q) (void)hipFree(q);
    for (float* q : {p->d_G, p->d_partial, p->d_loss_part, p->d_ss})
        if (q) (void)hipFree(q);
}

// T times the bytes one trial of a sweep holds stay within BN_PROBE_SWEEP_BYTES.  A trial holds its state, at batch > 0 also G, the row-group
// partials and the loss partials of a training step, at loss_rows > 0 the loss partials of bn_probe_sweep_loss (the same buffer)
int sweep_cap_check(int D, int C, int batch, int64_t loss_rows, int T) {
    const size_t E = (size_t)(D + 1) * C;
    size_t floats = 4 * E + (size_t)probe_n_ss(D, C);
    if (batch > 0) floats += (size_t)batch * C + (size_t)probe_group_cap(batch, D, C) * E;
    floats += std::max<size_t>((size_t)(batch + 15) / 16, (size_t)(loss_rows + 15) / 16);
    const size_t per = floats * sizeof(float);
    if (per * (size_t)T <= BN_PROBE_SWEEP_BYTES) return BN_OK;
    return fail(BN_ERR_UNSUPPORTED, "a sweep of %d trials of D=%d C=%d%s needs %zu bytes, over the cap of %llu: the largest T that fits is %d", T, D, C,
                batch > 0 ? " at this batch" : loss_rows > 0 ? " over these rows" : "", per * (size_t)T, (unsigned long long)BN_PROBE_SWEEP_BYTES,
                (int)(BN_PROBE_SWEEP_BYTES / per));
}

bn::ProbeSweepArgs sweep_args(const bn_probe_sweep* p, const uint8_t* d_active, size_t G_stride, size_t partial_stride, int loss_stride) {
    bn::ProbeSweepArgs w{};
    w.trials = p->d_trials; w.active = d_active; w.state = p->d_state; w.G = p->d_G; w.partial = p->d_partial; w.ss_part = p->d_ss;
    w.loss_part = p->d_loss_part; w.G_stride = G_stride; w.partial_stride = partial_stride; w.ss_stride = p->n_ss; w.loss_stride = loss_stride;
    w.T = p->T; w.E = (p->D + 1) * p->C;
    return w;
}

// What the next forward of `p` reads as its parameters: the shadow parameters themselves, or their fake-quantised copy, made here
const float* probe_forward_params(const bn_probe* p, hipStream_t s) {
    if (!p->qat_weights) return p->d_params;
    bn::launch_probe_qat_weights(p->d_params, p->d_wq, p->d_wq + (size_t)(p->D + 1) * p->C, p->D, p->C, p->qat_weights == 2, s);
    return p->d_wq;
}

// The forward of a single head under its QAT setting
bool probe_forward(const bn_probe* p, const bn::ProbeFwdArgs& f, int mode, int8_t* d_codes, hipStream_t s) {
    if (!p->qat_logits) return bn::launch_probe_fwd(f, mode, s);
    return bn::launch_probe_fwd_qat(f, bn::ProbeQatArgs{p->qat_s_out, (float)p->qat_z_out, d_codes}, mode, s);
}

// One epoch of a single fit (SWEEP = false: d_step_sizes and d_active are null) or of every active trial of a sweep.  A step is three
// launches, four when the batch is split into row groups; at small batches it is launch-bound, so nothing in the loop allocates or
// goes through a pointer to a function: SWEEP is a constant of the instantiation.
template <bool SWEEP>
int probe_epoch(ProbeOf<SWEEP>* p, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm, int64_t n, int batch,
                const float* d_step_sizes, const uint8_t* d_active, float* d_step_loss, void* stream) {
    if (int rc = probe_call_check(p, SWEEP ? "sweep" : "probe", d_X && d_Y && d_perm && d_step_loss && (!SWEEP || d_step_sizes))) return rc;
    if (int rc = probe_rows_check(n)) return rc;
    if (batch < 1 || batch > n) return fail(BN_ERR_ARG, "batch %d outside 1..%lld", batch, (long long)n);
    const int D = p->D, C = p->C, E = (D + 1) * C, T = p->T;
    if constexpr (SWEEP)
        if (int rc = sweep_cap_check(D, C, batch, 0, T)) return rc;
    hipStream_t s = (hipStream_t)stream;
    // one head's share of the three workspaces; a sweep's trials lie at these strides
    const size_t G_stride = (size_t)batch * C, partial_stride = (size_t)probe_group_cap(batch, D, C) * E;
    const int loss_stride = (batch + 15) / 16;
    if (int rc = probe_grow(&p->d_G, &p->G_bytes, (size_t)T * G_stride, s)) return rc;
    if (int rc = probe_grow(&p->d_partial, &p->partial_bytes, (size_t)T * partial_stride, s)) return rc;
    if (int rc = probe_grow(&p->d_loss_part, &p->loss_bytes, (size_t)T * loss_stride, s)) return rc;
    const bool softmax = p->act == BN_PROBE_ACT_SOFTMAX;
    const int ss_tiles = probe_n_ss_tiles(D, C), ss_reduce = probe_n_ss_reduce(E);
    bn::ProbeFwdArgs f{}; bn::ProbeDwArgs g{}; bn::ProbeUpdateArgs u{};   // first what stays the same from step to step
    f.X = d_X; f.Y = d_Y; f.D = D; f.C = C; f.softmax = softmax; f.seed = p->seed;
    f.row_weight = d_row_weight; f.loss_kind = p->loss; f.focal_gamma = p->gamma;
    g.X = d_X; g.D = D; g.C = C; g.E = E; g.seed = p->seed; u.E = E;
    [[maybe_unused]] bn::ProbeSweepArgs w{};
    if constexpr (SWEEP) {
        w = sweep_args(p, d_active, G_stride, partial_stride, loss_stride);
    } else {
        f.out = p->d_G; f.loss_part = p->d_loss_part;
        probe_dropout(p->drop, &f.drop_thresh, &f.drop_scale);
        g.G = p->d_G; g.partial = p->d_partial; g.ss_part = p->d_ss; g.drop_thresh = f.drop_thresh; g.drop_scale = f.drop_scale;
        u.params = p->d_params; u.m = p->d_m; u.v = p->d_v; u.grad = p->d_partial; u.ss_part = p->d_ss; u.loss_part = p->d_loss_part;
        u.optimizer = p->opt; u.weight_decay = p->wd; u.clip = p->clip;
    }
    const int64_t steps = (n + batch - 1) / batch;
    for (int64_t st = 0; st < steps; ++st, ++p->t) {
        const int B = (int)std::min<int64_t>(batch, n - st * batch);
        f.idx = g.idx = d_perm + st * batch;
        f.n = g.B = B;
        f.step = g.step = (uint32_t)p->t;
        f.g_scale = u.loss_scale = probe_mean_scale(softmax, B, C);
        bool fits;
        if constexpr (SWEEP) {
            fits = bn::launch_probe_sweep_fwd(f, w, 0, s);
        } else {   // (the gradient and the update act on the shadow parameters)
            f.W = probe_forward_params(p, s); f.b = f.W + (size_t)D * C;
            fits = probe_forward(p, f, 0, nullptr, s);
        }
        if (!fits) return fail(BN_ERR_DEVICE, "the probe forward kernel's LDS request was refused");
        int groups;
        probe_groups(B, D, C, &groups, &g.rows_per_group);   // from (B, D, C) alone: a sweep's trials split as a single fit does
        if (SWEEP ? (size_t)groups * E > partial_stride : (size_t)groups * E * sizeof(float) > p->partial_bytes)
            return fail(BN_ERR_UNSUPPORTED, "%d row groups exceed the gradient workspace", groups);
        if constexpr (SWEEP) bn::launch_probe_sweep_dw(g, w, groups, s); else bn::launch_probe_dw(g, groups, s);
        u.n_ss = ss_tiles;
        if (groups > 1) {
            if constexpr (SWEEP) bn::launch_probe_sweep_reduce(w, groups, s); else bn::launch_probe_reduce(p->d_partial, E, groups, p->d_ss, s);
            u.n_ss = ss_reduce;
        }
        u.n_loss = (B + 15) / 16; u.step_loss = d_step_loss + st * T;
        if constexpr (SWEEP) {
            bn::launch_probe_sweep_update(u, w, d_step_sizes + st * T * 2, s);
        } else {   // cosine decay to zero; Adam's bias correction folded into its step size (a sweep's caller uploads the same: device_step_sizes)
            const double frac = (double)std::min<int64_t>(p->t, p->total) / (double)p->total;
            const double lr_t = (double)p->lr * 0.5 * (1.0 + std::cos(M_PI * frac)), t1 = (double)(p->t + 1);
            u.lr = (float)lr_t; u.alpha = (float)(lr_t * std::sqrt(1.0 - std::pow(0.999, t1)) / (1.0 - std::pow(0.9, t1)));
            bn::launch_probe_update(u, s);
        }
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// The loss over n rows as they are (no dropout, no smoothing, no weights): out[0], or out[t] per active trial of a sweep
template <bool SWEEP>
int probe_loss(ProbeOf<SWEEP>* p, const float* d_X, const float* d_Y, int64_t n, const uint8_t* d_active, float* d_out, void* stream) {
    if (int rc = probe_call_check(p, SWEEP ? "sweep" : "probe", d_X && d_Y && d_out)) return rc;
    if (int rc = probe_rows_check(n)) return rc;
    if constexpr (SWEEP)
        if (int rc = sweep_cap_check(p->D, p->C, 0, n, p->T)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t parts = (size_t)(n + 15) / 16;
    if (int rc = probe_grow(&p->d_loss_part, &p->loss_bytes, (size_t)p->T * parts, s)) return rc;
    const bool softmax = p->act == BN_PROBE_ACT_SOFTMAX;
    const float scale = probe_mean_scale(softmax, n, p->C);
    bn::ProbeFwdArgs f{};
    f.X = d_X; f.Y = d_Y; f.n = n; f.D = p->D; f.C = p->C; f.softmax = softmax; f.loss_kind = p->loss; f.focal_gamma = p->gamma;
    [[maybe_unused]] bn::ProbeSweepArgs w{};
    if constexpr (SWEEP) {
        w = sweep_args(p, d_active, 0, 0, (int)parts);
    } else {
        f.W = probe_forward_params(p, s); f.b = f.W + (size_t)p->D * p->C; f.loss_part = p->d_loss_part;
    }
    bool fits;
    if constexpr (SWEEP) fits = bn::launch_probe_sweep_fwd(f, w, 1, s); else fits = probe_forward(p, f, 1, nullptr, s);
    if (!fits) return fail(BN_ERR_DEVICE, "the probe forward kernel's LDS request was refused");
    if constexpr (SWEEP) bn::launch_probe_sweep_loss_sum(w, (long)parts, scale, d_out, s); else bn::launch_probe_loss_sum(p->d_loss_part, (long)parts, scale, d_out, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// ------------------------------------------------------------------------------------------------ one hidden layer (bn_probe_mlp.hip)
int mlp_shape_check(int D, int H, int C, int activation) {
    if (int rc = probe_shape_check(D, C, activation)) return rc;
    if (H < 1 || H > BN_PROBE_MAX_D) return fail(BN_ERR_ARG, "hidden width H=%d outside 1..%d", H, BN_PROBE_MAX_D);
    return BN_OK;
}

size_t mlp_E1(int D, int H) { return (size_t)(D + 1) * H; }
size_t mlp_E(int D, int H, int C) { return mlp_E1(D, H) + (size_t)(H + 1) * C; }

// Rows per step of bn_probe_mlp_loss and bn_head_mlp_forward: the hidden activations of a step take at most 64 MiB; a multiple of 16
int64_t mlp_step_rows(int H) { return std::max<int64_t>(16, (int64_t)((64u << 20) / ((size_t)H * sizeof(float))) & ~(int64_t)15); }

// What a training step at `batch` rows holds besides the row-group partials: hd, dA, G, Yb, wb, the identity index and the loss partials
size_t mlp_batch_bytes(int batch, int H, int C) {
    return ((size_t)batch * (2 * (size_t)H + 2 * (size_t)C + 2) + (size_t)(batch + 15) / 16) * sizeof(float);
}

// Most row groups of both gradient launches for B rows of a fit at `batch` rows per step, as probe_group_cap has them: two workgroups per
// CU, at least 16 rows per group, everything inside BN_PROBE_WORKSPACE_BYTES.  0: not even one group fits.  Monotone in B.
int64_t mlp_group_cap(int B, int batch, int D, int H, int C) {
    const size_t E = mlp_E(D, H, C), other = mlp_batch_bytes(batch, H, C);
    if (other > BN_PROBE_WORKSPACE_BYTES || E * sizeof(float) > BN_PROBE_WORKSPACE_BYTES - other) return 0;
    const int tiles = probe_n_ss_tiles(D, H) + probe_n_ss_tiles(H, C);
    int64_t g = std::max<int64_t>(1, 512 / tiles);
    g = std::min<int64_t>(g, (int64_t)((BN_PROBE_WORKSPACE_BYTES - other) / (E * sizeof(float))));
    return std::min<int64_t>(g, (B + 15) / 16);
}

int mlp_n_ss(int D, int H, int C) { return std::max(probe_n_ss_tiles(D, H) + probe_n_ss_tiles(H, C), probe_n_ss_reduce((int)mlp_E(D, H, C))); }

// the four arrays of a head <-> the parameter vector (dir: true = into the vector)
hipError_t mlp_copy_head(float* P, float* W1, float* b1, float* W2, float* b2, int D, int H, int C, bool into, hipStream_t s) {
    float* at[4] = {P, P + (size_t)D * H, P + mlp_E1(D, H), P + mlp_E1(D, H) + (size_t)H * C};
    float* arr[4] = {W1, b1, W2, b2};
    const size_t n[4] = {(size_t)D * H, (size_t)H, (size_t)H * C, (size_t)C};
    for (int i = 0; i < 4; ++i) {
        const hipError_t e = hipMemcpyAsync(into ? at[i] : arr[i], into ? arr[i] : at[i], n[i] * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One epoch: per step hidden forward, output forward, dW2, hidden backward, dW1, [reduce], update
int mlp_epoch(bn_probe_mlp* p, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm, int64_t n, int batch,
              float* d_step_loss, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_X && d_Y && d_perm && d_step_loss)) return rc;
    if (int rc = probe_rows_check(n)) return rc;
    if (batch < 1 || batch > n) return fail(BN_ERR_ARG, "batch %d outside 1..%lld", batch, (long long)n);
    const int D = p->D, H = p->H, C = p->C, E1 = (int)mlp_E1(D, H), E = (int)mlp_E(D, H, C);
    const int64_t cap = mlp_group_cap(batch, batch, D, H, C);
    if (cap < 1)
        return fail(BN_ERR_UNSUPPORTED, "a step of %d rows of D=%d H=%d C=%d needs %zu bytes of workspace, over the cap of %u", batch, D, H, C,
                    mlp_batch_bytes(batch, H, C) + (size_t)E * sizeof(float), (unsigned)BN_PROBE_WORKSPACE_BYTES);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = probe_grow(&p->d_G, &p->G_bytes, (size_t)batch * C, s)) return rc;
    if (int rc = probe_grow(&p->d_partial, &p->partial_bytes, (size_t)cap * E, s)) return rc;
    if (int rc = probe_grow(&p->d_loss_part, &p->loss_bytes, (size_t)(batch + 15) / 16, s)) return rc;
    if (int rc = probe_grow(&p->d_hd, &p->hd_bytes, (size_t)batch * H, s)) return rc;
    if (int rc = probe_grow(&p->d_dA, &p->dA_bytes, (size_t)batch * H, s)) return rc;
    if (int rc = probe_grow(&p->d_Yb, &p->Yb_bytes, (size_t)batch * C, s)) return rc;
    if (int rc = probe_grow(&p->d_wb, &p->wb_bytes, (size_t)batch, s)) return rc;
    if ((size_t)batch * sizeof(int32_t) > p->iota_bytes) {
        if (int rc = grow_device_buffer(&p->d_iota, &p->iota_bytes, (size_t)batch * sizeof(int32_t), (size_t)batch * sizeof(int32_t), s, BN_ERR_NOMEM, "probe"))
            return rc;
        std::vector<int32_t> iota((size_t)batch);
        for (int i = 0; i < batch; ++i) iota[(size_t)i] = i;
        HIP_TRY(hipMemcpy(p->d_iota, iota.data(), (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));   // (synchronous: `iota` ends here)
    }
    const bool softmax = p->act == BN_PROBE_ACT_SOFTMAX;
    const int tiles1 = probe_n_ss_tiles(D, H), tiles2 = probe_n_ss_tiles(H, C);
    float *P1 = p->d_params, *P2 = p->d_params + E1;
    bn::ProbeMlpFwdArgs h{}; bn::ProbeFwdArgs f{}; bn::ProbeDwArgs g2{}, g1{}; bn::ProbeMlpBwdArgs b{}; bn::ProbeUpdateArgs u{};
    h.X = d_X; h.W1 = P1; h.b1 = P1 + (size_t)D * H; h.hd = p->d_hd; h.Y = d_Y; h.Yb = p->d_Yb; h.row_weight = d_row_weight; h.wb = p->d_wb;
    h.D = D; h.H = H; h.C = C; h.seed = p->seed; h.seed2 = p->seed ^ 0x48494444u;
    probe_dropout(p->drop, &h.drop_thresh, &h.drop_scale);
    // the output layer over (hd, Yb) in batch order: no idx, no dropout (hd carries drop2)
    f.X = p->d_hd; f.Y = p->d_Yb; f.W = P2; f.b = P2 + (size_t)H * C; f.out = p->d_G; f.loss_part = p->d_loss_part; f.D = H; f.C = C; f.softmax = softmax;
    f.drop_thresh = 0; f.drop_scale = 1.0f; f.seed = p->seed; f.row_weight = d_row_weight ? p->d_wb : nullptr; f.loss_kind = p->loss; f.focal_gamma = p->gamma;
    // both gradients write their slice of one vector: the stride between row groups is the whole vector
    g2.X = p->d_hd; g2.idx = (const int*)p->d_iota; g2.G = p->d_G; g2.partial = p->d_partial + E1; g2.ss_part = p->d_ss + tiles1;
    g2.D = H; g2.C = C; g2.E = E; g2.drop_thresh = 0; g2.drop_scale = 1.0f; g2.seed = p->seed;
    g1.X = d_X; g1.G = p->d_dA; g1.partial = p->d_partial; g1.ss_part = p->d_ss; g1.D = D; g1.C = H; g1.E = E;
    g1.drop_thresh = h.drop_thresh; g1.drop_scale = h.drop_scale; g1.seed = p->seed;
    b.G = p->d_G; b.W2 = P2; b.hd = p->d_hd; b.dA = p->d_dA; b.H = H; b.C = C; b.scale2 = h.drop_thresh ? h.drop_scale : 1.0f;
    u.params = p->d_params; u.m = p->d_m; u.v = p->d_v; u.grad = p->d_partial; u.ss_part = p->d_ss; u.loss_part = p->d_loss_part;
    u.E = E; u.optimizer = p->opt; u.weight_decay = p->wd; u.clip = p->clip;
    const int64_t steps = (n + batch - 1) / batch;
    for (int64_t st = 0; st < steps; ++st, ++p->t) {
        const int B = (int)std::min<int64_t>(batch, n - st * batch);
        h.idx = g1.idx = d_perm + st * batch;
        h.n = f.n = B; g1.B = g2.B = b.B = B;
        h.step = g1.step = g2.step = f.step = (uint32_t)p->t;
        f.g_scale = u.loss_scale = probe_mean_scale(softmax, B, C);
        if (!bn::launch_probe_mlp_hidden(h, true, s) || !bn::launch_probe_fwd(f, 0, s))
            return fail(BN_ERR_DEVICE, "the probe forward kernel's LDS request was refused");
        const int64_t gc = mlp_group_cap(B, batch, D, H, C);   // from the shapes alone
        const int rpg = (int)((((B + gc - 1) / gc) + 3) & ~(int64_t)3), groups = (B + rpg - 1) / rpg;
        if ((size_t)groups * E * sizeof(float) > p->partial_bytes) return fail(BN_ERR_UNSUPPORTED, "%d row groups exceed the gradient workspace", groups);
        g1.rows_per_group = g2.rows_per_group = rpg;
        bn::launch_probe_dw(g2, groups, s);
        bn::launch_probe_mlp_bwd(b, s);
        bn::launch_probe_dw(g1, groups, s);
        u.n_ss = tiles1 + tiles2;
        if (groups > 1) {
            bn::launch_probe_reduce(p->d_partial, E, groups, p->d_ss, s);
            u.n_ss = probe_n_ss_reduce(E);
        }
        u.n_loss = (B + 15) / 16; u.step_loss = d_step_loss + st;
        const double frac = (double)std::min<int64_t>(p->t, p->total) / (double)p->total;   // the schedule of bn_probe_epoch
        const double lr_t = (double)p->lr * 0.5 * (1.0 + std::cos(M_PI * frac)), t1 = (double)(p->t + 1);
        u.lr = (float)lr_t; u.alpha = (float)(lr_t * std::sqrt(1.0 - std::pow(0.999, t1)) / (1.0 - std::pow(0.9, t1)));
        bn::launch_probe_update(u, s);
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// hd of rows [r0, r0 + nb) as they lie, without dropout, into d_hd
bool mlp_hidden_plain(const float* d_X, int64_t r0, int64_t nb, int D, int H, const float* W1, const float* b1, float* d_hd, hipStream_t s) {
    bn::ProbeMlpFwdArgs h{};
    h.X = d_X + (size_t)r0 * D; h.W1 = W1; h.b1 = b1; h.hd = d_hd; h.n = nb; h.D = D; h.H = H;
    return bn::launch_probe_mlp_hidden(h, false, s);
}

}  // namespace

extern "C" {

int bn_probe_mlp_create(bn_ctx* ctx, int D, int H, int C, int activation, int optimizer, float lr, float weight_decay, float clipnorm, float dropout,
                        uint32_t seed, int64_t total_steps, const float* d_W1, const float* d_b1, const float* d_W2, const float* d_b2, bn_probe_mlp** out,
                        void* stream) {
    if (!out) return fail(BN_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = check_device(ctx)) return rc;
    if (int rc = mlp_shape_check(D, H, C, activation)) return rc;
    if (int rc = probe_hyper_check(-1, optimizer, lr, weight_decay, clipnorm, dropout)) return rc;
    if (total_steps < 1) return fail(BN_ERR_ARG, "total_steps must be >= 1");
    if (!d_W1 || !d_b1 || !d_W2 || !d_b2) return fail(BN_ERR_ARG, "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    bn_probe_mlp* p = new bn_probe_mlp();
    p->ctx = ctx; p->D = D; p->H = H; p->C = C; p->act = activation; p->opt = optimizer; p->lr = lr; p->wd = weight_decay; p->clip = clipnorm;
    p->drop = dropout; p->seed = seed; p->total = total_steps;
    const size_t E = mlp_E(D, H, C);
    if (hipMalloc(&p->d_params, 3 * E * sizeof(float)) != hipSuccess || hipMalloc(&p->d_ss, (size_t)mlp_n_ss(D, H, C) * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        bn_probe_mlp_destroy(p);
        return fail(BN_ERR_NOMEM, "hipMalloc of the probe's parameters failed");
    }
    p->d_m = p->d_params + E; p->d_v = p->d_m + E;
    hipError_t e = hipMemsetAsync(p->d_m, 0, 2 * E * sizeof(float), s);
    if (e == hipSuccess)
        e = mlp_copy_head(p->d_params, const_cast<float*>(d_W1), const_cast<float*>(d_b1), const_cast<float*>(d_W2), const_cast<float*>(d_b2), D, H, C, true, s);
    if (e != hipSuccess) {
        bn_probe_mlp_destroy(p);
        return fail(BN_ERR_DEVICE, "copying the initial weights failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return BN_OK;
}

void bn_probe_mlp_destroy(bn_probe_mlp* p) {
    if (!p) return;
    probe_free(p, {p->d_params, p->d_hd, p->d_dA, p->d_Yb, p->d_wb, p->d_iota});
    delete p;
}

int bn_probe_mlp_set_loss(bn_probe_mlp* p, int loss, float focal_gamma) { return probe_set_loss(p, "probe", loss, focal_gamma); }

int bn_probe_mlp_epoch_weighted(bn_probe_mlp* p, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm, int64_t n,
                                int batch, float* d_step_loss, void* stream) {
    return mlp_epoch(p, d_X, d_Y, d_row_weight, d_perm, n, batch, d_step_loss, stream);
}

int bn_probe_mlp_loss(bn_probe_mlp* p, const float* d_X, const float* d_Y, int64_t n, float* d_out, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_X && d_Y && d_out)) return rc;
    if (int rc = probe_rows_check(n)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int D = p->D, H = p->H, C = p->C;
    const size_t parts = (size_t)(n + 15) / 16;
    const int64_t step = std::min<int64_t>(mlp_step_rows(H), (n + 15) & ~(int64_t)15);
    if (int rc = probe_grow(&p->d_loss_part, &p->loss_bytes, parts, s)) return rc;
    if (int rc = probe_grow(&p->d_hd, &p->hd_bytes, (size_t)step * H, s)) return rc;
    const bool softmax = p->act == BN_PROBE_ACT_SOFTMAX;
    const float *P1 = p->d_params, *P2 = p->d_params + mlp_E1(D, H);
    bn::ProbeFwdArgs f{};
    f.X = p->d_hd; f.D = H; f.C = C; f.softmax = softmax; f.loss_kind = p->loss; f.focal_gamma = p->gamma; f.W = P2; f.b = P2 + (size_t)H * C;
    for (int64_t r0 = 0; r0 < n; r0 += step) {   // (a step is a multiple of 16 rows: the loss partials of the steps lie one behind the other)
        const int64_t nb = std::min<int64_t>(step, n - r0);
        f.Y = d_Y + (size_t)r0 * C; f.n = nb; f.loss_part = p->d_loss_part + r0 / 16;
        if (!mlp_hidden_plain(d_X, r0, nb, D, H, P1, P1 + (size_t)D * H, p->d_hd, s) || !bn::launch_probe_fwd(f, 1, s))
            return fail(BN_ERR_DEVICE, "the probe forward kernel's LDS request was refused");
    }
    bn::launch_probe_loss_sum(p->d_loss_part, (long)parts, probe_mean_scale(softmax, n, C), d_out, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_probe_mlp_get(bn_probe_mlp* p, float* d_W1, float* d_b1, float* d_W2, float* d_b2, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_W1 && d_b1 && d_W2 && d_b2)) return rc;
    HIP_TRY(mlp_copy_head(p->d_params, d_W1, d_b1, d_W2, d_b2, p->D, p->H, p->C, false, (hipStream_t)stream));
    return BN_OK;
}

int bn_probe_mlp_set(bn_probe_mlp* p, const float* d_W1, const float* d_b1, const float* d_W2, const float* d_b2, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_W1 && d_b1 && d_W2 && d_b2)) return rc;
    HIP_TRY(mlp_copy_head(p->d_params, const_cast<float*>(d_W1), const_cast<float*>(d_b1), const_cast<float*>(d_W2), const_cast<float*>(d_b2), p->D, p->H,
                          p->C, true, (hipStream_t)stream));
    return BN_OK;
}

int bn_head_mlp_forward(bn_ctx* ctx, const float* d_emb, int64_t n, int D, const float* d_W1, const float* d_b1, int H, const float* d_W2,
                        const float* d_b2, int C, int activation, float* d_scores, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = mlp_shape_check(D, H, C, activation)) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    if (n == 0) return BN_OK;
    if (!d_emb || !d_W1 || !d_b1 || !d_W2 || !d_b2 || !d_scores) return fail(BN_ERR_ARG, "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t step = std::min<int64_t>(mlp_step_rows(H), (n + 15) & ~(int64_t)15);
    const size_t need = (size_t)step * H * sizeof(float);
    if (int rc = grow_device_buffer(&ctx->d_mlp_work, &ctx->mlp_work_bytes, need, need, s, BN_ERR_NOMEM, "hidden layer")) return rc;
    float* d_hd = (float*)ctx->d_mlp_work;
    bn::ProbeFwdArgs a{};
    a.X = d_hd; a.W = d_W2; a.b = d_b2; a.D = H; a.C = C; a.softmax = activation == BN_PROBE_ACT_SOFTMAX;
    for (int64_t r0 = 0; r0 < n; r0 += step) {
        const int64_t nb = std::min<int64_t>(step, n - r0);
        a.out = d_scores + (size_t)r0 * C; a.n = nb;
        if (!mlp_hidden_plain(d_emb, r0, nb, D, H, d_W1, d_b1, d_hd, s) || !bn::launch_probe_fwd(a, 2, s))
            return fail(BN_ERR_DEVICE, "the head kernel's LDS request was refused");
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_head_forward(bn_ctx* ctx, const float* d_emb, int64_t n, int D, const float* d_W, const float* d_b, int C, int activation,
                    float* d_scores, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = probe_shape_check(D, C, activation)) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    if (n == 0) return BN_OK;
    if (!d_emb || !d_W || !d_b || !d_scores) return fail(BN_ERR_ARG, "null device pointer");
    bn::ProbeFwdArgs a{};
    a.X = d_emb; a.W = d_W; a.b = d_b; a.out = d_scores; a.n = n; a.D = D; a.C = C; a.softmax = activation == BN_PROBE_ACT_SOFTMAX;
    if (!bn::launch_probe_fwd(a, 2, (hipStream_t)stream)) return fail(BN_ERR_DEVICE, "the head kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// The exported INT8 head over int8 embedding rows (bn_head_i8.hip); a softmax head's scores come from the model's own softmax kernel
int bn_head_i8_forward(bn_ctx* ctx, const int8_t* d_rows, int64_t n, int D, const int8_t* d_w, const int32_t* d_bias, const int32_t* d_mult,
                       const int32_t* d_shift, int C, int zp_out, const int8_t* d_lut, int activation, float s_fc, int8_t* d_logit_bytes,
                       float* d_scores, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = probe_shape_check(D, C, activation)) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    if (zp_out < -128 || zp_out > 127) return fail(BN_ERR_ARG, "zero point %d outside -128..127", zp_out);
    const bool softmax = activation == BN_PROBE_ACT_SOFTMAX;
    if (softmax ? d_lut != nullptr : d_lut == nullptr) return fail(BN_ERR_ARG, "a sigmoid head takes its LOGISTIC table, a softmax head none");
    if (softmax && !d_logit_bytes) return fail(BN_ERR_ARG, "a softmax head needs d_logit_bytes: its scores are computed from them");
    if (n == 0) return BN_OK;
    if (!d_rows || !d_w || !d_bias || !d_mult || !d_shift || !d_scores) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_w % 16 || (uintptr_t)d_bias % 4 || (uintptr_t)d_mult % 4 || (uintptr_t)d_shift % 4 || (uintptr_t)d_lut % 4 || (uintptr_t)d_scores % 4)
        return fail(BN_ERR_ARG, "d_w must be 16-byte aligned, the int32 / float32 arrays and the table 4-byte aligned");
    bn::HeadI8Geom g{};
    if (!bn::head_i8_geometry((long)n, D, C, &g)) return fail(BN_ERR_ARG, "D=%d: no class tile fits the LDS", D);
    bn::HeadI8Args a{};
    a.rows = d_rows; a.w = d_w; a.bias = d_bias; a.mult = d_mult; a.shift = d_shift; a.lut = d_lut; a.logit = d_logit_bytes; a.scores = d_scores;
    a.n = (long)n; a.D = D; a.C = C; a.zp_out = zp_out; a.pass_tiles = g.pass_tiles; a.steps_per_wg = g.steps_per_wg;
    a.wide = C % 4 == 0 && (uintptr_t)d_scores % 16 == 0 && (uintptr_t)d_logit_bytes % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (!bn::launch_head_i8(a, g, s)) return fail(BN_ERR_DEVICE, "the INT8 head kernel's LDS request was refused");
    // one workgroup of 64 threads per row: slices keep a launch's thread count below 2^32
    constexpr int64_t kSoftmaxSlice = 1 << 24;
    for (int64_t r0 = 0; softmax && r0 < n; r0 += kSoftmaxSlice) {
        const int nb = (int)std::min<int64_t>(kSoftmaxSlice, n - r0);
        bn::launch_i8_head_softmax(d_logit_bytes + (size_t)r0 * C, d_scores + (size_t)r0 * C, nullptr, nb, C, zp_out, s_fc, 1.0f, s);
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// Classes per LDS pass of bn_head_i8_forward (head_i8_geometry, the launcher's own plan); host only, no device needed
int bn_head_i8_pass_classes(int D, int C) {
    if (int rc = probe_shape_check(D, C, BN_PROBE_ACT_SIGMOID)) return rc;
    bn::HeadI8Geom g{};
    if (!bn::head_i8_geometry(0, D, C, &g)) return fail(BN_ERR_ARG, "D=%d: no class tile fits the LDS", D);
    return 16 * g.pass_tiles;
}

// ------------------------------------------------------------------------------------------------------------ one head (bn_probe.hip)
int bn_probe_create(bn_ctx* ctx, int D, int C, int activation, int optimizer, float lr, float weight_decay, float clipnorm, float dropout,
                    uint32_t seed, int64_t total_steps, const float* d_W, const float* d_b, bn_probe** out, void* stream) {
    if (!out) return fail(BN_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = check_device(ctx)) return rc;
    if (int rc = probe_shape_check(D, C, activation)) return rc;
    if (int rc = probe_hyper_check(-1, optimizer, lr, weight_decay, clipnorm, dropout)) return rc;
    if (total_steps < 1) return fail(BN_ERR_ARG, "total_steps must be >= 1");
    if (!d_W || !d_b) return fail(BN_ERR_ARG, "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    bn_probe* p = new bn_probe();
    p->ctx = ctx; p->D = D; p->C = C; p->act = activation; p->opt = optimizer; p->lr = lr; p->wd = weight_decay; p->clip = clipnorm;
    p->drop = dropout; p->seed = seed; p->total = total_steps;
    const size_t E = (size_t)(D + 1) * C;
    if (hipMalloc(&p->d_params, 3 * E * sizeof(float)) != hipSuccess || hipMalloc(&p->d_ss, (size_t)probe_n_ss(D, C) * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        bn_probe_destroy(p);
        return fail(BN_ERR_NOMEM, "hipMalloc of the probe's parameters failed");
    }
    p->d_m = p->d_params + E; p->d_v = p->d_m + E;
    hipError_t e = hipMemsetAsync(p->d_m, 0, 2 * E * sizeof(float), s);
    if (e == hipSuccess) e = probe_copy_head(p->d_params, p->d_params + (size_t)D * C, d_W, d_b, D, C, s);
    if (e != hipSuccess) {
        bn_probe_destroy(p);
        return fail(BN_ERR_DEVICE, "copying the initial weights failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return BN_OK;
}

void bn_probe_destroy(bn_probe* p) {
    if (!p) return;
    probe_free(p, {p->d_params, p->d_wq});
    delete p;
}

int bn_probe_set_loss(bn_probe* p, int loss, float focal_gamma) { return probe_set_loss(p, "probe", loss, focal_gamma); }

int bn_probe_epoch(bn_probe* p, const float* d_X, const float* d_Y, const int32_t* d_perm, int64_t n, int batch, float* d_step_loss,
                   void* stream) {
    return probe_epoch<false>(p, d_X, d_Y, nullptr, d_perm, n, batch, nullptr, nullptr, d_step_loss, stream);
}

int bn_probe_epoch_weighted(bn_probe* p, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm, int64_t n,
                            int batch, float* d_step_loss, void* stream) {
    return probe_epoch<false>(p, d_X, d_Y, d_row_weight, d_perm, n, batch, nullptr, nullptr, d_step_loss, stream);
}

int bn_probe_loss(bn_probe* p, const float* d_X, const float* d_Y, int64_t n, float* d_out, void* stream) {
    return probe_loss<false>(p, d_X, d_Y, n, nullptr, d_out, stream);
}

int bn_probe_get(bn_probe* p, float* d_W, float* d_b, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_W && d_b)) return rc;
    HIP_TRY(probe_copy_head(d_W, d_b, p->d_params, p->d_params + (size_t)p->D * p->C, p->D, p->C, (hipStream_t)stream));
    return BN_OK;
}

int bn_probe_set(bn_probe* p, const float* d_W, const float* d_b, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_W && d_b)) return rc;
    HIP_TRY(probe_copy_head(p->d_params, p->d_params + (size_t)p->D * p->C, d_W, d_b, p->D, p->C, (hipStream_t)stream));
    return BN_OK;
}

// Quantisation-aware fine-tuning
int bn_probe_set_qat(bn_probe* p, int weight_mode, int quantize_logits, float s_out, int z_out) {
    if (!p) return fail(BN_ERR_ARG, "null probe");
    if (weight_mode < BN_PROBE_QAT_OFF || weight_mode > BN_PROBE_QAT_PER_TENSOR) return fail(BN_ERR_ARG, "unknown QAT weight mode %d", weight_mode);
    if (quantize_logits) {
        if (!std::isfinite(s_out) || !(s_out > 0.0f)) return fail(BN_ERR_ARG, "the logit scale %g must be finite and > 0", (double)s_out);
        if (z_out < -128 || z_out > 127) return fail(BN_ERR_ARG, "zero point %d outside -128..127", z_out);
    }
    if (weight_mode && !p->d_wq) {
        if (int rc = check_device(p->ctx)) return rc;
        if (hipMalloc(&p->d_wq, ((size_t)(p->D + 1) * p->C + p->C) * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            p->d_wq = nullptr;
            return fail(BN_ERR_NOMEM, "hipMalloc of the probe's fake-quantised parameters failed");
        }
    }
    p->qat_weights = weight_mode; p->qat_logits = quantize_logits ? 1 : 0;
    p->qat_s_out = quantize_logits ? s_out : 0.0f; p->qat_z_out = quantize_logits ? z_out : 0;
    return BN_OK;
}

int bn_probe_get_quantized(bn_probe* p, float* d_Wq, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_Wq)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(d_Wq, probe_forward_params(p, s), (size_t)p->D * p->C * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_probe_scores(bn_probe* p, const float* d_X, int64_t n, float* d_scores, int8_t* d_codes, void* stream) {
    if (int rc = probe_call_check(p, "probe", d_X && d_scores)) return rc;
    if (int rc = probe_rows_check(n)) return rc;
    if (d_codes && !p->qat_logits) return fail(BN_ERR_ARG, "d_codes needs the logits quantised (bn_probe_set_qat)");
    hipStream_t s = (hipStream_t)stream;
    bn::ProbeFwdArgs f{};
    f.X = d_X; f.out = d_scores; f.n = n; f.D = p->D; f.C = p->C; f.softmax = p->act == BN_PROBE_ACT_SOFTMAX;
    f.W = probe_forward_params(p, s); f.b = f.W + (size_t)p->D * p->C;
    if (!probe_forward(p, f, 2, d_codes, s)) return fail(BN_ERR_DEVICE, "the probe forward kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// ------------------------------------------------------------------------------------------- T heads in lock-step (bn_probe_sweep.hip)
int bn_probe_sweep_create(bn_ctx* ctx, int D, int C, int activation, int T, const bn_probe_trial* trials, uint32_t seed, int64_t total_steps,
                          const float* d_W, const float* d_b, bn_probe_sweep** out, void* stream) {
    if (!out) return fail(BN_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = check_device(ctx)) return rc;
    if (int rc = probe_shape_check(D, C, activation)) return rc;
    if (T < 1 || T > BN_PROBE_SWEEP_MAX_TRIALS) return fail(BN_ERR_ARG, "trial count T=%d outside 1..%d", T, BN_PROBE_SWEEP_MAX_TRIALS);
    if (!trials) return fail(BN_ERR_ARG, "null trial table");
    if (total_steps < 1) return fail(BN_ERR_ARG, "total_steps must be >= 1");
    if (!d_W || !d_b) return fail(BN_ERR_ARG, "null device pointer");
    std::vector<bn::ProbeSweepTrial> rows((size_t)T);
    for (int t = 0; t < T; ++t) {
        const bn_probe_trial& h = trials[t];
        if (int rc = probe_hyper_check(t, h.optimizer, h.lr, h.weight_decay, h.clipnorm, h.dropout)) return rc;
        if (!(h.label_smoothing >= 0.0f && h.label_smoothing < 1.0f))
            return fail(BN_ERR_ARG, "trial %d: label_smoothing %g outside [0, 1)", t, (double)h.label_smoothing);
        bn::ProbeSweepTrial& r = rows[(size_t)t];
        r.optimizer = h.optimizer; r.weight_decay = h.weight_decay; r.clip = h.clipnorm;
        probe_dropout(h.dropout, &r.drop_thresh, &r.drop_scale);
        const float eps = h.label_smoothing;
        r.smooth = eps > 0.0f;
        r.smooth_keep = 1.0f - eps;
        r.smooth_add = activation == BN_PROBE_ACT_SOFTMAX ? eps / (float)C : 0.5f * eps;
    }
    if (int rc = sweep_cap_check(D, C, 0, 0, T)) return rc;
    hipStream_t s = (hipStream_t)stream;
    bn_probe_sweep* p = new bn_probe_sweep();
    p->ctx = ctx; p->D = D; p->C = C; p->act = activation; p->T = T; p->seed = seed; p->total = total_steps;
    const size_t E = (size_t)(D + 1) * C;
    p->n_ss = probe_n_ss(D, C);
    if (hipMalloc(&p->d_state, (size_t)T * 4 * E * sizeof(float)) != hipSuccess || hipMalloc(&p->d_ss, (size_t)T * p->n_ss * sizeof(float)) != hipSuccess ||
        hipMalloc(&p->d_trials, (size_t)T * sizeof(bn::ProbeSweepTrial)) != hipSuccess) {
        (void)hipGetLastError();
        bn_probe_sweep_destroy(p);
        return fail(BN_ERR_NOMEM, "hipMalloc of the sweep's parameters failed");
    }
    hipError_t e = hipMemsetAsync(p->d_state, 0, (size_t)T * 4 * E * sizeof(float), s);
    for (int t = 0; t < T; ++t)
        for (int slot : {0, 3}) {   // the parameters and the snapshot
            float* dst = p->d_state + ((size_t)t * 4 + slot) * E;
            if (e == hipSuccess) e = probe_copy_head(dst, dst + (size_t)D * C, d_W, d_b, D, C, s);
        }
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_trials, rows.data(), (size_t)T * sizeof(bn::ProbeSweepTrial), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // `rows` is pageable host memory that ends with this call
    if (e != hipSuccess) {
        bn_probe_sweep_destroy(p);
        return fail(BN_ERR_DEVICE, "copying the initial weights failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return BN_OK;
}

void bn_probe_sweep_destroy(bn_probe_sweep* p) {
    if (!p) return;
    probe_free(p, {p->d_trials, p->d_state});
    delete p;
}

int bn_probe_sweep_set_loss(bn_probe_sweep* p, int loss, float focal_gamma) { return probe_set_loss(p, "sweep", loss, focal_gamma); }

int bn_probe_sweep_epoch(bn_probe_sweep* p, const float* d_X, const float* d_Y, const int32_t* d_perm, int64_t n, int batch,
                         const float* d_step_sizes, const uint8_t* d_active, float* d_step_loss, void* stream) {
    return probe_epoch<true>(p, d_X, d_Y, nullptr, d_perm, n, batch, d_step_sizes, d_active, d_step_loss, stream);
}

int bn_probe_sweep_epoch_weighted(bn_probe_sweep* p, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm,
                                  int64_t n, int batch, const float* d_step_sizes, const uint8_t* d_active, float* d_step_loss, void* stream) {
    return probe_epoch<true>(p, d_X, d_Y, d_row_weight, d_perm, n, batch, d_step_sizes, d_active, d_step_loss, stream);
}

int bn_probe_sweep_loss(bn_probe_sweep* p, const float* d_X, const float* d_Y, int64_t n, const uint8_t* d_active, float* d_out, void* stream) {
    return probe_loss<true>(p, d_X, d_Y, n, d_active, d_out, stream);
}

int bn_probe_sweep_snapshot(bn_probe_sweep* p, const uint8_t* d_mask, void* stream) {
    if (int rc = probe_call_check(p, "sweep", d_mask)) return rc;
    bn::launch_probe_sweep_snapshot(sweep_args(p, nullptr, 0, 0, 0), d_mask, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_probe_sweep_get(bn_probe_sweep* p, int trial, int which, float* d_W, float* d_b, void* stream) {
    if (int rc = probe_call_check(p, "sweep", true)) return rc;
    if (trial < 0 || trial >= p->T) return fail(BN_ERR_ARG, "trial %d outside 0..%d", trial, p->T - 1);
    if (which != BN_PROBE_SWEEP_CURRENT && which != BN_PROBE_SWEEP_SNAPSHOT) return fail(BN_ERR_ARG, "unknown slot %d", which);
    if (!d_W || !d_b) return fail(BN_ERR_ARG, "null device pointer");
    const size_t E = (size_t)(p->D + 1) * p->C;
    const float* src = p->d_state + ((size_t)trial * 4 + (which == BN_PROBE_SWEEP_SNAPSHOT ? 3 : 0)) * E;
    HIP_TRY(probe_copy_head(d_W, d_b, src, src + (size_t)p->D * p->C, p->D, p->C, (hipStream_t)stream));
    return BN_OK;
}

}  // extern "C"
