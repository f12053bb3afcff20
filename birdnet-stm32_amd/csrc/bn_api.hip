// bn_api.hip — the C ABI of libbirdnet_hip.so (include/birdnet_hip.h): context and model
// lifetime, packed-blob parsing, workspace allocation and the entry points that split a
// bn_forward()/bn_infer_audio() call into launch groups for the plan executor (bn_plan_run.hip).
// The entry points of the classifier head and its training (bn_head_forward, bn_head_i8_forward, bn_probe_*) are in bn_probe_api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bn_model.h"

namespace {

thread_local std::string g_err;

constexpr int kFft = 512;

struct OptName {
    const char* name;
    int bn::Options::*field;
};
const OptName kOptions[] = {
    {"f32_strip", &bn::Options::f32_strip},       {"f32_strip_th", &bn::Options::f32_strip_th},
    {"f32_front_staged", &bn::Options::f32_front_staged}, {"f32_front2", &bn::Options::f32_front2}, {"f32_pwdw", &bn::Options::f32_pwdw}, {"f32_tile_slice", &bn::Options::f32_tile_slice}, {"f32_pw_ws", &bn::Options::f32_pw_ws}, {"i8_pwdw", &bn::Options::i8_pwdw}, {"i8_pw_lds", &bn::Options::i8_pw_lds}, {"i8_pw_forms", &bn::Options::i8_pw_forms}, {"i8_add_tab", &bn::Options::i8_add_tab}, {"front_tpw", &bn::Options::front_tpw},
    {"wave_dwpw", &bn::Options::wave_dwpw},       {"i8_strip", &bn::Options::i8_strip},
    {"i8_strip_th", &bn::Options::i8_strip_th}, {"i8_dw_pool", &bn::Options::i8_dw_pool}, {"i8_tail_fclds", &bn::Options::i8_tail_fclds},   {"i8_tail", &bn::Options::i8_tail}, {"i8_tail_mfdw", &bn::Options::i8_tail_mfdw}, {"i8_mid", &bn::Options::i8_mid}, {"i8_mid_split", &bn::Options::i8_mid_split}, {"i8_satpack", &bn::Options::i8_satpack},
    {"i8_mel_generic", &bn::Options::i8_mel_generic}, {"stft_rowmajor", &bn::Options::stft_rowmajor},
    {"i8_strip_mfdw", &bn::Options::i8_strip_mfdw}, {"stft_exact", &bn::Options::stft_exact}, {"stft_flagcap", &bn::Options::stft_flagcap}, {"stft_guard", &bn::Options::stft_guard}, {"stft_audit", &bn::Options::stft_audit}, {"stft_minint", &bn::Options::stft_minint},
    {"ingest_blk", &bn::Options::ingest_blk},
    {"ingest_generic", &bn::Options::ingest_generic},
};

// BN_<NAME> environment variables seed the options once, when the library is loaded (A/B runs of bench.py from a shell)
bn::Options options_from_env() {
    bn::Options o;
    for (const OptName& e : kOptions) {
        std::string var = "BN_";
        for (const char* c = e.name; *c; ++c) var += (char)toupper((unsigned char)*c);
        if (const char* v = getenv(var.c_str())) o.*(e.field) = atoi(v);
    }
    return o;
}

}  // namespace

namespace bn {
thread_local Options g_opt;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace bn
using bn::fail;
using bn::kMaxGridBatch;
using bn::ProfScope;

bn::Options g_opt_default = options_from_env();   // the process default (bn_set_option); copied into bn::g_opt per API call
std::mutex g_opt_mu;

namespace bn {

int check_device(bn_ctx* ctx) {
    if (!ctx) return fail(BN_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    {   // the switches this call's launchers see: the process default, then the context's own
        std::lock_guard<std::mutex> lock(g_opt_mu);
        bn::g_opt = g_opt_default;
        for (const auto& ov : ctx->opt_override) bn::g_opt.*(ov.first) = ov.second;
    }
    return BN_OK;
}

// Grows a device buffer that a context or a probe owns to at least `need` bytes; `alloc` >= need is what it asks for when it has to.
// Never inside a capture: it waits for the stream first, whose work in flight may still use the old buffer.  A refused allocation is the
// caller's `code`, about its `what` workspace.
int grow_device_buffer(void** p, size_t* have, size_t need, size_t alloc, hipStream_t s, int code, const char* what) {
    if (need <= *have) return BN_OK;
    HIP_TRY(hipStreamSynchronize(s));
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipMalloc(p, alloc) != hipSuccess) {
        (void)hipGetLastError();
        return fail(code, "hipMalloc of %zu bytes for the %s workspace failed", alloc, what);
    }
    *have = alloc;
    return BN_OK;
}

}  // namespace bn
using bn::check_device;
using bn::grow_device_buffer;

namespace {

// What every entry point over an [n, D] matrix of embedding rows (bn_search_*, bn_kmeans_*, bn_density_*) checks first
int row_matrix_check(int dtype, int64_t n, int D, int max_D, int zero_point) {
    if (dtype != BN_DTYPE_F32 && dtype != BN_DTYPE_I8) return fail(BN_ERR_ARG, "unknown dtype %d", dtype);
    if (D < 1 || D > max_D) return fail(BN_ERR_ARG, "embedding width D=%d outside 1..%d", D, max_D);
    if (n < 0 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    if (dtype == BN_DTYPE_I8 && (zero_point < -128 || zero_point > 127)) return fail(BN_ERR_ARG, "zero point %d outside -128..127", zero_point);
    return BN_OK;
}

}  // namespace

extern "C" {

int bn_version(void) { return BN_ABI_VERSION; }

const char* bn_last_error(void) { return g_err.c_str(); }

int bn_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bn_ctx_create(int device, int max_batch, bn_ctx** out) {
    if (!out) return fail(BN_ERR_ARG, "out is null");
    *out = nullptr;
    if (max_batch <= 0) return fail(BN_ERR_ARG, "max_batch must be positive, got %d", max_batch);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(BN_ERR_DEVICE, "no HIP device is visible; libbirdnet_hip has no CPU fallback");
    if (device < 0 || device >= n) return fail(BN_ERR_ARG, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BN_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);

    bn_ctx* c = new bn_ctx();
    struct Guard {  // a failing HIP call below returns early: release what has been allocated so far
        bn_ctx* c;
        ~Guard() {
            if (c) bn_ctx_destroy(c);
        }
    } guard{c};
    c->device = device;
    c->max_batch = max_batch;
    // STFT tables in double, rounded once to float32
    std::vector<float> win(kFft);
    std::vector<float4> t256(256), t512(257);
    const double two_pi = 6.283185307179586476925286766559;
    // per-lane base angles; the kernel rebuilds window and split-pass twiddles from them (see bn_stft.hip)
    win.assign(64, 0.0f);
    for (int j = 0; j < 16; ++j) {
        const double t0 = two_pi * (2 * j) / 512.0, t1 = two_pi * (2 * j + 1) / 512.0;
        win[4 * j + 0] = (float)(-0.25 * cos(t0));
        win[4 * j + 1] = (float)(-0.25 * cos(t1));
        win[4 * j + 2] = (float)(0.25 * sin(t0));
        win[4 * j + 3] = (float)(0.25 * sin(t1));
    }
    for (int i = 0; i < 256; ++i) {  // w = exp(-2 pi i p / 256), stored with its rotation (-w.y, w.x)
        const float c = (float)cos(two_pi * i / 256.0), sn = (float)sin(two_pi * i / 256.0);
        t256[i] = make_float4(c, -sn, sn, c);
    }
    t512.assign(16, make_float4(0, 0, 0, 0));
    for (int j = 0; j < 16; ++j) {
        const float c = (float)cos(two_pi * j / 512.0), sn = (float)sin(two_pi * j / 512.0);
        t512[j] = make_float4(-sn, -c, -c, sn);
    }
    HIP_TRY(hipMalloc(&c->d_window, win.size() * sizeof(float)));
    HIP_TRY(hipMalloc(&c->d_tw256, t256.size() * sizeof(float4)));
    HIP_TRY(hipMalloc(&c->d_tw512, t512.size() * sizeof(float4)));
    HIP_TRY(hipMemcpy(c->d_window, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_tw256, t256.data(), t256.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_tw512, t512.data(), t512.size() * sizeof(float4), hipMemcpyHostToDevice));
    // float64 tables of the exactness pass: cos(2 pi j / 512) with the symmetries exact (cs[128] = 0, cs[j] = -cs[256 - j], ...),
    // the reference's periodic Hann window 0.5 - 0.5 cos(2 pi n / 512) from it
    std::vector<double> f64tab(2048);
    for (int j = 0; j < 512; ++j) {
        const int a2 = j <= 256 ? j : 512 - j;                 // cos is even about pi
        const int a3 = a2 <= 128 ? a2 : 256 - a2;              // and odd about pi / 2
        const double v = a3 <= 64 ? cos(two_pi * a3 / 512.0) : sin(two_pi * (128 - a3) / 512.0);
        f64tab[512 + j] = a2 <= 128 ? v : -v;
        if (a3 == 128) f64tab[512 + j] = 0.0;
    }
    for (int n = 0; n < 512; ++n) f64tab[n] = 0.5 - 0.5 * f64tab[512 + n];
    for (int j = 0; j < 512; ++j) {  // (cos, sin) pairs: sin(a) = cos(a - pi / 2)
        f64tab[1024 + 2 * j] = f64tab[512 + j];
        f64tab[1024 + 2 * j + 1] = f64tab[512 + ((j + 384) & 511)];
    }
    HIP_TRY(hipMalloc(&c->d_f64tab, f64tab.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(c->d_f64tab, f64tab.data(), f64tab.size() * sizeof(double), hipMemcpyHostToDevice));
    c->tables = bn::StftTables{c->d_window, c->d_tw256, c->d_tw512, c->d_f64tab, c->d_f64tab + 512, reinterpret_cast<const double2*>(c->d_f64tab + 1024)};
    // bn_ingest_resample's per-workgroup peak scratch (one float per >= 1024 resampled samples): sized here for windows that
    // yield max_batch 3 s chunks at 24 kHz (72 blocks per chunk) with headroom, so that the ingest call itself does not allocate
    // (no hidden device sync on that path); a call that needs more still grows it, once.
    c->block_peaks_elems = (size_t)max_batch * 128 + 65536;
    HIP_TRY(hipMalloc(&c->d_block_peaks, c->block_peaks_elems * sizeof(float)));
    guard.c = nullptr;
    *out = c;
    return BN_OK;
}

void bn_ctx_destroy(bn_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipFree(c->d_window);
    (void)hipFree(c->d_tw256);
    (void)hipFree(c->d_tw512);
    (void)hipFree(c->d_f64tab);
    (void)hipFree(c->d_block_peaks);
    if (c->d_rank_work) (void)hipFree(c->d_rank_work);
    if (c->d_search_work) (void)hipFree(c->d_search_work);
    if (c->d_kmeans_work) (void)hipFree(c->d_kmeans_work);
    if (c->d_tsne_work) (void)hipFree(c->d_tsne_work);
    if (c->d_pca_work) (void)hipFree(c->d_pca_work);
    if (c->d_propagate_work) (void)hipFree(c->d_propagate_work);
    if (c->d_select_work) (void)hipFree(c->d_select_work);
    if (c->d_boot_work) (void)hipFree(c->d_boot_work);
    if (c->d_mlp_work) (void)hipFree(c->d_mlp_work);
    delete c;
}

// Parse and validate a packed blob (host only): tables inside the blob, payloads aligned and in range, operator references in
// range, every operator's geometry against the slot and tensor sizes (bn_plan_check.hip).
static int parse_blob(const void* blob, size_t nbytes, BlobHeader& h, std::vector<SlotRec>& slots, std::vector<TensorRec>& tensors,
                      std::vector<OpRec>& ops) {
    if (!blob || nbytes < sizeof(BlobHeader)) return fail(BN_ERR_FORMAT, "blob too small (%zu bytes)", nbytes);
    const char* base = (const char*)blob;
    memcpy(&h, base, sizeof h);
    if (memcmp(h.magic, BN_BLOB_MAGIC, 8) != 0) return fail(BN_ERR_FORMAT, "bad blob magic");
    if (h.version != BN_BLOB_VERSION)
        return fail(BN_ERR_FORMAT, "blob version %u, library expects %u", h.version, BN_BLOB_VERSION);
    auto in_range = [&](uint64_t off, uint64_t len) { return off <= nbytes && len <= nbytes - off; };
    if (!in_range(h.slots_off, (uint64_t)h.n_slots * sizeof(SlotRec)) ||
        !in_range(h.tensors_off, (uint64_t)h.n_tensors * sizeof(TensorRec)) ||
        !in_range(h.ops_off, (uint64_t)h.n_ops * sizeof(OpRec)))
        return fail(BN_ERR_FORMAT, "blob tables exceed the blob size");
    slots.resize(h.n_slots);
    tensors.resize(h.n_tensors);
    ops.resize(h.n_ops);
    if (h.n_slots) memcpy(slots.data(), base + h.slots_off, h.n_slots * sizeof(SlotRec));
    if (h.n_tensors) memcpy(tensors.data(), base + h.tensors_off, h.n_tensors * sizeof(TensorRec));
    if (h.n_ops) memcpy(ops.data(), base + h.ops_off, h.n_ops * sizeof(OpRec));
    for (const TensorRec& t : tensors)
        if (!in_range(t.offset, t.nbytes) || (t.offset & 255)) return fail(BN_ERR_FORMAT, "tensor payload out of range or misaligned");
    for (const SlotRec& sl : slots)
        if (sl.bytes_per_chunk > (1ull << 32)) return fail(BN_ERR_FORMAT, "slot of %llu bytes per chunk", (unsigned long long)sl.bytes_per_chunk);
    for (const OpRec& o : ops) {
        for (int k = 0; k < BN_OP_NT; ++k)
            if (o.t[k] >= (int)h.n_tensors) return fail(BN_ERR_FORMAT, "operator references tensor %d of %u", o.t[k], h.n_tensors);
        const int ids[3] = {o.in0, o.in1, o.out};
        for (int id : ids)
            if (id >= (int)h.n_slots || (id < 0 && id != BN_SLOT_INPUT && id != BN_SLOT_SCORES && id != BN_SLOT_LOGITS && id != BN_SLOT_AUDIO && id != BN_SLOT_NONE))
                return fail(BN_ERR_FORMAT, "operator references slot %d of %u", id, h.n_slots);
    }
    std::string why;
    if (!bn::check_plan(h, slots, tensors, ops, why)) return fail(BN_ERR_FORMAT, "%s", why.c_str());
    return BN_OK;
}

int bn_blob_check(const void* blob, size_t nbytes) {
    BlobHeader h;
    std::vector<SlotRec> slots;
    std::vector<TensorRec> tensors;
    std::vector<OpRec> ops;
    return parse_blob(blob, nbytes, h, slots, tensors, ops);
}

int bn_model_load(bn_ctx* ctx, const void* blob, size_t nbytes, bn_model** out) {
    if (!out) return fail(BN_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = check_device(ctx)) return rc;
    bn_model* m = new bn_model();
    m->ctx = ctx;
    if (int rc = parse_blob(blob, nbytes, m->hdr, m->slots, m->tensors, m->ops)) {
        delete m;
        return rc;
    }
    if (int rc = bn::prepare_plan(m, blob)) {  // embedding mark, per-operator records, scratch sizes (bn_plan_run.hip)
        delete m;
        return rc;
    }
    const BlobHeader& h = m->hdr;
    const char* base = (const char*)blob;
    size_t lo = nbytes, hi = 0;
    for (const TensorRec& t : m->tensors)
        if (t.nbytes) {
            lo = t.offset < lo ? (size_t)t.offset : lo;
            hi = t.offset + t.nbytes > hi ? (size_t)(t.offset + t.nbytes) : hi;
        }
    auto cleanup_fail = [&](int code) {
        bn_model_free(m);
        return code;
    };
    if (hi > lo) {
        m->consts_base = lo;
        m->consts_bytes = hi - lo;
        if (hipMalloc(&m->d_consts, m->consts_bytes) != hipSuccess)
            return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of %zu constant bytes failed", m->consts_bytes));
        if (hipMemcpy(m->d_consts, base + lo, m->consts_bytes, hipMemcpyHostToDevice) != hipSuccess)
            return cleanup_fail(fail(BN_ERR_DEVICE, "copying constants to the device failed"));
    }
    const size_t mb = (size_t)ctx->max_batch;
    m->d_slots.assign(h.n_slots, nullptr);
    for (uint32_t i = 0; i < h.n_slots; ++i) {
        const size_t bytes = mb * m->slots[i].bytes_per_chunk;
        if (bytes == 0) continue;
        if (hipMalloc(&m->d_slots[i], bytes) != hipSuccess)
            return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of %zu workspace bytes (slot %u) failed", bytes, i));
        m->workspace_bytes += bytes;
    }
    if (h.input_kind == BN_INPUT_SPECTROGRAM) {
        const size_t bytes = mb * h.input_elems * sizeof(float);
        if (hipMalloc(&m->d_spec, bytes) != hipSuccess)
            return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of %zu spectrogram workspace bytes failed", bytes));
        m->workspace_bytes += bytes;
    }
    if (m->guard_form_ok && h.dtype == BN_DTYPE_I8) {
        // exactness pass of the audio path (plans with another zero point take the float64 STFT for every bin): per chunk W bounds, W / 16 tile records, a list of flagged elements, counters
        const size_t W = h.spec_width, n_tiles = (W + 15) / 16, t64 = (W + 63) / 64;
        const int cap = 1 << 20;  // a chunk's count beyond this = one of its mel-mixer workgroups gave up (more in doubt than it keeps)
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t o = off;
            off += (bytes + 255) & ~(size_t)255;
            return o;
        };
        const size_t o_eps = take(mb * W * 4), o_rec = take(mb * n_tiles * bn::kGuardRec * 4), o_list = take(mb * 4), o_cnt = take(mb * 4),
                     o_dirty = take(mb * 4), o_work = take(mb * t64 * 4), o_nw = take(4 * (mb / kMaxGridBatch + 1)), o_hard = take(2 * mb * 4),
                     o_nh = take(8 * (mb / kMaxGridBatch + 1)), o_audit = take(8);
        if (hipMalloc(&m->d_guard, off) != hipSuccess) return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of %zu exactness-pass bytes failed", off));
        m->workspace_bytes += off;
        char* g = m->d_guard;
        m->guard = bn::StftGuard{(float*)(g + o_eps), (int*)(g + o_rec), (float*)(g + o_list), (int*)(g + o_cnt), cap, (int*)(g + o_dirty),
                                 (int*)(g + o_work), (int*)(g + o_nw), (int*)(g + o_hard), (int*)(g + o_nh), (int)mb};
        m->d_audit = (int*)(g + o_audit);
    }
    if (hipMalloc(&m->d_minmax, mb * 2 * sizeof(float)) != hipSuccess ||
        hipMalloc(&m->d_smax, mb * sizeof(float)) != hipSuccess)
        return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of reduction scratch failed"));
    m->workspace_bytes += mb * 3 * sizeof(float);
    if (m->pool8_C) {
        if (hipMalloc(&m->d_pool8, mb * m->pool8_C * sizeof(int32_t)) != hipSuccess)
            return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of pooling scratch failed"));
        if (hipMemset(m->d_pool8, 0, mb * m->pool8_C * sizeof(int32_t)) != hipSuccess) return cleanup_fail(fail(BN_ERR_DEVICE, "clearing the pooling scratch failed"));
        m->workspace_bytes += mb * m->pool8_C * sizeof(int32_t);
    }
    if (m->gap_part_elems) {
        if (hipMalloc(&m->d_gap_part, mb * m->gap_part_elems * sizeof(float)) != hipSuccess)
            return cleanup_fail(fail(BN_ERR_NOMEM, "hipMalloc of pooling scratch failed"));
        m->workspace_bytes += mb * m->gap_part_elems * sizeof(float);
    }
    *out = m;
    return BN_OK;
}

void bn_model_free(bn_model* m) {
    if (!m) return;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    (void)hipFree(m->d_consts);
    for (char* p : m->d_slots) (void)hipFree(p);
    (void)hipFree(m->d_spec);
    (void)hipFree(m->d_minmax);
    (void)hipFree(m->d_guard);
    (void)hipFree(m->d_smax);
    (void)hipFree(m->d_gap_part);
    (void)hipFree(m->d_pool8);
    for (auto& r : m->ev_used) {
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    for (hipEvent_t e : m->ev_free) (void)hipEventDestroy(e);
    delete m;
}

int bn_model_get_info(const bn_model* m, bn_model_info* out) {
    if (!m || !out) return fail(BN_ERR_ARG, "null argument");
    out->dtype = (int32_t)m->hdr.dtype;
    out->input_kind = (int32_t)m->hdr.input_kind;
    out->input_elems = (int32_t)m->hdr.input_elems;
    out->fft_bins = (int32_t)m->hdr.fft_bins;
    out->spec_width = (int32_t)m->hdr.spec_width;
    out->num_classes = (int32_t)m->hdr.num_classes;
    out->n_ops = (int32_t)m->hdr.n_ops;
    out->max_batch = m->ctx->max_batch;
    out->workspace_bytes = (int64_t)m->workspace_bytes;
    out->const_bytes = (int64_t)m->consts_bytes;
    return BN_OK;
}

static int stft_mag_impl(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W, int normalize, float* d_spec,
                         float* d_minmax, void* stream, bool tile_major, bool exact = false);

int bn_stft_mag(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W, int normalize,
                float* d_spec, float* d_minmax, void* stream) {
    return stft_mag_impl(ctx, d_audio, B, T, n_fft, hop, W, normalize, d_spec, d_minmax, stream, false);
}

int bn_stft_mag_exact(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W, int normalize,
                      float* d_spec, float* d_minmax, void* stream) {
    return stft_mag_impl(ctx, d_audio, B, T, n_fft, hop, W, normalize, d_spec, d_minmax, stream, false, true);
}

// tile_major: spectrogram as [W/16][257][16] per chunk (private to bn_infer_audio; the public entry point keeps [257][W])
static int stft_mag_impl(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W, int normalize, float* d_spec,
                         float* d_minmax, void* stream, bool tile_major, bool exact) {
    if (int rc = check_device(ctx)) return rc;
    if (!d_audio || !d_spec || !d_minmax) return fail(BN_ERR_ARG, "null device pointer");
    if (n_fft != kFft) return fail(BN_ERR_UNSUPPORTED, "n_fft=%d: only 512 is implemented", n_fft);
    if (B < 0 || T <= 0 || W <= 0 || hop <= 0) return fail(BN_ERR_ARG, "bad shape B=%d T=%d hop=%d W=%d", B, T, hop, W);
    if (1 + T / hop < W)
        return fail(BN_ERR_ARG, "T=%d hop=%d gives %d frames, fewer than spec_width=%d", T, hop, 1 + T / hop, W);
    if (B == 0) return BN_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t per_chunk = (size_t)(kFft / 2 + 1) * W;
    for (int b0 = 0; b0 < B; b0 += kMaxGridBatch) {
        const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
        bn::launch_minmax_init(d_minmax + 2 * (size_t)b0, nb, s);
        if (exact)  // every bin as a float64 DFT: the reference's values (bn_stft_exact.hip)
            bn::launch_stft512_f64(ctx->tables, d_audio + (size_t)b0 * T, nb, T, hop, W, d_spec + b0 * per_chunk, d_minmax + 2 * (size_t)b0, s,
                                   tile_major);
        else
            bn::launch_stft512(ctx->tables, d_audio + (size_t)b0 * T, nb, T, hop, W, d_spec + b0 * per_chunk,
                               d_minmax + 2 * (size_t)b0, s, tile_major);
        if (normalize)
            bn::launch_spec_normalize(d_spec + b0 * per_chunk, d_minmax + 2 * (size_t)b0, nb, (int)per_chunk, s);
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_mel_spectrogram(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W, const float* d_mel_w,
                       const int32_t* d_mel_bands, int n_mels, int mode, int mag_scale, double pcen_b, const float* d_dct,
                       int n_mfcc, float* d_work, float* d_out, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (!d_audio || !d_mel_w || !d_mel_bands || !d_work || !d_out) return fail(BN_ERR_ARG, "null device pointer");
    if (n_fft != kFft) return fail(BN_ERR_UNSUPPORTED, "n_fft=%d: only 512 is implemented", n_fft);
    if (B < 0 || T <= 0 || W <= 0 || hop <= 0 || n_mels <= 0) return fail(BN_ERR_ARG, "bad shape B=%d T=%d hop=%d W=%d mels=%d", B, T, hop, W, n_mels);
    if (1 + T / hop < W)
        return fail(BN_ERR_ARG, "T=%d hop=%d gives %d frames, fewer than spec_width=%d", T, hop, 1 + T / hop, W);
    if (mode < BN_SPEC_MEL || mode > BN_SPEC_MFCC) return fail(BN_ERR_ARG, "unknown spectrogram mode %d", mode);
    if (mag_scale < BN_MAG_NONE || mag_scale > BN_MAG_DB) return fail(BN_ERR_ARG, "unknown mag_scale %d", mag_scale);
    if (mode != BN_SPEC_MEL) mag_scale = BN_MAG_NONE;  // the reference applies mag_scale only in 'mel' / 'linear' mode
    if (mode == BN_SPEC_MFCC && (!d_dct || n_mfcc <= 0 || n_mfcc > n_mels)) return fail(BN_ERR_ARG, "mfcc needs 0 < n_mfcc <= n_mels and a DCT matrix");
    // mfcc: the reference takes the dB reference and floor over ALL 1 + T / hop frames and cuts to W after the DCT
    const int Wall = mode == BN_SPEC_MFCC ? 1 + T / hop : W;
    if ((n_mels * Wall) % 4) return fail(BN_ERR_UNSUPPORTED, "n_mels * frames must be a multiple of 4");
    if (bn::melspec_finish_lds_bytes(n_mels, Wall, W, mode, mag_scale, n_mfcc) + 64 > 160 * 1024)
        return fail(BN_ERR_UNSUPPORTED, "a %d x %d mel map (mode %d) does not fit one workgroup's LDS", n_mels, Wall, mode);
    if (B == 0) return BN_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t per = (size_t)n_mels * Wall;
    const size_t per_out = mode == BN_SPEC_MFCC ? (size_t)n_mfcc * W : per;
    for (int b0 = 0; b0 < B; b0 += kMaxGridBatch) {
        const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
        float* mel = d_work + (size_t)b0 * per;
        float* minmax = d_work + (size_t)B * per + 2 * (size_t)b0;
        bn::launch_minmax_init(minmax, nb, s);
        if (!bn::launch_stft512_mel(ctx->tables, d_audio + (size_t)b0 * T, nb, T, hop, Wall, mel, n_mels, d_mel_w, d_mel_bands, minmax, s,
                                    mode == BN_SPEC_MFCC))
            return fail(BN_ERR_UNSUPPORTED, "n_mels=%d: the fused STFT+mel kernel takes at most 128 mel bins", n_mels);
        if (!bn::launch_melspec_finish(mel, d_out + (size_t)b0 * per_out, d_dct, nb, n_mels, Wall, W, mode, mag_scale, n_mfcc, pcen_b, s))
            return fail(BN_ERR_DEVICE, "could not raise the LDS limit of the spectrogram finishing kernel");
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

// the checks of an embedding request; *esize = bytes per embedding value
static int emb_check(const bn_model* m, const void* d_emb, int emb_dtype, size_t* esize) {
    *esize = 0;
    if (!d_emb) return BN_OK;
    if (m->emb_dim <= 0) return fail(BN_ERR_UNSUPPORTED, "this model's plan marks no embedding operator (lower it with this build)");
    if (emb_dtype != BN_EMB_F32 && emb_dtype != BN_EMB_I8) return fail(BN_ERR_ARG, "unknown embedding dtype %d", emb_dtype);
    if (emb_dtype == BN_EMB_I8 && m->hdr.dtype != BN_DTYPE_I8) return fail(BN_ERR_ARG, "BN_EMB_I8 needs an INT8 plan; float32 plans give BN_EMB_F32");
    if ((uintptr_t)d_emb % (emb_dtype == BN_EMB_I8 ? 4 : 16)) return fail(BN_ERR_ARG, "d_emb must be 16-byte (float32) / 4-byte (int8) aligned");
    *esize = emb_dtype == BN_EMB_I8 ? 1 : 4;
    return BN_OK;
}

static int forward_impl(bn_model* m, const float* d_input, const float* d_minmax, int B, float* d_scores, float* d_logits, void* d_emb,
                        int emb_dtype, void* stream);
static int infer_audio_impl(bn_model* m, const float* d_audio, int B, int T, int hop, float* d_scores, float* d_logits, void* d_emb,
                            int emb_dtype, void* stream);

int bn_forward(bn_model* m, const float* d_input, const float* d_minmax, int B, float* d_scores, float* d_logits,
               void* stream) {
    return forward_impl(m, d_input, d_minmax, B, d_scores, d_logits, nullptr, BN_EMB_F32, stream);
}

int bn_forward_embed(bn_model* m, const float* d_input, const float* d_minmax, int B, float* d_scores, float* d_logits, void* d_emb,
                     int emb_dtype, void* stream) {
    return forward_impl(m, d_input, d_minmax, B, d_scores, d_logits, d_emb, emb_dtype, stream);
}

int bn_infer_audio(bn_model* m, const float* d_audio, int B, int T, int hop, float* d_scores, float* d_logits,
                   void* stream) {
    return infer_audio_impl(m, d_audio, B, T, hop, d_scores, d_logits, nullptr, BN_EMB_F32, stream);
}

int bn_infer_audio_embed(bn_model* m, const float* d_audio, int B, int T, int hop, float* d_scores, float* d_logits, void* d_emb,
                         int emb_dtype, void* stream) {
    return infer_audio_impl(m, d_audio, B, T, hop, d_scores, d_logits, d_emb, emb_dtype, stream);
}

int bn_model_get_embedding_info(const bn_model* m, int* dim, int* dtype, float* scale, int* zero_point) {
    if (!m) return fail(BN_ERR_ARG, "null model");
    if (m->emb_dim <= 0) return fail(BN_ERR_UNSUPPORTED, "this model's plan marks no embedding operator (lower it with this build)");
    if (dim) *dim = m->emb_dim;
    if (dtype) *dtype = m->hdr.dtype == BN_DTYPE_I8 ? BN_EMB_I8 : BN_EMB_F32;
    if (scale) *scale = m->emb_scale;
    if (zero_point) *zero_point = m->emb_zp;
    return BN_OK;
}

}  // extern "C"

static int forward_impl(bn_model* m, const float* d_input, const float* d_minmax, int B, float* d_scores, float* d_logits, void* d_emb,
                        int emb_dtype, void* stream) {
    if (!m) return fail(BN_ERR_ARG, "null model");
    size_t esize = 0;
    if (int rc = emb_check(m, d_emb, emb_dtype, &esize)) return rc;
    const size_t D = (size_t)m->emb_dim;
    if (int rc = check_device(m->ctx)) return rc;
    if (!d_input || !d_scores) return fail(BN_ERR_ARG, "null device pointer");
    if (B < 0 || B > m->ctx->max_batch)
        return fail(BN_ERR_ARG, "batch %d exceeds the context's max_batch %d", B, m->ctx->max_batch);
    if (B == 0) return BN_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t in_stride = m->hdr.input_elems, C = m->hdr.num_classes;
    for (int b0 = 0; b0 < B; b0 += kMaxGridBatch) {
        const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
        const bn::RunArgs ra{d_input + b0 * in_stride, d_minmax ? d_minmax + 2 * (size_t)b0 : nullptr, nb, d_scores + b0 * C,
                             d_logits ? d_logits + b0 * C : nullptr, d_emb ? (char*)d_emb + b0 * D * esize : nullptr, emb_dtype, s};
        if (int rc = bn::run_plan(m, ra)) return rc;
    }
    return BN_OK;
}

static int infer_audio_impl(bn_model* m, const float* d_audio, int B, int T, int hop, float* d_scores, float* d_logits, void* d_emb,
                            int emb_dtype, void* stream) {
    if (!m) return fail(BN_ERR_ARG, "null model");
    size_t esize = 0;
    if (int rc = emb_check(m, d_emb, emb_dtype, &esize)) return rc;
    const size_t D = (size_t)m->emb_dim;
    if (m->hdr.input_kind != BN_INPUT_SPECTROGRAM)
        return fail(BN_ERR_UNSUPPORTED, "bn_infer_audio needs a hybrid-frontend model; feed waveforms to bn_forward");
    if (B < 0 || B > m->ctx->max_batch)
        return fail(BN_ERR_ARG, "batch %d exceeds the context's max_batch %d", B, m->ctx->max_batch);
    const int F = (int)m->hdr.fft_bins, W = (int)m->hdr.spec_width;
    if (F != kFft / 2 + 1) return fail(BN_ERR_UNSUPPORTED, "model expects %d frequency bins; the STFT kernel gives 257", F);
    bool audio_plan = false;
    for (const OpRec& o : m->ops) audio_plan |= o.p[BN_OP_PATH] == BN_PATH_AUDIO;
    if (audio_plan) {
        // the plan holds operators that start from the waveform (fused STFT + mel mixer): no spectrogram in HBM
        if (int rc = check_device(m->ctx)) return rc;
        if (!d_audio || !d_scores) return fail(BN_ERR_ARG, "null device pointer");
        if (T <= 0 || hop <= 0 || 1 + T / hop < W) return fail(BN_ERR_ARG, "bad audio geometry T=%d hop=%d W=%d", T, hop, W);
        if (B == 0) return BN_OK;
        const size_t C = m->hdr.num_classes;
        for (int b0 = 0; b0 < B; b0 += kMaxGridBatch) {
            const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
            const bn::RunArgs ra{nullptr, nullptr, nb, d_scores + b0 * C, d_logits ? d_logits + b0 * C : nullptr,
                                 d_emb ? (char*)d_emb + b0 * D * esize : nullptr, emb_dtype, (hipStream_t)stream, d_audio + (size_t)b0 * T, T, hop};
            if (int rc = bn::run_plan(m, ra)) return rc;
        }
        return BN_OK;
    }
    // un-normalised magnitudes + per-chunk min/max; the plan's first operator normalises while loading
    if (int rc = check_device(m->ctx)) return rc;
    if (!d_audio || !d_scores) return fail(BN_ERR_ARG, "null device pointer");
    if (B == 0) return BN_OK;
    const bool tiled = m->spec_tiled_ok && !bn::g_opt.stft_rowmajor;  // option stft_rowmajor: keep the reference layout (A/B)
    hipStream_t s = (hipStream_t)stream;
    const size_t in_stride = m->hdr.input_elems, C = m->hdr.num_classes;
    // INT8 plans: the quantised input bytes must be the reference's (float64 STFT).  Production form: float32 STFT with error bounds,
    // exact min / max, doubtful bytes listed by the first operator and recomputed in float64 behind it (bn_stft_exact.hip);
    // plans / options outside that form (debug plans, row-major layout, generic mel kernel) take the float64 STFT for every bin.
    const bool i8 = m->hdr.dtype == BN_DTYPE_I8;
    const int exact_opt = i8 ? bn::g_opt.stft_exact : 0;
    const bool guarded = exact_opt == 2 && tiled && m->d_guard && !bn::g_opt.i8_mel_generic && W % 16 == 0 && W <= 1024;
    // (Sub-batching the STFT -> first operator pair for the Infinity Cache and a two-stream skewed schedule were measured and removed:
    // slower / no gain)
    int rc = BN_OK;
    if (guarded) {
        // profiling entries: n_ops = the float32 STFT kernel, n_ops + 1 = exact min / max, n_ops + 2 = the float64 pass behind the first operator
        if (T <= 0 || hop <= 0 || 1 + T / hop < W) rc = fail(BN_ERR_ARG, "T=%d hop=%d gives %d frames, fewer than spec_width=%d", T, hop, hop > 0 ? 1 + T / hop : 0, W);
        if (m->d_audit) HIP_TRY(hipMemsetAsync(m->d_audit, 0, 2 * sizeof(int), s));
        for (int b0 = 0; rc == BN_OK && b0 < B; b0 += kMaxGridBatch) {
            const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
            bn::StftGuard g = bn::guard_slice(m, (size_t)b0, bn::SpecStage{tiled, true, d_audio + (size_t)b0 * T, T, hop});
            {
                ProfScope prof(m, (int)m->ops.size(), s);
                bn::launch_stft512(m->ctx->tables, d_audio + (size_t)b0 * T, nb, T, hop, W, m->d_spec + b0 * in_stride, m->d_minmax + 2 * (size_t)b0, s,
                                   true, &g);
            }
            ProfScope prof(m, (int)m->ops.size() + 1, s);
            bn::launch_stft_minmax_exact(m->ctx->tables, d_audio + (size_t)b0 * T, nb, T, hop, W, m->d_spec + b0 * in_stride, true, g,
                                         m->d_minmax + 2 * (size_t)b0, s);
        }
    } else {
        ProfScope prof(m, (int)m->ops.size(), s);
        rc = stft_mag_impl(m->ctx, d_audio, B, T, kFft, hop, W, /*normalize=*/0, m->d_spec, m->d_minmax, stream, tiled, exact_opt != 0);
    }
    if (rc == BN_OK) {
        for (int b0 = 0; b0 < B; b0 += kMaxGridBatch) {
            const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
            bn::RunArgs ra{m->d_spec + b0 * in_stride, m->d_minmax + 2 * (size_t)b0, nb, d_scores + b0 * C, d_logits ? d_logits + b0 * C : nullptr,
                           d_emb ? (char*)d_emb + b0 * D * esize : nullptr, emb_dtype, s};
            ra.slot_b0 = (size_t)b0;
            ra.spec = bn::SpecStage{tiled, guarded, d_audio + (size_t)b0 * T, T, hop};
            rc = bn::run_plan(m, ra);
            if (rc != BN_OK) break;
        }
    }
    m->last_tiled = tiled;
    m->last_B = rc == BN_OK ? B : 0;
    return rc;
}

extern "C" {

int bn_debug_tail_form(const bn_model* m, int* form, int* lds_bytes) {
    if (!m || !form || !lds_bytes) return fail(BN_ERR_ARG, "null argument");
    *form = 0;
    *lds_bytes = 0;
    for (size_t oi = 0; oi < m->ops.size(); ++oi) {
        if (m->ops[oi].kind != BN_OP_I8_TAIL || !m->prep[oi]->ok) continue;
        const bn::OpPrep& pr = *m->prep[oi];
        *form = pr.alt_ok ? 2 : 1;
        *lds_bytes = pr.alt_ok ? pr.chain.lds_bytes : pr.tail.lds_bytes;
    }
    return BN_OK;
}

int bn_debug_mid_form(const bn_model* m, int* form, int* lds_bytes) {
    if (!m || !form || !lds_bytes) return fail(BN_ERR_ARG, "null argument");
    *form = 0;
    *lds_bytes = 0;
    for (size_t oi = 0; oi < m->ops.size(); ++oi)
        if (m->ops[oi].kind == BN_OP_I8_MID && m->prep[oi]->ok) {
            *form = 1;
            *lds_bytes = m->prep[oi]->chain.lds_bytes;
        }
    return BN_OK;
}

int bn_debug_satpack_form(const bn_model* m, int* mid, int* tail, int* front) {
    if (!m || !mid || !tail || !front) return fail(BN_ERR_ARG, "null argument");
    *mid = *tail = *front = -1;
    for (size_t oi = 0; oi < m->ops.size(); ++oi) {
        const bn::OpPrep& pr = *m->prep[oi];
        namespace k = bn::op::i8_front;
        const OpRec& o = m->ops[oi];
        if (o.kind == BN_OP_I8_FRONT && o.p[k::strip] && o.t[k::strip_cst] >= 0 &&
            bn::i8_front_strip_supported(o.p[k::H0], o.p[k::W0], o.p[k::C], o.p[k::N], o.p[k::OH], o.p[k::OW]))
            *front = bn::front_strip_satpack_ok(o.p[k::stem_amin], o.p[k::stem_amax]) ? 1 : 0;
        if (m->ops[oi].kind == BN_OP_I8_MID && pr.ok) *mid = pr.chain.satpack;
        if (m->ops[oi].kind == BN_OP_I8_TAIL && pr.ok && pr.alt_ok) *tail = pr.chain.satpack;
    }
    return BN_OK;
}

int bn_debug_mid_plan(const bn_model* m, int* out, int n) {
    if (!m || !out || n < 1) return fail(BN_ERR_ARG, "null argument");
    out[0] = 0;
    for (size_t oi = 0; oi < m->ops.size(); ++oi)
        if (m->ops[oi].kind == BN_OP_I8_MID && m->prep[oi]->ok && m->prep[oi]->alt_ok) {
            if (!bn::tail2_plan_dump(m->prep[oi]->resident, out, n)) return fail(BN_ERR_ARG, "n=%d is too small for the plan", n);
            break;
        }
    return BN_OK;
}

int bn_debug_mid_split_giveups(bn_ctx* ctx, int64_t* count) {
    if (!ctx || !count) return fail(BN_ERR_ARG, "null argument");
    if (int rc = check_device(ctx)) return rc;
    const long n = bn::tail2_giveups();
    if (n < 0) return fail(BN_ERR_DEVICE, "could not read the chunk barriers' give-up counter");
    *count = n;
    return BN_OK;
}

int bn_debug_guard_stats(bn_model* m, int B, int64_t* out) {
    if (!m || !out) return fail(BN_ERR_ARG, "null argument");
    if (int rc = check_device(m->ctx)) return rc;
    if (!m->d_guard) return fail(BN_ERR_UNSUPPORTED, "the plan has no exactness pass");
    if (B <= 0 || B > m->last_B || B > kMaxGridBatch) return fail(BN_ERR_ARG, "B=%d: the last bn_infer_audio call left %d spectrograms", B, m->last_B);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<int> cnt((size_t)B);
    int nw = 0, nh[2] = {0, 0};
    HIP_TRY(hipMemcpy(cnt.data(), m->guard.count, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&nw, m->guard.n_work, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nh, m->guard.n_hard, 2 * sizeof(int), hipMemcpyDeviceToHost));
    int64_t total = 0, mx = 0;
    for (int c : cnt) {
        c %= m->guard.cap + 1;   // (every workgroup of the mixer that hands its chunk over adds cap + 1: a marker, not elements)
        total += c;
        if (c > mx) mx = c;
    }
    out[0] = total;
    out[1] = mx;
    out[2] = nw;
    out[3] = nh[0];
    out[4] = nh[1];
    int au[2] = {0, 0};
    if (m->d_audit) HIP_TRY(hipMemcpy(au, m->d_audit, sizeof au, hipMemcpyDeviceToHost));
    out[5] = au[0];
    out[6] = au[1];
    std::vector<float> lo((size_t)B);   // chunks whose minimum was enclosed in an interval instead of settled (option stft_minint)
    HIP_TRY(hipMemcpy(lo.data(), m->guard.mn_lo, (size_t)B * sizeof(float), hipMemcpyDeviceToHost));
    int64_t wide = 0;
    for (float v : lo) wide += v >= 0.0f;
    out[7] = wide;
    return BN_OK;
}

int bn_debug_input_bytes(bn_model* m, int B, int8_t* d_out, void* stream) {
    if (!m || !d_out) return fail(BN_ERR_ARG, "null argument");
    if (int rc = check_device(m->ctx)) return rc;
    namespace k = bn::op::i8_dwpw;
    const OpRec* first = nullptr;
    for (const OpRec& o : m->ops)
        if (o.in0 == BN_SLOT_INPUT && o.kind == BN_OP_I8_DWPW && o.p[k::q_at_load] && o.p[k::transposed]) first = &o;
    if (!first || !m->d_spec) return fail(BN_ERR_UNSUPPORTED, "the plan's first operator is not the mel mixer with QUANTIZE fused into its load");
    if (B <= 0 || B > m->last_B || B > kMaxGridBatch) return fail(BN_ERR_ARG, "B=%d: the last bn_infer_audio call left %d spectrograms", B, m->last_B);
    bn::launch_spec_bytes(m->d_spec, m->d_minmax, B, (int)m->hdr.spec_width, m->last_tiled, first->f[k::qscale], first->p[k::qzp], d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_ingest_resample(bn_ctx* ctx, const void* d_pcm, int sample_format, int channels, const int64_t* d_in_off,
                       const int64_t* d_out_off, int n_windows, int64_t max_in_len, int64_t max_out_len, const float* d_taps,
                       int up, int down, int taps_per_phase, int n_pre_remove, float* d_mono, float* d_peak, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (!d_pcm || !d_in_off || !d_out_off || !d_mono || !d_peak) return fail(BN_ERR_ARG, "null device pointer");
    if (sample_format < BN_PCM_S16 || sample_format > BN_PCM_F32) return fail(BN_ERR_ARG, "unknown sample format %d", sample_format);
    if (channels < 1 || channels > 8)
        return fail(BN_ERR_UNSUPPORTED, "%d channels: the channel mean is implemented for 1..8 channels", channels);
    if (n_windows < 0 || max_in_len < 0 || max_out_len < 0 || up < 1 || down < 1 || taps_per_phase < 0 || n_pre_remove < 0)
        return fail(BN_ERR_ARG, "bad ingest geometry");
    if (taps_per_phase > 0 && !d_taps) return fail(BN_ERR_ARG, "null filter");
    if (taps_per_phase == 0 && up != down) return fail(BN_ERR_ARG, "up=%d down=%d needs a filter", up, down);
    if (n_windows == 0 || max_out_len == 0) return BN_OK;
    if (n_windows > 65535) return fail(BN_ERR_ARG, "at most 65535 windows per call");
    if ((double)(max_out_len + n_pre_remove + 4096) * down >= 4294967296.0 || (double)max_in_len * up >= 4294967296.0)
        return fail(BN_ERR_UNSUPPORTED, "window too long for the 32-bit polyphase index (%lld samples, up=%d, down=%d)",
                    (long long)max_in_len, up, down);
    const size_t lds = bn::ingest_resample_lds_bytes(up, down, taps_per_phase, bn::ingest_resample_block(up, down, taps_per_phase));
    const bool fast_kernel = (up == 1 && (down == 2 || down == 4)) || (up > 1 && up <= 256 && (taps_per_phase == 21 || taps_per_phase == 29 || taps_per_phase == 39));
    if (lds > (fast_kernel ? 64 : 156) * 1024)  // (only the generic kernel's limit is raised to the CU's 160 KB)
        return fail(BN_ERR_UNSUPPORTED, "resampling ratio %d/%d needs %zu bytes of LDS per workgroup (limit %d)", up, down, lds, (fast_kernel ? 64 : 156) * 1024);
    hipStream_t s = (hipStream_t)stream;
    const size_t need = bn::ingest_partial_elems(n_windows, (long)max_out_len, up, down, taps_per_phase);
    if (need > ctx->block_peaks_elems) {  // growing frees the old buffer, which waits for launches still using it
        if (ctx->d_block_peaks) HIP_TRY(hipFree(ctx->d_block_peaks));
        ctx->d_block_peaks = nullptr;
        ctx->block_peaks_elems = 0;
        HIP_TRY(hipMalloc(&ctx->d_block_peaks, need * sizeof(float)));
        ctx->block_peaks_elems = need;
    }
    bn::launch_ingest_resample(d_pcm, sample_format, channels, (const long*)d_in_off, (const long*)d_out_off, n_windows,
                               (long)max_out_len, d_taps, up, down, taps_per_phase, n_pre_remove, d_mono, ctx->d_block_peaks,
                               d_peak, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_ingest_resample_span(bn_ctx* ctx, const void* d_pcm, int sample_format, int channels, int64_t s0, int64_t n_staged, int64_t n_in,
                            int64_t o0, int64_t o1, const float* d_taps, int up, int down, int taps_per_phase, int n_pre_remove,
                            float* d_mono_window, float* d_peak, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (!d_mono_window || !d_peak) return fail(BN_ERR_ARG, "null device pointer");
    if (sample_format < BN_PCM_S16 || sample_format > BN_PCM_F32) return fail(BN_ERR_ARG, "unknown sample format %d", sample_format);
    if (channels < 1 || channels > 8)
        return fail(BN_ERR_UNSUPPORTED, "%d channels: the channel mean is implemented for 1..8 channels", channels);
    if (s0 < 0 || n_staged < 0 || n_in < 0 || o0 < 0 || o1 < o0 || up < 1 || down < 1 || taps_per_phase < 0 || n_pre_remove < 0)
        return fail(BN_ERR_ARG, "bad span geometry");
    if (taps_per_phase > 0 && !d_taps) return fail(BN_ERR_ARG, "null filter");
    if (taps_per_phase == 0 && up != down) return fail(BN_ERR_ARG, "up=%d down=%d needs a filter", up, down);
    // 64-bit positions: (n + pre) * down and n_in * up stay far below 2^63 for windows of up to 2^40 frames (years of audio)
    if (n_in >= ((int64_t)1 << 40) || up >= (1 << 20) || down >= (1 << 20))
        return fail(BN_ERR_UNSUPPORTED, "window of %lld frames at up=%d down=%d is beyond the resampler's 64-bit positions", (long long)n_in, up, down);
    const int64_t n_out = taps_per_phase == 0 ? n_in : (n_in * up + down - 1) / down;
    if (o1 > n_out) return fail(BN_ERR_ARG, "outputs [%lld, %lld) lie beyond the window's %lld outputs", (long long)o0, (long long)o1, (long long)n_out);
    if (o0 == o1) return BN_OK;
    const int blk = bn::ingest_resample_block(up, down, taps_per_phase);
    if ((uint64_t)blk * (uint64_t)down + (uint64_t)up >= ((uint64_t)1 << 32))
        return fail(BN_ERR_UNSUPPORTED, "down=%d: a workgroup's %d outputs overflow the 32-bit in-workgroup phase index", down, blk);
    if ((o1 - o0 + blk - 1) / blk >= ((int64_t)1 << 31)) return fail(BN_ERR_UNSUPPORTED, "span of %lld outputs is too long for one launch", (long long)(o1 - o0));
    // the input frames outputs [o0, o1) touch, clipped to the window, must all be staged
    int64_t need_lo, need_hi;
    if (taps_per_phase == 0) {
        need_lo = o0;
        need_hi = o1;
    } else {
        need_lo = (o0 + n_pre_remove) * (int64_t)down / up - (taps_per_phase - 1);
        need_hi = (o1 - 1 + n_pre_remove) * (int64_t)down / up + 1;
    }
    need_lo = need_lo < 0 ? 0 : need_lo;
    need_hi = need_hi > n_in ? n_in : need_hi;
    if (need_lo < need_hi && (need_lo < s0 || need_hi > s0 + n_staged))
        return fail(BN_ERR_ARG, "outputs [%lld, %lld) need input frames [%lld, %lld); staged are [%lld, %lld)", (long long)o0, (long long)o1,
                    (long long)need_lo, (long long)need_hi, (long long)s0, (long long)(s0 + n_staged));
    if (need_lo < need_hi && !d_pcm) return fail(BN_ERR_ARG, "null device pointer");
    const size_t lds = bn::ingest_resample_lds_bytes(up, down, taps_per_phase, blk);
    const bool fast_kernel = (up == 1 && (down == 2 || down == 4)) || (up > 1 && up <= 256 && (taps_per_phase == 21 || taps_per_phase == 29 || taps_per_phase == 39));
    if (lds > (fast_kernel ? 64 : 156) * 1024)
        return fail(BN_ERR_UNSUPPORTED, "resampling ratio %d/%d needs %zu bytes of LDS per workgroup (limit %d)", up, down, lds, (fast_kernel ? 64 : 156) * 1024);
    const size_t need = (size_t)((o1 - o0 + blk - 1) / blk);
    if (need > ctx->block_peaks_elems) {  // growing frees the old buffer, which waits for launches still using it
        if (ctx->d_block_peaks) HIP_TRY(hipFree(ctx->d_block_peaks));
        ctx->d_block_peaks = nullptr;
        ctx->block_peaks_elems = 0;
        HIP_TRY(hipMalloc(&ctx->d_block_peaks, need * sizeof(float)));
        ctx->block_peaks_elems = need;
    }
    bn::launch_ingest_resample_span(d_pcm, sample_format, channels, (long)s0, (long)n_staged, (long)n_in, (long)o0, (long)o1, d_taps, up, down,
                                    taps_per_phase, n_pre_remove, d_mono_window, ctx->d_block_peaks, d_peak, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_ingest_chunks(bn_ctx* ctx, const float* d_mono, const float* d_peak, const int64_t* d_chunk_src,
                     const int32_t* d_chunk_valid, const int32_t* d_chunk_window, int n_chunks, int chunk_len,
                     float* d_chunks, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n_chunks < 0 || chunk_len <= 0) return fail(BN_ERR_ARG, "bad chunk geometry n=%d T=%d", n_chunks, chunk_len);
    if (n_chunks == 0) return BN_OK;
    if (!d_mono || !d_peak || !d_chunk_src || !d_chunk_valid || !d_chunk_window || !d_chunks)
        return fail(BN_ERR_ARG, "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    for (int c0 = 0; c0 < n_chunks; c0 += kMaxGridBatch) {
        const int nc = n_chunks - c0 < kMaxGridBatch ? n_chunks - c0 : kMaxGridBatch;
        bn::launch_ingest_chunks(d_mono, d_peak, (const long*)d_chunk_src + c0, d_chunk_valid + c0, d_chunk_window + c0, nc,
                                 chunk_len, d_chunks + (size_t)c0 * chunk_len, s);
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_chunk_peak_normalize(bn_ctx* ctx, const float* d_x, int B, int T, float eps, float* d_y, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (B < 0 || T <= 0) return fail(BN_ERR_ARG, "bad shape B=%d T=%d", B, T);
    if (B == 0) return BN_OK;
    if (!d_x || !d_y) return fail(BN_ERR_ARG, "null device pointer");
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += kMaxGridBatch) {
        const int nb = B - b0 < kMaxGridBatch ? B - b0 : kMaxGridBatch;
        bn::launch_chunk_peaknorm(d_x + (size_t)b0 * T, d_y + (size_t)b0 * T, nb, T, eps, s);
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_pool_scores(bn_ctx* ctx, const float* d_scores, const int64_t* d_file_off, int n_files, int n_classes, int method,
                   float beta, float* d_pooled, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n_files < 0 || n_classes <= 0) return fail(BN_ERR_ARG, "bad pooling geometry files=%d classes=%d", n_files, n_classes);
    if (method < BN_POOL_AVG || method > BN_POOL_LME) return fail(BN_ERR_ARG, "Unsupported pooling method: %d", method);
    if (n_files == 0) return BN_OK;
    if (!d_scores || !d_file_off || !d_pooled) return fail(BN_ERR_ARG, "null device pointer");
    if ((int64_t)n_files * n_classes > 0x7fffffffLL) return fail(BN_ERR_ARG, "files x classes exceeds 2^31");
    bn::launch_pool_scores(d_scores, (const long*)d_file_off, n_files, n_classes, method, beta, d_pooled, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_short_time_energy(bn_ctx* ctx, const float* d_mono, const float* d_peak, const int64_t* d_win_off, const int32_t* d_win_index,
                         const int64_t* d_frame_off, int n_windows, int frame_len, int hop, float* d_ste, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n_windows < 0 || frame_len <= 0 || hop <= 0) return fail(BN_ERR_ARG, "bad energy geometry windows=%d frame_len=%d hop=%d", n_windows, frame_len, hop);
    if (frame_len != 1024 || hop != 512)
        return fail(BN_ERR_UNSUPPORTED, "frame_len=%d hop=%d: only frames of 1024 at hops of 512 are implemented", frame_len, hop);
    if (n_windows == 0) return BN_OK;
    if (n_windows > 65535) return fail(BN_ERR_ARG, "at most 65535 windows per call");
    if (!d_mono || !d_peak || !d_win_off || !d_win_index || !d_frame_off || !d_ste) return fail(BN_ERR_ARG, "null device pointer");
    bn::launch_short_time_energy(d_mono, d_peak, (const long*)d_win_off, d_win_index, (const long*)d_frame_off, n_windows, d_ste, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_activity_counts(bn_ctx* ctx, const float* d_x, int B, int64_t n, const int32_t* d_idx, int m, float k, int32_t* d_active, float* d_stats,
                       void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (B < 0 || n < 1 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad feature matrix %d x %lld", B, (long long)n);
    if (m < 1 || m > 512) return fail(BN_ERR_ARG, "m=%d: the median is taken over 1..512 elements", m);
    if (!(k == k)) return fail(BN_ERR_ARG, "k is not a number");
    if (B == 0) return BN_OK;
    if (!d_x || !d_idx || !d_active) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_x % 4 || (uintptr_t)d_idx % 4) return fail(BN_ERR_ARG, "d_x and d_idx must be 4-byte aligned");
    bn::launch_activity_counts(d_x, B, (long)n, d_idx, m, k, d_active, d_stats, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_rank_orders(bn_ctx* ctx, const float* d_scores, int n_rows, int n_classes, int32_t* d_cols, int32_t* d_flat, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n_rows < 0 || n_classes <= 0) return fail(BN_ERR_ARG, "bad score matrix %d x %d", n_rows, n_classes);
    if (n_rows == 0) return BN_OK;
    if (!d_scores || !d_cols || !d_flat) return fail(BN_ERR_ARG, "null device pointer");
    if ((int64_t)n_rows * n_classes > 0x3fffffffLL) return fail(BN_ERR_ARG, "rows x classes exceeds 2^30");
    const size_t need = bn::rank_orders_workspace(n_rows, n_classes);
    // (grown outside any capture: the call is made once per evaluation, behind the last inference)
    if (int rc = grow_device_buffer(&ctx->d_rank_work, &ctx->rank_work_bytes, need, need + need / 4, (hipStream_t)stream, BN_ERR_DEVICE, "sort")) return rc;
    if (!bn::launch_rank_orders(d_scores, n_rows, n_classes, d_cols, d_flat, ctx->d_rank_work, ctx->rank_work_bytes, (hipStream_t)stream)) {
        (void)hipGetLastError();
        return fail(BN_ERR_DEVICE, "the device sort failed");
    }
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_debug_op_output(bn_model* m, int op_index, int B, void* d_dst, size_t dst_bytes, size_t* bytes_per_chunk,
                       void* stream) {
    if (!m) return fail(BN_ERR_ARG, "null model");
    if (op_index < 0 || op_index >= (int)m->ops.size()) return fail(BN_ERR_ARG, "op_index %d out of range", op_index);
    const int sid = m->ops[op_index].out;
    if (sid < 0) return fail(BN_ERR_ARG, "operator %d writes a caller buffer, not a workspace slot", op_index);
    // valid: the operator ran, or its twin of the other entry path wrote the same slot (plans keep one operator per path for the first stages)
    bool valid = (size_t)op_index < m->out_valid.size() && m->out_valid[op_index];
    if (!valid && (size_t)sid < m->slot_valid.size() && m->slot_valid[sid]) valid = true;
    if (d_dst && !valid)
        return fail(BN_ERR_UNSUPPORTED, "operator %d did not write its output in the last forward call: a fused kernel keeps that map on chip under the "
                                        "current options", op_index);
    const size_t per = m->slots[sid].bytes_per_chunk;
    if (bytes_per_chunk) *bytes_per_chunk = per;
    if (!d_dst) return BN_OK;
    if (B < 0 || B > m->ctx->max_batch || dst_bytes < per * (size_t)B) return fail(BN_ERR_ARG, "destination too small");
    if (int rc = check_device(m->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(d_dst, m->d_slots[sid], per * (size_t)B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BN_OK;
}

int bn_debug_requant(bn_ctx* ctx, const int32_t* d_x, const int32_t* d_mult, const int32_t* d_shift, int n, int mode, int zero_point,
                     int32_t* d_out, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 0 || mode < 0 || mode > 3) return fail(BN_ERR_ARG, "bad n / mode");
    if (n == 0) return BN_OK;
    if (!d_x || !d_mult || !d_shift || !d_out) return fail(BN_ERR_ARG, "null device pointer");
    bn::launch_debug_requant(d_x, d_mult, d_shift, n, mode, zero_point, d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_debug_satpack(bn_ctx* ctx, const int32_t* d_a, const int32_t* d_b, const int32_t* d_s, int n, int mode, uint32_t* d_out, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 0 || mode < 0 || mode > 1) return fail(BN_ERR_ARG, "bad n / mode");
    if (n == 0) return BN_OK;
    if (!d_a || !d_b || !d_s || !d_out) return fail(BN_ERR_ARG, "null device pointer");
    bn::launch_debug_satpack(d_a, d_b, d_s, n, mode, d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_profile_enable(bn_model* m, int enable) {
    if (!m) return fail(BN_ERR_ARG, "null model");
    m->profiling = enable != 0;
    return BN_OK;
}

int bn_profile_only(bn_model* m, int op_index) {
    if (!m) return fail(BN_ERR_ARG, "null model");
    if (op_index < -1 || op_index > (int)m->ops.size() + 2) return fail(BN_ERR_ARG, "op_index %d out of range", op_index);
    m->prof_only = op_index;
    return BN_OK;
}

int bn_profile_collect(bn_model* m, double* total_ms, int64_t* launches, int n) {
    if (!m || !total_ms || !launches) return fail(BN_ERR_ARG, "null argument");
    if (n < (int)m->ops.size() + 1) return fail(BN_ERR_ARG, "need room for n_ops + 1 entries");
    if (int rc = check_device(m->ctx)) return rc;
    for (int i = 0; i < n; ++i) {
        total_ms[i] = 0.0;
        launches[i] = 0;
    }
    for (auto& r : m->ev_used) {
        HIP_TRY(hipEventSynchronize(r.stop));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r.start, r.stop));
        const int slot = r.op < n ? r.op : (int)m->ops.size();  // a caller without room for the exactness-pass entries gets them under the STFT stage
        total_ms[slot] += ms;
        launches[slot] += 1;
        m->ev_free.push_back(r.start);
        m->ev_free.push_back(r.stop);
    }
    m->ev_used.clear();
    return BN_OK;
}

int bn_set_option(const char* name, int value) {
    if (!name) return fail(BN_ERR_ARG, "null option name");
    for (const OptName& e : kOptions)
        if (strcmp(name, e.name) == 0) {
            std::lock_guard<std::mutex> lock(g_opt_mu);
            g_opt_default.*(e.field) = value;
            return BN_OK;
        }
    return fail(BN_ERR_ARG, "unknown option '%s'", name);
}

int bn_ctx_set_option(bn_ctx* ctx, const char* name, int value) {
    if (!ctx || !name) return fail(BN_ERR_ARG, "null argument");
    for (const OptName& e : kOptions)
        if (strcmp(name, e.name) == 0) {
            std::lock_guard<std::mutex> lock(g_opt_mu);
            for (auto& ov : ctx->opt_override)
                if (ov.first == e.field) {
                    ov.second = value;
                    return BN_OK;
                }
            ctx->opt_override.emplace_back(e.field, value);
            return BN_OK;
        }
    return fail(BN_ERR_ARG, "unknown option '%s'", name);
}

int bn_ctx_get_option(bn_ctx* ctx, const char* name, int* value) {
    if (!ctx || !name || !value) return fail(BN_ERR_ARG, "null argument");
    for (const OptName& e : kOptions)
        if (strcmp(name, e.name) == 0) {
            std::lock_guard<std::mutex> lock(g_opt_mu);
            *value = g_opt_default.*(e.field);
            for (const auto& ov : ctx->opt_override)
                if (ov.first == e.field) *value = ov.second;
            return BN_OK;
        }
    return fail(BN_ERR_ARG, "unknown option '%s'", name);
}

int bn_ctx_reset_options(bn_ctx* ctx) {
    if (!ctx) return fail(BN_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(g_opt_mu);
    ctx->opt_override.clear();
    return BN_OK;
}

void* bn_host_alloc_pinned(bn_ctx* ctx, size_t bytes) {
    if (!ctx || bytes == 0) {
        fail(BN_ERR_ARG, "null context or empty allocation");
        return nullptr;
    }
    if (check_device(ctx) != BN_OK) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(BN_ERR_DEVICE, "hipHostMalloc of %zu bytes failed", bytes);
        return nullptr;
    }
    return p;
}

int bn_host_free_pinned(void* p) {
    if (p && hipHostFree(p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(BN_ERR_DEVICE, "hipHostFree failed");
    }
    return BN_OK;
}

int bn_preload_kernels(bn_ctx* ctx) {
    if (!ctx) return fail(BN_ERR_ARG, "null context");
    if (int rc = check_device(ctx)) return rc;
    // The runtime loads a device code object at the first launch of one of its kernels (a few ms each, and every other thread's launches and
    // copies wait meanwhile).  A caller with idle time before its first batch — the evaluate pipeline while the first files are read — asks here.
    bn::preload_ingest(); bn::preload_stft(); bn::preload_stft_exact(); bn::preload_i8_fused(); bn::preload_i8_strip(); bn::preload_i8_tail2();
    bn::preload_i8_tail(); bn::preload_i8(); bn::preload_i8_pw(); bn::preload_f32(); bn::preload_f32_fused(); bn::preload_f32_strip();
    bn::preload_f32_pw(); bn::preload_melspec(); bn::preload_sort(); bn::preload_probe(); bn::preload_probe_sweep(); bn::preload_probe_mlp(); bn::preload_activity(); bn::preload_search(); bn::preload_augment(); bn::preload_kmeans(); bn::preload_silhouette(); bn::preload_density(); bn::preload_tsne(); bn::preload_propagate(); bn::preload_select(); bn::preload_indices(); bn::preload_pca(); bn::preload_bootstrap(); bn::preload_head_i8();
    return BN_OK;
}

int bn_get_option(const char* name, int* value) {
    if (!name || !value) return fail(BN_ERR_ARG, "null argument");
    for (const OptName& e : kOptions)
        if (strcmp(name, e.name) == 0) {
            std::lock_guard<std::mutex> lock(g_opt_mu);
            *value = g_opt_default.*(e.field);
            return BN_OK;
        }
    return fail(BN_ERR_ARG, "unknown option '%s'", name);
}

const char* bn_kernel_names(void) {
    return "ingest_resample_kernel\ningest_decimate_kernel\ningest_peak_kernel\ningest_chunks_kernel\nchunk_peaknorm_kernel\npool_scores_kernel\nstft512_mag_kernel\nspec_normalize_kernel\nmelspec_finish_kernel\nf32_mel_kernel\nf32_melfin_kernel\nf32_mag_kernel\nf32_rawfe_kernel\nf32_stem_kernel\nf32_dw_kernel\n"
           "f32_pw_kernel\nf32_pw_ws_kernel\nf32_dwpw_kernel\nf32_dwpw_wave_kernel\nf32_strip_kernel\nf32_front_strip_kernel\nf32_front2_kernel\nf32_pwdw_kernel\nf32_dw_stream_kernel\nf32_front_kernel\nf32_gap_kernel\nf32_gap_dense_kernel\nf32_gap_dense_emb_kernel\nf32_dense_kernel\nf32_segate_kernel\nf32_scale_kernel\nf32_attnpool_kernel\n"
           "i8_quant_kernel\ni8_mel_kernel\ni8_stem_kernel\ni8_dw_kernel\ni8_pw_kernel\ni8_dwpw_kernel\ni8_mel_mfma_kernel\ni8_strip_kernel\ni8_strip_mf_kernel\ni8_front_strip_kernel\ni8_front_kernel\ni8_tail_kernel\ni8_tail_emb_kernel\ni8_tail2_kernel\ni8_tail2_emb_kernel\ni8_mid2_kernel\ni8_mean_kernel\ni8_fc_kernel\ni8_scale_kernel\ni8_maxnorm_kernel\ni8_rawfe_kernel\ni8_pwdw_kernel\ni8_dw_stream_kernel\ni8_stem_stream_kernel\ni8_segate_kernel\ni8_pw_wave_kernel\ni8_pw_lds_kernel\ni8_attnpool_kernel\n"
           "i8_head_kernel\ni8_head_softmax_kernel\nemb_store_kernel\nprobe_fwd_kernel\nprobe_dw_kernel\nprobe_reduce_kernel\nprobe_update_kernel\nprobe_loss_sum_kernel\nprobe_sweep_snapshot_kernel\nste_kernel\nactivity_count_kernel\nsearch_inv_norms_kernel\nsearch_score_kernel\nsearch_merge_kernel\naugment_kernel\nkmeans_assign_kernel\nkmeans_keys_kernel\nkmeans_offsets_kernel\nkmeans_segments_kernel\nkmeans_partial_kernel\nkmeans_fold_kernel\nkmeans_scale_kernel\nsilhouette_means_kernel\ndensity_nearest_kernel\ntsne_perplexity_kernel\ntsne_repulsion_kernel\ntsne_fold_kernel\ntsne_z_kernel\ntsne_attraction_kernel\ntsne_update_kernel\npropagate_step_kernel\npropagate_delta_kernel\npropagate_decide_kernel\nselect_pass_kernel\nacoustic_indices_kernel\npca_colsum_kernel\npca_colsum_fold_kernel\npca_gram_kernel\npca_gram_fold_kernel\npca_transform_kernel\nbootstrap_table_kernel\nbootstrap_reject_kernel\nbootstrap_prepare_kernel\nbootstrap_resample_kernel\nhead_i8_kernel";
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------------------- search (bn_search.hip)
extern "C" {

int bn_search_inv_norms(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, float* d_inv, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_SEARCH_MAX_D, zero_point)) return rc;
    if (!d_rows || !d_inv) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if (n == 0) return BN_OK;
    bn::launch_search_inv_norms(d_rows, dtype == BN_DTYPE_I8, (long)n, D, zero_point, d_inv, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_search_topk(bn_ctx* ctx, const void* d_db, int dtype, int64_t n, int D, int zero_point, const float* d_db_inv, const void* d_queries,
                   int64_t Q, const float* d_q_inv, int metric, const int32_t* d_db_group, const int32_t* d_q_group, int k, int32_t* d_idx,
                   float* d_score, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_SEARCH_MAX_D, zero_point)) return rc;
    if (k < 1 || k > BN_SEARCH_MAX_K) return fail(BN_ERR_ARG, "k=%d outside 1..%d", k, BN_SEARCH_MAX_K);
    if (Q < 0 || Q > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad query count %lld", (long long)Q);
    if (metric != BN_SEARCH_COSINE && metric != BN_SEARCH_DOT) return fail(BN_ERR_ARG, "unknown metric %d", metric);
    if (!d_db || !d_queries || !d_idx || !d_score) return fail(BN_ERR_ARG, "null device pointer");
    if (metric == BN_SEARCH_COSINE && (!d_db_inv || !d_q_inv)) return fail(BN_ERR_ARG, "the cosine metric needs both inverse-norm arrays");
    if ((d_db_group == nullptr) != (d_q_group == nullptr)) return fail(BN_ERR_ARG, "d_db_group and d_q_group go together");
    if (dtype == BN_DTYPE_F32 && ((uintptr_t)d_db % 4 || (uintptr_t)d_queries % 4)) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if (Q == 0) return BN_OK;
    const bool i8 = dtype == BN_DTYPE_I8;
    hipStream_t s = (hipStream_t)stream;
    bn::SearchGeom g{};
    if (!bn::search_geometry((long)n, D, (int)Q, k, i8, &g)) return fail(BN_ERR_ARG, "D=%d k=%d: no query tile fits the LDS", D, k);
    // queries per launch: whole passes whose partial lists fit the workspace bound
    const size_t per_query = (size_t)g.nwg * k * (sizeof(float) + sizeof(int32_t));
    const int pass_q = 16 * g.nt;
    int64_t group = (int64_t)(BN_SEARCH_WORKSPACE_BYTES / per_query) / pass_q * pass_q;
    if (group < pass_q) group = pass_q;
    if (group > Q) group = Q;
    const size_t need = (size_t)group * per_query;
    if (int rc = grow_device_buffer(&ctx->d_search_work, &ctx->search_work_bytes, need, need, s, BN_ERR_NOMEM, "search")) return rc;
    float* part_score = (float*)ctx->d_search_work;
    int* part_idx = (int*)(part_score + (size_t)group * g.nwg * k);
    const size_t row_bytes = (size_t)D * (i8 ? 1 : 4);
    for (int64_t q0 = 0; q0 < Q; q0 += group) {
        const int nq = (int)std::min<int64_t>(group, Q - q0);
        bn::SearchArgs a{};
        a.db = d_db; a.q = (const char*)d_queries + (size_t)q0 * row_bytes;
        a.db_inv = d_db_inv; a.q_inv = d_q_inv ? d_q_inv + q0 : nullptr;
        a.db_group = d_db_group; a.q_group = d_q_group ? d_q_group + q0 : nullptr;
        a.part_score = part_score; a.part_idx = part_idx;
        a.n = (int)n; a.D = D; a.Q = nq; a.k = k; a.zp = i8 ? zero_point : 0; a.cosine = metric == BN_SEARCH_COSINE;
        a.steps_per_wg = g.steps_per_wg;
        if (!bn::launch_search_scores(a, g, i8, s)) return fail(BN_ERR_DEVICE, "the search kernel's LDS request was refused");
        bn::launch_search_merge(part_score, part_idx, g.nwg, nq, k, d_idx + (size_t)q0 * k, d_score + (size_t)q0 * k, s);
        HIP_TRY(hipGetLastError());
    }
    return BN_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------------------- density (bn_density.hip)
extern "C" {

int bn_density_nearest(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_inv, const float* d_core,
                       const int32_t* d_comp, uint64_t* d_best, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_DENSITY_MAX_D, zero_point)) return rc;
    if (n > BN_DENSITY_MAX_N) return fail(BN_ERR_ARG, "%lld rows: a tree holds at most %d", (long long)n, BN_DENSITY_MAX_N);
    if (!d_rows || !d_inv || !d_core || !d_comp || !d_best) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_inv % 4 || (uintptr_t)d_core % 4 || (uintptr_t)d_comp % 4 || (uintptr_t)d_best % 8)
        return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned, d_best 8-byte aligned");
    if (n == 0) return BN_OK;
    const bool i8 = dtype == BN_DTYPE_I8;
    hipStream_t s = (hipStream_t)stream;
    bn::DensityGeom g{};
    if (!bn::density_geometry((long)n, D, i8, &g)) return fail(BN_ERR_ARG, "D=%d: no tile of rows fits the LDS", D);
    HIP_TRY(hipMemsetAsync(d_best, 0, (size_t)n * sizeof(uint64_t), s));
    bn::DensityArgs a{};
    a.rows = d_rows; a.inv = d_inv; a.core = d_core; a.comp = d_comp; a.best = (unsigned long long*)d_best;
    a.n = (int)n; a.D = D; a.zp = i8 ? zero_point : 0; a.steps_per_wg = g.steps_per_wg;
    if (!bn::launch_density_nearest(a, g, i8, s)) return fail(BN_ERR_DEVICE, "the density kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------------------- k-means (bn_kmeans.hip)
namespace {

int kmeans_shape_check(int dtype, int64_t n, int D, int K, int zero_point) {
    if (int rc = row_matrix_check(dtype, n, D, BN_KMEANS_MAX_D, zero_point)) return rc;
    if (K < 1 || K > BN_KMEANS_MAX_K) return fail(BN_ERR_ARG, "K=%d outside 1..%d", K, BN_KMEANS_MAX_K);
    return BN_OK;
}

}  // namespace

extern "C" {

int bn_kmeans_assign(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_row_inv, const float* d_centroids,
                     const float* d_cent_inv, int K, const int32_t* d_prev_label, int32_t* d_label, float* d_score, int64_t* d_changed, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = kmeans_shape_check(dtype, n, D, K, zero_point)) return rc;
    if (!d_rows || !d_row_inv || !d_centroids || !d_cent_inv || !d_label || !d_score || !d_changed) return fail(BN_ERR_ARG, "null device pointer");
    if (d_prev_label == d_label) return fail(BN_ERR_ARG, "d_prev_label must not be d_label");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_row_inv % 4 || (uintptr_t)d_centroids % 4 || (uintptr_t)d_cent_inv % 4 || (uintptr_t)d_prev_label % 4 || (uintptr_t)d_label % 4 ||
        (uintptr_t)d_score % 4 || (uintptr_t)d_changed % 8)
        return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned, d_changed 8-byte aligned");
    const bool i8 = dtype == BN_DTYPE_I8;
    hipStream_t s = (hipStream_t)stream;
    bn::KmeansGeom g{};
    if (!bn::kmeans_geometry((long)n, D, K, &g)) return fail(BN_ERR_ARG, "D=%d: no centroid tile fits the LDS", D);
    HIP_TRY(hipMemsetAsync(d_changed, 0, sizeof(int64_t), s));
    if (n == 0) return BN_OK;
    bn::KmeansAssignArgs a{};
    a.rows = d_rows; a.row_inv = d_row_inv; a.cent = d_centroids; a.cent_inv = d_cent_inv; a.prev = d_prev_label; a.label = d_label; a.score = d_score;
    a.changed = (unsigned long long*)d_changed;
    a.n = (int)n; a.D = D; a.K = K; a.zp = i8 ? zero_point : 0; a.steps_per_wg = g.steps_per_wg;
    if (!bn::launch_kmeans_assign(a, g, i8, s)) return fail(BN_ERR_DEVICE, "the assignment kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_kmeans_accumulate(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_row_inv, const int32_t* d_label, int K,
                         int accumulate, float* d_sums, int64_t* d_counts, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = kmeans_shape_check(dtype, n, D, K, zero_point)) return rc;
    if (!d_rows || !d_row_inv || !d_label || !d_sums || !d_counts) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_row_inv % 4 || (uintptr_t)d_label % 4 || (uintptr_t)d_sums % 4 || (uintptr_t)d_counts % 8)
        return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned, d_counts 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (!accumulate) {
            HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)K * D * sizeof(float), s));
            HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)K * sizeof(int64_t), s));
        }
        return BN_OK;
    }
    const size_t need = bn::kmeans_accumulate_workspace((long)n, D, K);
    if (int rc = grow_device_buffer(&ctx->d_kmeans_work, &ctx->kmeans_work_bytes, need, need, s, BN_ERR_NOMEM, "k-means")) return rc;
    if (!bn::launch_kmeans_accumulate(d_rows, dtype == BN_DTYPE_I8, (long)n, D, zero_point, d_row_inv, d_label, K, accumulate != 0, d_sums, (long long*)d_counts,
                                      ctx->d_kmeans_work, ctx->kmeans_work_bytes, s))
        return fail(BN_ERR_DEVICE, "the sort of the rows by label failed");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_kmeans_centroids(bn_ctx* ctx, const float* d_sums, const int64_t* d_counts, int K, int D, float* d_centroids, float* d_cent_inv, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = kmeans_shape_check(BN_DTYPE_F32, 0, D, K, 0)) return rc;
    if (!d_sums || !d_counts || !d_centroids || !d_cent_inv) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_sums % 4 || (uintptr_t)d_centroids % 4 || (uintptr_t)d_cent_inv % 4 || (uintptr_t)d_counts % 8)
        return fail(BN_ERR_ARG, "float32 arrays must be 4-byte aligned, d_counts 8-byte aligned");
    bn::launch_kmeans_centroids(d_sums, (const long long*)d_counts, K, D, d_centroids, d_cent_inv, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------- silhouette (bn_silhouette.hip)
extern "C" {

int bn_silhouette_means(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_row_inv, const int32_t* d_label,
                        const float* d_sums, const float* d_weight, int K, float* d_own, float* d_other, int32_t* d_nearest, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = kmeans_shape_check(dtype, n, D, K, zero_point)) return rc;
    if (!d_rows || !d_row_inv || !d_label || !d_sums || !d_weight || !d_own || !d_other || !d_nearest) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_row_inv % 4 || (uintptr_t)d_label % 4 || (uintptr_t)d_sums % 4 || (uintptr_t)d_weight % 4 || (uintptr_t)d_own % 4 ||
        (uintptr_t)d_other % 4 || (uintptr_t)d_nearest % 4)
        return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned");
    const bool i8 = dtype == BN_DTYPE_I8;
    bn::KmeansGeom g{};
    if (!bn::kmeans_geometry((long)n, D, K, &g)) return fail(BN_ERR_ARG, "D=%d: no tile of sums fits the LDS", D);
    if (n == 0) return BN_OK;
    bn::SilhouetteArgs a{};
    a.rows = d_rows; a.row_inv = d_row_inv; a.label = d_label; a.sums = d_sums; a.weight = d_weight; a.own = d_own; a.other = d_other; a.nearest = d_nearest;
    a.n = (int)n; a.D = D; a.K = K; a.zp = i8 ? zero_point : 0; a.steps_per_wg = g.steps_per_wg;
    if (!bn::launch_silhouette_means(a, g, i8, (hipStream_t)stream)) return fail(BN_ERR_DEVICE, "the silhouette kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------ t-SNE (bn_tsne.hip)
extern "C" {

int bn_tsne_perplexity(bn_ctx* ctx, const float* d_score, int64_t n, int k, double perplexity, float* d_p, double* d_beta, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 1 || n > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    if (k < 1 || k > BN_TSNE_MAX_K) return fail(BN_ERR_ARG, "k=%d outside 1..%d", k, BN_TSNE_MAX_K);
    if (!(perplexity >= 1.0) || 3.0 * perplexity > (double)BN_TSNE_MAX_K) return fail(BN_ERR_ARG, "perplexity %g outside 1..%d/3", perplexity, BN_TSNE_MAX_K);
    if (!d_score || !d_p || !d_beta) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_score % 4 || (uintptr_t)d_p % 4 || (uintptr_t)d_beta % 8) return fail(BN_ERR_ARG, "float32 arrays must be 4-byte aligned, d_beta 8-byte aligned");
    bn::launch_tsne_perplexity(d_score, (long)n, k, perplexity, d_p, d_beta, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_tsne_gradient(bn_ctx* ctx, const float* d_y, int64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, float exaggeration,
                     float* d_grad, double* d_z, double* d_kl_rows, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 2 || n > BN_TSNE_MAX_N) return fail(BN_ERR_ARG, "row count %lld outside 2..%d", (long long)n, BN_TSNE_MAX_N);
    if (!std::isfinite(exaggeration)) return fail(BN_ERR_ARG, "the exaggeration is not finite");
    if (!d_y || !d_rowptr || !d_col || !d_val || !d_grad || !d_z) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_y % 8 || (uintptr_t)d_grad % 8 || (uintptr_t)d_rowptr % 8 || (uintptr_t)d_z % 8 || (uintptr_t)d_kl_rows % 8 || (uintptr_t)d_col % 4 ||
        (uintptr_t)d_val % 4)
        return fail(BN_ERR_ARG, "d_y, d_grad, d_rowptr, d_z and d_kl_rows must be 8-byte aligned, d_col and d_val 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t need = bn::tsne_gradient_workspace((long)n);
    if (int rc = grow_device_buffer(&ctx->d_tsne_work, &ctx->tsne_work_bytes, need, need, s, BN_ERR_NOMEM, "t-SNE")) return rc;
    bn::launch_tsne_gradient(d_y, (long)n, (const long long*)d_rowptr, d_col, d_val, exaggeration, d_grad, d_z, d_kl_rows, ctx->d_tsne_work, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_tsne_update(bn_ctx* ctx, float* d_y, const float* d_grad, float* d_update, float* d_gains, int64_t n, float lr, float momentum, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 1 || n > 0x3fffffffLL) return fail(BN_ERR_ARG, "bad row count %lld", (long long)n);
    if (!std::isfinite(lr) || !std::isfinite(momentum)) return fail(BN_ERR_ARG, "learning rate and momentum must be finite");
    if (!d_y || !d_grad || !d_update || !d_gains) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_y % 4 || (uintptr_t)d_grad % 4 || (uintptr_t)d_update % 4 || (uintptr_t)d_gains % 4) return fail(BN_ERR_ARG, "float32 arrays must be 4-byte aligned");
    bn::launch_tsne_update(d_y, d_grad, d_update, d_gains, (long)n, lr, momentum, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------- label spreading (bn_propagate.hip)
extern "C" {

int bn_propagate_step(bn_ctx* ctx, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, const float* d_f, const int32_t* d_seed_label,
                      int64_t n, int C, float alpha, float* d_f_next, double* d_delta, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 1 || n > BN_PROPAGATE_MAX_N) return fail(BN_ERR_ARG, "row count %lld outside 1..%d", (long long)n, BN_PROPAGATE_MAX_N);
    if (C < 1 || C > BN_PROPAGATE_MAX_CLASSES) return fail(BN_ERR_ARG, "C=%d outside 1..%d", C, BN_PROPAGATE_MAX_CLASSES);
    if (!(alpha > 0.0f && alpha < 1.0f)) return fail(BN_ERR_ARG, "alpha %g outside (0, 1)", (double)alpha);
    if (!d_rowptr || !d_col || !d_val || !d_f || !d_seed_label || !d_f_next) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_rowptr % 8 || (uintptr_t)d_delta % 8 || (uintptr_t)d_col % 4 || (uintptr_t)d_val % 4 || (uintptr_t)d_f % 4 || (uintptr_t)d_seed_label % 4 ||
        (uintptr_t)d_f_next % 4)
        return fail(BN_ERR_ARG, "d_rowptr and d_delta must be 8-byte aligned, the other arrays 4-byte aligned");
    const uintptr_t fa = (uintptr_t)d_f, fb = (uintptr_t)d_f_next, bytes = (uintptr_t)n * (uintptr_t)C * sizeof(float);
    if (fa < fb + bytes && fb < fa + bytes) return fail(BN_ERR_ARG, "d_f_next overlaps d_f");
    hipStream_t s = (hipStream_t)stream;
    if (d_delta) {
        const size_t need = bn::propagate_workspace((long)n);
        if (int rc = grow_device_buffer(&ctx->d_propagate_work, &ctx->propagate_work_bytes, need, need, s, BN_ERR_NOMEM, "label spreading")) return rc;
    }
    bn::launch_propagate_step((const long long*)d_rowptr, d_col, d_val, d_f, d_seed_label, (long)n, C, alpha, d_f_next, d_delta, ctx->d_propagate_work, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_propagate_decide(bn_ctx* ctx, const float* d_f, int64_t n, int C, int32_t* d_label, float* d_score, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n < 1 || n > BN_PROPAGATE_MAX_N) return fail(BN_ERR_ARG, "row count %lld outside 1..%d", (long long)n, BN_PROPAGATE_MAX_N);
    if (C < 1 || C > BN_PROPAGATE_MAX_CLASSES) return fail(BN_ERR_ARG, "C=%d outside 1..%d", C, BN_PROPAGATE_MAX_CLASSES);
    if (!d_f || !d_label || !d_score) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_f % 4 || (uintptr_t)d_label % 4 || (uintptr_t)d_score % 4) return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned");
    bn::launch_propagate_decide(d_f, (long)n, C, d_label, d_score, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- farthest-first traversal (bn_select.hip)
extern "C" {

int bn_select_run(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_inv, const float* d_weight, float* d_m,
                  int32_t* d_nearest, int32_t* d_picked, int forced, int steps, float* d_key, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_SEARCH_MAX_D, zero_point)) return rc;
    if (steps < 0 || forced < 0 || forced > steps) return fail(BN_ERR_ARG, "forced=%d steps=%d: 0 <= forced <= steps", forced, steps);
    if (!d_rows || !d_inv || !d_m || !d_nearest || !d_picked || !d_key) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_inv % 4 || (uintptr_t)d_weight % 4 || (uintptr_t)d_m % 4 || (uintptr_t)d_nearest % 4 || (uintptr_t)d_picked % 4 || (uintptr_t)d_key % 4)
        return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned");
    if (steps == 0) return BN_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t need = bn::select_workspace();
    if (int rc = grow_device_buffer(&ctx->d_select_work, &ctx->select_work_bytes, need, need, s, BN_ERR_NOMEM, "selection")) return rc;
    bn::launch_select_run(d_rows, dtype == BN_DTYPE_I8, (long)n, D, zero_point, d_inv, d_weight, d_m, d_nearest, d_picked, forced, steps, d_key,
                          ctx->d_select_work, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------------------- acoustic indices (bn_indices.hip)
extern "C" {

int bn_acoustic_indices(bn_ctx* ctx, const float* d_spec, const float* d_minmax, int B, int F, int W, const bn_indices_params* params, float* d_out,
                        float* d_spectral, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (F != BN_INDICES_BINS) return fail(BN_ERR_UNSUPPORTED, "F=%d: only %d bins (n_fft = 512) are implemented", F, BN_INDICES_BINS);
    if (W < BN_INDICES_MIN_W || W > BN_INDICES_MAX_W) return fail(BN_ERR_ARG, "W=%d: %d .. %d frames", W, BN_INDICES_MIN_W, BN_INDICES_MAX_W);
    if (B < 0) return fail(BN_ERR_ARG, "B=%d", B);
    if (!d_spec || !d_minmax || !params || !d_out) return fail(BN_ERR_ARG, "null pointer");
    if ((uintptr_t)d_spec % 4 || (uintptr_t)d_minmax % 4 || (uintptr_t)d_out % 4 || (uintptr_t)d_spectral % 4)
        return fail(BN_ERR_ARG, "float32 arrays must be 4-byte aligned");
    const bn_indices_params& p = *params;
    if (p.anthro_k0 < 0 || p.anthro_k0 > p.anthro_k1 || p.anthro_k1 > F)
        return fail(BN_ERR_ARG, "anthrophony bins [%d, %d): 0 <= k0 <= k1 <= %d", p.anthro_k0, p.anthro_k1, F);
    if (p.bio_k0 < 0 || p.bio_k0 > p.bio_k1 || p.bio_k1 > F) return fail(BN_ERR_ARG, "biophony bins [%d, %d): 0 <= k0 <= k1 <= %d", p.bio_k0, p.bio_k1, F);
    if (p.n_bands < 0 || p.n_bands > BN_INDICES_MAX_BANDS) return fail(BN_ERR_ARG, "n_bands=%d: 0 .. %d", p.n_bands, BN_INDICES_MAX_BANDS);
    for (int i = 0; i <= p.n_bands; ++i)
        if (p.band_edge[i] < 0 || p.band_edge[i] > F || (i > 0 && p.band_edge[i] < p.band_edge[i - 1]))
            return fail(BN_ERR_ARG, "band edge %d is bin %d: edges ascend within 0 .. %d", i, p.band_edge[i], F);
    if (!(p.cover_ratio >= 0.0f) || !std::isfinite(p.cover_ratio) || !(p.df_khz >= 0.0f) || !std::isfinite(p.df_khz))
        return fail(BN_ERR_ARG, "cover_ratio and df_khz must be finite and >= 0");
    if (B == 0) return BN_OK;
    bn::launch_acoustic_indices(d_spec, d_minmax, B, W, p, d_out, d_spectral, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------ principal components (bn_pca.hip)
extern "C" {

int bn_pca_colsum(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, double* d_sum, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_PCA_MAX_D, zero_point)) return rc;
    if (!d_sum || (n > 0 && !d_rows)) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_sum % 8) return fail(BN_ERR_ARG, "d_sum must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)D * sizeof(double), s));
        return BN_OK;
    }
    const size_t need = bn::pca_colsum_workspace((long)n, D);
    if (int rc = grow_device_buffer(&ctx->d_pca_work, &ctx->pca_work_bytes, need, need, s, BN_ERR_NOMEM, "PCA")) return rc;
    bn::launch_pca_colsum(d_rows, dtype == BN_DTYPE_I8, (long)n, D, zero_point, d_sum, ctx->d_pca_work, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_pca_gram(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_mean, double* d_gram, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_PCA_MAX_D, zero_point)) return rc;
    if (!d_gram || (n > 0 && !d_rows)) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_I8 && d_mean) return fail(BN_ERR_ARG, "int8 rows take no mean: the result is the exact integer matrix");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_mean % 4 || (uintptr_t)d_gram % 8) return fail(BN_ERR_ARG, "d_mean must be 4-byte aligned, d_gram 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_gram, 0, (size_t)D * D * sizeof(double), s));
        return BN_OK;
    }
    const size_t need = bn::pca_gram_workspace((long)n, D);
    if (int rc = grow_device_buffer(&ctx->d_pca_work, &ctx->pca_work_bytes, need, need, s, BN_ERR_NOMEM, "PCA")) return rc;
    bn::launch_pca_gram(d_rows, dtype == BN_DTYPE_I8, (long)n, D, zero_point, d_mean, d_gram, ctx->d_pca_work, s);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_pca_transform(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_mean, const float* d_W, int r,
                     float* d_out, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = row_matrix_check(dtype, n, D, BN_PCA_MAX_D, zero_point)) return rc;
    if (r < 1 || r > D) return fail(BN_ERR_ARG, "r=%d outside 1..D=%d", r, D);
    if (!d_W || (n > 0 && (!d_rows || !d_out))) return fail(BN_ERR_ARG, "null device pointer");
    if (dtype == BN_DTYPE_F32 && (uintptr_t)d_rows % 4) return fail(BN_ERR_ARG, "float32 rows must be 4-byte aligned");
    if ((uintptr_t)d_mean % 4 || (uintptr_t)d_W % 4 || (uintptr_t)d_out % 4) return fail(BN_ERR_ARG, "float32 arrays must be 4-byte aligned");
    if (n == 0) return BN_OK;
    const bool i8 = dtype == BN_DTYPE_I8;
    bn::PcaTransformGeom g{};
    if (!bn::pca_transform_geometry((long)n, D, r, &g)) return fail(BN_ERR_ARG, "D=%d: no tile of W fits the LDS", D);
    bn::PcaTransformArgs a{};
    a.rows = d_rows; a.mean = d_mean; a.W = d_W; a.out = d_out;
    a.n = (int)n; a.D = D; a.r = r; a.zp = i8 ? zero_point : 0; a.steps_per_wg = g.steps_per_wg;
    if (!bn::launch_pca_transform(a, g, i8, (hipStream_t)stream)) return fail(BN_ERR_DEVICE, "the transform kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------- augmentation (bn_augment.hip)
extern "C" {

int bn_augment_inputs(bn_ctx* ctx, const float* d_x, int64_t n_rows, int F, int W, const int32_t* d_nsrc, const int32_t* d_src, const float* d_gain,
                      const int32_t* d_fmask, int nf, const int32_t* d_tmask, int nt, int64_t m, float* d_out, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (n_rows < 1 || n_rows > 0x7fffffffLL || m < 0 || m > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad row counts n_rows=%lld m=%lld", (long long)n_rows, (long long)m);
    if (F < 1 || W < 1 || (int64_t)F * W > BN_AUGMENT_MAX_ROW) return fail(BN_ERR_ARG, "bad row shape %d x %d (at most %d elements)", F, W, BN_AUGMENT_MAX_ROW);
    if (nf < 0 || nf > BN_AUGMENT_MAX_MASKS || nt < 0 || nt > BN_AUGMENT_MAX_MASKS)
        return fail(BN_ERR_ARG, "nf=%d nt=%d: at most %d masks per axis", nf, nt, BN_AUGMENT_MAX_MASKS);
    if ((nf > 0) != (d_fmask != nullptr) || (nt > 0) != (d_tmask != nullptr)) return fail(BN_ERR_ARG, "a mask table and its count go together");
    if (!d_x || !d_nsrc || !d_src || !d_gain || !d_out) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_x % 4 || (uintptr_t)d_out % 4 || (uintptr_t)d_nsrc % 4 || (uintptr_t)d_src % 4 || (uintptr_t)d_gain % 4 || (uintptr_t)d_fmask % 4 ||
        (uintptr_t)d_tmask % 4)
        return fail(BN_ERR_ARG, "rows and tables must be 4-byte aligned");
    const size_t E = (size_t)F * W;
    const uintptr_t x0 = (uintptr_t)d_x, x1 = x0 + (size_t)n_rows * E * 4, o0 = (uintptr_t)d_out, o1 = o0 + (size_t)m * E * 4;
    if (o0 < x1 && x0 < o1) return fail(BN_ERR_ARG, "d_out overlaps d_x");
    if (m == 0) return BN_OK;
    bn::launch_augment(d_x, (long)n_rows, W, (int)E, d_nsrc, d_src, d_gain, d_fmask, nf, d_tmask, nt, (long)m, d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------- bootstrap (bn_bootstrap.hip)
namespace {

int bootstrap_rows_check(int n) {
    if (n < 1 || n > BN_BOOTSTRAP_MAX_N) return fail(BN_ERR_ARG, "n=%d outside 1..%d", n, BN_BOOTSTRAP_MAX_N);
    return BN_OK;
}

}  // namespace

extern "C" {

int bn_bootstrap_rejections(bn_ctx* ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo, uint32_t bound, int64_t p_begin,
                            int64_t p_end, int64_t* h_positions, int64_t capacity, int64_t* h_count, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (!h_count || (capacity > 0 && !h_positions)) return fail(BN_ERR_ARG, "null pointer");
    *h_count = 0;
    if (bound < 1) return fail(BN_ERR_ARG, "bound must be 1 .. 2^32 - 1");
    if (p_begin < 0 || p_end < p_begin || p_end - p_begin > (1LL << 40) || p_end > (1LL << 62)) return fail(BN_ERR_ARG, "bad raw range [%lld, %lld)", (long long)p_begin, (long long)p_end);
    if (capacity < 0 || capacity > 0x7fffffffLL) return fail(BN_ERR_ARG, "bad capacity %lld", (long long)capacity);
    if ((0x100000000ULL - bound) % bound == 0 || p_end == p_begin) return BN_OK;   // nothing is ever rejected
    hipStream_t s = (hipStream_t)stream;
    const size_t need = bn::bootstrap_reject_workspace((long)capacity);
    if (int rc = grow_device_buffer(&ctx->d_boot_work, &ctx->boot_work_bytes, need, need, s, BN_ERR_NOMEM, "bootstrap")) return rc;
    const unsigned long long gen[4] = {state_hi, state_lo, inc_hi, inc_lo};
    bn::launch_bootstrap_reject(gen, bound, p_begin, p_end, ctx->d_boot_work, (long)capacity, s);
    HIP_TRY(hipGetLastError());
    unsigned found = 0;
    HIP_TRY(hipMemcpyAsync(&found, (char*)ctx->d_boot_work + 2048, sizeof found, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *h_count = found;
    if ((int64_t)found > capacity) return fail(BN_ERR_NOMEM, "%u rejected positions, the list holds %lld", found, (long long)capacity);
    if (found) {
        HIP_TRY(hipMemcpyAsync(h_positions, (char*)ctx->d_boot_work + 2048 + 256, (size_t)found * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return BN_OK;
}

int bn_bootstrap_counts(bn_ctx* ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo, int n, int B, const int64_t* d_ranges,
                        uint32_t* d_counts, void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = bootstrap_rows_check(n)) return rc;
    if (B < 0) return fail(BN_ERR_ARG, "bad resample count %d", B);
    if (B == 0) return BN_OK;
    if (!d_ranges || !d_counts) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_ranges % 8 || (uintptr_t)d_counts % 4) return fail(BN_ERR_ARG, "d_ranges must be 8-byte aligned, d_counts 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t need = bn::bootstrap_ap_workspace(n, 0);
    if (int rc = grow_device_buffer(&ctx->d_boot_work, &ctx->boot_work_bytes, need, need, s, BN_ERR_NOMEM, "bootstrap")) return rc;
    const unsigned long long gen[4] = {state_hi, state_lo, inc_hi, inc_lo};
    if (!bn::launch_bootstrap_counts(gen, n, B, (const long long*)d_ranges, d_counts, ctx->d_boot_work, s))
        return fail(BN_ERR_DEVICE, "the resample kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

int bn_bootstrap_ap(bn_ctx* ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo, int n, int n_classes, const float* d_scores,
                    const uint8_t* d_truth, const int32_t* d_cols, const int32_t* d_classes, int n_selected, int B, const int64_t* d_ranges, double* d_ap,
                    void* stream) {
    if (int rc = check_device(ctx)) return rc;
    if (int rc = bootstrap_rows_check(n)) return rc;
    if (n_classes < 1 || (int64_t)n * n_classes > 0x3fffffffLL) return fail(BN_ERR_ARG, "bad score matrix %d x %d", n, n_classes);
    if (n_selected < 0 || n_selected > 65535 || B < 0 || (int64_t)n_selected * B > 0x7fffffffLL)
        return fail(BN_ERR_ARG, "bad selection: %d classes x %d resamples", n_selected, B);
    if (n_selected == 0 || B == 0) return BN_OK;
    if (!d_scores || !d_truth || !d_cols || !d_classes || !d_ranges || !d_ap) return fail(BN_ERR_ARG, "null device pointer");
    if ((uintptr_t)d_scores % 4 || (uintptr_t)d_cols % 4 || (uintptr_t)d_classes % 4 || (uintptr_t)d_ranges % 8 || (uintptr_t)d_ap % 8)
        return fail(BN_ERR_ARG, "float32 / int32 arrays must be 4-byte aligned, d_ranges and d_ap 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t need = bn::bootstrap_ap_workspace(n, n_selected);
    if (int rc = grow_device_buffer(&ctx->d_boot_work, &ctx->boot_work_bytes, need, need, s, BN_ERR_NOMEM, "bootstrap")) return rc;
    const unsigned long long gen[4] = {state_hi, state_lo, inc_hi, inc_lo};
    if (!bn::launch_bootstrap_ap(gen, n, n_classes, d_scores, d_truth, d_cols, d_classes, n_selected, B, (const long long*)d_ranges, d_ap, ctx->d_boot_work, s))
        return fail(BN_ERR_DEVICE, "the resample kernel's LDS request was refused");
    HIP_TRY(hipGetLastError());
    return BN_OK;
}

}  // extern "C"
