// bn_kernels.h — host-callable launchers of the gfx950 kernels (internal, not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "bn_blob.h"
#include "bn_chain_plan.h"
#include "../../include/birdnet_hip.h"

namespace bn {

// Run-time switches of the launchers (A/B runs, tests).  The process default is set through the C ABI (bn_set_option; the BN_* environment
// variables of the same names seed it ONCE when the library is loaded — nothing on a launch path reads the environment); a context may
// override single switches for itself (bn_ctx_set_option), so two models in one process can run under different options.  What the launchers
// read is `g_opt`: a per-thread copy that every API entry point refreshes from the default and its context's overrides (bn_api.hip: check_device).
struct Options {
    int f32_strip = 1;         // float32 row-streaming strip kernels (0: tile kernels everywhere)
    int f32_strip_th = 0;      // force the rows per strip (0: the launcher's choice)
    int f32_front_staged = 1;  // LDS-staged form of the float32 front strip kernel
    int i8_pwdw = 0;           // 1: expand 1x1 + depthwise 3x3 of exported inverted-residual graphs as one kernel (i8_pwdw_kernel; bit-identical, but
                               // measured 1.5-1.8 x SLOWER than the two kernels: off by default)
    int f32_pw_ws = 1;         // plain 1x1 convolutions with Cin > 128 through the persistent producer / consumer kernel (bn_f32_pw.hip)
    int f32_tile_slice = 0;    // > 0: cap on the 16-column tiles per workgroup slice of the f32 tile kernel (0: the default cap of 16)
    int f32_pwdw = 2;          // expand 1x1 + depthwise 3x3 of inverted-residual blocks as one kernel (the expanded map stays in LDS); 2: it also
                               // hands the squeeze-excite gate behind it per-row-block channel sums (1: the gate pools the map itself, bit-identical to 0)
    int f32_front2 = 1;        // front block + first residual block as one kernel (the map between them stays in LDS)
    int front_tpw = 0;         // tiles per workgroup of the float32 front tile kernel (0: auto)
    int wave_dwpw = 1;         // wave-autonomous variant of the small float32 fused block
    int i8_strip = 1;          // INT8 strip kernels (0: generic fused block everywhere)
    int i8_strip_th = 0;       // force the rows per wave of the INT8 strip kernels (0: auto)
    int i8_dw_pool = 1;        // the row-streaming depthwise kernel of exported graphs adds up what it stores for the squeeze-excite MEAN behind it
                               // (integer sums, order-free: bit-identical); 0: i8_segate_kernel reads the whole map again
    int i8_pw_lds = 1;         // dense 1x1 convolutions (Cin 192 / 384 / 768) of exported INT8 graphs through i8_pw_lds_kernel (bn_i8_pw.hip): weights of a
                               // slice of output channels resident in LDS, squeeze-excite MUL applied on load (0: tile kernel + i8_scale)
    int i8_pw_forms = 1;       // i8_pw_wave_kernel / i8_dw_stream_kernel pick their requantisation form at compile time where the operator's constants allow
                               // (sign-free one-multiply-add form behind ReLU, branch-free right-shift form elsewhere); 0: the runtime-uniform general code
    int i8_add_tab = 1;        // projections with a residual ADD (i8_pw_wave / i8_pw_lds kernels): the ADD as one lookup in a 64 KB table in LDS
                               // (1024-thread workgroups, one per CU); 0: two 256-entry rescale tables + the output requantisation on the vector ALU
    int i8_tail_fclds = 1;     // the fused tail's head reads the classifier matrix from an LDS copy (0: from memory, 64 dependent loads per thread)
    int i8_tail = 1;           // stage 3-4 + MEAN + FC + head of the INT8 graph as one kernel (0: one launch per block)
    int i8_mid = 1;            // stage 2 of the shipped INT8 graph (a stride-2 block + two residual blocks on a 16 x 32 map) as one kernel with the maps of two
                               // chunks in LDS (i8_mid2_kernel: depthwise stage on the matrix cores); 0: one strip kernel per block
    int i8_tail_mfdw = 1;      // ... with the depthwise stage on the matrix cores (i8_tail2_kernel) where the plan carries its constants; 0: i8_tail_kernel
    int i8_mel_generic = 0;    // run the mel mixer through the generic fused block
    int stft_rowmajor = 0;     // keep the reference spectrogram layout inside bn_infer_audio (default: tile-major)
    int i8_mid_split = 1;      // i8_mid2_kernel with every block's constants resident in LDS (staged once) and barriers over the 4 waves of a chunk slot instead of the
                               // workgroup: its two halves run as independent streams; 0 (or a plan whose resident placement does not fit): parts staged per block
    int i8_satpack = 3;        // shift, clamp and byte packing of a requantisation as v_ashr_pk_i8_i32 where the clamp is the int8 range (bn_requant.h: sat_pack2):
                               // bit 0 = the fused chains (i8_mid2_kernel, i8_tail2_kernel; tail2_satpack_ok decides per plan), bit 1 = the stem rows of i8_front_strip_kernel (front_strip_satpack_ok); 0: med3 + shift + v_perm everywhere
    int i8_strip_mfdw = 1;     // stage1_ds2-shaped blocks (32 -> 32 channels, stride 1, residual ADD): depthwise 3x3 on the matrix cores (i8_strip_mf_kernel); 0: i8_strip_kernel
    int stft_exact = 2;        // INT8 plans from audio: 2 = float32 STFT + float64 pass over the doubtful elements (bit-exact input bytes,
                               // bn_stft_exact.hip; plans / options the guarded kernels do not cover take 1), 1 = every bin as a float64
                               // DFT (same bytes, ~10 x slower), 0 = plain float32 STFT (round 2: ~3e-6 of the input bytes off by one)
    int stft_guard = 0;        // the bound |S' - S| <= eps the exactness pass works with (bn_quant_in.h): 0 = empirical (4 x the largest error seen over 2.2e11
                               // elements), 1 = proven (the worst case over all rounding patterns, derived in docs/exactness.md: ~25 x wider, most chunks
                               // end on the float64 routes), 2 = TEST ONLY: the empirical constants / 1024 and no quantiser slack — too small on purpose, so that the audit has something to find
    int stft_audit = 0;        // 1: the guarded mel mixer also re-evaluates in float64 the elements it did NOT flag but that lie within 4 bounds of a rounding
                               // boundary (the near misses) and counts those whose kept byte is wrong — bn_debug_guard_stats out[5] audited, out[6] violations
    int stft_minint = 1;       // 1: a chunk whose MINIMUM has too many candidates to settle one by one (noise-free tones, chirps, flat spectra: every near-zero bin
                               // is one) keeps the fast path with the minimum ENCLOSED in an interval that widens the band of doubt (docs/exactness.md);
                               // 0: such a chunk is recomputed as a whole float64 spectrogram (rounds 3-4)
    int stft_flagcap = 1022;   // elements in doubt a workgroup of the INT8 mel mixer re-evaluates itself before it hands the chunk over (tests lower it)
    int ingest_blk = 0;        // outputs per workgroup of the resampler (0: auto)
    int ingest_generic = 0;    // generic polyphase kernel instead of the phase-per-thread form
};
extern thread_local Options g_opt;

// A kernel that needs more than the default 64 KB of dynamic LDS has its limit raised with hipFuncSetAttribute — per DEVICE (the attribute
// belongs to the current device's copy of the function; bn_ctx_create takes a device index) and only when the request grows.  false: the
// runtime refused (the caller falls back or reports the launch error).
inline bool ensure_dynamic_lds(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> allowed;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = allowed[{kernel, dev}];
    if (bytes <= have) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    have = bytes;
    return true;
}

// Load-time validation of a packed plan (bn_plan_check.hip): every operator's geometry against the slot and tensor sizes.
bool check_plan(const BlobHeader& h, const std::vector<SlotRec>& slots, const std::vector<TensorRec>& tensors,
                const std::vector<OpRec>& ops, std::string& err);

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share an L2).  Tiles that share input rows
// (3x3 halos, the residual of the same positions) should meet in ONE L2, so the linear tile index is permuted: XCD k walks
// the k-th eighth of the tile range.  A bijection on [0, nb); the tail nb % 8 maps to itself.
__device__ __forceinline__ int xcd_tile(int b, int nb) {
    const int nb8 = nb & ~7;
    return b < nb8 ? (b & 7) * (nb8 >> 3) + (b >> 3) : b;
}

// Read-only tables every STFT launch needs (built once per context, in double, stored f32).
struct StftTables {
    const float* window;    // [16][4] per-lane window base: (-0.25 cos th_j0, -0.25 cos th_j1, 0.25 sin th_j0, 0.25 sin th_j1),
                            //         th_je = 2 pi (2 j + e) / 512; the 1/2 of the real-FFT split is folded into the window
    const float4* tw256;    // [256] (w, w_rot): w = exp(-2 pi i p / 256), w_rot = (-w.y, w.x)
    const float4* tw512;    // [16] per-lane split-pass base: (-sin a_j, -cos a_j, -cos a_j, sin a_j), a_j = 2 pi j / 512
    const double* hann64;   // [512] 0.5 - 0.5 cos(2 pi n / 512): the reference's float64 window (bn_stft_exact.hip)
    const double* cs64;     // [512] cos(2 pi j / 512) with exact symmetries (sin by index shift)
    const double2* cs2;     // [512] (cos, sin)(2 pi j / 512): the same values as pairs
};

// Exactness pass of the INT8 audio path (bn_stft_exact.hip explains the five kernels).
// Record of one (chunk, 16-frame tile) of stft512_mag_kernel<., GUARD> for stft_minmax_exact_kernel, in ints:
//   [0] L bits  [1] U bits  [2] n_max  [3] n_min   (lower end of the tile's largest element, upper end of its smallest, candidate threads counted)
//   [kRecExtra ..) lower end of the tile's smallest element (bits), the thread that gave U
//   [kRecEnt ..)   candidate threads as (thread id, upper (maximum) / lower (minimum) end of what its extreme element can be), the s-th of
//                  the maximum at rec_max_entry(s), of the minimum at rec_min_entry(s): they alternate, so that what is used comes first —
//                  header, extras, three threads of the maximum and two of the minimum are the record's first 64-byte line, which is all
//                  that an ordinary tile writes and stft_minmax_exact_kernel reads of it.  Only min(n, kGuardCand) entries of each kind are
//                  written; the rest of the record holds whatever it held.
// kGuardCand = 62 (round 5; 30 before): a STATIONARY tone has every frame's peak within the bound of every other's — 16 frames x 2-4 threads of a
// tile are candidates of the maximum, and an overflowing record gave such chunks to the float64 STFT as a whole.
constexpr int kGuardCand = 62;
constexpr int kRecExtra = 4, kRecEnt = 6;
constexpr int rec_max_entry(int s) { return kRecEnt + 4 * s; }
constexpr int rec_min_entry(int s) { return kRecEnt + 4 * s + 2; }
constexpr int kGuardRec = 256;   // pitch between records, in ints
static_assert(rec_min_entry(kGuardCand - 1) + 2 <= kGuardRec && kRecEnt % 2 == 0, "a record holds kGuardCand entries of each kind, each 8-byte aligned");
constexpr int kGuardBudget = 48;    // candidates of the MINIMUM stft_minmax_exact_kernel settles one by one (half of it) before it encloses the minimum in an interval
constexpr int kGuardMaxBudget = 1024;   // float64 re-evaluations it spends on a chunk's MAXIMUM before it gives the chunk up (a wave per chunk: ~1.3 us per four)
struct StftGuard {
    float* eps;    // [B][W] per-frame bound on |S' - S|
    int* rec;      // [B][ceil(W / 16)][kGuardRec]
    float* mn_lo;  // [B] >= 0: stft_minmax_exact_kernel could only ENCLOSE the chunk's minimum (flat / noise-free spectra: too many candidates) —
                   // minmax[2 b] is an upper end, this the lower end; -1: minmax[2 b] is the exact minimum
    int* count;    // [B] elements found in doubt; > cap: a workgroup of the mixer gave up on the chunk
    int cap;
    int* dirty;    // [B] bit per 64-frame block whose quantised bytes changed
    int* work;     // [B * ceil(W / 64)] dirty (chunk, block) pairs
    int* n_work;   // [1]
    int* hard;     // [2][hard_cap] chunks recomputed as whole float64 spectrograms: behind the min / max pass, behind the fix pass
    int* n_hard;   // [2]
    int hard_cap;
    const float* audio;  // [B][T] the chunks' samples, their geometry and the float64 tables: the mel mixer re-evaluates the elements it finds
    int T, hop;          // in doubt itself (set per call by bn_infer_audio)
    StftTables tabs;
    float k_l2, k_peak;  // the frame part of the bound: eps_f = k_l2 ||x_t||_2 + k_peak max_k S'_tk (option stft_guard picks the constants)
    int* audit;          // [2] elements audited, violations (option stft_audit; null: no audit)
    float audit_scale;   // the audit's band = kAuditBands x (audit_scale eps + slack): 1, or what the test mode divided the constants by
    float slack_scale;   // 1; 0 in the test mode (stft_guard = 2), which drops the quantiser's own slack as well so that real errors escape the band
    int min_interval;    // option stft_minint: enclose the minimum instead of giving the chunk up (0: round-4 behaviour)
    int flag_cap;        // elements in doubt a workgroup of the mel mixer keeps (<= its LDS list; option stft_flagcap: tests lower it to reach the give-up path)
};

// ---- STFT ------------------------------------------------------------------------------
void launch_minmax_init(float* minmax, int B, hipStream_t s);
// tile_major: spectrogram written as [W/16][257][16] instead of [257][W] (needs W % 16 == 0; private layout of bn_infer_audio)
void launch_stft512(const StftTables& tb, const float* audio, int B, int T, int hop, int W, float* spec,
                    float* minmax, hipStream_t s, bool tile_major = false, const StftGuard* guard = nullptr);
// every bin as a float64 DFT, |.| by numpy's formula: the reference's values (bn_stft_exact.hip); minmax as launch_stft512
void launch_stft512_f64(const StftTables& tb, const float* audio, int B, int T, int hop, int W, float* spec, float* minmax, hipStream_t s,
                        bool tile_major = false);
void launch_spec_bytes(const float* spec, const float* minmax, int B, int W, bool tile_major, float qscale, int qzp, int8_t* out, hipStream_t s);
void launch_stft_minmax_exact(const StftTables& tb, const float* audio, int B, int T, int hop, int W, float* spec, bool tile_major,
                              const StftGuard& g, float* minmax, hipStream_t s);
void launch_stft_fix(const StftTables& tb, const float* audio, int B, int T, int hop, int W, float* spec, bool tile_major, const StftGuard& g,
                     const float* minmax, float qscale, int qzp, hipStream_t s);
bool launch_stft512_mel(const StftTables& tb, const float* audio, int B, int T, int hop, int W, float* mel_out, int M,
                        const float* wvals, const int* bands, float* minmax, hipStream_t s, int square = 0);
// per-chunk finishing pass of the precomputed-frontend spectrogram modes (bn_melspec.hip)
size_t melspec_finish_lds_bytes(int M, int W, int Wout, int mode, int mag, int n_mfcc);
bool launch_melspec_finish(const float* mel, float* out, const float* dct, int B, int M, int W, int Wout, int mode, int mag,
                           int n_mfcc, double pcen_b, hipStream_t s);
void launch_spec_normalize(float* spec, const float* minmax, int B, int per_chunk, hipStream_t s);

// ---- ingest and pooling (bn_ingest.hip) ---------------------------------------------------
size_t ingest_resample_lds_bytes(int up, int down, int hpp, int blk);
int ingest_resample_block(int up, int down, int hpp);
size_t ingest_partial_elems(int n_files, long max_out, int up, int down, int hpp);
void launch_ingest_resample(const void* pcm, int fmt, int ch, const long* in_off, const long* out_off, int n_files,
                            long max_out, const float* taps, int up, int down, int hpp, int n_pre_remove, float* mono,
                            float* partial, float* peak, hipStream_t s);
// outputs [o0, o1) of one window of n_win frames whose frames [s0, s0 + n_staged) lie at pcm; output n -> mono[n]; peak = max(peak, ...)
void launch_ingest_resample_span(const void* pcm, int fmt, int ch, long s0, long n_staged, long n_win, long o0, long o1, const float* taps,
                                 int up, int down, int hpp, int n_pre_remove, float* mono, float* partial, float* peak, hipStream_t s);
void launch_ingest_chunks(const float* mono, const float* peak, const long* src, const int* valid, const int* file,
                          int n_chunks, int T, float* out, hipStream_t s);
void launch_chunk_peaknorm(const float* x, float* y, int B, int T, float eps, hipStream_t s);
void launch_pool_scores(const float* scores, const long* seg, int F, int C, int method, float beta, float* out,
                        hipStream_t s);

// ---- float32 plan ------------------------------------------------------------------------
void launch_f32_mel(const float* spec, const float* minmax, float* out, float* smax, int B, int F, int W, int M,
                    const float* wvals, const int* bands, const float* magp, int mag, int norm, hipStream_t s);
void launch_f32_melfin(const float* melraw, const float* minmax, float* out, int B, int M, int W, const float* wsum,
                       const float* magp, int mag, int norm, hipStream_t s);
void launch_f32_rawfe(const float* x, float* out, int B, int T, int W, int M, int stride, int pad_left, const float* fb,
                      const float* bias, const float* magp, int mag, hipStream_t s);
void launch_f32_mag(float* x, const float* smax, int B, int M, int W, const float* magp, int mag, hipStream_t s);
void launch_u32_fill(uint32_t* p, uint32_t v, int n, hipStream_t s);
void launch_f32_stem(const float* x, float* y, int B, int H, int W, int Cout, int sh, int sw, int act, int OH, int OW,
                     int pt, int pl, const float* w, const float* bias, hipStream_t s);
// returns true when the row-streaming kernel ran (only it writes gap_part, the per-strip channel sums for a squeeze-excite gate behind the stage)
bool launch_f32_dw(const float* x, float* y, int B, int H, int W, int C, int sh, int sw, int act, int OH, int OW,
                   int pt, int pl, const float* w, const float* bias, float* gap_part, hipStream_t s);
void launch_f32_pw(const float* x, const float* res, const float* gate, float* y, int B, int P, int Cin, int Cout,
                   int act, const float* w, const float* bias, hipStream_t s);
void launch_f32_segate(const float* x, float* gate, int B, int P, int C, int Cr, const float* w1, const float* w2,
                       const float* part /* [B][R][C] partial channel sums instead of x, or null */, int R, hipStream_t s);
void launch_f32_scale(const float* x, const float* gate, float* y, int B, int P, int C, hipStream_t s);
void launch_f32_gap(const float* x, float* y, int B, int P, int C, hipStream_t s);
void launch_f32_dense(const float* x, float* scores, float* logits, int B, int Cin, int Cout, int act, const float* w,
                      const float* bias, hipStream_t s);
void launch_f32_attnpool(const float* x, float* y, int B, int P, int C, const float* score, hipStream_t s);

// Fused depthwise 3x3 -> pointwise 1x1 block (bn_f32_fused.hip); has_dw = 0 gives a plain 1x1 convolution.
struct DwPwArgs {
    const float* x;      // [B][H][W][Cin]
    const float* res;    // [B][OH][OW][Cout] or null
    const float* gate;   // [B][Cin] or null (squeeze-excite gate; only without the depthwise stage)
    float* y;            // [B][OH][OW][Cout]
    const float* dw_w;   // [3][3][Cin]
    const float* dw_b;   // [Cin]
    const float* pw_w;   // fragment order [Cin/16][Cout/16][64][4]
    const float* pw_b;   // [Cout]
    int B, H, W, Cin, Cout, sh, sw, pt, pl, OH, OW, TH, TW, NB, dw_act, pw_act, has_dw;
};
bool f32_dwpw_supported(int Cin, int Cout);
// stem 3x3 (1 -> C channels, stride 1x2) + depthwise 3x3 stride 2 + pointwise C -> N in one kernel (bn_f32_fused.hip)
bool f32_front_supported(int H0, int W0, int C, int N, int OH, int OW);
void launch_f32_front(const float* fe, float* y, int B, int H0, int W0, int C, int N, int OH, int OW, int stem_act,
                      int dw_act, int pw_act, const float* stem_w, const float* stem_b, const float* dw_w, const float* dw_b,
                      const float* pw_w, const float* pw_b, const float* minmax, const float* wsum, const float* magp, int mag,
                      hipStream_t s);
void launch_f32_gap_dense(const float* x, float* scores, float* logits, int B, int P, int Cin, int Cout, int act, const float* w,
                          const float* bias, hipStream_t s, float* emb = nullptr);   // emb: [B][Cin] pooled vectors as well (f32_gap_dense_emb_kernel)
// the embedding of an operator whose output slot holds it ([B][D], unfused plans): an int8 copy, a float32 dequantisation (q - zp) * scale
// or a float32 copy (bn_embed.hip).  src_i8: the slot holds int8 bytes; dst_f32: write float32.  D % 4 == 0; dst 16-byte aligned (float32) / 4-byte (int8).
void launch_emb_store(const void* src, bool src_i8, void* dst, bool dst_f32, int B, int D, float scale, int zp, hipStream_t s);
void launch_f32_dwpw(const DwPwArgs& a, hipStream_t s);
// persistent two-role kernel for plain 1x1 convolutions with Cin > 128 (bn_f32_pw.hip); false: not its shape
bool launch_f32_pw_ws(const DwPwArgs& a, hipStream_t s);
// row-streaming strip kernel for the wide early blocks (bn_f32_strip.hip); launch_f32_dwpw picks it when supported
struct F32FrontStripArgs {
    const float* fe;      // [B][H0][W0]: frontend map, or raw mel energies when minmax != null
    float* y;             // [B][OH][OW][32]
    const float* stem_w; const float* stem_b;  // [3][3][16], [16]
    const float* dw_w; const float* dw_b;      // [3][3][16], [16]
    const float* pw_w; const float* pw_b;      // fragment order [1][2][64][4], [32]
    const float* minmax; const float* wsum; const float* magp;  // finalising mode (see f32_front_kernel)
    int B, H0, W0, OH, OW, TH, stem_act, dw_act, pw_act, mag;
};
bool f32_front_strip_supported(int H0, int W0, int C, int N, int OH, int OW);
void launch_f32_front_strip(F32FrontStripArgs a, hipStream_t s);
// stand-alone depthwise 3x3 as a row-streaming kernel (bn_f32_strip.hip); false = shape not taken, use launch_f32_dw's own kernel
int f32_dw_stream_strips(int B, int C, int OH, int OW);  // partial sums per chunk and channel that launch_f32_dw_stream writes into gap_part
bool launch_f32_dw_stream(const float* x, float* y, int B, int H, int W, int C, int sh, int sw, int act, int OH, int OW, int pt, int pl,
                          const float* w, const float* bias, float* gap_part /* [B][f32_dw_stream_strips][C] or null */, hipStream_t s);
bool f32_strip_supported(const DwPwArgs& a);
void launch_f32_strip(DwPwArgs a, hipStream_t s);
// front block + the residual block behind it (32 -> 32, stride 1) in one kernel, the map between them in LDS (bn_f32_strip.hip)
bool f32_pwdw_supported(const DwPwArgs& expand, int dH, int dW, int dC, int dsh, int dsw, int dOH, int dOW);
struct F32StemIn {  // a stem convolution (3x3, one input channel) computed inside f32_pwdw_kernel instead of being read from memory
    const float* fe;  // [B][H0][W0]
    const float* w;   // [3][3][C]
    const float* b;   // [C]
    int H0, W0, sh, sw, pt, pl, act;
};
bool launch_f32_pwdw(const DwPwArgs& expand, const float* dw_w, const float* dw_b, float* y, int dsh, int dOH, int dOW, int dpt, int dpl, int dw_act,
                     const F32StemIn* stem, float* gap_part /* [B][ceil(dOH / f32_pwdw_rows(dOH))][hid] or null */, hipStream_t s);
int f32_pwdw_rows(int dOH);
bool f32_front2_supported(const F32FrontStripArgs& f, const DwPwArgs& d);
bool launch_f32_front2(const F32FrontStripArgs& f, const DwPwArgs& d, hipStream_t s);

// ---- INT8 plan -----------------------------------------------------------------------------
void launch_i8_quant(const float* spec, const float* minmax, int8_t* out, int B, int F, int W, int Kp, int zp,
                     int fill, float scale, hipStream_t s);
void launch_i8_mel(const int8_t* x, int8_t* y, int B, int W, int Kp, int M, int zp_out, int amin, int amax,
                   const int8_t* w, const int32_t* bias, const int32_t* mult, const int32_t* shift, const int8_t* lut,
                   hipStream_t s);
struct I8ConvGeom {
    int H, W, C, sh, sw, OH, OW, pt, pl, zp_in, zp_out, amin, amax;
    int rq_right = 0;  // every multiplier >= 0 and every shift < 0 (set at load): the row-streaming kernels take the branch-free requantisation
};
void launch_i8_stem(const int8_t* x, int8_t* y, int B, const I8ConvGeom& g, const int8_t* w, const int32_t* bias,
                    const int32_t* mult, const int32_t* shift, hipStream_t s);
void launch_i8_dw(const int8_t* x, int8_t* y, int B, const I8ConvGeom& g, const int8_t* w, const int32_t* bias,
                  const int32_t* mult, const int32_t* shift, hipStream_t s);
// the same as a row-streaming kernel (bn_i8_strip.hip); false = shape not taken, use launch_i8_dw
bool launch_i8_dw_stream(const int8_t* x, int8_t* y, int B, const I8ConvGeom& g, const int8_t* w, const int32_t* bias, const int32_t* mult,
                         const int32_t* shift, hipStream_t s, int32_t* pool = nullptr);  // pool: [B][C] int32, += the sum of every output byte (zeroed by the caller)
bool launch_i8_stem_stream(const int8_t* x, int8_t* y, int B, const I8ConvGeom& g, const int8_t* w, const int32_t* bias, const int32_t* mult,
                           const int32_t* shift, hipStream_t s);  // the single-channel 3x3 stem in the same form
struct I8AddParams {
    int enabled, z1, m1, s1, m2, s2, mo, so, zo, amin, amax;
};
void launch_i8_pw(const int8_t* x, const int8_t* res, int8_t* y, int B, int P, int Cin, int Cout, int zp_out, int amin,
                  int amax, const I8AddParams& add, const int8_t* w, const int32_t* bias, const int32_t* mult,
                  const int32_t* shift, hipStream_t s);
void launch_i8_mean(const int8_t* x, int8_t* y, int B, int P, int C, int zp_in, int mult, int shift, int zp_out,
                    hipStream_t s);
// w: [Cout][Cin rounded up to a multiple of 4], zero padded; lut: optional int8 table applied to the result (LOGISTIC behind the layer)
void launch_i8_fc(const int8_t* x, int8_t* y, int B, int Cin, int Cout, int zp_out, int amin, int amax, const int8_t* w,
                  const int32_t* bias, const int32_t* mult, const int32_t* shift, const int8_t* lut, hipStream_t s);
// MEAN -> FULLY_CONNECTED -> FULLY_CONNECTED (optional tables behind each) of a squeeze-excite gate as one kernel per chunk (C % 4 == 0)
void launch_i8_segate(const int8_t* x, int8_t* y, int B, int P, int C, int zp_in, int mean_mult, int mean_shift, int mean_zp, int R, int zo1, int amin1,
                      int amax1, const int8_t* w1, const int32_t* b1, const int32_t* m1, const int32_t* s1, const int8_t* lut1, int zo2, int amin2,
                      int amax2, const int8_t* w2, const int32_t* b2, const int32_t* m2, const int32_t* s2, const int8_t* lut2, hipStream_t s, int32_t* sums = nullptr);  // sums: [B][C] channel sums of x already taken (read, then zeroed for the next user); null: the kernel pools x itself
void launch_i8_scale(const int8_t* x, const int8_t* gate, int8_t* y, int B, int P, int C, int zx, int zg, int mult, int shift, int zo,
                     int amin, int amax, hipStream_t s);
// per-chunk max -> denominator byte -> DIV table row [-> per-channel table]: [C][W] int8 -> [C][W] int8 (W a multiple of 4)
void launch_i8_rawfe(const float* x, int8_t* y, int B, int T, int W, int M, int stride, int pad_left, float q_scale, int q_zp, int zp_out, int amin,
                     int amax, const int8_t* w, const int32_t* bias, const int32_t* mult, const int32_t* shift, const int8_t* lut, hipStream_t s);
void launch_i8_maxnorm(const int8_t* x, int8_t* y, int B, int C, int W, const int8_t* den_tab, const int8_t* div_tab, const int8_t* lut, hipStream_t s);
// attention pooling of an exported graph: p = the operator's parameters (P C fc_bias fc_mult fc_shift fc_zo form zx za mul_mult mul_shift mul_zo mul_lo
// mul_hi sum_mult sum_shift sum_zo), w the score vector, table the softmax tables (models/_quant.py: softmax_tables); false = geometry not taken
bool launch_i8_attnpool(const int8_t* x, int8_t* y, int B, const int* p, const int8_t* w, const int32_t* table, hipStream_t s);
void launch_i8_head_softmax(const int8_t* x, float* scores, float* logits, int B, int C, int zp_fc, float s_fc, float beta, hipStream_t s);
void launch_i8_head(const int8_t* x, float* scores, float* logits, int B, int C, int zp_fc, int zp_out, float s_fc,
                    float s_out, const int8_t* lut, hipStream_t s);

// mode 0: sat_pack2(a, b, s); mode 1: sat_pack2_hi on a destination of 0x1234BEEF; out[i] = the whole register
void launch_debug_satpack(const int32_t* a, const int32_t* b, const int32_t* s, int n, int mode, uint32_t* out, hipStream_t st);
void launch_debug_requant(const int32_t* x, const int32_t* mult, const int32_t* shift, int n, int mode, int zp, int32_t* out, hipStream_t s);

// Fused INT8 depthwise 3x3 -> pointwise 1x1 block on the int8 matrix cores (bn_i8_fused.hip).
// has_dw = 0: plain 1x1 convolution; transposed = 1: output [chunk][n][position] with an optional per-channel table
// (the frontend's mel mixer + PWL).
struct DwPw8Args {
    const int8_t* x;
    const int8_t* res;
    int8_t* y;
    const int8_t* dw_w;       // [3][3][Cin]
    const int32_t* dw_b;      // [Cin], holds bias - zp_in * sum of the nine weights
    const int32_t* dw_mult;
    const int32_t* dw_shift;
    const int8_t* pw_w;       // fragment order [Kp/64][Cout/16][64 lanes][16]
    const int32_t* pw_b;      // [Cout], zero point folded
    const int32_t* pw_mult;
    const int32_t* pw_shift;
    const int8_t* lut;        // [Cout][256] or null
    int B, H, W, Cin, Cout, sh, sw, pt, pl, OH, OW, TH, TW, NB, has_dw, transposed;
    int dw_zp_in, dw_zp_out, dw_amin, dw_amax, pw_zp_out, pw_amin, pw_amax;
    I8AddParams add;
    int rq_right;  // every multiplier >= 0 and every shift < 0 in this operator (set at load): branch-free requantisation
    // mel mixer only: QUANTIZE fused into the load — x is unused, the input is the float32 spectrogram [B][qF][W]
    const float* qx;       // null = int8 input in x
    const float* qminmax;  // [B][2] per-chunk min / max for the (S - min) / (max - min + 1e-10) normalisation, or null
    float qscale;
    int qzp, qfill, qF;
    int qtiled;            // the spectrogram is tile-major [W/16][qF][16] (written by launch_stft512(..., tile_major))
    // exactness pass of the audio path (bn_stft_exact.hip): qmode 1 lists the elements whose byte may differ from the reference's,
    // qmode 2 runs only the (chunk, 64-frame block) pairs of qguard.work
    int qmode;
    StftGuard qguard;
    // plain 1x1 convolution behind a squeeze-excite MUL (i8_pw_wave_kernel only): x is the UNSCALED map, the gate is applied on load
    const int8_t* gate;    // [B][Cin] or null
    int g_zx, g_zg, g_mult, g_shift, g_zo, g_amin, g_amax;
    // plain 1x1 convolution + ADD: the whole ADD as a table [256 residual byte patterns][own value + 128] (packer: add_table) or null
    const int8_t* add_tab;
};
bool i8_dwpw_supported(int Cin, int Cout);
bool i8_pwdw_supported(const DwPw8Args& expand, const I8ConvGeom& dw);
bool launch_i8_pwdw(const DwPw8Args& expand, const I8ConvGeom& dw, const int8_t* dw_w, const int32_t* dw_b, const int32_t* dw_mult, const int32_t* dw_shift,
                    int8_t* y, hipStream_t s);
bool i8_pw_lds_supported(const DwPw8Args& a);   // bn_i8_pw.hip
void launch_i8_pw_lds(const DwPw8Args& a, hipStream_t s);
bool i8_pw_wave_takes(const DwPw8Args& a);  // the wave-level 1x1 convolution kernel (the only one that applies DwPw8Args::gate) runs this operator
bool i8_mel_mfma_supported(const DwPw8Args& a);
// Wave-autonomous strip kernel for the same block at Cin, Cout in {32, 64} (bn_i8_strip.hip); `cst` is the constant block
// the packer prepares (models/_lower_i8.py: strip_constants).  With the ADD the residual must be the block input x.
struct Strip8Args {
    const int8_t* x;
    int8_t* y;
    const int32_t* cst;
    int B, H, W, OH, OW, TH, pt, pl;
    int zp_in, dw_lo, dw_hi;
    int pw_lo, pw_hi, pw_zp_out;  // with the ADD: clamp bounds + 128 (the block's own value is kept as a table index)
    I8AddParams add;
    const int8_t* add_tab;  // [256][256]: (residual byte pattern, own value + 128) -> output of the TFLite ADD (packer: add_table)
};
struct FrontStrip8Args {
    const int8_t* fe;   // [B][H0][W0]
    int8_t* y;          // [B][OH][OW][32]
    const int32_t* cst; // models/_lower_i8.py: front_strip_constants
    int B, H0, W0, OH, OW, TH;
    int zp_fe, st_lo, st_hi, zp_st, dw_lo, dw_hi, pw_lo, pw_hi;
    int satpack;        // the stem rows' shift-saturate-pack form: (st_lo, st_hi) = (-128, 127) and option i8_satpack bit 1 (front_strip_satpack_ok)
};
// the stem's clamp is the int8 range: the saturation of v_ashr_pk_i8_i32 is the clamp
inline bool front_strip_satpack_ok(int st_lo, int st_hi) { return st_lo == -128 && st_hi == 127; }
bool i8_front_strip_supported(int H0, int W0, int C, int N, int OH, int OW);
void launch_i8_front_strip(FrontStrip8Args a, hipStream_t s);
bool i8_strip_supported(int Cin, int Cout, int stride, int OW, bool add);
void launch_i8_strip(Strip8Args a, int Cin, int Cout, int stride, hipStream_t s);
// The back half of the INT8 graph as one kernel with the maps in LDS (bn_i8_tail.hip).  Tail8Args, Tail2Args, the kTail* / kMidG constants and the
// host-side planners that fill the arguments (tail_plan, tail2_plan, ...) are in bn_chain_plan.h, which has no HIP in it.
// The embedding output of the fused tail kernels: the pooled vector the head reads, stored by the kernels' embedding instantiations
// (i8_tail_emb_kernel, i8_tail2_emb_kernel), whose kernel argument is WithEmb<Args> — the scores-only kernels keep their argument layout.
struct EmbOut {
    void* emb;            // [B][C] int8 bytes (f32 = 0; 4-byte aligned) or float32 (q - zp) * scale (f32 = 1; 16-byte aligned)
    int f32, zp;
    float scale;
};
template <class Args>
struct WithEmb {
    Args a;               // (first: the kernel-argument pointer addresses both)
    EmbOut e;
};
bool launch_i8_tail(Tail8Args a, hipStream_t s, const EmbOut* emb = nullptr);   // emb: also store the pooled vectors

// The same back half with the DEPTHWISE stage on the matrix cores too (bn_i8_tail2.hip): 8 waves per workgroup, maps in place.
long tail2_giveups();                     // chunk barriers that gave up waiting (0 in a working build)
bool launch_i8_tail2(Tail2Args a, hipStream_t s, const EmbOut* emb = nullptr);
bool launch_i8_mid2(Tail2Args a, hipStream_t s);

// INT8 stem 3x3 + depthwise 3x3 stride 2 + pointwise in one kernel (bn_i8_fused.hip)
struct I8FrontParams {
    const int8_t* stem_w; const int32_t* stem_b; const int32_t* stem_mult; const int32_t* stem_shift;
    const int8_t* dw_w; const int32_t* dw_b; const int32_t* dw_mult; const int32_t* dw_shift;
    const int8_t* pw_w; const int32_t* pw_b; const int32_t* pw_mult; const int32_t* pw_shift;
    int H0, W0, C, N, OH, OW;
    int stem_zp_in, stem_zp_out, stem_amin, stem_amax, dw_zp_out, dw_amin, dw_amax, pw_zp_out, pw_amin, pw_amax;
    int rq_right;
};
bool i8_front_supported(int H0, int W0, int C, int N, int OH, int OW);
void launch_i8_front(const I8FrontParams& q, const int8_t* fe, int8_t* y, int B, hipStream_t s);
void launch_i8_dwpw(const DwPw8Args& a, hipStream_t s);

// One per source file with kernels: load that file's device code object now (bn_preload_kernels)
void preload_f32(); void preload_f32_fused(); void preload_f32_pw(); void preload_f32_strip(); void preload_i8(); void preload_i8_fused();
void preload_i8_pw(); void preload_i8_strip(); void preload_i8_tail(); void preload_i8_tail2(); void preload_ingest(); void preload_melspec();
void preload_stft(); void preload_stft_exact(); void preload_sort(); void preload_probe(); void preload_probe_sweep(); void preload_activity(); void preload_search(); void preload_augment(); void preload_kmeans(); void preload_silhouette(); void preload_density(); void preload_tsne(); void preload_propagate(); void preload_select(); void preload_indices(); void preload_pca(); void preload_bootstrap(); void preload_head_i8();

// bn_probe.hip: a classifier head on embeddings (bn_head_forward) and its training step (bn_probe_*)
struct ProbeFwdArgs {
    const float* X;        // [*, D] embedding rows
    const float* Y;        // [*, C] targets (modes 0 and 1)
    const int* idx;        // [n] row of X / Y behind batch row i, or null: row i itself
    const float* W;        // [D, C]
    const float* b;        // [C]
    float* out;            // mode 0: G [n, C] = dLoss/dlogits, mode 2: scores [n, C]
    float* loss_part;      // [ceil(n / 16)] modes 0 and 1
    long n;
    int D, C, softmax;
    uint32_t drop_thresh;  // keep iff draw >= drop_thresh (0: no dropout)
    float drop_scale;      // 1 / (1 - p)
    uint32_t seed, step;
    float g_scale;         // 1 / (n C) (sigmoid) or 1 / n (softmax)
    // what a long-tailed training set needs (bn_probe_step.h); shared by all trials of a sweep.  All three off (null, CE, any gamma)
    // launches the instantiation without them: today's statements, no multiplication by a loaded 1.0
    const float* row_weight;   // [rows of X] one weight per row, indexed through idx like Y; mode 0 only; null: off
    int loss_kind;             // BN_PROBE_LOSS_CE or BN_PROBE_LOSS_FOCAL (sigmoid only); modes 0 and 1
    float focal_gamma;
};
struct ProbeDwArgs {
    const float* X; const int* idx; const float* G;
    float* partial;        // [row groups][(D + 1) * C]
    float* ss_part;        // [tiles] sums of squares (written with one row group only)
    int B, D, C, E, rows_per_group;
    uint32_t drop_thresh; float drop_scale; uint32_t seed, step;
};
struct ProbeUpdateArgs {
    float* params; float* m; float* v; const float* grad;   // [(D + 1) * C] each, the bias is row D
    const float* ss_part; int n_ss;
    const float* loss_part; int n_loss; float loss_scale; float* step_loss;
    int E, optimizer;      // BN_PROBE_OPT_* (include/birdnet_hip.h)
    float lr, alpha, weight_decay, clip;
};
bool launch_probe_fwd(const ProbeFwdArgs& a, int mode, hipStream_t s);   // false: the runtime refused the LDS request
void launch_probe_dw(const ProbeDwArgs& a, int row_groups, hipStream_t s);
void launch_probe_reduce(float* partial, int E, int groups, float* ss_part, hipStream_t s);
void launch_probe_update(const ProbeUpdateArgs& a, hipStream_t s);
void launch_probe_loss_sum(const float* part, long n, float scale, float* out, hipStream_t s);
// Quantisation-aware fine-tuning of one head (bn_probe_set_qat).  The logits on the exported logit tensor's grid: the
// forward kernel's EXT = 2 instantiations, which take this where a sweep's take ProbeSweepArgs (a sweep has no QAT).
struct ProbeQatArgs {
    float s_out, z_out;    // the logit tensor's scale and its zero point as a float (an integer in -128..127)
    int8_t* codes;         // mode 2: [n, C] the clamped codes, or null
};
bool launch_probe_fwd_qat(const ProbeFwdArgs& a, const ProbeQatArgs& q, int mode, hipStream_t s);   // false: the LDS request was refused
// The weights as quantize_weights will write them: Pq [(D + 1) * C] from the shadow parameters P (row D, the bias, copied), through
// amax [C] = max_k |P[k, c]|; per_tensor: one scale from the largest amax
void launch_probe_qat_weights(const float* P, float* Pq, float* amax, int D, int C, bool per_tensor, hipStream_t s);

// bn_probe_mlp.hip: the hidden layer of a head with one (bn_probe_mlp_*, bn_head_mlp_forward).  Its output layer, both
// weight gradients, the reduction and the update are the launches above, on buffers in batch order.
struct ProbeMlpFwdArgs {
    const float* X;        // [*, D] embedding rows
    const int* idx;        // [n] row of X / Y behind batch row i, or null: row i itself
    const float* W1;       // [D, H]
    const float* b1;       // [H]
    float* hd;             // [n, H] relu(drop1(x) W1 + b1) * drop2, in batch order
    // training only: what the output layer's forward reads through idx, copied into batch order next to hd
    const float* Y; float* Yb;                 // [*, C] -> [n, C]
    const float* row_weight; float* wb;        // [*] -> [n], or null: no weights
    long n;
    int D, H, C;
    uint32_t drop_thresh;  // of both masks: keep iff draw >= drop_thresh (0: no dropout)
    float drop_scale;
    uint32_t seed, seed2, step;   // drop1's seed (the linear head's) and drop2's
};
struct ProbeMlpBwdArgs {
    const float* G;        // [B, C] dLoss/dlogits
    const float* W2;       // [H, C]
    const float* hd;       // [B, H]: dA is zero where hd is (the ReLU gate and drop2's mask in one)
    float* dA;             // [B, H]
    int B, H, C;
    float scale2;          // drop2's 1 / (1 - p), 1 without dropout
};
bool launch_probe_mlp_hidden(const ProbeMlpFwdArgs& a, bool train, hipStream_t s);   // false: the runtime refused the LDS request
void launch_probe_mlp_bwd(const ProbeMlpBwdArgs& a, hipStream_t s);
void preload_probe_mlp();

// bn_probe_sweep.hip: T heads trained in lock-step (bn_probe_sweep_*).  The kernels are those of bn_probe.hip with the trial as one more
// grid axis; what differs per trial is read from a table in device memory, and a trial whose byte of `active` is 0 returns at once.
struct ProbeSweepTrial {       // one row of the device table
    int optimizer;             // BN_PROBE_OPT_*
    float weight_decay, clip;
    uint32_t drop_thresh;      // of the shared draw: keep iff draw >= drop_thresh (0: no dropout)
    float drop_scale;
    int smooth;                // label smoothing on: y' = fl(fl(y * smooth_keep) + smooth_add) (bn_probe_step.h)
    float smooth_keep, smooth_add;
};
struct ProbeSweepArgs {
    const ProbeSweepTrial* trials;
    const uint8_t* active;     // [T] or null: every trial
    float* state;              // [T][4][E]: parameters, m, v, best-weights snapshot
    float* G;                  // [T][G_stride]
    float* partial;            // [T][partial_stride]
    float* ss_part;            // [T][ss_stride]
    float* loss_part;          // [T][loss_stride]
    size_t G_stride, partial_stride;
    int ss_stride, loss_stride, T, E;
};
// `f.W`, `f.b`, `f.out`, `f.loss_part`, `f.drop_*` are filled per trial on the device (mode 1: no dropout, no smoothing)
bool launch_probe_sweep_fwd(const ProbeFwdArgs& f, const ProbeSweepArgs& w, int mode, hipStream_t s);
void launch_probe_sweep_dw(const ProbeDwArgs& g, const ProbeSweepArgs& w, int row_groups, hipStream_t s);
void launch_probe_sweep_reduce(const ProbeSweepArgs& w, int groups, hipStream_t s);
// `u.lr` / `u.alpha` of trial t are step_sizes[2 t], [2 t + 1]; its loss goes to u.step_loss[t]
void launch_probe_sweep_update(const ProbeUpdateArgs& u, const ProbeSweepArgs& w, const float* step_sizes, hipStream_t s);
void launch_probe_sweep_loss_sum(const ProbeSweepArgs& w, long n_parts, float scale, float* out, hipStream_t s);
void launch_probe_sweep_snapshot(const ProbeSweepArgs& w, const uint8_t* mask, hipStream_t s);

// bn_activity.hip: the reductions behind chunk selection.  Short-time energy (frames of 1024 at hops of 512) of windows [win_off[w], win_off[w+1])
// of the resampled mono buffer, divided by peak[win_index[w]] first, written to ste[frame_off[w] ...]; and per row of x [B][n] the median / MAD /
// threshold over |x[idx[0..m)]| (m <= 512) with the number of elements above the threshold (stats [B][3] may be null).
void launch_short_time_energy(const float* mono, const float* peak, const long* win_off, const int* win_index, const long* frame_off, int n_windows,
                              float* ste, hipStream_t s);
void launch_activity_counts(const float* x, int B, long n, const int* idx, int m, float k, int* active, float* stats, hipStream_t s);

// bn_sort.hip: descending orders of the score matrix for the ranking metrics (per class [C][N] row indices, flattened [N*C] flat indices)
size_t rank_orders_workspace(int N, int C);
bool launch_rank_orders(const float* d_scores, int N, int C, int* d_cols, int* d_flat, void* d_work, size_t work_bytes, hipStream_t s);

// bn_search.hip: the k best rows per query by cosine or dot score (bn_search_*)
struct SearchArgs {
    const void* db;          // [n, D] float32 or int8 rows
    const void* q;           // [Q, D] queries of the same type
    const float* db_inv;     // [n] inverse norms (cosine)
    const float* q_inv;      // [Q]
    const int* db_group;     // [n] or null
    const int* q_group;      // [Q] (with db_group)
    float* part_score;       // [Q][workgroups][k] partial lists
    int* part_idx;
    int n, D, Q, k, zp, cosine;
    long steps_per_wg;       // steps of BN_SEARCH_STEP_ROWS rows a workgroup streams
};
struct SearchGeom {
    int nt;                  // query tiles of 16 per pass
    int nwg;                 // workgroups along the rows
    long steps_per_wg;
    size_t lds;
};
bool search_geometry(long n, int D, int Q, int k, bool i8, SearchGeom* g);   // from the shapes only; false: no tile fits the LDS
void launch_search_inv_norms(const void* rows, bool i8, long n, int D, int zp, float* inv, hipStream_t s);
bool launch_search_scores(const SearchArgs& a, const SearchGeom& g, bool i8, hipStream_t s);   // false: the runtime refused the LDS request
void launch_search_merge(const float* part_score, const int* part_idx, int nwg, int Q, int k, int* out_idx, float* out_score, hipStream_t s);

// bn_head_i8.hip: the exported INT8 classifier head over int8 embedding rows (bn_head_i8_forward)
struct HeadI8Args {
    const int8_t* rows;      // [n, D] embedding bytes
    const int8_t* w;         // [C, D rounded up to 64] weights, zero beyond D
    const int32_t* bias;     // [C] with -z_in * sum(w) folded in
    const int32_t* mult;     // [C]
    const int32_t* shift;    // [C]
    const int8_t* lut;       // LOGISTIC table by byte + 128 (sigmoid head), or null
    int8_t* logit;           // [n, C] requantised classifier output, or null
    float* scores;           // [n, C], written when there is a table
    long n;
    int D, C, zp_out;
    int pass_tiles;          // class tiles of 16 a workgroup holds in LDS
    int wide;                // C % 4 == 0 and the outputs aligned for it: a lane's four classes go out as one store each
    long steps_per_wg;       // steps of BN_HEAD_I8_STEP_ROWS rows a workgroup streams
};
struct HeadI8Geom {
    int nt;                  // class tiles multiplied per pass over a step's rows
    int pass_tiles;          // class tiles per LDS pass, a multiple of nt
    int passes;              // second grid axis
    int nwg;                 // workgroups along the rows
    long steps_per_wg;
    size_t lds;
};
bool head_i8_geometry(long n, int D, int C, HeadI8Geom* g);   // from the shapes only; false: no tile fits the LDS
bool launch_head_i8(const HeadI8Args& a, const HeadI8Geom& g, hipStream_t s);   // false: the runtime refused the LDS request

// bn_kmeans.hip: spherical k-means, one Lloyd iteration = an assignment and an update (bn_kmeans_*)
struct KmeansAssignArgs {
    const void* rows;        // [n, D] float32 or int8 rows
    const float* row_inv;    // [n] inverse norms
    const float* cent;       // [K, D] float32 centroids
    const float* cent_inv;   // [K]
    const int* prev;         // [n] labels of the previous assignment, or null
    int* label;              // [n] best centroid, -1 for a zero row
    float* score;            // [n]
    unsigned long long* changed;   // rows whose label differs from prev (every non-zero row without prev), added to
    int n, D, K, zp;
    long steps_per_wg;       // steps of BN_KMEANS_STEP_ROWS rows a workgroup streams
};
struct KmeansGeom {
    int nt;                  // centroid subtiles of 16 per LDS tile
    int tiles;               // LDS tiles the K centroids take
    int nwg;                 // workgroups along the rows
    long steps_per_wg;
    size_t lds;
};
bool kmeans_geometry(long n, int D, int K, KmeansGeom* g);   // from the shapes only; false: no tile fits the LDS
bool launch_kmeans_assign(const KmeansAssignArgs& a, const KmeansGeom& g, bool i8, hipStream_t s);   // false: the runtime refused the LDS request
size_t kmeans_accumulate_workspace(long n, int D, int K);
bool launch_kmeans_accumulate(const void* rows, bool i8, long n, int D, int zp, const float* row_inv, const int* label, int K, int accumulate, float* sums,
                              long long* counts, void* d_work, size_t work_bytes, hipStream_t s);
void launch_kmeans_centroids(const float* sums, const long long* counts, int K, int D, float* cent, float* cent_inv, hipStream_t s);

// bn_silhouette.hip: a labelling's mean cosines, the rows against the K sums of their clusters (bn_silhouette_means)
struct SilhouetteArgs {
    const void* rows;        // [n, D] float32 or int8 rows
    const float* row_inv;    // [n] inverse norms
    const int* label;        // [n] the labelling; outside 0 .. K-1: the row takes no part
    const float* sums;       // [K, D] float32 sums of the normalised members
    const float* weight;     // [K] 1 / members, 0 for an empty cluster
    float* own;              // [n] mean cosine to the row's own cluster
    float* other;            // [n] the highest mean cosine to another non-empty cluster
    int* nearest;            // [n] that cluster, -1 without one
    int n, D, K, zp;
    long steps_per_wg;       // steps of BN_KMEANS_STEP_ROWS rows a workgroup streams
};
bool launch_silhouette_means(const SilhouetteArgs& a, const KmeansGeom& g, bool i8, hipStream_t s);   // g: kmeans_geometry(n, D, K); false: the runtime refused the LDS request

// bn_density.hip: one Borůvka round over the mutual-reachability graph of the rows (bn_density_nearest)
struct DensityArgs {
    const void* rows;        // [n, D] float32 or int8 rows
    const float* inv;        // [n] inverse norms
    const float* core;       // [n] core scores
    const int* comp;         // [n] component of every row, < 0: the row takes no part
    unsigned long long* best;   // [n] keys, zeroed by the launcher's caller; the kernel only raises them
    int n, D, zp;
    long steps_per_wg;       // steps of BN_DENSITY_STEP_ROWS rows a workgroup streams
};
struct DensityGeom {
    int nt;                  // staged subtiles of 16 rows per LDS tile
    int tiles;               // first grid axis: LDS tiles the n rows take
    int nwg;                 // second grid axis: workgroups along the streamed rows
    long steps_per_wg;
    size_t lds;
};
bool density_geometry(long n, int D, bool i8, DensityGeom* g);   // from the shapes only; false: no tile fits the LDS
bool launch_density_nearest(const DensityArgs& a, const DensityGeom& g, bool i8, hipStream_t s);   // false: the runtime refused the LDS request

// bn_tsne.hip: exact t-SNE over a 2-D map — conditional affinities, gradient (all-pairs repulsion, CSR attraction) and update (bn_tsne_*)
void launch_tsne_perplexity(const float* score, long n, int k, double perplexity, float* p, double* beta, hipStream_t s);
size_t tsne_gradient_workspace(long n);
void launch_tsne_gradient(const float* y, long n, const long long* rowptr, const int* col, const float* val, float exaggeration, float* grad, double* z,
                          double* kl_rows, void* d_work, hipStream_t s);
void launch_tsne_update(float* y, const float* grad, float* update, float* gains, long n, float lr, float momentum, hipStream_t s);

// bn_propagate.hip: label spreading over a fixed CSR matrix — one update with its float64 change, and the decision per row (bn_propagate_*)
size_t propagate_workspace(long n);   // the rows' parts of the change
void launch_propagate_step(const long long* rowptr, const int* col, const float* val, const float* f, const int* seed_label, long n, int C, float alpha,
                           float* f_next, double* delta, void* d_work, hipStream_t s);
void launch_propagate_decide(const float* f, long n, int C, int* label, float* score, hipStream_t s);

// bn_select.hip: farthest-first traversal, one launch per pass over the rows (bn_select_run)
struct SelectArgs {
    const void* rows;        // [n, D] float32 or int8 rows
    const float* inv;        // [n] inverse norms
    const float* weight;     // [n] or null: all 1
    float* m;                // [n] the highest score to a row taken so far, +inf for a taken row
    int* nearest;            // [n] the row that gave it
    int* picked;             // [steps]
    float* key;              // [steps]
    const float* part_key_in;   // the previous pass's partials, nprev of them
    const int* part_row_in;
    float* part_key_out;     // this pass's, one per workgroup
    int* part_row_out;
    int n, D, zp, t, pass, nprev;
    long steps_per_wg;       // steps of BN_SELECT_STEP_ROWS rows a workgroup streams
};
size_t select_workspace();   // the two alternating partial buffers
void launch_select_run(const void* rows, bool i8, long n, int D, int zp, const float* inv, const float* weight, float* m, int* nearest, int* picked, int forced,
                       int steps, float* key, void* d_work, hipStream_t s);

// bn_indices.hip: acoustic indices of raw STFT magnitudes, one workgroup per chunk (bn_acoustic_indices)
void launch_acoustic_indices(const float* spec, const float* minmax, int B, int W, const bn_indices_params& prm, float* out, float* spectral,
                             hipStream_t s);

// bn_pca.hip: column sums, scatter matrix and projection of embedding rows (bn_pca_*)
struct PcaColsumGeom {
    int dc;                  // columns a workgroup's lanes cover at a time (a power of two)
    int nwg;                 // row ranges
    long rows_per_wg;
};
struct PcaGramGeom {
    int pairs;               // first grid axis: pairs of macro tiles of the upper triangle
    int ranges;              // second grid axis: row ranges of whole runs
    long rows_per_range;
};
struct PcaTransformArgs {
    const void* rows;        // [n, D] float32 or int8 rows
    const float* mean;       // [D] or null
    const float* W;          // [r, D]
    float* out;              // [n, r]
    int n, D, r, zp;
    long steps_per_wg;       // steps of BN_PCA_STEP_ROWS rows a workgroup streams
};
struct PcaTransformGeom {
    int nt;                  // subtiles of 16 rows of W per LDS tile
    int tiles;               // LDS tiles the r rows of W take
    int nwg;                 // workgroups along the rows
    long steps_per_wg;
    size_t lds;
};
void pca_colsum_geometry(long n, int D, PcaColsumGeom* g);   // from the shapes only
void pca_gram_geometry(long n, int D, PcaGramGeom* g);
bool pca_transform_geometry(long n, int D, int r, PcaTransformGeom* g);   // false: no tile fits the LDS
size_t pca_colsum_workspace(long n, int D);
size_t pca_gram_workspace(long n, int D);
void launch_pca_colsum(const void* rows, bool i8, long n, int D, int zp, double* sum, void* d_work, hipStream_t s);
void launch_pca_gram(const void* rows, bool i8, long n, int D, int zp, const float* mean, double* gram, void* d_work, hipStream_t s);
bool launch_pca_transform(const PcaTransformArgs& a, const PcaTransformGeom& g, bool i8, hipStream_t s);   // false: the runtime refused the LDS request

// bn_bootstrap.hip: numpy's bounded draws reproduced on the device and the average precision of every resample (bn_bootstrap_*);
// gen = (state.hi, state.lo, inc.hi, inc.lo) of the PCG64
size_t bootstrap_reject_workspace(long capacity);
size_t bootstrap_ap_workspace(int n, int n_sel);
void launch_bootstrap_reject(const unsigned long long gen[4], unsigned n, long long p_begin, long long p_end, void* d_work, long capacity, hipStream_t s);
bool launch_bootstrap_counts(const unsigned long long gen[4], int n, int B, const long long* d_ranges, unsigned* d_counts, void* d_work, hipStream_t s);   // false: the runtime refused the LDS request
bool launch_bootstrap_ap(const unsigned long long gen[4], int n, int C, const float* d_scores, const unsigned char* d_truth, const int* d_cols,
                         const int* d_classes, int n_sel, int B, const long long* d_ranges, double* d_ap, void* d_work, hipStream_t s);

// bn_augment.hip: mixup and SpecAugment over resident model-input rows of E = F * W floats (bn_augment_inputs)
void launch_augment(const float* x, long n_rows, int W, int E, const int* nsrc, const int* src, const float* gain, const int* fmask, int nf,
                    const int* tmask, int nt, long m, float* out, hipStream_t s);

}  // namespace bn
