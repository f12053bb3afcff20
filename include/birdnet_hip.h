/*
 * birdnet_hip.h — C ABI of libbirdnet_hip.so: the MI355X (gfx950) implementation of the
 * birdnet-stm32 per-chunk inference hot path
 *
 *     3 s audio chunk -> windowed STFT magnitude -> hybrid mel mixer -> PWL/PCEN
 *                     -> DS-CNN (float32 or bit-faithful INT8) -> class scores.
 *
 * This is the drop-in boundary.  Every entry point names the reference interface it
 * replaces (paths relative to the reference repository birdnet-team/birdnet-stm32):
 *
 *   bn_stft_mag      <- birdnet_stm32/audio/spectrogram.py:24-33,61,106-115,133,149
 *   bn_stft_mag_exact   (the same call site, float64 arithmetic like librosa's)
 *                       get_spectrogram_from_audio(audio, n_fft, mel_bins=-1, spec_width)
 *                       as called per chunk by evaluation/metrics.py:55-61
 *   bn_model_load    <- birdnet_stm32/models/runners.py:98-114 load_model_runner(model_path)
 *                       (tf.lite.Interpreter(...)+allocate_tensors / keras load_model)
 *   bn_forward       <- birdnet_stm32/models/runners.py:29-45 KerasRunner.predict and
 *                       :82-95 TFLiteRunner.predict  (x_batch [B,257,W,1] f32 -> [B,C] f32)
 *   bn_infer_audio   <- the two above back to back, i.e. the body of the chunk loop in
 *                       evaluation/metrics.py:55-61 + :129-141, without the host round trip
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Return value 0 = success, negative = error; bn_last_error() gives the message
 *     (thread-local, valid until the next failing call on that thread).
 *   - Every `d_*` pointer is DEVICE memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()).  The library allocates only its own workspace, at bn_model_load time,
 *     sized for the context's max_batch.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 *     enqueued asynchronously on it; the caller synchronises.
 *   - One bn_ctx per device per host thread; a bn_model is not re-entrant (it owns its
 *     activation workspace), like the reference's TFLite interpreter.
 *   - There is no CPU fallback anywhere: without a gfx950 device every compute entry
 *     point fails with BN_ERR_DEVICE.
 */
#ifndef BIRDNET_HIP_H
#define BIRDNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BN_ABI_VERSION 3

#if defined(__GNUC__)
#define BN_API __attribute__((visibility("default")))
#else
#define BN_API
#endif

/* error codes (negative) */
#define BN_OK 0
#define BN_ERR_ARG (-1)      /* bad argument / shape mismatch */
#define BN_ERR_DEVICE (-2)   /* HIP runtime error, or no usable device */
#define BN_ERR_FORMAT (-3)   /* malformed model blob */
#define BN_ERR_UNSUPPORTED (-4)
#define BN_ERR_NOMEM (-5)

typedef struct bn_ctx bn_ctx;
typedef struct bn_model bn_model;

/* arithmetic type a model computes in */
#define BN_DTYPE_F32 0
#define BN_DTYPE_I8 1

/* what bn_forward's d_input holds */
#define BN_INPUT_SPECTROGRAM 0 /* [B, F, W] float32 linear STFT magnitude (hybrid frontend) */
#define BN_INPUT_WAVEFORM 1    /* [B, T] float32 (raw frontend) */
#define BN_INPUT_MEL 2         /* [B, M, W] float32 precomputed (mel / log-mel / MFCC) spectrogram, passed through */

typedef struct bn_model_info {
    int32_t dtype;          /* BN_DTYPE_* */
    int32_t input_kind;     /* BN_INPUT_* */
    int32_t input_elems;    /* float32 elements per chunk at the runner boundary (F*W or T) */
    int32_t fft_bins;       /* F (hybrid) or 0 */
    int32_t spec_width;     /* W */
    int32_t num_classes;    /* C */
    int32_t n_ops;          /* device-plan operators */
    int32_t max_batch;      /* batch the workspace was sized for */
    int64_t workspace_bytes;
    int64_t const_bytes;    /* weights resident in HBM */
} bn_model_info;

BN_API int bn_version(void);
BN_API const char* bn_last_error(void);

/* Number of HIP devices visible to the process (0 if none). */
BN_API int bn_device_count(void);

/* Create a context on `device`; workspaces of models loaded through it are sized for
 * `max_batch` chunks per call. */
BN_API int bn_ctx_create(int device, int max_batch, bn_ctx** out);
BN_API void bn_ctx_destroy(bn_ctx* ctx);

/* Parse a packed model blob (produced by birdnet_stm32.models._pack from a .keras or
 * .tflite file), copy its constants to HBM and allocate the activation workspace.
 * The blob may be freed by the caller after the call returns. */
BN_API int bn_model_load(bn_ctx* ctx, const void* blob, size_t nbytes, bn_model** out);
/* Validate a packed blob without loading it (host only, needs no device): the checks bn_model_load runs before it allocates —
 * tables and payloads inside the blob, operator references in range, every operator's geometry against the slot and tensor
 * sizes it addresses.  BN_ERR_FORMAT + bn_last_error() on the first violation.  (Reference counterpart: the flatbuffer
 * verification inside tf.lite.Interpreter(model_path=...), birdnet_stm32/models/runners.py:57.) */
BN_API int bn_blob_check(const void* blob, size_t nbytes);
BN_API void bn_model_free(bn_model* model);
BN_API int bn_model_get_info(const bn_model* model, bn_model_info* out);

/* Batched linear-magnitude STFT with the evaluate path's framing (centre zero padding of
 * n_fft/2, periodic Hann, frame t = samples [t*hop - n_fft/2, t*hop + n_fft/2), first W
 * frames kept).
 *   d_audio  [B, T] float32
 *   d_spec   [B, n_fft/2+1, W] float32 (frequency-major, like the reference's ndarray)
 *   d_minmax [B, 2] float32 (per-chunk min, max of the magnitudes) — required
 *   normalize != 0: d_spec <- (S - min) / (max - min + 1e-10) per chunk, in place
 * Only n_fft = 512 is implemented (the reference's firmware FFT has the same limit). */
BN_API int bn_stft_mag(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W,
                int normalize, float* d_spec, float* d_minmax, void* stream);

/* The same spectrogram with the reference's arithmetic, value for value: window product and DFT of every bin in float64, the
 * result rounded to complex64, |.| by numpy's float32 formula (birdnet_stm32/audio/spectrogram.py:106-115: np.abs(librosa.stft(...))),
 * float32 min-max normalisation (:12-21).  About ten times slower than bn_stft_mag (a float32 FFT, within 2e-6 of the peak of
 * these values); bn_infer_audio reaches the same INT8 input bytes at full speed by recomputing only the elements in doubt. */
BN_API int bn_stft_mag_exact(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W,
                      int normalize, float* d_spec, float* d_minmax, void* stream);

/* Forward pass from the runner boundary.
 *   d_input   [B, input_elems] float32 (model_info.input_kind says what it is)
 *   d_minmax  NULL, or [B,2]: treat d_input as UN-normalised magnitudes and apply the
 *             min-max normalisation while loading (saves one pass; same float32 arithmetic)
 *   d_scores  [B, C] float32 class scores (sigmoid/softmax output; dequantised for INT8)
 *   d_logits  NULL or [B, C] float32 pre-activation outputs of the classifier
 */
BN_API int bn_forward(bn_model* model, const float* d_input, const float* d_minmax, int B,
               float* d_scores, float* d_logits, void* stream);

/* audio chunks -> scores: bn_stft_mag (into the model's workspace) + bn_forward. */
BN_API int bn_infer_audio(bn_model* model, const float* d_audio, int B, int T, int hop,
                   float* d_scores, float* d_logits, void* stream);

/* ---- embeddings: the pooled feature vector in front of the classifier head ------------------------------
 * The output of the plan operator whose result feeds the classifier: GAP / int8 MEAN or attention pooling (after the optional
 * embedding convolution), D values per chunk.  Squeeze-excite pools are not embeddings.  The fused kernels store it from where they
 * pool it; requesting it changes no score.  Forms of d_emb ([B, D]; 16-byte aligned for float32, 4-byte for int8):
 *   BN_EMB_F32  float32; INT8 plans: the bytes dequantised as (float)(q - zero_point) * scale (float32 arithmetic)
 *   BN_EMB_I8   the int8 bytes themselves (INT8 plans only: BN_ERR_ARG on a float32 plan)
 * A plan without a marked embedding operator (older blobs) answers BN_ERR_UNSUPPORTED. */
#define BN_EMB_F32 0
#define BN_EMB_I8 1

/* *dim = D, *dtype = BN_EMB_I8 (INT8 plan) or BN_EMB_F32, *scale / *zero_point = the int8 tensor's quantisation (1 / 0 on float32
 * plans).  Any output pointer may be NULL. */
BN_API int bn_model_get_embedding_info(const bn_model* model, int* dim, int* dtype, float* scale, int* zero_point);

/* bn_forward / bn_infer_audio that also write the embedding of every chunk to d_emb (NULL: exactly the call without it) */
BN_API int bn_forward_embed(bn_model* model, const float* d_input, const float* d_minmax, int B, float* d_scores,
               float* d_logits, void* d_emb, int emb_dtype, void* stream);
BN_API int bn_infer_audio_embed(bn_model* model, const float* d_audio, int B, int T, int hop, float* d_scores,
               float* d_logits, void* d_emb, int emb_dtype, void* stream);

/* ---- the steps either side of the path ------------------------- */

/* sample formats of bn_ingest_resample's interleaved PCM (libsndfile's float scaling: /2^15, /2^23, /2^31) */
#define BN_PCM_S16 0
#define BN_PCM_S24 1 /* packed 3-byte little endian */
#define BN_PCM_S32 2
#define BN_PCM_F32 3

/* Decode + mono mix + polyphase resampling + absolute peak of a batch of audio windows that share one
 * (format, channel count, rate pair) — the device form of load_audio_window's arithmetic
 * (reference: birdnet_stm32/audio/io.py:112-124: y.mean(axis=1), fast_resample -> scipy.signal.resample_poly,
 * np.max(np.abs(y))).  Operation order is numpy's / scipy's, so the result is bit-identical to theirs.
 *   d_pcm       interleaved frames of all windows back to back
 *   d_in_off    [n_windows+1] frame offsets of the windows in d_pcm
 *   d_out_off   [n_windows+1] sample offsets of the resampled windows in d_mono;
 *               d_out_off[i+1]-d_out_off[i] = ceil(n_in * up / down)
 *   d_taps      [up][taps_per_phase] polyphase filter, phase-major, the coefficient for the OLDEST input sample
 *               first (scipy upfirdn's transposed, flipped layout of the zero-padded resample_poly filter);
 *               taps_per_phase = 0 with up == down: no resampling (same rate)
 *   n_pre_remove  leading filter-delay outputs resample_poly drops
 *   d_mono      resampled mono float32, NOT yet peak-normalised
 *   d_peak      [n_windows] max |y| per window
 * Channels 1..8.  Window length * up and output length * down must stay below 2^32. */
BN_API int bn_ingest_resample(bn_ctx* ctx, const void* d_pcm, int sample_format, int channels,
                       const int64_t* d_in_off, const int64_t* d_out_off, int n_windows, int64_t max_in_len,
                       int64_t max_out_len, const float* d_taps, int up, int down, int taps_per_phase,
                       int n_pre_remove, float* d_mono, float* d_peak, void* stream);

/* bn_ingest_resample for a SPAN of ONE window: outputs [o0, o1) of a window of n_in frames whose input frames are only partly
 * staged — long recordings are resampled span by span through a staging buffer.  Same kernels, same bits: a window resampled as
 * any sequence of spans equals the window resampled at once (and scipy's resample_poly).  Positions are 64-bit: no length limit
 * below 2^40 frames.
 *   d_pcm          interleaved frames [s0, s0 + n_staged) of the window (frame s0 first)
 *   o0, o1         outputs to compute, 0 <= o0 <= o1 <= ceil(n_in * up / down) (n_in without resampling)
 *   d_mono_window  output sample 0 of the window: output n is written to d_mono_window[n]
 *   d_peak         ONE float, the window's max |y|: the spans' maxima are folded into it with fmax, in stream order — zero it
 *                  before the first span
 * The staged frames must cover every input that outputs [o0, o1) touch (for output n the taps_per_phase frames ending at
 * floor((n + n_pre_remove) * down / up)), clipped to [0, n_in); BN_ERR_ARG names the missing range otherwise.  Frames outside
 * [0, n_in) read as zeros.  The filter arguments are those of bn_ingest_resample. */
BN_API int bn_ingest_resample_span(bn_ctx* ctx, const void* d_pcm, int sample_format, int channels, int64_t s0, int64_t n_staged,
                       int64_t n_in, int64_t o0, int64_t o1, const float* d_taps, int up, int down, int taps_per_phase,
                       int n_pre_remove, float* d_mono_window, float* d_peak, void* stream);

/* Fixed-length chunks of peak-normalised audio (reference: audio/io.py:122-124 `y / peak` when peak > 0, then
 * split_audio_into_chunks :133-174; the host computes the start positions, which depend only on lengths).
 *   d_chunk_src    [n_chunks] absolute sample offset of the chunk's first sample in d_mono
 *   d_chunk_valid  [n_chunks] samples to copy (< chunk_len only for a window shorter than one chunk: right zero pad)
 *   d_chunk_window [n_chunks] index into d_peak
 *   d_chunks       [n_chunks, chunk_len] float32 — the [B, T] input of bn_infer_audio / bn_stft_mag */
BN_API int bn_ingest_chunks(bn_ctx* ctx, const float* d_mono, const float* d_peak, const int64_t* d_chunk_src,
                     const int32_t* d_chunk_valid, const int32_t* d_chunk_window, int n_chunks, int chunk_len,
                     float* d_chunks, void* stream);

/* ---- chunk selection: the two per-sample reductions of the reference's audio/activity.py -----------------------------------
 * Both repeat, operation for operation, the float32 order that birdnet_stm32/audio/activity.py documents (short_time_energy,
 * activity_stats), so their outputs equal that module's bit for bit.  Percentile, regions, ratios and ranking stay on the host.
 *
 * Short-time energy (reference: audio/activity.py:12-30 `_short_time_energy`, called by smart_crop :75-77 with 1024 / 512 for every
 * chunk of at least 4096 samples): for window w = d_mono[d_win_off[w] : d_win_off[w+1]] of the un-normalised buffer bn_ingest_resample
 * wrote, d_ste[d_frame_off[w] + f] = mean((y / peak)[512 f : 512 f + 1024]^2), peak = d_peak[d_win_index[w]] (divided only when
 * peak > 0, as bn_ingest_chunks does).  Only full frames: window w gives min(1 + (len - 1024) / 512, d_frame_off[w+1] - d_frame_off[w])
 * frames, none when len < 1024 -- a window the caller wants skipped gets an empty slice of d_ste.
 *   d_win_off [n_windows + 1] int64, d_win_index [n_windows] int32, d_frame_off [n_windows + 1] int64
 * frame_len / hop other than 1024 / 512 answer BN_ERR_UNSUPPORTED; at most 65535 windows per call. */
BN_API int bn_short_time_energy(bn_ctx* ctx, const float* d_mono, const float* d_peak, const int64_t* d_win_off, const int32_t* d_win_index,
                         const int64_t* d_frame_off, int n_windows, int frame_len, int hop, float* d_ste, void* stream);

/* Activity counts (reference: audio/activity.py:188-209 `get_activity_ratio` up to np.count_nonzero): for every row of d_x [B, n]
 * (finite float32; rows need only 4-byte alignment) sort |x[d_idx[0..m)]| (1 <= m <= 512; the host passes
 * np.linspace(0, n - 1, 512, dtype=int), or the identity with m = n when n <= 512), median = mean of the two middle values, mad = the same of
 * |v - median| plus 1e-10, thresh = median + k * mad (two roundings), and count the row's elements with |x| > thresh.
 *   d_active [B] int32 counts; d_stats [B, 3] float32 (median, mad, thresh), may be NULL.  Indices outside [0, n) are clamped. */
BN_API int bn_activity_counts(bn_ctx* ctx, const float* d_x, int B, int64_t n, const int32_t* d_idx, int m, float k, int32_t* d_active,
                       float* d_stats, void* stream);

/* The sorts behind the ranking metrics (reference: sklearn roc_auc_score / average_precision_score, birdnet_stm32/evaluation/metrics.py:155-190,
 * each of which argsorts on the host): descending, stable orders of the [n_rows, n_classes] float32 score matrix, on the device it lives on.
 *   d_cols [n_classes, n_rows] int32 — for class c the row indices by descending score of column c
 *   d_flat [n_rows * n_classes] int32 — flat indices (row * n_classes + class) by descending score
 * Scores must be finite (the caller checks, as the metrics do).  The workspace lives in the context and grows on demand. */
BN_API int bn_rank_orders(bn_ctx* ctx, const float* d_scores, int n_rows, int n_classes, int32_t* d_cols, int32_t* d_flat, void* stream);

/* Per-chunk peak normalisation y = x / (max|x| + eps) of the raw frontend's model input (reference:
 * birdnet_stm32/evaluation/metrics.py:62-69, with eps = 1e-6): d_x, d_y [B, T] float32 (may alias). */
BN_API int bn_chunk_peak_normalize(bn_ctx* ctx, const float* d_x, int B, int T, float eps, float* d_y, void* stream);

/* pooling methods of bn_pool_scores (reference names: 'avg'|'mean'|'average', 'max', 'lme'|'log_mean_exp'|...) */
#define BN_POOL_AVG 0
#define BN_POOL_MAX 1
#define BN_POOL_LME 2

/* File-level pooling of chunk scores (reference: birdnet_stm32/evaluation/pooling.py:6-47 pool_scores /
 * lme_pooling, called once per file by evaluation/metrics.py:143-146), for all files of a batch at once.
 *   d_scores   [n_rows, n_classes] float32, the rows of one file contiguous
 *   d_file_off [n_files+1] row offsets; an empty file pools to zeros
 *   d_pooled   [n_files, n_classes]
 * mean and max are bit-identical to numpy's float32 result; lme = (m + log(mean(exp(beta s - m)) + 1e-12)) / beta. */
BN_API int bn_pool_scores(bn_ctx* ctx, const float* d_scores, const int64_t* d_file_off, int n_files, int n_classes,
                   int method, float beta, float* d_pooled, void* stream);

/* ---- precomputed frontends ---------------------------------------------- */

/* spectrogram modes / magnitude scalings of get_spectrogram_from_audio (reference: audio/spectrogram.py:24-33) */
#define BN_SPEC_MEL 0    /* mode='mel': magnitude mel spectrogram, then mag_scale, then min-max normalise */
#define BN_SPEC_LOGMEL 1 /* mode='log_mel': log1p(magnitude mel), normalise */
#define BN_SPEC_MFCC 2   /* mode='mfcc': power mel -> dB (ref=max, 80 dB floor) -> orthonormal DCT-II, first n_mfcc rows, normalise */
#define BN_MAG_NONE 0
#define BN_MAG_PWL 1
#define BN_MAG_PCEN 2
#define BN_MAG_DB 3

/* Batched get_spectrogram_from_audio(audio, sample_rate, n_fft=512, mel_bins > 0, spec_width, mag_scale, mode, n_mfcc)
 * (reference: birdnet_stm32/audio/spectrogram.py:61-149, as called per chunk by evaluation/metrics.py:49-54 for the
 * 'librosa' frontend and by the data generator for 'log_mel' / 'mfcc'): hop-framed STFT magnitude (same kernel as
 * bn_stft_mag) mixed by the Slaney mel basis while still in LDS, then one finishing pass per chunk.
 *   d_audio     [B, T] float32
 *   d_mel_w / d_mel_bands   band-sparse mel basis (librosa.filters.mel(sr, 512, n_mels, fmin=150, fmax=sr//2)):
 *               d_mel_bands = int32 [3, n_mels] (first bin, band length, offset into d_mel_w), d_mel_w the
 *               non-zero runs back to back — what birdnet_stm32.models._lower_f32.mel_bands() produces
 *   pcen_b      smoothing coefficient of librosa.pcen for (sample_rate, hop): (sqrt(1+4T^2)-1)/(2T^2), T = 0.4 sr / hop
 *               (only read for mag_scale = BN_MAG_PCEN)
 *   d_dct       [n_mfcc, n_mels] orthonormal DCT-II rows (only for mode = BN_SPEC_MFCC), else NULL
 *   d_work      scratch, B * (n_mels * (1 + T / hop) + 2) floats (mfcc takes its dB reference over all frames, like the
 *               reference, and cuts to W afterwards; the other modes use only the first W frames)
 *   d_out       [B, n_mels, W] (mel, log_mel) or [B, n_mfcc, W] (mfcc), values in [0, 1] */
BN_API int bn_mel_spectrogram(bn_ctx* ctx, const float* d_audio, int B, int T, int n_fft, int hop, int W,
                       const float* d_mel_w, const int32_t* d_mel_bands, int n_mels, int mode, int mag_scale,
                       double pcen_b, const float* d_dct, int n_mfcc, float* d_work, float* d_out, void* stream);

/* Test hook: number of plan operators' outputs and a copy of one of them.
 * `op_index` in [0, n_ops); the element type/shape is what the packer recorded.
 * Valid until the next forward call.  BN_ERR_UNSUPPORTED when the operator's output was not written by that call: a fused kernel
 * kept the map on chip under the current options (front block pairs, expand + depthwise pairs, squeeze-excite gates, the blocks the
 * fused tail covers); bn_set_option switches the fusion off for a per-layer look. */
BN_API int bn_debug_op_output(bn_model* model, int op_index, int B, void* d_dst, size_t dst_bytes,
                       size_t* bytes_per_chunk, void* stream);

/* Test hook: the device's fixed-point requantisation, element-wise on n (accumulator, multiplier, shift) triples — TFLite's
 * MultiplyByQuantizedMultiplier as every INT8 kernel here computes it (csrc/bn_requant.h).  mode 0: the form the generic kernels
 * call; 1: the literal gemmlowp definitions (SaturatingRoundingDoublingHighMul + RoundingDivideByPOT); 2: the branch-free
 * right-shift form (needs multiplier >= 0, shift < 0); 3: the strip kernels' form with rounding offset and zero_point folded into
 * one addend (same preconditions, shift >= -22), zero point subtracted again.  (Reference: the int8 kernels inside
 * tf.lite.Interpreter.invoke, birdnet_stm32/models/runners.py:93.) */
/* Test hook: the int8 bytes the graph's QUANTIZE (op #0) made of the spectrograms of the last bn_infer_audio call on an INT8 plan,
 * d_out [B, 257, W] frequency-major (the production plan never stores them: QUANTIZE is fused into the mel mixer's load).  It is a VIEW:
 * the bytes are recomputed from the spectrogram the call left behind with the graph's exact QUANTIZE chain, not read back from the mixer's
 * tile — tests that check the bytes check the scores (or the pre-sigmoid bytes) as well, which is what the network consumed. */
BN_API int bn_debug_input_bytes(bn_model* model, int B, int8_t* d_out, void* stream);
/* Test hook (synchronises the device): counters of the exactness pass of the last bn_infer_audio call on an INT8 plan (first launch group) —
 * out[0] elements listed as in doubt (sum over the B chunks), out[1] the largest count of one chunk, out[2] (chunk, 64-frame block) pairs
 * whose bytes changed, out[3] / out[4] chunks recomputed as whole float64 spectrograms behind the min / max pass and behind the fix pass,
 * out[5] / out[6] (option stft_audit = 1) elements the audit re-evaluated although the bound did not put them in doubt — the near misses within
 * four bounds of a rounding boundary — and how many of them had a kept byte different from the exact one (violations of the bound: must be 0),
 * out[7] chunks whose minimum the min / max pass enclosed in an interval instead of settling it (option stft_minint; noise-free and flat spectra).
 * `out` holds 8 values. */
BN_API int bn_debug_guard_stats(bn_model* model, int B, int64_t* out);
/* Test hook: which form of the fused INT8 tail operator (BN_OP_I8_TAIL; reference operators #36-#55 of the shipped graph) this model's plan can
 * run — *form = 0 none (per-block operators), 1 = i8_tail_kernel only, 2 = also i8_tail2_kernel (depthwise stage on the matrix cores, the
 * default where available; option i8_tail_mfdw); *lds_bytes = the LDS that form's plan asks for. */
BN_API int bn_debug_tail_form(const bn_model* model, int* form, int* lds_bytes);
/* Test hook: *form = 1 when the plan's fused stage-2 chain (BN_OP_I8_MID: three blocks of the shipped graph as i8_mid2_kernel; option i8_mid)
 * passed the library's LDS plan and runs by default, else 0 (its three strip kernels run instead). */
BN_API int bn_debug_mid_form(const bn_model* model, int* form, int* lds_bytes);
/* Test hook: the RESIDENT LDS placement of the fused stage-2 chain (option i8_mid_split: every block's constants staged once, barriers over the
 * waves of one chunk only).  out[0] = 1 when the model has the chain and the placement fits (what i8_mid2_kernel then runs by default), else 0
 * and nothing more is written; out[1] = LDS bytes, out[2] = bytes of the maps at offset 0, out[3] = offset of the barrier counters (16 bytes),
 * out[4] = blocks; then per block: offset and bytes of its depthwise part, its pointwise part and its zero-point row (bytes 0: none).
 * n >= 5 + 6 * blocks.  bn_debug_mid_split_giveups: *count = chunk barriers whose bounded wait ran out since the library was loaded (waits
 * for the device; 0 in a working build). */
BN_API int bn_debug_mid_plan(const bn_model* model, int* out, int n);
/* Test hook: which requantisation tail the plan's fused INT8 kernels run by default — *mid for i8_mid2_kernel, *tail for i8_tail2_kernel, *front
 * for the stem rows of i8_front_strip_kernel: 1 = shift, clamp and byte packing as one packed shift-and-saturate instruction (every stored
 * clamp of the chain / the stem's clamp is the int8 range; option i8_satpack bit 0 switches the chains' off, bit 1 the stem's), 0 = a narrower
 * clamp keeps the three-instruction form, -1 = the plan does not run that kernel. */
BN_API int bn_debug_satpack_form(const bn_model* model, int* mid, int* tail, int* front);
BN_API int bn_debug_mid_split_giveups(bn_ctx* ctx, int64_t* count);

BN_API int bn_debug_requant(bn_ctx* ctx, const int32_t* d_x, const int32_t* d_mult, const int32_t* d_shift, int n, int mode,
                     int zero_point, int32_t* d_out, void* stream);
/* Test hook: the kernels' packed shift-and-saturate primitives on arrays — d_out[i] = the whole destination register.  mode 0: bytes
 * (sat_i8(a >> s), sat_i8(b >> s)) in the low half, the high half zero; mode 1: the same pair into the high half of a register that held
 * 0x1234BEEF, its low half kept.  s counts with its low five bits. */
BN_API int bn_debug_satpack(bn_ctx* ctx, const int32_t* d_a, const int32_t* d_b, const int32_t* d_s, int n, int mode, uint32_t* d_out, void* stream);

/* Per-operator timing with HIP events recorded on the launch stream.  While enabled, every plan
 * operator of bn_forward / bn_infer_audio is bracketed by an event pair (index n_ops = the STFT
 * stage of bn_infer_audio).  bn_profile_collect waits for the recorded events, adds the elapsed
 * milliseconds and launch counts per operator into total_ms[n] / launches[n] (n >= n_ops + 1)
 * and forgets them.  INT8 plans from audio have two more entries, n_ops + 1 (exact min / max of the spectrogram) and n_ops + 2 (whole-chunk
 * float64 fallback + second run of the mel mixer): with n >= n_ops + 3 they are reported on their own, else under the STFT stage. */
BN_API int bn_profile_enable(bn_model* model, int enable);
/* Restrict the event pairs to ONE operator (op_index in [0, n_ops]; -1 = every operator again).  A pair per operator costs
 * ~6 % of a 1.5 ms step; bracketing only the kernel under study keeps the timed region undisturbed. */
BN_API int bn_profile_only(bn_model* model, int op_index);
BN_API int bn_profile_collect(bn_model* model, double* total_ms, int64_t* launches, int n);

/* Run-time switches of the kernel launchers, for A/B measurements and tests (process-wide; the defaults are the production
 * choices).  Names: "f32_strip", "f32_strip_th", "f32_front_staged", "f32_front2", "f32_pwdw", "f32_tile_slice", "f32_pw_ws", "i8_pwdw", "i8_pw_lds", "i8_pw_forms", "i8_add_tab", "front_tpw", "wave_dwpw", "i8_strip", "i8_strip_mfdw", "i8_strip_th",
 * "i8_dw_pool", "i8_tail_fclds", "i8_tail", "i8_tail_mfdw", "i8_mid", "i8_mid_split", "i8_satpack", "i8_mel_generic", "stft_rowmajor", "stft_exact", "stft_flagcap", "stft_guard", "stft_audit", "stft_minint", "ingest_blk", "ingest_generic" (csrc/bn_kernels.h: Options says
 * what each selects).  An environment variable BN_<NAME IN CAPITALS> seeds the value once when the library is loaded; no
 * launch reads the environment.  The reference has no counterpart (tf.lite.Interpreter's delegates / num_threads arguments,
 * birdnet_stm32/models/runners.py:57, are the closest thing).  Unknown name: BN_ERR_ARG. */
BN_API int bn_set_option(const char* name, int value);
BN_API int bn_get_option(const char* name, int* value);
/* The same switches per context: bn_set_option sets the PROCESS DEFAULT, bn_ctx_set_option overrides one switch for the launches made through
 * this context (and the models loaded into it) only, so two models in one process can run under different options; bn_ctx_get_option reads the
 * effective value, bn_ctx_reset_options drops the context's overrides.  (The reference's counterpart is per-interpreter state: every
 * tf.lite.Interpreter of models/runners.py:57 carries its own settings.) */
BN_API int bn_ctx_set_option(bn_ctx* ctx, const char* name, int value);
BN_API int bn_ctx_get_option(bn_ctx* ctx, const char* name, int* value);
BN_API int bn_ctx_reset_options(bn_ctx* ctx);

/* Page-locked host memory for the staging buffers a caller copies audio from (hipHostMalloc / hipHostFree).  Through a foreign-function binding
 * the call runs WITHOUT the host language's interpreter lock: page-locking 256 MiB takes ~17 ms, and an allocation made through PyTorch's
 * pinned allocator holds the GIL for all of it — the reader thread of the evaluate pipeline stood still meanwhile (tools/_cold_trace.py).
 * NULL on failure (bn_last_error).  (Reference counterpart: none — it hands numpy arrays to tf.lite.Interpreter.set_tensor, runners.py:84.) */
BN_API void* bn_host_alloc_pinned(bn_ctx* ctx, size_t bytes);
BN_API int bn_host_free_pinned(void* p);

/* ---- A classifier head on frozen embeddings: scores = act(dropout(x) W + b) (csrc/bn_probe.hip) --------------------------------
 * (Reference counterpart: birdnet_stm32/training/linear_probe.py — Dropout -> Dense(len(classes)) behind the pooled vector, trained by
 * Keras with the backbone frozen.  Here the backbone has already run: the rows of X are embeddings, bn_forward_embed's output.)
 * All arithmetic is float32; the products run on the f32-input matrix instruction (exact f32).  W is [D, C] row-major, b is [C],
 * 1 <= D <= BN_PROBE_MAX_D, 1 <= C <= BN_PROBE_MAX_C. */
#define BN_PROBE_MAX_D 2048
#define BN_PROBE_MAX_C 4096
#define BN_PROBE_ACT_SIGMOID 0 /* loss: binary cross-entropy, mean over rows x classes (Keras: p clipped to [1e-7, 1 - 1e-7]) */
#define BN_PROBE_ACT_SOFTMAX 1 /* loss: categorical cross-entropy, mean over rows */
#define BN_PROBE_OPT_ADAM 0    /* Keras defaults: beta 0.9 / 0.999, eps 1e-7 added to sqrt(v), bias correction folded into the step size */
#define BN_PROBE_OPT_ADAMW 1   /* ... and w -= lr_t * weight_decay * w in front of the step (weights and bias) */
#define BN_PROBE_OPT_SGD 2     /* momentum 0.9, Keras form: v = 0.9 v - lr_t g; w += v */
/* Bound on the gradient workspace of one bn_probe: the batch is split into row groups whose partial gradients ((D + 1) * C floats each,
 * 32 MiB for the largest head) are added in a fixed order, and the number of groups is chosen from the shapes so that they fit. */
#define BN_PROBE_WORKSPACE_BYTES (256u << 20)

typedef struct bn_probe bn_probe;

/* d_scores[n, C] = act(d_emb[n, D] d_W + d_b): the scores of a head over n embedding rows (the forward tiles of the training step). */
BN_API int bn_head_forward(bn_ctx* ctx, const float* d_emb, int64_t n, int D, const float* d_W, const float* d_b, int C, int activation,
                    float* d_scores, void* stream);

/* The INT8 head of an exported model (conversion/head_export.py; csrc/bn_head_i8.hip) over n rows of int8 embedding bytes, as the
 * FULLY_CONNECTED [-> LOGISTIC] -> DEQUANTIZE [-> SOFTMAX] tail of the .tflite computes it:
 *   q[i, c] = clamp(MultiplyByQuantizedMultiplier(sum_k rows[i, k] * w[c, k] + bias[c], mult[c], shift[c]) + zp_out, -128, 127)
 * d_w [C, Kp] int8 with Kp = D rounded up to a multiple of 64, zero beyond D, 16-byte aligned; d_bias [C] int32 holds the layer's bias
 * minus (embedding zero point) * sum_k w[c, k]; d_mult / d_shift [C] the per-class Q31 multiplier and exponent.  Every accumulator must
 * fit int32 and its requantisation the fast forms' domain (csrc/bn_requant.h); the exporter refuses a head that does not.
 * BN_PROBE_ACT_SIGMOID: d_lut is the 256-entry int8 LOGISTIC table indexed by q + 128 (output scale 1/256, zero point -128) and
 *   d_scores[i, c] = (d_lut[q + 128] + 128) / 256; d_logit_bytes [n, C] receives q when it is not NULL.
 * BN_PROBE_ACT_SOFTMAX: d_lut is NULL, d_logit_bytes is required, and d_scores is the float32 softmax (beta 1) of s_fc * (q - zp_out)
 *   per row, by the kernel that ends a softmax model's plan (launched in slices of 2^24 rows).  s_fc is read for softmax only.
 * 1 <= D <= BN_PROBE_MAX_D, 1 <= C <= BN_PROBE_MAX_C, 0 <= n < 2^31 (n == 0 launches nothing).  Rows go in steps of
 * BN_HEAD_I8_STEP_ROWS, at least BN_HEAD_I8_MIN_WG_STEPS steps per workgroup, at most BN_HEAD_I8_MAX_WGS workgroups per pass over the
 * classes; a pass holds as many class tiles of 16 as fit BN_HEAD_I8_LDS_BYTES.  Rows on a 16-byte boundary with D % 16 == 0 take the wide
 * loads.  Nothing synchronises with the host inside the call. */
#define BN_HEAD_I8_STEP_ROWS 64
#define BN_HEAD_I8_MIN_WG_STEPS 8
#define BN_HEAD_I8_MAX_WGS 1024
#define BN_HEAD_I8_LDS_BYTES (160 * 1024)
BN_API int bn_head_i8_forward(bn_ctx* ctx, const int8_t* d_rows, int64_t n, int D, const int8_t* d_w, const int32_t* d_bias,
                       const int32_t* d_mult, const int32_t* d_shift, int C, int zp_out, const int8_t* d_lut, int activation, float s_fc,
                       int8_t* d_logit_bytes, float* d_scores, void* stream);

/* Classes a workgroup of bn_head_i8_forward holds in LDS per pass (a multiple of 16; more classes take further passes on the second grid
 * axis), from (D, C) alone; negative on bad arguments.  No device is needed. */
BN_API int bn_head_i8_pass_classes(int D, int C);

/* A head in training.  d_W / d_b: the initial values (copied; the optimiser state starts at zero).  Learning rate of global step t
 * (0-based, counted over all bn_probe_epoch calls): lr * 0.5 * (1 + cos(pi * min(t, total_steps) / total_steps)).  clipnorm > 0: the
 * gradient of W and b together is scaled by clipnorm / norm when its norm exceeds clipnorm.  dropout in [0, 1): element (row i of the
 * batch, column j) of step t is kept (and scaled by 1 / (1 - dropout)) iff a 24-bit hash of (seed, t, i, j) is >= ceil(dropout * 2^24)
 * (DESIGN.md 5d gives the function; it is stateless). */
BN_API int bn_probe_create(bn_ctx* ctx, int D, int C, int activation, int optimizer, float lr, float weight_decay, float clipnorm,
                    float dropout, uint32_t seed, int64_t total_steps, const float* d_W, const float* d_b, bn_probe** out, void* stream);
/* Waits for the device to finish (steps still enqueued use the probe's buffers), then frees the probe. */
BN_API void bn_probe_destroy(bn_probe* probe);
/* Enqueues the ceil(n / batch) steps of one epoch: step s trains on rows d_perm[s * batch ...] (int32 row numbers into d_X [*, D] and
 * d_Y [*, C]; the last batch may be short, means are over its real rows) and writes its loss to d_step_loss[s].  Nothing synchronises
 * with the host inside the call; the same inputs give the same bits on every run (no floating-point atomics).  On an error the steps
 * enqueued before it still run and count as taken. */
BN_API int bn_probe_epoch(bn_probe* probe, const float* d_X, const float* d_Y, const int32_t* d_perm, int64_t n, int batch,
                   float* d_step_loss, void* stream);
/* *d_out = the mean loss of the current weights over rows 0 .. n-1 of d_X / d_Y, without dropout (validation). */
BN_API int bn_probe_loss(bn_probe* probe, const float* d_X, const float* d_Y, int64_t n, float* d_out, void* stream);
/* Copy the weights [D, C] and bias [C] out of / into the probe (device pointers; the optimiser state is left alone). */
BN_API int bn_probe_get(bn_probe* probe, float* d_W, float* d_b, void* stream);
BN_API int bn_probe_set(bn_probe* probe, const float* d_W, const float* d_b, void* stream);
/* Long-tailed training sets.  The loss of the steps and of bn_probe_loss from here on: BN_PROBE_LOSS_CE (the default of a new probe) or
 * BN_PROBE_LOSS_FOCAL, the focal form of the sigmoid head's binary cross-entropy with y the target, p the sigmoid, pc = p clipped to
 * [1e-7, 1 - 1e-7]:  bce = -(y log pc + (1 - y) log(1 - pc)),  q = 1 - (y pc + (1 - y)(1 - pc)),  f = exp(focal_gamma log q),
 * loss = f bce,  dloss/dz = f (p - y) - focal_gamma (f / q) (2 y - 1) pc (1 - pc) bce.  focal_gamma = 0 is the cross-entropy in value
 * (computed by the focal statements).  Refused (BN_ERR_ARG, nothing changes): a null probe, an unknown loss, focal on a softmax probe, a
 * negative or non-finite focal_gamma (checked for either loss). */
#define BN_PROBE_LOSS_CE 0
#define BN_PROBE_LOSS_FOCAL 1
BN_API int bn_probe_set_loss(bn_probe* probe, int loss, float focal_gamma);
/* bn_probe_epoch with one weight per row: d_row_weight is float32 [rows of d_X], indexed through d_perm like d_Y; the loss and the
 * gradient of the elements of row i are multiplied by d_row_weight[i], and the means still divide by the batch's rows x classes (or
 * rows), not by the sum of the weights (Keras' sum_over_batch_size).  Null: no weights, bn_probe_epoch itself.  bn_probe_loss is never
 * weighted.  Here as in bn_probe_epoch, n is the length of d_perm, not the row count of d_X: a row number may occur any number of times
 * (upsampling a minority class without a second copy of its rows), and n may exceed the rows of d_X.  Two occurrences of a row in one
 * batch draw different dropout masks (the draw is per position in the batch). */
BN_API int bn_probe_epoch_weighted(bn_probe* probe, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm,
                            int64_t n, int batch, float* d_step_loss, void* stream);
/* Quantisation-aware fine-tuning of the head for the INT8 export (reference counterpart: `train --qat`, training/qat.py).  From the next
 * step and the next bn_probe_loss on, the forward sees what the exported head will compute; the gradient and the optimiser keep acting
 * on the full-precision (shadow) parameters, which bn_probe_get returns: the plain straight-through estimator.  Off on a new probe.
 *   weight_mode     BN_PROBE_QAT_PER_CLASS / _PER_TENSOR: in front of every forward the weights [D, C] are replaced by
 *                   float(q) * float(s) with s = max(amax_c, 5e-7) / 127, q = clip(rint(w / s), -127, 127) in float64, amax_c the largest
 *                   |w| of class c (of the whole matrix with _PER_TENSOR): the rule of the exporter's weight quantiser, bit for bit.  The
 *                   bias stays full precision.  BN_PROBE_QAT_OFF: the weights as they are.
 *   quantize_logits != 0: between the bias add and the activation, in float32 with a rounding after every operation,
 *                   k = rintf(z / s_out) + z_out, kc = min(max(k, -128), 127), zq = (kc - z_out) * s_out; the activation and the loss take
 *                   zq, and dLoss/dz is dLoss/dzq where k == kc and 0 where the code clamps.  (s_out, z_out) are the exported logit
 *                   tensor's parameters.  The sigmoid's 1/256 output grid is not modelled.
 * Refused (BN_ERR_ARG, nothing changes): a null probe, an unknown weight_mode, and with quantize_logits a non-finite or non-positive
 * s_out or a z_out outside [-128, 127].  A sweep has no QAT: fine-tune its winner as a bn_probe. */
#define BN_PROBE_QAT_OFF 0
#define BN_PROBE_QAT_PER_CLASS 1
#define BN_PROBE_QAT_PER_TENSOR 2
BN_API int bn_probe_set_qat(bn_probe* probe, int weight_mode, int quantize_logits, float s_out, int z_out);
/* The weights [D, C] the next forward would read (device pointer): fake-quantised under the current weight_mode, else the probe's own. */
BN_API int bn_probe_get_quantized(bn_probe* probe, float* d_Wq, void* stream);
/* Scores [n, C] of rows 0 .. n-1 of d_X under the probe's current QAT setting, without dropout (bn_head_forward when QAT is off).
 * d_codes, int8 [n, C] or null: the clamped logit codes kc; needs quantize_logits. */
BN_API int bn_probe_scores(bn_probe* probe, const float* d_X, int64_t n, float* d_scores, int8_t* d_codes, void* stream);

/* ---- A head with one hidden layer (csrc/bn_probe_mlp.hip) --------------------------------------------------------------------------
 *   a = drop1(x) W1 + b1 [B, H];  h = relu(a);  z = drop2(h) W2 + b2 [B, C];  scores = act(z)
 * W1 [D, H], b1 [H], W2 [H, C], b2 [C], row-major float32; 1 <= D, H <= BN_PROBE_MAX_D, 1 <= C <= BN_PROBE_MAX_C.  drop1 is bn_probe's
 * mask (seed, step, row in batch, column of x), drop2 the same draw and rate over [B, H] with seed ^ 0x48494444.  The loss, the row
 * weights, the schedule, the clip (one global norm over all four arrays) and the optimisers are bn_probe's; the entries mirror
 * bn_probe_create / _destroy / _set_loss / _epoch_weighted / _loss / _get / _set, with the same checks.  The buffers of a training step
 * (activations, gradients of the batch, row-group partials) stay within BN_PROBE_WORKSPACE_BYTES: a batch that would need more is refused
 * with BN_ERR_UNSUPPORTED.  The same inputs and seed give the same bits. */
typedef struct bn_probe_mlp bn_probe_mlp;
BN_API int bn_probe_mlp_create(bn_ctx* ctx, int D, int H, int C, int activation, int optimizer, float lr, float weight_decay, float clipnorm,
                        float dropout, uint32_t seed, int64_t total_steps, const float* d_W1, const float* d_b1, const float* d_W2,
                        const float* d_b2, bn_probe_mlp** out, void* stream);
BN_API void bn_probe_mlp_destroy(bn_probe_mlp* probe);
BN_API int bn_probe_mlp_set_loss(bn_probe_mlp* probe, int loss, float focal_gamma);
/* d_row_weight: float32 [rows of d_X] or null.  d_step_loss: float32 [ceil(n / batch)]. */
BN_API int bn_probe_mlp_epoch_weighted(bn_probe_mlp* probe, const float* d_X, const float* d_Y, const float* d_row_weight, const int32_t* d_perm,
                                int64_t n, int batch, float* d_step_loss, void* stream);
/* d_out[0]: the loss over rows 0 .. n-1 as they are (no dropout, no weights). */
BN_API int bn_probe_mlp_loss(bn_probe_mlp* probe, const float* d_X, const float* d_Y, int64_t n, float* d_out, void* stream);
BN_API int bn_probe_mlp_get(bn_probe_mlp* probe, float* d_W1, float* d_b1, float* d_W2, float* d_b2, void* stream);
BN_API int bn_probe_mlp_set(bn_probe_mlp* probe, const float* d_W1, const float* d_b1, const float* d_W2, const float* d_b2, void* stream);
/* d_scores[n, C] = act(relu(d_emb[n, D] d_W1 + d_b1) d_W2 + d_b2): the scores of such a head.  0 <= n < 2^31 (n == 0 launches nothing).
 * Rows go in steps whose hidden activations take at most 64 MiB of a workspace the context keeps. */
BN_API int bn_head_mlp_forward(bn_ctx* ctx, const float* d_emb, int64_t n, int D, const float* d_W1, const float* d_b1, int H, const float* d_W2,
                        const float* d_b2, int C, int activation, float* d_scores, void* stream);

/* ---- A hyperparameter sweep: T heads trained in lock-step on the same rows (csrc/bn_probe_sweep.hip) ---------------------------------
 * (Reference counterpart: `train --tune`, training/tuner.py, which trains its trials one after another.)  The trials share D, C, the
 * activation, the batch, X / Y, the permutation, the step counter, the dropout draw (each trial has its own threshold on it) and the
 * initial weights; a training step of all T trials is the three (four) launches of bn_probe_epoch's step with the trial as one more grid
 * axis.  A trial with label_smoothing == 0 has the bits of a bn_probe with the same hyperparameters and seed: weights, bias, step
 * losses, validation losses.  Label smoothing (Keras): y' = y (1 - eps) + 0.5 eps (sigmoid) or + eps / C (softmax) in the training loss
 * and its gradient; bn_probe_sweep_loss takes the targets as they are.  In float32: keep = fl(1 - eps), add = fl(0.5 eps) or
 * fl(eps / fl(C)), y' = fl(fl(y keep) + add). */
#define BN_PROBE_SWEEP_MAX_TRIALS 64
/* Bound on the device memory of one sweep: per trial the parameters, Adam's m and v and the best-weights snapshot ((D + 1) * C floats
 * each), G [batch, C], the row-group partials of its gradient (as many groups as a single fit of that batch uses, never fewer) and the
 * loss / norm partials (one loss partial per 16 rows of a batch, or of the rows of bn_probe_sweep_loss).  A call that would need more is
 * refused with the largest T that fits. */
#define BN_PROBE_SWEEP_BYTES (2048ull << 20)
#define BN_PROBE_SWEEP_CURRENT 0  /* bn_probe_sweep_get: the parameters as they are */
#define BN_PROBE_SWEEP_SNAPSHOT 1 /* ... as bn_probe_sweep_snapshot last kept them (the initial weights before the first one) */

typedef struct bn_probe_trial {
    int32_t optimizer;     /* BN_PROBE_OPT_* */
    float lr;              /* kept for the record: the step sizes come with every epoch (below) */
    float weight_decay;    /* adamw only */
    float clipnorm;        /* 0: no clipping */
    float dropout;         /* [0, 1) */
    float label_smoothing; /* [0, 1) */
} bn_probe_trial;

typedef struct bn_probe_sweep bn_probe_sweep;

/* trials: a host array of T rows, 1 <= T <= BN_PROBE_SWEEP_MAX_TRIALS.  d_W / d_b: the initial values of every trial (copied, also into
 * the snapshot slots; the optimiser states start at zero).  seed, total_steps: as bn_probe_create (total_steps is kept for the record). */
BN_API int bn_probe_sweep_create(bn_ctx* ctx, int D, int C, int activation, int T, const bn_probe_trial* trials, uint32_t seed,
                          int64_t total_steps, const float* d_W, const float* d_b, bn_probe_sweep** out, void* stream);
/* Waits for the device to finish, then frees the sweep. */
BN_API void bn_probe_sweep_destroy(bn_probe_sweep* sweep);
/* The ceil(n / batch) steps of one epoch for every trial t with d_active[t] != 0 (uint8 [T]; null: all).  d_step_sizes: float32
 * [steps, T, 2], (lr_t, alpha_t) of trial t at each step of this epoch: the cosine-decayed learning rate and Adam's step size with the
 * bias correction folded in, as bn_probe_epoch computes them on the host in float64.  d_step_loss: float32 [steps, T]; entries of
 * inactive trials are not written, and neither are their parameters, optimiser state or snapshot.  The step counter (the dropout
 * draw's) advances by the steps of the epoch for all trials.  Nothing synchronises with the host; no floating-point atomics. */
BN_API int bn_probe_sweep_epoch(bn_probe_sweep* sweep, const float* d_X, const float* d_Y, const int32_t* d_perm, int64_t n, int batch,
                         const float* d_step_sizes, const uint8_t* d_active, float* d_step_loss, void* stream);
/* d_out[t] = the mean loss of trial t's current weights over rows 0 .. n-1 of d_X / d_Y, without dropout or smoothing, for every trial
 * with d_active[t] != 0 (null: all); other entries are not written. */
BN_API int bn_probe_sweep_loss(bn_probe_sweep* sweep, const float* d_X, const float* d_Y, int64_t n, const uint8_t* d_active, float* d_out,
                        void* stream);
/* Copies the parameters of every trial with d_mask[t] != 0 (uint8 [T]) into its best-weights slot, on the device. */
BN_API int bn_probe_sweep_snapshot(bn_probe_sweep* sweep, const uint8_t* d_mask, void* stream);
/* The weights [D, C] and bias [C] of one trial (device pointers), which: BN_PROBE_SWEEP_CURRENT or BN_PROBE_SWEEP_SNAPSHOT. */
BN_API int bn_probe_sweep_get(bn_probe_sweep* sweep, int trial, int which, float* d_W, float* d_b, void* stream);
/* bn_probe_set_loss and bn_probe_epoch_weighted for a sweep: the loss kind, focal_gamma and the row weights are shared by all trials
 * (they are no fields of bn_probe_trial); label smoothing comes first, the focal loss sees the smoothed target.  bn_probe_sweep_loss
 * uses the loss that was set, unweighted and unsmoothed.  A trial with label_smoothing == 0 still has the bits of a bn_probe with the
 * same loss, weights and rows. */
BN_API int bn_probe_sweep_set_loss(bn_probe_sweep* sweep, int loss, float focal_gamma);
BN_API int bn_probe_sweep_epoch_weighted(bn_probe_sweep* sweep, const float* d_X, const float* d_Y, const float* d_row_weight,
                                  const int32_t* d_perm, int64_t n, int batch, const float* d_step_sizes, const uint8_t* d_active,
                                  float* d_step_loss, void* stream);

/* ---- Query by example: the k best rows of an embedding matrix per query (csrc/bn_search.hip; no reference counterpart) -------------
 * Rows and queries are BN_DTYPE_F32 values or the BN_DTYPE_I8 bytes of bn_forward_embed with their zero point; both sides have the same
 * type.  dot is the float32 inner product (its summation order is the implementation's) or, for int8, the exact int32 inner product of
 * (byte - zero_point) rounded once to float32.  inv = 1 / sqrt(sum of squares), both correctly rounded, 0 for a zero row.  Scores:
 * BN_SEARCH_DOT dot, BN_SEARCH_COSINE fl(fl(dot * inv_query) * inv_row).  Results per query are ordered by score descending and, among
 * equal scores, by row index ascending; when fewer than k rows qualify the remaining slots hold index -1 and score -inf.  With both
 * group arrays given, a row whose group equals the query's does not qualify.  Inputs must be finite.
 * 1 <= D <= BN_SEARCH_MAX_D, 1 <= k <= BN_SEARCH_MAX_K, 0 <= n < 2^31, Q >= 0.  float32 rows need 4-byte alignment (16 with D % 4 == 0
 * takes the wide loads; int8: 16 with D % 16 == 0).  The same inputs give the same bits on every run. */
#define BN_SEARCH_COSINE 0
#define BN_SEARCH_DOT 1
#define BN_SEARCH_MAX_K 128
#define BN_SEARCH_MAX_D 2048
/* How the rows are dealt to workgroups — from (n, D, Q, k) alone: steps of BN_SEARCH_STEP_ROWS rows, at least BN_SEARCH_MIN_WG_STEPS
 * steps per workgroup, at most BN_SEARCH_MAX_WGS workgroups per pass over the rows; a pass holds 16, 32 or 64 queries in
 * BN_SEARCH_LDS_BYTES of LDS.  The partial lists of a call take at most BN_SEARCH_WORKSPACE_BYTES (more queries run as further launches). */
#define BN_SEARCH_STEP_ROWS 64
#define BN_SEARCH_MIN_WG_STEPS 8
#define BN_SEARCH_MAX_WGS 1024
#define BN_SEARCH_LDS_BYTES (160 * 1024)
#define BN_SEARCH_WORKSPACE_BYTES (128u << 20)

/* d_inv[n] = inverse norms of the rows of d_rows [n, D] (zero_point is read for BN_DTYPE_I8 only). */
BN_API int bn_search_inv_norms(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, float* d_inv, void* stream);
/* d_idx [Q, k] int32 and d_score [Q, k] float32: the k best rows of d_db [n, D] for each row of d_queries [Q, D].  d_db_inv [n] and
 * d_q_inv [Q] come from bn_search_inv_norms and may be NULL for BN_SEARCH_DOT; d_db_group [n] / d_q_group [Q] int32, both or neither.
 * Nothing synchronises with the host inside the call unless the context's workspace has to grow. */
BN_API int bn_search_topk(bn_ctx* ctx, const void* d_db, int dtype, int64_t n, int D, int zero_point, const float* d_db_inv, const void* d_queries,
                   int64_t Q, const float* d_q_inv, int metric, const int32_t* d_db_group, const int32_t* d_q_group, int k, int32_t* d_idx,
                   float* d_score, void* stream);

/* ---- Clustering: spherical k-means over an embedding matrix (csrc/bn_kmeans.hip; no reference counterpart) ---------------------------
 * Rows are BN_DTYPE_F32 values or the BN_DTYPE_I8 bytes of bn_forward_embed with their zero point; an int8 row means
 * float32(byte - zero_point), which is exact, and everything after that is float32.  Centroids are float32 [K, D].  Inverse norms of rows
 * and centroids come from bn_search_inv_norms.  One Lloyd iteration is bn_kmeans_assign, bn_kmeans_accumulate and bn_kmeans_centroids.
 *   score[i, c] = fl(fl(dot(x_i, C_c) * inv_row[i]) * inv_cent[c])   (the dot product's summation order is the implementation's)
 *   label[i]    = the centroid with the highest score, the lowest index among equal scores; a zero row (inv_row == 0) gets label -1 and
 *                 score 0 and takes no part in sums, counts or the changed count
 *   S[c]        = sum over the members of c, in ascending row order, of fl(inv_row[i] * x_i): segments of BN_KMEANS_SEGMENT_ROWS members are
 *                 summed one after the other and folded in segment order, so the order follows from (labels, n, D, K) alone
 * 1 <= D <= BN_KMEANS_MAX_D, 1 <= K <= BN_KMEANS_MAX_K, 0 <= n < 2^31.  float32 rows need 4-byte alignment (16 with D % 4 == 0 takes the
 * wide loads; int8: 16 with D % 16 == 0).  No floating-point atomics: the same inputs give the same bits on every run.  A refused call
 * returns BN_ERR_ARG and writes nothing. */
#define BN_KMEANS_MAX_K 4096
#define BN_KMEANS_MAX_D 2048
/* How the work is dealt — from (n, D, K) alone.  Assignment: the centroids sit in LDS in tiles of 16, 32, 64 or BN_KMEANS_MAX_TILE, the
 * smallest that holds K or else the largest whose rows of (D rounded up to 64, plus 4) floats fit BN_KMEANS_LDS_BYTES; rows go in steps of
 * BN_KMEANS_STEP_ROWS, at least BN_KMEANS_MIN_WG_STEPS steps per workgroup, at most BN_KMEANS_MAX_WGS workgroups.  Update: a workgroup
 * per segment of at most BN_KMEANS_SEGMENT_ROWS members of a cluster. */
#define BN_KMEANS_LDS_BYTES (160 * 1024)
#define BN_KMEANS_MAX_TILE 128
#define BN_KMEANS_STEP_ROWS 64
#define BN_KMEANS_MIN_WG_STEPS 8
#define BN_KMEANS_MAX_WGS 1024
#define BN_KMEANS_SEGMENT_ROWS 256

/* d_label [n] int32 and d_score [n] float32 of the rows of d_rows [n, D] against d_centroids [K, D].  *d_changed (int64, 8-byte aligned)
 * is set to the number of non-zero rows whose label differs from d_prev_label [n] (NULL: every non-zero row counts).  d_prev_label must
 * not be d_label.  With more centroids than one LDS tile holds, d_label / d_score carry the best of the tiles seen so far while the call
 * runs: they hold the result once it has finished, and nothing else may read or write them meanwhile.  Nothing synchronises with the host
 * inside the call. */
BN_API int bn_kmeans_assign(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_row_inv,
                     const float* d_centroids, const float* d_cent_inv, int K, const int32_t* d_prev_label, int32_t* d_label, float* d_score,
                     int64_t* d_changed, void* stream);
/* d_sums [K, D] float32 and d_counts [K] int64 from the rows and their labels (a label outside 0 .. K-1 belongs to no cluster).  With
 * accumulate != 0 the results are added to what d_sums / d_counts hold, the old sum first: an index larger than the device budget is
 * processed block by block.  Nothing synchronises with the host inside the call unless the context's workspace has to grow. */
BN_API int bn_kmeans_accumulate(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_row_inv,
                         const int32_t* d_label, int K, int accumulate, float* d_sums, int64_t* d_counts, void* stream);
/* d_centroids[c] = fl(d_sums[c] * inv_norm(d_sums[c])) for every cluster with d_counts[c] > 0 (the others keep their centroid), then
 * d_cent_inv [K] = the inverse norms of the centroids. */
BN_API int bn_kmeans_centroids(bn_ctx* ctx, const float* d_sums, const int64_t* d_counts, int K, int D, float* d_centroids, float* d_cent_inv,
                        void* stream);

/* ---- Silhouette: the mean cosines of a labelling's rows to its clusters (csrc/bn_silhouette.hip; no reference counterpart) -------------
 * (birdnet_stm32/evaluation/silhouette.py is the specification.)  With x^_i the normalised row and S_c the sum of the normalised members
 * of cluster c (bn_kmeans_accumulate's d_sums), sum over j in c of (1 - x^_i . x^_j) = n_c - x^_i . S_c: the exact cosine silhouette of
 * every row needs the rows against the K sums once.  Rows, dtypes, inverse norms and the dot product have bn_kmeans_assign's meaning.
 *   m[i, c]    = fl(fl(dot(x_i, S_c) * inv_row[i]) * w[c])       w[c] = float32(1 / n_c), 0 for an empty cluster: the caller's d_weight
 *   live(i)    = inv_row[i] != 0 and 0 <= label[i] < K
 *   own[i]     = m[i, label[i]]
 *   other[i]   = the highest m[i, c] over c != label[i] with w[c] != 0;  nearest[i] = that c, the lowest index among equal values
 * A row that is not live gets own = other = 0 and nearest = -1; a live row without another non-empty cluster gets other = 0 and
 * nearest = -1.  The silhouette itself is the host's: a = (1 - own) n_A / (n_A - 1), b = 1 - other, s = (b - a) / max(a, b).
 * The limits and the alignment rules are bn_kmeans_assign's, and so is the deal of the work (the sums take the centroids' place in LDS).
 * No atomics: the same inputs give the same bits on every run.  A refused call returns BN_ERR_ARG and writes nothing. */

/* d_own [n], d_other [n] float32 and d_nearest [n] int32 of the rows of d_rows [n, D] with labels d_label [n] against d_sums [K, D] and
 * d_weight [K].  With more sums than one LDS tile holds, the three outputs carry the values of the tiles seen so far while the call runs:
 * they hold the result once it has finished, and nothing else may read or write them meanwhile.  Nothing synchronises with the host
 * inside the call. */
BN_API int bn_silhouette_means(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_row_inv,
                        const int32_t* d_label, const float* d_sums, const float* d_weight, int K, float* d_own, float* d_other,
                        int32_t* d_nearest, void* stream);

/* ---- Density clustering: one Borůvka round of the mutual-reachability spanning tree (csrc/bn_density.hip; no reference counterpart) ----
 * (HDBSCAN over cosine scores; birdnet_stm32/evaluation/density.py is the specification.)  Rows, dot and inv have bn_search's meaning.
 *   s_ij = fl(dot_ij * fl(inv_i * inv_j))      one value per pair, whichever end it is looked at from
 *   m_ij = min(s_ij, core_i, core_j)           the mutual-reachability score; a negative zero counts as the positive one
 *   d_best[i] = the key of the best (m_ij, j) over the rows j with comp[j] >= 0 and comp[j] != comp[i]: m descending, then j ascending.
 *               key = (image of m) << 32 | (0xFFFFFFFF - j), where the image of a float32 with bits u is ~u for a set sign bit and
 *               u | 0x80000000 otherwise, so a larger key is a better pair; 0 where there is no such row or comp[i] < 0.
 * Cores are finite or +inf.  The bests of the tiles and workgroups meet in a 64-bit integer atomicMax: a maximum under a total order, so
 * the same inputs give the same bits on every run; no floating-point atomics.  1 <= D <= BN_DENSITY_MAX_D, 0 <= n <= BN_DENSITY_MAX_N.
 * float32 rows need 4-byte alignment (16 with D % 4 == 0 takes the wide loads; int8: 16 with D % 16 == 0), d_best 8-byte alignment.  A
 * refused call returns BN_ERR_ARG and writes nothing.  Nothing synchronises with the host inside the call. */
#define BN_DENSITY_MAX_N (1 << 20)
#define BN_DENSITY_MAX_D 2048
/* How the work is dealt — from (n, D, dtype) alone.  A workgroup stages a tile of 16, 32, 64 or BN_DENSITY_MAX_TILE rows in LDS: the largest
 * whose rows (D rounded up to 64 elements, plus 16 bytes) fit BN_DENSITY_LDS_BYTES, halved while half of it still holds all n rows.  The
 * first grid axis holds the ceil(n / tile) tiles.  Against its tile a workgroup streams a range of all rows in steps of BN_DENSITY_STEP_ROWS,
 * at least BN_DENSITY_MIN_WG_STEPS steps per workgroup, at most BN_DENSITY_MAX_ROW_WGS ranges: the second grid axis. */
#define BN_DENSITY_LDS_BYTES (160 * 1024)
#define BN_DENSITY_MAX_TILE 128
#define BN_DENSITY_STEP_ROWS 64
#define BN_DENSITY_MIN_WG_STEPS 32
#define BN_DENSITY_MAX_ROW_WGS 256
BN_API int bn_density_nearest(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_inv,
                       const float* d_core, const int32_t* d_comp, uint64_t* d_best, void* stream);

/* ---- Projection: exact t-SNE with k-nearest-neighbour affinities and all-pairs repulsion (csrc/bn_tsne.hip; no reference counterpart) ----
 * (van der Maaten's formulas with the constants of scikit-learn 1.7's sklearn.manifold.TSNE; birdnet_stm32/evaluation/project.py is the
 * specification.)  A map is Y [n, 2] float32.  With w_ij = 1 / (1 + |y_i - y_j|^2):
 *   A_i  = sum over the entries j of row i of the CSR matrix P of p_ij w_ij (y_i - y_j)
 *   R_i  = sum over j != i of w_ij^2 (y_i - y_j),   z_i = sum over j != i of w_ij,   Z = sum over i of z_i
 *   grad_i = 4 (exaggeration * A_i - R_i / Z)
 * Everything per pair is float32: differences, 1 + dx^2 + dy^2 as two fused multiply-adds, the hardware reciprocal (1 ulp), products and
 * fused accumulation.  j = i is left out by index; equal points are legal (w = 1, no force).  Within a range of BN_TSNE_SPLIT_J columns
 * R_i and z_i are summed over j ascending in two chains, the even and the odd columns of every LDS tile (an odd last column goes to the
 * first), which are added at the end; the ranges are then added in ascending order; a row of P is summed by 16 lanes, each over
 * every 16th entry, then across the lanes in a fixed tree; Z is one float64 sum of the float32 z_i in a fixed order; R_i / Z is a float64
 * division rounded once to float32.  No floating-point atomics: the same inputs give the same bits on every run.  A refused call returns
 * BN_ERR_ARG and writes nothing.  Nothing synchronises with the host inside a call unless the context's workspace has to grow. */
/* How the repulsion is dealt — from n alone: a workgroup owns BN_TSNE_TILE_I rows and stages the columns of its range through LDS in
 * tiles of BN_TSNE_TILE_J points; the second grid axis holds ceil(n / BN_TSNE_SPLIT_J) column ranges.  A row of P goes to
 * BN_TSNE_ROW_LANES lanes.  bn_tsne_perplexity gives a row to BN_TSNE_ROW_LANES lanes as well, k <= BN_TSNE_MAX_K. */
#define BN_TSNE_TILE_I 256
#define BN_TSNE_TILE_J 1024
#define BN_TSNE_SPLIT_J 4096
#define BN_TSNE_ROW_LANES 16
#define BN_TSNE_MAX_K 128
#define BN_TSNE_MAX_N (1 << 21)   /* rows of a map: the column ranges are the second grid axis, their partial sums n * ceil(n / BN_TSNE_SPLIT_J) * 16 bytes */
#define BN_TSNE_MAX_PERPLEXITY_STEPS 100

/* Conditional affinities from the cosine scores of bn_search_topk: d_score [n, k] float32 -> d_p [n, k] float32 and d_beta [n] float64.
 * Per row, in float64: d2_j = max(0, fl32(2 - 2 s_j)), m = min d2, p_j = exp(-beta (d2_j - m)), S = sum p_j,
 * H = log S + beta sum (d2_j - m) p_j / S.  beta starts at 1 and follows scikit-learn's search (_binary_search_perplexity): doubled or
 * halved while its interval is open on that side, bisected afterwards, until |H - log(perplexity)| <= 1e-5 or
 * BN_TSNE_MAX_PERPLEXITY_STEPS values have been tried; the last value tried stands.  d_p = fl32(p_j / S) for that beta.  Scores must be
 * finite.  Refused: n < 1 or n >= 2^31, k outside 1..BN_TSNE_MAX_K, perplexity not in [1, BN_TSNE_MAX_K / 3], a NULL pointer, d_score /
 * d_p not 4-byte or d_beta not 8-byte aligned. */
BN_API int bn_tsne_perplexity(bn_ctx* ctx, const float* d_score, int64_t n, int k, double perplexity, float* d_p, double* d_beta, void* stream);
/* d_grad [n, 2] float32 and *d_z (float64) of the map d_y [n, 2] under P = (d_rowptr [n + 1] int64, d_col int32, d_val float32), a CSR
 * matrix whose rows may hold anything from 0 to n - 1 entries; with d_kl_rows (float64 [n], may be NULL) also
 * kl_i = sum over the entries of row i with p_ij > 0 of p_ij log(p_ij (1 + |y_i - y_j|^2)) in float64, summed like A_i; the Kullback-Leibler
 * divergence of P is sum kl_i + (sum p_ij) log Z.  The device tables are not trusted further than their sizes: row bounds are clipped to
 * 0 .. d_rowptr[n] and columns to 0 .. n - 1, so a bad matrix gives wrong numbers, never a stray read beyond d_rowptr[n] entries.
 * Refused: n < 2 or n > BN_TSNE_MAX_N, an exaggeration that is not finite, a NULL pointer other than d_kl_rows, d_y / d_grad / d_rowptr / d_z /
 * d_kl_rows not 8-byte or d_col / d_val not 4-byte aligned. */
BN_API int bn_tsne_gradient(bn_ctx* ctx, const float* d_y, int64_t n, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val,
                     float exaggeration, float* d_grad, double* d_z, double* d_kl_rows, void* stream);
/* One step of scikit-learn's _gradient_descent over the 2 n elements of d_y, d_grad, d_update and d_gains, every operation rounded to
 * float32 and nothing fused:  inc = update * grad < 0;  gains = inc ? gains + 0.2 : gains * 0.8;  gains = max(gains, 0.01);
 * update = momentum * update - lr * (gains * grad);  y += update.  d_y, d_update and d_gains are rewritten, d_grad is only read.
 * Refused: n < 1 or n >= 2^30, lr or momentum not finite, a NULL pointer, an array not 4-byte aligned. */
BN_API int bn_tsne_update(bn_ctx* ctx, float* d_y, const float* d_grad, float* d_update, float* d_gains, int64_t n, float lr, float momentum,
                   void* stream);

/* ---- Label spreading over a fixed sparse graph (csrc/bn_propagate.hip; no reference counterpart) ------------------------------------
 * (Zhou et al. 2004, scikit-learn's LabelSpreading; birdnet_stm32/evaluation/propagate.py is the specification.)  S = (d_rowptr [n + 1]
 * int64, d_col int32, d_val float32) is a CSR matrix whose rows may hold anything from 0 to n - 1 entries, F [n, C] float32 the label
 * matrix, d_seed_label [n] int32 the class of a labelled row and -1 (or anything outside 0 .. C - 1) for the others.  One update:
 *   acc = 0;  for the entries of row i in stored order: acc = fl(acc + fl(S_ij * F[j, c]));  F_next[i, c] = fl(fl(alpha * acc) + y),
 *   y = fl(1 - alpha) where d_seed_label[i] == c, else 0
 * in float32, every operation rounded on its own, nothing fused.  One lane adds all the entries of an (i, c), so the order is the matrix's:
 * no sum across lanes, no floating-point atomics, the same inputs give the same bits on every run and numpy reproduces them.  The device
 * tables are not trusted further than their sizes: row bounds are clipped to 0 .. d_rowptr[n], and an entry whose column lies outside
 * 0 .. n - 1 contributes nothing, so a bad matrix gives wrong numbers, never a stray read beyond d_rowptr[n] entries.  A refused call
 * returns BN_ERR_ARG and writes nothing.  Nothing synchronises with the host inside a call unless the context's workspace has to grow. */
/* How the rows are dealt — from C and the alignment of the two F arrays alone: with C % 4 == 0 and both arrays 16-byte aligned a lane owns
 * four neighbouring classes (16-byte loads), otherwise one; a row goes to the smallest power of two of lanes that covers its classes, at
 * most BN_PROPAGATE_MAX_ROW_LANES, and a lane takes every further class (or four) at that stride. */
#define BN_PROPAGATE_MAX_CLASSES 4096
#define BN_PROPAGATE_MAX_N (1 << 21)
#define BN_PROPAGATE_MAX_ROW_LANES 64
/* d_f_next [n, C] = one update of d_f [n, C]; with d_delta (float64, may be NULL) also *d_delta = sum over (i, c) of |F_next - F|, every
 * difference exact in float64: per row each lane over its classes in ascending order, the row's lanes in a fixed tree, then the rows in
 * one fixed order.  *d_delta stays on the device; a NULL d_delta is left alone and costs nothing.
 * Refused: n < 1 or n > BN_PROPAGATE_MAX_N, C outside 1..BN_PROPAGATE_MAX_CLASSES, alpha not in (0, 1), a NULL pointer other than d_delta,
 * d_rowptr / d_delta not 8-byte or another array not 4-byte aligned, d_f_next overlapping d_f. */
BN_API int bn_propagate_step(bn_ctx* ctx, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, const float* d_f,
                             const int32_t* d_seed_label, int64_t n, int C, float alpha, float* d_f_next, double* d_delta, void* stream);
/* Per row of d_f [n, C]: d_label = the first class with the largest value (float32 comparison), d_score = fl(F[i, label] / sum_c F[i, c]),
 * the sum in float32 in the implementation's fixed order; a row whose sum is 0 gets -1 and 0.  Values are finite and >= 0.
 * Refused: n < 1 or n > BN_PROPAGATE_MAX_N, C outside 1..BN_PROPAGATE_MAX_CLASSES, a NULL pointer, an array not 4-byte aligned. */
BN_API int bn_propagate_decide(bn_ctx* ctx, const float* d_f, int64_t n, int C, int32_t* d_label, float* d_score, void* stream);

/* ---- Selection: farthest-first traversal over an embedding matrix (csrc/bn_select.hip; no reference counterpart) ----------------------
 * (k-centre greedy, the core-set selection of Sener & Savarese 2018; birdnet_stm32/evaluation/select.py is the specification.)  Rows, dot
 * and inv have bn_search's meaning.  The state is d_m [n] float32 — the highest score of a row to any row taken so far, -inf for none yet,
 * +inf for a taken row — and d_nearest [n] int32, the row that gave it.
 *   score(i, c) = fl(fl(dot(x_i, x_c) * inv[i]) * inv[c])
 *   key[i]      = fl(u_i * fl(1 - m_i)), u_i = d_weight[i] (finite, >= 0; 1 without weights); -inf for a zero row (inv == 0), for a taken
 *                 row and for a NaN
 *   a pick      = the row with the highest key, the lowest index among equal keys (float comparison); -1 with key -inf when no key is
 *                 above -inf, and then nothing changes
 *   taking c    = for every live, untaken row i != c: s = score(i, c); s > m_i sets m_i = s, nearest_i = c (strict: the earlier centre
 *                 stands on a tie); then m_c = +inf, nearest_c = c
 * The float32 dot product of a row is four fused multiply-add chains, one per lane over the lane's 16-byte pieces of every 64 bytes in
 * ascending order, added as (l0 + l1) + (l2 + l3); the int8 one is exact in int32.  No atomics: the same inputs give the same bits on
 * every run, and a run of a + b steps equals a run of a steps followed by one of b.
 * 1 <= D <= BN_SEARCH_MAX_D, 0 <= n < 2^31, 0 <= forced <= steps.  float32 rows need 4-byte alignment (16 with D % 4 == 0 takes the wide
 * loads; int8: 16 with D % 16 == 0).  A refused call returns BN_ERR_ARG and writes nothing. */
/* How the rows are dealt to workgroups — from n alone: steps of BN_SELECT_STEP_ROWS rows (the row streamer's step), at least
 * BN_SELECT_MIN_WG_STEPS steps per workgroup, at most BN_SELECT_MAX_WGS workgroups.  A pass is one launch; every workgroup leaves one
 * partial (key, row), and every workgroup of the next pass folds all of them: BN_SELECT_MAX_WGS bounds that fold at 8 KiB. */
#define BN_SELECT_STEP_ROWS 64
#define BN_SELECT_MIN_WG_STEPS 2
#define BN_SELECT_MAX_WGS 1024
/* `steps` picks over d_rows [n, D].  The first `forced` entries of d_picked [steps] are given and are taken in order (an entry outside
 * 0 .. n-1, or one naming a zero row, is skipped; their d_key entries are left alone); entries forced .. steps-1 are chosen as above and
 * written with their keys to d_key [steps].  d_weight may be NULL.  forced = 0 starts from the state as given.  All launches (steps + 1 at
 * the most) are enqueued by the call; nothing synchronises with the host inside it unless the context's workspace has to be allocated. */
BN_API int bn_select_run(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_inv, const float* d_weight,
                         float* d_m, int32_t* d_nearest, int32_t* d_picked, int forced, int steps, float* d_key, void* stream);

/* ---- Acoustic indices of raw STFT magnitudes (csrc/bn_indices.hip; no reference counterpart) -------------------------------------------
 * (birdnet_stm32/evaluation/indices.py is the specification: ACI, spectral and temporal entropy, NDSI, the bioacoustic index, ADI and AEI
 * per chunk, and the three per-bin channels of false-colour long-duration spectrograms.)  With S [F, W] one chunk's magnitudes as
 * bn_stft_mag(normalize = 0) leaves them, P = S * S, r_f = sum_t S, p_f = sum_t P, e_t = sum_f P, smax the chunk's maximum (d_minmax[b][1];
 * the minimum is not read), thr = fl32(smax * cover_ratio), H(v) = -sum q ln q / ln(len v) over q = v / sum v (0 for an all-zero v):
 *   d_out[b]      = { aci, hf, ht, h, ndsi, bi, adi, aei }                                            BN_INDICES_SCALARS float32
 *     aci  = sum_f ACI_f              hf = H(p)      ht = H(e)      h = hf * ht
 *     ndsi = (B - A) / (B + A), A / B = sum of p_f over bins [anthro_k0, anthro_k1) / [bio_k0, bio_k1); 0 when A + B = 0
 *     bi   = sum over [bio_k0, bio_k1) of (L_f - min L_f) * df_khz, L_f = 10 log10(max(p_f / W, 1e-12 smax^2)); 0 when smax = 0
 *     adi  = -sum q ln q, q = c / sum c, c_b = (cells of bins [band_edge[b], band_edge[b+1]) with S > thr) / (cells of the band)
 *     aei  = 2 sum_i i x_(i) / (n sum x) - (n + 1) / n over the ascending c (i from 1); adi = aei = 0 when sum c = 0
 *   d_spectral[b] = { ACI_f [F], ENT_f [F], CVR_f [F] } (may be NULL: the scalars are the same)
 *     ACI_f = sum_{t >= 1} |S[f,t] - S[f,t-1]| / r_f (0 where r_f = 0)    ENT_f = 1 - H(P[f, :]) (0 where p_f = 0)
 *     CVR_f = fl32(count_t(S[f,t] > thr)) / fl32(W)
 * One workgroup per chunk and one pass over its F * W floats.  Sums are float32 in a fixed order (a lane's elements, then a tree over the
 * lanes), counts are integers, and ACI_f, CVR_f and ndsi are single correctly rounded divisions of their sums; no atomics: the same input
 * gives the same bits on every run.  Rows are read with 16-byte loads where d_spec is 16-byte aligned and W % 4 == 0, with the same bits
 * from any other layout.  F must be BN_INDICES_BINS (the STFT's own limit): BN_ERR_UNSUPPORTED otherwise.  Refused with BN_ERR_ARG, nothing
 * launched: W outside BN_INDICES_MIN_W .. BN_INDICES_MAX_W, B < 0, a NULL pointer other than d_spectral, an array not 4-byte aligned, a
 * bin range outside 0 <= k0 <= k1 <= F, n_bands outside 0 .. BN_INDICES_MAX_BANDS, band edges that decrease or leave 0 .. F, a
 * cover_ratio or df_khz that is negative or not finite.  B = 0 does nothing. */
#define BN_INDICES_SCALARS 8
#define BN_INDICES_BINS 257
#define BN_INDICES_MIN_W 2
#define BN_INDICES_MAX_W 1024
#define BN_INDICES_MAX_BANDS 16
typedef struct bn_indices_params {
    int32_t anthro_k0, anthro_k1;                     /* bins of the anthrophony band (NDSI) */
    int32_t bio_k0, bio_k1;                           /* bins of the biophony band (NDSI, BI) */
    int32_t n_bands;                                  /* bands of ADI / AEI */
    int32_t band_edge[BN_INDICES_MAX_BANDS + 1];      /* band b holds bins [band_edge[b], band_edge[b + 1]); entries past n_bands are ignored */
    float cover_ratio;                                /* fl32(10^(db / 20)): the cover threshold as a share of the chunk's maximum */
    float df_khz;                                     /* sample_rate / 512 / 1000 */
} bn_indices_params;
BN_API int bn_acoustic_indices(bn_ctx* ctx, const float* d_spec, const float* d_minmax, int B, int F, int W, const bn_indices_params* params,
                               float* d_out, float* d_spectral, void* stream);

/* ---- Principal components: column sums, scatter matrix and projection of embedding rows (csrc/bn_pca.hip; no reference counterpart) ----
 * (birdnet_stm32/evaluation/reduce.py is the specification; the eigen-decomposition stays on the host.)  Rows have bn_search's meaning: an
 * int8 row is byte - zero_point.  With c_i = fl32(x_i - mean) (x_i itself where d_mean is NULL; an int8 x is made float32 first, which is exact):
 *   bn_pca_colsum      d_sum[d]     = sum_i x_id                float64, rows in a fixed order; the int8 result is the exact integer
 *   bn_pca_gram        d_gram[a][b] = sum_i c_ia c_ib           float32 products of the matrix cores accumulate in float32 for at most
 *                                                               BN_PCA_RUN_ROWS rows, the runs' sums are added in float64 in ascending order.
 *                                                               Per entry |error| <= (BN_PCA_RUN_ROWS + 1) 2^-24 sum_i |c_ia c_ib|.  int8 needs
 *                                                               d_mean == NULL and gives the exact integer sum_i x_ia x_ib (a run stays
 *                                                               below 2^24).  Only the upper triangle is multiplied: d_gram == d_gram^T bit
 *                                                               for bit.
 *   bn_pca_transform   d_out[i][k]  = sum_d W_kd c_id           one float32 fused chain of the matrix cores over d ascending (zeros beyond D):
 *                                                               |error| <= (D + 2) 2^-24 sum_d |W_kd c_id|
 * 1 <= D <= BN_PCA_MAX_D, 1 <= r <= D, 0 <= n < 2^31.  float32 rows need 4-byte alignment (16 with D % 4 == 0 takes the wide loads; int8: 16
 * with D % 16 == 0), d_sum and d_gram 8-byte alignment.  A refused call returns BN_ERR_ARG and writes nothing; n = 0 writes zeros (nothing
 * for the transform).  No floating-point atomics: the same inputs give the same bits on every run.  Nothing synchronises with the host
 * inside a call unless the context's workspace has to grow. */
#define BN_PCA_MAX_D 2048
/* How the work is dealt — from (n, D, dtype[, r]) alone.
 * Column sums: lanes across min(BN_PCA_COLSUM_COLS, D rounded up to a power of two) columns at a time, the other lanes of the 256 take
 * every G-th row; ceil(n / BN_PCA_COLSUM_MIN_ROWS) row ranges, at most BN_PCA_COLSUM_MAX_WGS.
 * Scatter matrix: features in macro tiles of BN_PCA_MACRO; the first grid axis holds the M (M + 1) / 2 pairs of the upper triangle.  Rows in
 * runs of BN_PCA_RUN_ROWS, staged through LDS BN_PCA_STAGE_ROWS at a time; the second grid axis holds
 * min(ceil(BN_PCA_GRAM_TARGET_WGS / pairs), BN_PCA_GRAM_MAX_RANGES, runs) ranges of whole runs, evened out.
 * Transform: a tile of 16, 32, 64 or BN_PCA_MAX_TILE rows of W in LDS, the smallest that holds r and the largest that fits
 * BN_PCA_LDS_BYTES with the mean; rows in steps of BN_PCA_STEP_ROWS, at least BN_PCA_MIN_WG_STEPS per workgroup, at most BN_PCA_MAX_WGS. */
#define BN_PCA_RUN_ROWS 256
#define BN_PCA_STAGE_ROWS 64
#define BN_PCA_MACRO 64
#define BN_PCA_GRAM_TARGET_WGS 1024
#define BN_PCA_GRAM_MAX_RANGES 256
#define BN_PCA_COLSUM_COLS 256
#define BN_PCA_COLSUM_MIN_ROWS 256
#define BN_PCA_COLSUM_MAX_WGS 1024
#define BN_PCA_LDS_BYTES (160 * 1024)
#define BN_PCA_MAX_TILE 128
#define BN_PCA_STEP_ROWS 64
#define BN_PCA_MIN_WG_STEPS 8
#define BN_PCA_MAX_WGS 1024
BN_API int bn_pca_colsum(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, double* d_sum /* [D] */, void* stream);
/* d_mean [D] float32 or NULL (required NULL for BN_DTYPE_I8); d_gram [D, D] float64. */
BN_API int bn_pca_gram(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_mean, double* d_gram,
                       void* stream);
/* d_mean [D] float32 or NULL, d_W [r, D] float32, d_out [n, r] float32; d_out must not overlap the inputs. */
BN_API int bn_pca_transform(bn_ctx* ctx, const void* d_rows, int dtype, int64_t n, int D, int zero_point, const float* d_mean, const float* d_W,
                            int r, float* d_out, void* stream);

/* ---- Bootstrap of the per-class average precision (csrc/bn_bootstrap.hip) -----------------------------------------------------------
 * (reference: birdnet_stm32/evaluation/metrics.py:239-318 `bootstrap_ap_ci`: one np.random.default_rng(seed) consumed class by class,
 * rng.integers(0, n, size=n) per resample, sklearn's average_precision_score on the picked rows.)  The draws are numpy's own, reproduced on
 * the device; birdnet_stm32/evaluation/bootstrap.py restates them and is the specification.  The generator is a PCG64 given as
 * (state_hi, state_lo, inc_hi, inc_lo), the two 128-bit integers of `rng.bit_generator.state`, with no spare 32-bit half.  Its 32-bit
 * stream is indexed by RAW POSITION: 2 q is the low half of the q-th next 64-bit output, 2 q + 1 the high half.  A draw below `bound` is
 * Lemire's: m = x * bound, rejected when (m mod 2^32) < (2^32 - bound) mod bound, else m >> 32.  A resample is a raw range [p0, p1) that
 * holds its n accepted values; rejected values inside it are skipped.
 *   BN_BOOTSTRAP_MAX_N   rows per class: a multiplicity is <= n, so two of them share a 32-bit LDS word and the counters of a workgroup take
 *                        64 KiB of the CU's 160 KiB. */
#define BN_BOOTSTRAP_MAX_N 32768

/* The rejection scan (reference :286 `rng.integers`, numpy's buffered_bounded_lemire_uint32): *h_count = how many raw positions in
 * [p_begin, p_end) hold a value that `bound` rejects, h_positions[0 .. *h_count) those positions in NO particular order (host memory; the call
 * waits for the stream).  More than `capacity` of them: BN_ERR_NOMEM, *h_count still set, h_positions untouched.  A bound that divides 2^32
 * rejects nothing and launches nothing.  0 <= p_begin <= p_end, p_end - p_begin <= 2^40. */
BN_API int bn_bootstrap_rejections(bn_ctx* ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo, uint32_t bound,
                            int64_t p_begin, int64_t p_end, int64_t* h_positions, int64_t capacity, int64_t* h_count, void* stream);
/* d_counts [B, n] uint32: how often resample b draws row i (reference :286, np.bincount of the picked indices), for the resamples whose raw
 * ranges are d_ranges [B, 2] int64 (p0, p1).  1 <= n <= BN_BOOTSTRAP_MAX_N.  The kernel cannot trust the device table: a range is clipped to
 * 2 n + 64 positions, so a bad one gives wrong counts, never a long loop or a stray access. */
BN_API int bn_bootstrap_counts(bn_ctx* ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo, int n, int B,
                        const int64_t* d_ranges, uint32_t* d_counts, void* stream);
/* d_ap [n_selected, B] float64: the average precision (reference :287-293, sklearn average_precision_score) of resample b of class
 * d_classes[j], NaN where the reference drops the resample (no positive or no negative among the picked rows).
 *   d_scores [n, n_classes] float32, finite; d_truth [n, n_classes] uint8, 0 or 1; d_cols [n_classes, n] int32 from bn_rank_orders;
 *   d_classes [n_selected] int32 column indices; d_ranges [n_selected * B, 2] int64, class-major.
 * Each term (tps / K - tps_prev / K) * (tps / seen) is the float64 expression the library evaluates, bit for bit; the terms are summed in a
 * fixed order that is not numpy's pairwise one: |d_ap - library| <= 2 n 2^-53.  No floating-point atomics.  Nothing synchronises with the
 * host inside the call unless the context's workspace has to grow. */
BN_API int bn_bootstrap_ap(bn_ctx* ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi, uint64_t inc_lo, int n, int n_classes,
                    const float* d_scores, const uint8_t* d_truth, const int32_t* d_cols, const int32_t* d_classes, int n_selected, int B,
                    const int64_t* d_ranges, double* d_ap, void* stream);

/* ---- Probe augmentation: mixup and SpecAugment over resident model inputs (csrc/bn_augment.hip) --------------------------------------
 * (reference: audio/augmentation.py:10-120 as data/generator.py:169-170 and :406-418 apply them: every sample is masked in the loader, the
 * batch is mixed afterwards.)  d_x holds n_rows un-augmented rows of E = F * W float32 (the raw frontend: F = 1, W = T).  Output row r:
 *   masked(x[s])(f, t) = +0.0f where f lies in any [f0, f0 + width) of d_fmask[s] or t in any of d_tmask[s], x[s](f, t) elsewhere -- the
 *                        masks belong to the SOURCE row s; a mask reaching past F or W is clipped, a width <= 0 masks nothing;
 *   d_nsrc[r] == 1:  out[r] = masked(x[src0])                       unmasked elements are copied bit for bit (no multiply)
 *   d_nsrc[r] == 2:  out[r] = fl(fl(g0 * v0) + fl(g1 * v1))         every product and sum rounded to float32, nothing fused,
 *   d_nsrc[r] == 3:  out[r] = fl(fl(fl(g0 * v0) + fl(g1 * v1)) + fl(g2 * v2))    float32 subnormals kept
 * which is numpy's np.sum(gains[:, None] * masked[src], axis=0), including its start from +0.0 (products that are all -0.0 sum to +0.0); birdnet_stm32/training/augment.py `augment_reference` is the specification and
 * the results equal it bit for bit.
 *   d_nsrc [m] int32, d_src [m, 3] int32, d_gain [m, 3] float32 (slots past nsrc are not read as sources);
 *   d_fmask [n_rows, nf, 2] / d_tmask [n_rows, nt, 2] int32 (start, width), NULL exactly when the count is 0; counts <= BN_AUGMENT_MAX_MASKS.
 * The host cannot see the device tables: the kernel clamps nsrc to 1..3 and every source index to [0, n_rows), so a bad plan gives a wrong
 * row, never a stray read.  Rows and tables need 4-byte alignment only; d_out [m, E] must not overlap d_x.  F * W <= BN_AUGMENT_MAX_ROW. */
#define BN_AUGMENT_MAX_MASKS 4
#define BN_AUGMENT_MAX_ROW (1 << 28)
BN_API int bn_augment_inputs(bn_ctx* ctx, const float* d_x, int64_t n_rows, int F, int W, const int32_t* d_nsrc, const int32_t* d_src,
                      const float* d_gain, const int32_t* d_fmask, int nf, const int32_t* d_tmask, int nt, int64_t m, float* d_out, void* stream);

/* Loads every device code object of the library now.  The HIP runtime loads one at the first launch of any of its kernels (a few ms each; launches
 * and copies of OTHER threads wait meanwhile), which a first batch otherwise pays one file after the other on its critical path; a caller with idle
 * time before that batch (the evaluate pipeline while the first files are being read) calls this instead.  Idempotent.  (Reference counterpart:
 * tf.lite.Interpreter.allocate_tensors(), models/runners.py:58 — the one-off preparation before the first invoke.) */
BN_API int bn_preload_kernels(bn_ctx* ctx);

/* Names of the HIP kernels a forward pass launches, '\n'-separated (for profiling tools). */
BN_API const char* bn_kernel_names(void);

#ifdef __cplusplus
}
#endif
#endif /* BIRDNET_HIP_H */
