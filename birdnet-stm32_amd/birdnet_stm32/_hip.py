"""ctypes binding of ``libbirdnet_hip.so`` (C ABI: ``include/birdnet_hip.h``).

The reference binds its accelerated path through ``tf.lite.Interpreter`` (reference:
birdnet_stm32/models/runners.py:57); here the same role is played by a plain C ABI loaded
with ``ctypes`` (``cffi`` is not installed on the target image).  PyTorch is imported first on
purpose: it loads the process's HIP runtime (``libamdhip64.so``), and ``libbirdnet_hip.so``
must bind to that same runtime instance so that device pointers and ``hipStream_t`` handles
coming from torch tensors are valid inside the library.

There is no fallback: if the shared object is missing or no gfx950 device is present, loading
or context creation raises.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # .../birdnet-stm32_amd
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libbirdnet_hip.so")

ABI_VERSION = 3

# every symbol include/birdnet_hip.h declares
EXPORTS = (
    "bn_version", "bn_last_error", "bn_device_count", "bn_ctx_create", "bn_ctx_destroy", "bn_model_load",
    "bn_model_free", "bn_model_get_info", "bn_stft_mag", "bn_forward", "bn_infer_audio", "bn_debug_op_output",
    "bn_kernel_names", "bn_profile_enable", "bn_profile_collect", "bn_ingest_resample", "bn_ingest_chunks",
    "bn_pool_scores", "bn_mel_spectrogram", "bn_profile_only", "bn_chunk_peak_normalize", "bn_set_option", "bn_get_option", "bn_ctx_set_option", "bn_ctx_get_option", "bn_ctx_reset_options", "bn_preload_kernels", "bn_host_alloc_pinned", "bn_host_free_pinned", "bn_rank_orders",
    "bn_blob_check", "bn_debug_requant", "bn_stft_mag_exact", "bn_debug_input_bytes", "bn_debug_guard_stats", "bn_debug_tail_form", "bn_debug_mid_form", "bn_debug_mid_plan", "bn_debug_mid_split_giveups", "bn_debug_satpack", "bn_debug_satpack_form",
    "bn_forward_embed", "bn_infer_audio_embed", "bn_model_get_embedding_info", "bn_ingest_resample_span",
    "bn_head_forward", "bn_probe_create", "bn_probe_destroy", "bn_probe_epoch", "bn_probe_loss", "bn_probe_get", "bn_probe_set",
    "bn_probe_sweep_create", "bn_probe_sweep_destroy", "bn_probe_sweep_epoch", "bn_probe_sweep_loss", "bn_probe_sweep_snapshot", "bn_probe_sweep_get",
    "bn_probe_set_loss", "bn_probe_epoch_weighted", "bn_probe_sweep_set_loss", "bn_probe_sweep_epoch_weighted",
    "bn_probe_set_qat", "bn_probe_get_quantized", "bn_probe_scores",
    "bn_probe_mlp_create", "bn_probe_mlp_destroy", "bn_probe_mlp_set_loss", "bn_probe_mlp_epoch_weighted", "bn_probe_mlp_loss", "bn_probe_mlp_get",
    "bn_probe_mlp_set", "bn_head_mlp_forward",
    "bn_short_time_energy", "bn_activity_counts", "bn_search_inv_norms", "bn_search_topk", "bn_augment_inputs",
    "bn_kmeans_assign", "bn_kmeans_accumulate", "bn_kmeans_centroids",
    "bn_silhouette_means",
    "bn_density_nearest",
    "bn_tsne_perplexity", "bn_tsne_gradient", "bn_tsne_update",
    "bn_propagate_step", "bn_propagate_decide",
    "bn_select_run",
    "bn_acoustic_indices",
    "bn_pca_colsum", "bn_pca_gram", "bn_pca_transform",
    "bn_bootstrap_rejections", "bn_bootstrap_counts", "bn_bootstrap_ap", "bn_head_i8_forward", "bn_head_i8_pass_classes",
)  # fmt: skip

EMB_F32, EMB_I8 = 0, 1  # BN_EMB_* (include/birdnet_hip.h)
PROBE_ACTIVATIONS = {"sigmoid": 0, "softmax": 1}  # BN_PROBE_ACT_*
PROBE_OPTIMIZERS = {"adam": 0, "adamw": 1, "sgd": 2}  # BN_PROBE_OPT_*
PROBE_LOSSES = {"auto": 0, "focal": 1}  # BN_PROBE_LOSS_* ("auto": the activation's cross-entropy)
PROBE_QAT_WEIGHTS = {"off": 0, "per_class": 1, "per_tensor": 2}  # BN_PROBE_QAT_*
PROBE_MAX_D, PROBE_MAX_C = 2048, 4096
PROBE_SWEEP_MAX_TRIALS = 64  # BN_PROBE_SWEEP_MAX_TRIALS
PROBE_SWEEP_CURRENT, PROBE_SWEEP_SNAPSHOT = 0, 1  # BN_PROBE_SWEEP_*
HEAD_I8_STEP_ROWS, HEAD_I8_MIN_WG_STEPS, HEAD_I8_MAX_WGS, HEAD_I8_LDS_BYTES = 64, 8, 1024, 160 * 1024  # BN_HEAD_I8_*: how bn_head_i8_forward deals rows



def head_i8_pass_classes(D: int, C: int) -> int:
    """Classes per LDS pass of ``bn_head_i8_forward`` (``bn_head_i8_pass_classes``: the launcher's own plan); more classes take further passes."""
    v = int(load_library().bn_head_i8_pass_classes(int(D), int(C)))
    check(min(v, 0))
    return v


class ProbeTrialStruct(ctypes.Structure):
    """bn_probe_trial (include/birdnet_hip.h)."""

    _fields_ = [("optimizer", ctypes.c_int32), ("lr", ctypes.c_float), ("weight_decay", ctypes.c_float), ("clipnorm", ctypes.c_float),
                ("dropout", ctypes.c_float), ("label_smoothing", ctypes.c_float)]


DTYPE_F32, DTYPE_I8 = 0, 1  # BN_DTYPE_*
SEARCH_METRICS = {"cosine": 0, "dot": 1}  # BN_SEARCH_*
SEARCH_MAX_K, SEARCH_MAX_D = 128, 2048
AUGMENT_MAX_MASKS = 4  # BN_AUGMENT_MAX_MASKS
SEARCH_STEP_ROWS, SEARCH_MIN_WG_STEPS, SEARCH_MAX_WGS = 64, 8, 1024  # how bn_search_topk deals rows to workgroups (include/birdnet_hip.h)
# bn_kmeans_* (include/birdnet_hip.h): limits, and the constants the centroid tiles, the row steps and the update's segments follow from;
# bn_silhouette_means has the same limits and deals its work by the same constants (the cluster sums take the centroids' place in LDS)
KMEANS_MAX_K, KMEANS_MAX_D = 4096, 2048
BOOTSTRAP_MAX_N = 32768  # BN_BOOTSTRAP_MAX_N
KMEANS_LDS_BYTES, KMEANS_MAX_TILE, KMEANS_STEP_ROWS, KMEANS_MIN_WG_STEPS, KMEANS_MAX_WGS, KMEANS_SEGMENT_ROWS = 160 * 1024, 128, 64, 8, 1024, 256
# bn_tsne_* (include/birdnet_hip.h): rows of a repulsion workgroup, points per LDS tile, columns per range of the second grid axis, lanes per row
TSNE_TILE_I, TSNE_TILE_J, TSNE_SPLIT_J, TSNE_ROW_LANES, TSNE_MAX_K, TSNE_MAX_N = 256, 1024, 4096, 16, 128, 1 << 21
# bn_propagate_* (include/birdnet_hip.h): limits, and the most lanes a row's classes are dealt to
PROPAGATE_MAX_CLASSES, PROPAGATE_MAX_N, PROPAGATE_MAX_ROW_LANES = 4096, 1 << 21, 64
# bn_select_run (include/birdnet_hip.h): how the rows are dealt to workgroups; a pass folds at most SELECT_MAX_WGS partial picks
SELECT_STEP_ROWS, SELECT_MIN_WG_STEPS, SELECT_MAX_WGS = 64, 2, 1024
# bn_density_nearest (include/birdnet_hip.h): limits, and the constants the staged tile and the streamed row ranges follow from
DENSITY_MAX_N, DENSITY_MAX_D = 1 << 20, 2048
DENSITY_LDS_BYTES, DENSITY_MAX_TILE, DENSITY_STEP_ROWS, DENSITY_MIN_WG_STEPS, DENSITY_MAX_ROW_WGS = 160 * 1024, 128, 64, 32, 256
# bn_pca_* (include/birdnet_hip.h): the limit, the rows whose products stay in float32 accumulators, and the constants the row ranges follow from
PCA_MAX_D, PCA_RUN_ROWS, PCA_STAGE_ROWS, PCA_MACRO, PCA_GRAM_TARGET_WGS, PCA_GRAM_MAX_RANGES = 2048, 256, 64, 64, 1024, 256
PCA_COLSUM_COLS, PCA_COLSUM_MIN_ROWS, PCA_COLSUM_MAX_WGS = 256, 256, 1024
PCA_LDS_BYTES, PCA_MAX_TILE, PCA_STEP_ROWS, PCA_MIN_WG_STEPS, PCA_MAX_WGS = 160 * 1024, 128, 64, 8, 1024


def pca_gram_rows_per_range(n: int, D: int) -> int:
    """Rows of the range a workgroup of ``bn_pca_gram`` sums, a whole number of runs (``pca_gram_geometry`` of csrc/bn_pca.hip)."""
    m = -(-int(D) // PCA_MACRO)
    pairs = m * (m + 1) // 2
    runs = -(-int(n) // PCA_RUN_ROWS)
    ranges = max(1, min(-(-PCA_GRAM_TARGET_WGS // pairs), PCA_GRAM_MAX_RANGES, runs))
    return max(1, -(-runs // ranges)) * PCA_RUN_ROWS


def pca_tile_rows(D: int, r: int) -> int:
    """Rows of ``W`` per LDS tile of ``bn_pca_transform`` (``pca_transform_geometry`` of csrc/bn_pca.hip)."""
    dp = -(-int(D) // 64) * 64
    nt = 1
    while nt < PCA_MAX_TILE // 16 and 16 * nt < r:
        nt *= 2
    while nt > 1 and 16 * nt * (dp + 4) * 4 + dp * 4 > PCA_LDS_BYTES:
        nt //= 2
    return 16 * nt


def density_tile_rows(n: int, D: int, int8: bool) -> int:
    """Rows per LDS tile of ``bn_density_nearest`` (``density_geometry`` of csrc/bn_density.hip)."""
    pitch_bytes = -(-int(D) // 64) * 64 + 16 if int8 else (-(-int(D) // 64) * 64 + 4) * 4
    nt = DENSITY_MAX_TILE // 16
    while nt > 1 and 16 * nt * pitch_bytes > DENSITY_LDS_BYTES:
        nt //= 2
    while nt > 1 and 16 * (nt // 2) >= n:
        nt //= 2
    return 16 * nt


def density_rows_per_workgroup(n: int) -> int:
    """Rows of the range a workgroup of ``bn_density_nearest`` streams (``split_rows`` of csrc/bn_rowstream.h)."""
    steps = -(-int(n) // DENSITY_STEP_ROWS)
    wgs = min(max(-(-steps // DENSITY_MIN_WG_STEPS), 1), DENSITY_MAX_ROW_WGS)
    return -(-steps // wgs) * DENSITY_STEP_ROWS


def kmeans_tile_centroids(D: int, K: int) -> int:
    """Centroids per LDS tile of ``bn_kmeans_assign`` (``kmeans_geometry`` of csrc/bn_kmeans.hip)."""
    pitch_bytes = (-(-int(D) // 64) * 64 + 4) * 4
    nt = 1
    while nt < KMEANS_MAX_TILE // 16 and 16 * nt < K:
        nt *= 2
    while nt > 1 and 16 * nt * pitch_bytes > KMEANS_LDS_BYTES:
        nt //= 2
    return 16 * nt


# launcher switches of bn_set_option (include/birdnet_hip.h); the production defaults are what a fresh process has
OPTION_NAMES = ("f32_strip", "f32_strip_th", "f32_front_staged", "f32_front2", "f32_pwdw", "f32_tile_slice", "f32_pw_ws", "i8_pwdw", "i8_pw_lds", "i8_pw_forms", "i8_add_tab", "front_tpw", "wave_dwpw", "i8_strip", "i8_strip_mfdw", "i8_strip_th", "i8_dw_pool", "i8_tail_fclds", "i8_tail", "i8_tail_mfdw", "i8_mid",
                "i8_mel_generic", "stft_rowmajor", "stft_exact", "stft_flagcap", "stft_guard", "stft_audit", "stft_minint", "ingest_blk", "ingest_generic")
# scheduling switches that change no result and no kernel's name (same bn_set_option; listed apart from the tuple above)
# ("i8_satpack": bit 0 = the fused chains' shift-saturate-pack epilogues, bit 1 = the front strip's stem rows; same bytes in fewer instructions)
SCHEDULING_OPTION_NAMES = ("i8_mid_split", "i8_satpack")


class BnModelInfo(ctypes.Structure):
    _fields_ = [
        ("dtype", c_int32), ("input_kind", c_int32), ("input_elems", c_int32), ("fft_bins", c_int32),
        ("spec_width", c_int32), ("num_classes", c_int32), ("n_ops", c_int32), ("max_batch", c_int32),
        ("workspace_bytes", c_int64), ("const_bytes", c_int64),
    ]  # fmt: skip


class HipError(RuntimeError):
    """A libbirdnet_hip call returned a negative status."""


_lib = None


def load_library(path: str | None = None):
    """Load (once) and type the shared library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("BIRDNET_HIP_LIB", LIB_PATH)
    if not os.path.isfile(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C birdnet-stm32_amd/csrc`). There is no CPU fallback for this path."
        )
    import torch  # noqa: F401  (brings in the HIP runtime this library must share)

    lib = ctypes.CDLL(path)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise RuntimeError(f"{path} does not export {name}")
    lib.bn_version.restype = c_int
    lib.bn_last_error.restype = c_char_p
    lib.bn_device_count.restype = c_int
    lib.bn_ctx_create.argtypes = [c_int, c_int, POINTER(c_void_p)]
    lib.bn_ctx_destroy.argtypes = [c_void_p]
    lib.bn_ctx_destroy.restype = None
    lib.bn_model_load.argtypes = [c_void_p, c_char_p, c_size_t, POINTER(c_void_p)]
    lib.bn_model_free.argtypes = [c_void_p]
    lib.bn_model_free.restype = None
    lib.bn_model_get_info.argtypes = [c_void_p, POINTER(BnModelInfo)]
    lib.bn_stft_mag.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_stft_mag_exact.argtypes = lib.bn_stft_mag.argtypes
    lib.bn_debug_input_bytes.argtypes = [c_void_p, c_int, c_void_p, c_void_p]
    lib.bn_debug_guard_stats.argtypes = [c_void_p, c_int, POINTER(c_int64)]
    lib.bn_debug_tail_form.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.bn_debug_mid_form.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.bn_debug_mid_plan.argtypes = [c_void_p, POINTER(c_int), c_int]
    lib.bn_debug_mid_split_giveups.argtypes = [c_void_p, POINTER(c_int64)]
    lib.bn_debug_satpack.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.bn_debug_satpack_form.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]
    lib.bn_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_infer_audio.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_forward_embed.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    lib.bn_infer_audio_embed.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
    lib.bn_model_get_embedding_info.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_float), POINTER(c_int)]
    lib.bn_debug_op_output.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, POINTER(c_size_t), c_void_p]
    lib.bn_kernel_names.restype = c_char_p
    lib.bn_profile_enable.argtypes = [c_void_p, c_int]
    lib.bn_profile_only.argtypes = [c_void_p, c_int]
    lib.bn_chunk_peak_normalize.argtypes = [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]
    lib.bn_profile_collect.argtypes = [c_void_p, POINTER(ctypes.c_double), POINTER(c_int64), c_int]
    lib.bn_ingest_resample.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int64, c_int64,
                                       c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_ingest_resample_span.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                            c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_ingest_chunks.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                     c_void_p]
    lib.bn_pool_scores.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]
    lib.bn_mel_spectrogram.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                       ctypes.c_double, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_blob_check.argtypes = [c_char_p, c_size_t]
    lib.bn_debug_requant.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.bn_set_option.argtypes = [c_char_p, c_int]
    lib.bn_get_option.argtypes = [c_char_p, POINTER(c_int)]
    lib.bn_ctx_set_option.argtypes = [c_void_p, c_char_p, c_int]
    lib.bn_ctx_get_option.argtypes = [c_void_p, c_char_p, POINTER(c_int)]
    lib.bn_ctx_reset_options.argtypes = [c_void_p]
    lib.bn_preload_kernels.argtypes = [c_void_p]
    lib.bn_rank_orders.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_short_time_energy.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.bn_activity_counts.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p]
    lib.bn_search_inv_norms.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p]
    lib.bn_search_topk.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_kmeans_assign.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]
    lib.bn_kmeans_accumulate.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_kmeans_centroids.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_silhouette_means.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p]
    lib.bn_density_nearest.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_tsne_perplexity.argtypes = [c_void_p, c_void_p, c_int64, c_int, ctypes.c_double, c_void_p, c_void_p, c_void_p]
    lib.bn_tsne_gradient.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_tsne_update.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p]
    lib.bn_propagate_step.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p]
    lib.bn_propagate_decide.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_select_run.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.bn_acoustic_indices.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_pca_colsum.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p]
    lib.bn_pca_gram.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_pca_transform.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    u64 = ctypes.c_uint64
    lib.bn_bootstrap_rejections.argtypes = [c_void_p, u64, u64, u64, u64, ctypes.c_uint32, c_int64, c_int64, c_void_p, c_int64, POINTER(c_int64), c_void_p]
    lib.bn_bootstrap_counts.argtypes = [c_void_p, u64, u64, u64, u64, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_bootstrap_ap.argtypes = [c_void_p, u64, u64, u64, u64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_augment_inputs.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64,
                                      c_void_p, c_void_p]
    lib.bn_host_alloc_pinned.argtypes = [c_void_p, ctypes.c_size_t]
    lib.bn_host_alloc_pinned.restype = c_void_p
    lib.bn_host_free_pinned.argtypes = [c_void_p]
    lib.bn_head_forward.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.bn_head_i8_forward.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_float,
                                       c_void_p, c_void_p, c_void_p]
    lib.bn_head_i8_pass_classes.argtypes = [c_int, c_int]
    lib.bn_probe_create.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, ctypes.c_uint32, c_int64,
                                    c_void_p, c_void_p, POINTER(c_void_p), c_void_p]
    lib.bn_probe_destroy.argtypes = [c_void_p]
    lib.bn_probe_destroy.restype = None
    lib.bn_probe_epoch.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]
    lib.bn_probe_loss.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
    lib.bn_probe_get.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_set.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_sweep_create.argtypes = [c_void_p, c_int, c_int, c_int, c_int, POINTER(ProbeTrialStruct), ctypes.c_uint32, c_int64, c_void_p, c_void_p,
                                          POINTER(c_void_p), c_void_p]
    lib.bn_probe_sweep_destroy.argtypes = [c_void_p]
    lib.bn_probe_sweep_destroy.restype = None
    lib.bn_probe_sweep_epoch.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_sweep_loss.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_sweep_snapshot.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.bn_probe_sweep_get.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_set_loss.argtypes = [c_void_p, c_int, c_float]
    lib.bn_probe_epoch_weighted.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]
    lib.bn_probe_sweep_set_loss.argtypes = [c_void_p, c_int, c_float]
    lib.bn_probe_set_qat.argtypes = [c_void_p, c_int, c_int, c_float, c_int]
    lib.bn_probe_get_quantized.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.bn_probe_scores.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_mlp_create.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, ctypes.c_uint32, c_int64,
                                        c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), c_void_p]
    lib.bn_probe_mlp_destroy.argtypes = [c_void_p]
    lib.bn_probe_mlp_destroy.restype = None
    lib.bn_probe_mlp_set_loss.argtypes = [c_void_p, c_int, c_float]
    lib.bn_probe_mlp_epoch_weighted.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]
    lib.bn_probe_mlp_loss.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
    lib.bn_probe_mlp_get.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_probe_mlp_set.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.bn_head_mlp_forward.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.bn_probe_sweep_epoch_weighted.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    if lib.bn_version() != ABI_VERSION:
        raise RuntimeError(f"libbirdnet_hip ABI {lib.bn_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load_library().bn_last_error()
        raise HipError(f"libbirdnet_hip error {rc}: {msg.decode('utf-8', 'replace') if msg else ''}")


def blob_check(blob: bytes) -> None:
    """``bn_blob_check``: raise :class:`HipError` unless ``blob`` is a well-formed plan (host only, no device needed)."""
    check(load_library().bn_blob_check(blob, len(blob)))


def set_option(name: str, value: int) -> None:
    """``bn_set_option``: process-wide launcher switch (A/B runs, tests)."""
    check(load_library().bn_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = c_int()
    check(load_library().bn_get_option(name.encode(), byref(v)))
    return int(v.value)


class options:
    """``with options(i8_strip=0, i8_strip_th=3): ...`` — set launcher switches, restore the previous values on exit."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def loaded_hip_runtimes() -> list[str]:
    """Paths of every libamdhip64 mapped in this process (must be exactly one)."""
    seen = set()
    with open("/proc/self/maps") as fh:
        for line in fh:
            if "libamdhip64" in line:
                seen.add(line.split()[-1])
    return sorted(seen)


class Context:
    """Owns a ``bn_ctx`` on one device."""

    def __init__(self, device: int = 0, max_batch: int = 1024):
        self.lib = load_library()
        self.device, self.max_batch = int(device), int(max_batch)
        h = c_void_p()
        check(self.lib.bn_ctx_create(self.device, self.max_batch, byref(h)))
        self.handle = h
        rts = loaded_hip_runtimes()
        if len(rts) != 1:
            raise RuntimeError(f"expected one HIP runtime in the process, found {rts}")

    def set_option(self, name: str, value: int) -> None:
        """``bn_ctx_set_option``: a launcher switch for this context only (``set_option`` of the module sets the process default)."""
        check(self.lib.bn_ctx_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        """The value the launches through this context see: its own override, else the process default."""
        v = c_int()
        check(self.lib.bn_ctx_get_option(self.handle, name.encode(), byref(v)))
        return v.value

    def reset_options(self) -> None:
        check(self.lib.bn_ctx_reset_options(self.handle))

    def alloc_pinned(self, nbytes: int) -> int:
        """Address of ``nbytes`` of page-locked host memory (``bn_host_alloc_pinned``; the GIL is released for the call); free with ``free_pinned``."""
        p = self.lib.bn_host_alloc_pinned(self.handle, int(nbytes))
        if not p:
            raise HipError(f"bn_host_alloc_pinned({nbytes}): {self.lib.bn_last_error().decode()}")
        return int(p)

    def free_pinned(self, ptr: int) -> None:
        check(self.lib.bn_host_free_pinned(c_void_p(int(ptr))))

    def preload_kernels(self) -> None:
        """Load every device code object of the library now instead of at each kernel's first launch (``bn_preload_kernels``)."""
        check(self.lib.bn_preload_kernels(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.bn_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


class Model:
    """Owns a ``bn_model`` (constants in HBM + activation workspace)."""

    def __init__(self, ctx: Context, blob: bytes):
        self.ctx = ctx
        self.lib = ctx.lib
        h = c_void_p()
        check(self.lib.bn_model_load(ctx.handle, blob, len(blob), byref(h)))
        self.handle = h
        info = BnModelInfo()
        check(self.lib.bn_model_get_info(h, byref(info)))
        self.info = info

    def close(self):
        if getattr(self, "handle", None):
            self.lib.bn_model_free(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


__all__ = ["load_library", "check", "Context", "Model", "HipError", "BnModelInfo", "EXPORTS", "LIB_PATH", "c_float", "set_option", "get_option",
           "options", "OPTION_NAMES", "SCHEDULING_OPTION_NAMES"]
