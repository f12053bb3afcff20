"""Inference runners with the reference's ``predict(x_batch) -> [B, C]`` interface, on MI355X.

Drop-in for birdnet_stm32/models/runners.py (reference :14-114): ``load_model_runner(path)``
dispatches on the file suffix exactly as the reference does (``.tflite`` -> INT8 graph,
anything else -> Keras archive) and returns an object whose ``predict`` takes the same float32
batches (hybrid frontend: ``[B, 257, W, 1]`` normalised linear spectrograms) and returns fresh
float32 ``[B, C]`` arrays.  Instead of ``tf.lite.Interpreter`` / ``tf.keras`` the runner
lowers the file to a device plan and executes it through ``libbirdnet_hip.so``.

Beyond the reference interface the runner exposes device-resident entry points used by the
batched evaluator and the throughput benchmark:

* ``predict_device(x)``  — torch tensor in HBM -> torch tensor in HBM, no host copies;
* ``infer_audio_device(audio)`` — ``[B, T]`` waveform chunks in HBM -> scores, the STFT, frontend
  and network all on the GPU.

Like the reference's interpreter (``resize_tensor_input``), any batch size is accepted; batches
larger than the workspace are processed in slices.
"""

from __future__ import annotations

import ctypes

import numpy as np

from birdnet_stm32 import _hip
from birdnet_stm32.models import _pack as pk


class HipRunner:
    """Executes a lowered plan on one MI355X."""

    def __init__(self, plan: pk.Plan, device: int = 0, max_batch: int = 1024, ctx: "_hip.Context | None" = None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device visible: HipRunner has no CPU fallback")
        self._torch = torch
        self.plan = plan
        self.device = torch.device("cuda", device)
        self.ctx = ctx if ctx is not None else _hip.Context(device, max_batch)   # (load_model_runner creates it early when it prepares the pipeline)
        self.model = _hip.Model(self.ctx, plan.to_blob())
        self.lib = self.ctx.lib
        info = self.model.info
        self.max_batch = int(max_batch)
        self.num_classes = int(info.num_classes)
        self.input_elems = int(info.input_elems)
        self.fft_bins, self.spec_width = int(info.fft_bins), int(info.spec_width)
        self.dtype = "i8" if info.dtype == pk.DTYPE_I8 else "f32"
        self.input_kind = int(info.input_kind)
        self._precomputed: dict | None = None  # spectrogram settings of a precomputed-frontend model (configure_precomputed)

    # -- helpers ----------------------------------------------------------------------------
    def _stream(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _check_dev(self, t, name: str):
        torch = self._torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor")
        if t.device != self.device:
            raise ValueError(f"{name} lives on {t.device}, runner on {self.device}")

    # -- reference interface ------------------------------------------------------------------
    def predict(self, x_batch: np.ndarray) -> np.ndarray:
        """Forward pass on a host batch; same contract as the reference's runners (:29-45, :82-95)."""
        torch = self._torch
        x = np.ascontiguousarray(np.asarray(x_batch).astype(np.float32, copy=False))
        if x.ndim < 2 or int(np.prod(x.shape[1:])) != self.input_elems:
            want = f"[B, {self.fft_bins}, {self.spec_width}, 1]" if self.fft_bins else f"[B, {self.input_elems}, 1]"
            raise ValueError(f"expected input of shape {want}, got {x.shape}")
        B = x.shape[0]
        out = np.empty((B, self.num_classes), np.float32)
        for b0 in range(0, B, self.max_batch):
            xb = torch.from_numpy(x[b0 : b0 + self.max_batch].reshape(-1, self.input_elems)).to(self.device)
            out[b0 : b0 + xb.shape[0]] = self.predict_device(xb).cpu().numpy()
        return out

    def embed(self, x_batch: np.ndarray, dtype: str = "float32") -> np.ndarray:
        """Embeddings of a host batch (same input contract as :meth:`predict`): ``[B, D]`` float32, or int8 bytes on an INT8 model."""
        torch = self._torch
        x = np.ascontiguousarray(np.asarray(x_batch).astype(np.float32, copy=False))
        if x.ndim < 2 or int(np.prod(x.shape[1:])) != self.input_elems:
            want = f"[B, {self.fft_bins}, {self.spec_width}, 1]" if self.fft_bins else f"[B, {self.input_elems}, 1]"
            raise ValueError(f"expected input of shape {want}, got {x.shape}")
        D = self.embedding_info()["dim"]
        B = x.shape[0]
        out = np.empty((B, D), np.dtype(dtype))
        for b0 in range(0, B, self.max_batch):
            xb = torch.from_numpy(x[b0 : b0 + self.max_batch].reshape(-1, self.input_elems)).to(self.device)
            out[b0 : b0 + xb.shape[0]] = self.predict_device(xb, return_embeddings=True, emb_dtype=dtype)[1].cpu().numpy()
        return out

    def embedding_info(self) -> dict:
        """``{"dim", "dtype", "scale", "zero_point"}`` of the model's embedding (the pooled vector in front of the classifier head);
        ``dtype`` is the plan's native form ("int8" on INT8 models: ``(q - zero_point) * scale`` is the float32 form)."""
        dim, dt, zp, sc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
        _hip.check(self.lib.bn_model_get_embedding_info(self.model.handle, ctypes.byref(dim), ctypes.byref(dt), ctypes.byref(sc), ctypes.byref(zp)))
        return {"dim": int(dim.value), "dtype": "int8" if dt.value == _hip.EMB_I8 else "float32", "scale": float(sc.value), "zero_point": int(zp.value)}

    def _emb_buffer(self, B: int, emb_dtype: str, emb_out=None):
        """(tensor [B, D], BN_EMB_* code) for an embedding request: ``emb_out`` checked (the kernels write B x D values into it), or a new tensor."""
        torch = self._torch
        if emb_dtype not in ("float32", "int8"):
            raise ValueError(f"emb_dtype must be 'float32' or 'int8', not {emb_dtype!r}")
        D = self.embedding_info()["dim"]
        code = _hip.EMB_I8 if emb_dtype == "int8" else _hip.EMB_F32
        want = torch.int8 if code == _hip.EMB_I8 else torch.float32
        if emb_out is None:
            return torch.empty((B, D), dtype=want, device=self.device), code
        if not (isinstance(emb_out, torch.Tensor) and emb_out.device == self.device and emb_out.dtype == want and emb_out.is_contiguous()
                and tuple(emb_out.shape) == (B, D)):
            raise ValueError(f"emb_out must be a contiguous {want} tensor of shape ({B}, {D}) on {self.device}")
        return emb_out, code

    # -- device-resident interface --------------------------------------------------------------
    def predict_device(self, x, minmax=None, return_logits: bool = False, return_embeddings: bool = False, emb_dtype: str = "float32",
                       emb_out=None):
        """``x``: CUDA float32 ``[B, input_elems]`` (any trailing shape with that many elements).

        ``return_embeddings``: also return the ``[B, D]`` embeddings (``emb_dtype`` "float32", or "int8" on INT8 models; written into
        ``emb_out`` when given) as the last element of a tuple: ``(scores, emb)`` or ``(scores, logits, emb)``."""
        torch = self._torch
        self._check_dev(x, "x")
        B = x.shape[0]
        if x.numel() != B * self.input_elems:
            raise ValueError(f"input has {x.numel() // max(B, 1)} elements per chunk, model expects {self.input_elems}")
        scores = torch.empty((B, self.num_classes), dtype=torch.float32, device=self.device)
        logits = torch.empty_like(scores) if return_logits else None
        if minmax is not None:
            self._check_dev(minmax, "minmax")
        emb, code = (None, 0)
        if return_embeddings:
            emb, code = self._emb_buffer(B, emb_dtype, emb_out)
        with torch.cuda.device(self.device):
            for b0 in range(0, B, self.max_batch):
                nb = min(self.max_batch, B - b0)
                if emb is not None:
                    _hip.check(self.lib.bn_forward_embed(self.model.handle, x[b0:].data_ptr(), minmax[b0:].data_ptr() if minmax is not None else None, nb,
                                                         scores[b0:].data_ptr(), logits[b0:].data_ptr() if logits is not None else None,
                                                         emb[b0:].data_ptr(), code, self._stream()))
                    continue
                _hip.check(
                    self.lib.bn_forward(
                        self.model.handle,
                        x[b0:].data_ptr(),
                        minmax[b0:].data_ptr() if minmax is not None else None,
                        nb,
                        scores[b0:].data_ptr(),
                        logits[b0:].data_ptr() if logits is not None else None,
                        self._stream(),
                    )
                )
        if emb is not None:
            return (scores, logits, emb) if return_logits else (scores, emb)
        return (scores, logits) if return_logits else scores

    def configure_precomputed(self, audio_frontend: str, sample_rate: int, mag_scale: str = "none", n_fft: int = 512,
                              num_mels: int | None = None, n_mfcc: int = 20) -> None:
        """Tell a precomputed-frontend runner ('librosa' | 'log_mel' | 'mfcc') how its input spectrograms are made, so that
        ``infer_audio_device`` can start from waveforms.  The graph itself only passes the map through (reference:
        models/frontend.py:296-297); which host transform feeds it is a property of the training config
        (``audio_frontend``, ``mag_scale``, ``num_mels``, ``n_mfcc``: reference evaluation/metrics.py:49-54, data/generator)."""
        from birdnet_stm32.models.frontend import normalize_frontend_name

        name = normalize_frontend_name(audio_frontend)
        if name not in ("librosa", "log_mel", "mfcc"):
            raise ValueError(f"'{audio_frontend}' is not a precomputed frontend")
        if self.input_kind != pk.INPUT_MEL:
            raise ValueError("this model does not take precomputed spectrograms")
        rows = self.input_elems // self.spec_width
        mels = int(num_mels) if num_mels is not None else rows
        if (n_mfcc if name == "mfcc" else mels) != rows:
            raise ValueError(f"model input has {rows} rows; frontend '{name}' with num_mels={mels}, n_mfcc={n_mfcc} does not produce that")
        self._precomputed = {"mode": {"librosa": "mel", "log_mel": "log_mel", "mfcc": "mfcc"}[name], "sample_rate": int(sample_rate),
                             "mag_scale": mag_scale if name == "librosa" else "none", "n_fft": int(n_fft), "mel_bins": mels, "n_mfcc": int(n_mfcc)}

    def model_inputs_device(self, audio, hop: int | None = None):
        """``audio``: CUDA float32 ``[B, T]`` chunks -> the model inputs ``[B, input_elems]`` that ``predict_device`` takes: what
        ``infer_audio_device`` computes in front of the network, kept (``evaluation.embeddings.embed_files(keep_inputs=True)``, the
        augmented probe fit).  Hybrid models: the normalised STFT magnitudes (``stft_device``); the fused audio path of
        ``infer_audio_device`` forms the same map inside its kernels, rounded its own way on float32 plans."""
        torch = self._torch
        self._check_dev(audio, "audio")
        if self.input_kind == pk.INPUT_MEL:
            if self._precomputed is None:
                raise ValueError("precomputed-frontend model: call configure_precomputed(audio_frontend, sample_rate, mag_scale, ...) first")
            from birdnet_stm32.audio.spectrogram import mel_spectrograms_device

            c = self._precomputed
            spec = mel_spectrograms_device(self.ctx, audio, c["sample_rate"], c["n_fft"], c["mel_bins"], self.spec_width, c["mag_scale"],
                                           c["mode"], c["n_mfcc"])
            return spec.view(spec.shape[0], -1)
        if self.input_kind == pk.INPUT_WAVEFORM:
            # raw frontend: the model input is the chunk divided by (its peak + 1e-6) (reference: evaluation/metrics.py:62-69)
            if audio.shape[1] != self.input_elems:
                raise ValueError(f"raw-frontend model expects {self.input_elems} samples per chunk, got {audio.shape[1]}")
            x = torch.empty_like(audio)
            with torch.cuda.device(self.device):
                _hip.check(self.lib.bn_chunk_peak_normalize(self.ctx.handle, audio.data_ptr(), audio.shape[0], audio.shape[1], 1e-6,
                                                            x.data_ptr(), self._stream()))
            return x
        spec = self.stft_device(audio, hop=hop, normalize=True)
        return spec.view(spec.shape[0], -1)

    def input_shape(self) -> tuple[int, int]:
        """``(F, W)`` of a model-input row as the augmentation sees it: ``(1, T)`` for the raw frontend, else ``(rows, spec_width)``."""
        if self.input_kind == pk.INPUT_WAVEFORM:
            return 1, int(self.input_elems)
        return int(self.input_elems) // int(self.spec_width), int(self.spec_width)

    def infer_audio_device(self, audio, hop: int | None = None, return_logits: bool = False, out=None, return_embeddings: bool = False,
                           emb_dtype: str = "float32", emb_out=None):
        """``audio``: CUDA float32 ``[B, T]`` chunks -> scores ``[B, C]`` (STFT + frontend + network on the GPU).

        ``return_embeddings``: as in :meth:`predict_device` — the result is ``(scores, emb)`` or ``(scores, logits, emb)``; ``emb_out``
        (``[B, D]`` CUDA tensor of ``emb_dtype``) receives the embeddings in place when given."""
        torch = self._torch
        self._check_dev(audio, "audio")
        kw = dict(return_embeddings=True, emb_dtype=emb_dtype, emb_out=emb_out) if return_embeddings else {}
        if self.input_kind in (pk.INPUT_MEL, pk.INPUT_WAVEFORM):
            res = self.predict_device(self.model_inputs_device(audio), return_logits=return_logits, **kw)
            if out is not None:
                out.copy_(res[0] if isinstance(res, tuple) else res)
            return res
        B, T = audio.shape
        hop = int(hop) if hop is not None else T // self.spec_width
        scores = out if out is not None else torch.empty((B, self.num_classes), dtype=torch.float32, device=self.device)
        logits = torch.empty_like(scores) if return_logits else None
        emb, code = (None, 0)
        if return_embeddings:
            emb, code = self._emb_buffer(B, emb_dtype, emb_out)
        with torch.cuda.device(self.device):
            for b0 in range(0, B, self.max_batch):
                nb = min(self.max_batch, B - b0)
                if emb is not None:
                    _hip.check(self.lib.bn_infer_audio_embed(self.model.handle, audio[b0:].data_ptr(), nb, T, hop, scores[b0:].data_ptr(),
                                                             logits[b0:].data_ptr() if logits is not None else None, emb[b0:].data_ptr(), code,
                                                             self._stream()))
                    continue
                _hip.check(
                    self.lib.bn_infer_audio(
                        self.model.handle, audio[b0:].data_ptr(), nb, T, hop, scores[b0:].data_ptr(),
                        logits[b0:].data_ptr() if logits is not None else None, self._stream(),
                    )
                )  # fmt: skip
        if emb is not None:
            return (scores, logits, emb) if return_logits else (scores, emb)
        return (scores, logits) if return_logits else scores

    def stft_device(self, audio, n_fft: int = 512, hop: int | None = None, spec_width: int | None = None, normalize: bool = True,
                    exact: bool = False):
        """Batched ``get_spectrogram_from_audio(mel_bins=-1)`` on the GPU: ``[B, T]`` -> ``[B, n_fft//2+1, W]``."""
        return stft_device(self.ctx, audio, n_fft, hop, spec_width or self.spec_width, normalize, exact=exact)

    def op_output(self, op_index: int, B: int) -> np.ndarray:
        """Test hook: activation written by plan operator ``op_index`` in the last forward call."""
        torch = self._torch
        op = self.plan.ops[op_index]
        per = ctypes.c_size_t()
        _hip.check(self.lib.bn_debug_op_output(self.model.handle, op_index, B, None, 0, ctypes.byref(per), None))
        buf = torch.empty((B, per.value), dtype=torch.uint8, device=self.device)
        _hip.check(self.lib.bn_debug_op_output(self.model.handle, op_index, B, buf.data_ptr(), buf.numel(), ctypes.byref(per), self._stream()))
        torch.cuda.synchronize(self.device)
        # activations are densely packed [B][elements]; the slot's bytes_per_chunk is only its capacity
        raw = buf.cpu().numpy().reshape(-1)
        n = int(np.prod(op.out_shape))
        dt = np.dtype(op.out_dtype)
        return raw[: B * n * dt.itemsize].copy().view(dt).reshape(B, *op.out_shape)

    def input_bytes(self, B: int) -> np.ndarray:
        """Test hook: the int8 bytes QUANTIZE made of the spectrograms of the last ``infer_audio_device`` call, ``[B, 257, W]``."""
        torch = self._torch
        out = torch.empty((B, self.fft_bins, self.spec_width), dtype=torch.int8, device=self.device)
        _hip.check(self.lib.bn_debug_input_bytes(self.model.handle, B, out.data_ptr(), self._stream()))
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy()

    def guard_stats(self, B: int) -> dict:
        """Test hook: counters of the exactness pass of the last ``infer_audio_device`` call (INT8 plans)."""
        out = (ctypes.c_int64 * 8)()
        _hip.check(self.lib.bn_debug_guard_stats(self.model.handle, B, out))
        return {"listed": int(out[0]), "listed_max": int(out[1]), "dirty_blocks": int(out[2]), "whole_minmax": int(out[3]), "whole_fix": int(out[4]),
                "audited": int(out[5]), "audit_violations": int(out[6]), "interval_min": int(out[7])}

    def tail_form(self) -> tuple[int, int]:
        """Test hook: (form, LDS bytes) of the fused INT8 tail operator this plan can run — 0 none, 1 ``i8_tail_kernel``, 2 also
        ``i8_tail2_kernel`` (depthwise stage on the matrix cores)."""
        form, lds = ctypes.c_int(0), ctypes.c_int(0)
        _hip.check(self.lib.bn_debug_tail_form(self.model.handle, ctypes.byref(form), ctypes.byref(lds)))
        return form.value, lds.value

    def mid_form(self) -> tuple[int, int]:
        """Test hook: (1, LDS bytes) when the plan's fused stage-2 chain (``i8_mid2_kernel``) passed the library's LDS plan, else (0, 0)."""
        form, lds = ctypes.c_int(0), ctypes.c_int(0)
        _hip.check(self.lib.bn_debug_mid_form(self.model.handle, ctypes.byref(form), ctypes.byref(lds)))
        return form.value, lds.value

    def satpack_form(self) -> tuple[int, int, int]:
        """Test hook: the requantisation tail of (``i8_mid2_kernel``, ``i8_tail2_kernel``, the stem rows of ``i8_front_strip_kernel``) in this
        plan — 1 the packed shift-and-saturate form (every clamp in front of a stored byte is the int8 range), 0 the clamp-shift-pack form,
        -1 the plan does not run that kernel."""
        mid, tail, front = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _hip.check(self.lib.bn_debug_satpack_form(self.model.handle, ctypes.byref(mid), ctypes.byref(tail), ctypes.byref(front)))
        return mid.value, tail.value, front.value

    def mid_plan(self) -> dict | None:
        """Test hook: the resident LDS placement of the fused stage-2 chain (option ``i8_mid_split``), ``None`` where the plan has none.
        ``parts`` = (offset, bytes) of every block's depthwise part, pointwise part and zero-point row."""
        out = (ctypes.c_int * 64)()
        _hip.check(self.lib.bn_debug_mid_plan(self.model.handle, out, 64))
        if not out[0]:
            return None
        parts = [(out[5 + 6 * i + 2 * k], out[6 + 6 * i + 2 * k]) for i in range(out[4]) for k in range(3) if out[6 + 6 * i + 2 * k]]
        return {"lds_bytes": out[1], "map_bytes": out[2], "bar_off": out[3], "blocks": out[4], "parts": parts}

    def mid_split_giveups(self) -> int:
        """Test hook: chunk barriers of ``i8_mid2_kernel`` whose bounded wait ran out since the library was loaded (0 in a working build)."""
        n = ctypes.c_int64(0)
        _hip.check(self.lib.bn_debug_mid_split_giveups(self.ctx.handle, ctypes.byref(n)))
        return int(n.value)

    # -- per-operator timing (HIP events on the launch stream) ------------------------------------
    def profile(self, enable: bool) -> None:
        _hip.check(self.lib.bn_profile_enable(self.model.handle, int(bool(enable))))

    def profile_only(self, op_index: int) -> None:
        """Bracket only operator ``op_index`` with events (-1: all operators again)."""
        _hip.check(self.lib.bn_profile_only(self.model.handle, int(op_index)))

    def profile_collect(self) -> list[dict]:
        """Elapsed time per plan operator since the last collect; behind the operators: the STFT stage and (INT8 plans from audio)
        the two float64 passes of the exactness pass (csrc/bn_stft_exact.hip)."""
        n = len(self.plan.ops) + 3
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        _hip.check(self.lib.bn_profile_collect(self.model.handle, ms, cnt, n))
        rows = []
        for i in range(n):
            if i < len(self.plan.ops):
                op = self.plan.ops[i]
                rows.append({"op": i, "kind": pk.KIND_NAMES[op.kind], "name": op.name, "ms": ms[i], "launches": int(cnt[i]), "p": list(op.p)})
            else:
                kind, name = (("stft512", "stft"), ("stft_minmax_exact", "exact min/max"), ("stft512_f64_list", "float64 pass + redo"))[i - len(self.plan.ops)]
                rows.append({"op": i, "kind": kind, "name": name, "ms": ms[i], "launches": int(cnt[i]), "p": []})
        return rows

    def close(self):
        import sys

        pl = sys.modules.get("birdnet_stm32.audio.pipeline")
        if pl is not None:   # (a helper thread of prepare_for_evaluate may still be page-locking through this context)
            while pl._PREPARE:
                pl._PREPARE.pop().join()
        self.model.close()
        self.ctx.close()


def stft_device(ctx: _hip.Context, audio, n_fft: int = 512, hop: int | None = None, spec_width: int = 256, normalize: bool = True,
                return_minmax: bool = False, exact: bool = False):
    """``bn_stft_mag`` on CUDA tensors: float32 ``[B, T]`` -> float32 ``[B, n_fft//2+1, spec_width]``.

    ``exact=True`` calls ``bn_stft_mag_exact``: the reference's float64 arithmetic value for value (about ten times slower)."""
    import torch

    if not (audio.is_cuda and audio.dtype == torch.float32 and audio.is_contiguous() and audio.dim() == 2):
        raise ValueError("audio must be a contiguous float32 CUDA tensor [B, T]")
    B, T = audio.shape
    hop = int(hop) if hop is not None else T // spec_width
    spec = torch.empty((B, n_fft // 2 + 1, spec_width), dtype=torch.float32, device=audio.device)
    minmax = torch.empty((B, 2), dtype=torch.float32, device=audio.device)
    with torch.cuda.device(audio.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(audio.device).cuda_stream)
        fn = ctx.lib.bn_stft_mag_exact if exact else ctx.lib.bn_stft_mag
        _hip.check(fn(ctx.handle, audio.data_ptr(), B, T, n_fft, hop, spec_width, int(normalize), spec.data_ptr(), minmax.data_ptr(), stream))
    return (spec, minmax) if return_minmax else spec


def lower_model_file(model_path: str, keep_all: bool = False, frontend_norm: bool | None = None, fuse: bool = True) -> pk.Plan:
    """Read a `.tflite` or `.keras` file and lower it to a device plan (no GPU needed)."""
    if model_path.lower().endswith(".tflite"):
        from birdnet_stm32.models._lower_i8 import lower_i8
        from birdnet_stm32.models._tflite_reader import load_tflite

        return lower_i8(load_tflite(model_path), keep_all=keep_all, fuse=fuse)
    from birdnet_stm32.models._keras_loader import load_keras_archive
    from birdnet_stm32.models._lower_f32 import lower_f32

    return lower_f32(load_keras_archive(model_path, frontend_norm=frontend_norm), keep_all=keep_all, fuse=fuse)


def load_model_runner(model_path: str, device: int = 0, max_batch: int = 1024, keep_all: bool = False,
                      frontend_norm: bool | None = None, fuse: bool = True, prepare_pipeline: bool = False) -> HipRunner:
    """Load a `.keras` or `.tflite` model and return a runner with ``predict()`` (reference :98-114).

    ``prepare_pipeline``: the caller is going to ``evaluate`` files with this runner (the CLI does) — the context is created first and, while the
    model file is parsed and lowered, a helper thread loads the library's code objects and page-locks the evaluate pipeline's staging slabs
    (``audio.pipeline.prepare_for_evaluate``: 768 MiB of page-locked memory, kept until ``release_pinned_slabs()``)."""
    ctx = None
    if prepare_pipeline:
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device visible: HipRunner has no CPU fallback")
        from birdnet_stm32.audio.pipeline import prepare_for_evaluate

        ctx = _hip.Context(device, max_batch)
        prepare_for_evaluate(ctx, torch)
    plan = lower_model_file(model_path, keep_all=keep_all, frontend_norm=frontend_norm, fuse=fuse)
    return HipRunner(plan, device=device, max_batch=max_batch, ctx=ctx)
