"""Weight fake-quantisation used by the reference's QAT fine-tuning (reference: birdnet_stm32/training/qat.py:30-61).

``fake_quantize_weights`` mirrors the reference's function: pure array arithmetic (asymmetric min/max grid of ``2**num_bits - 1``
steps per output channel, quantise then dequantise), which serves the conversion checks as the "what survives 8 bits" reference point.

The Keras callback around it fine-tunes the whole model.  Here the backbone is frozen and already INT8, so the part of it that applies
is the fine-tune of the probe head, and that lives in ``training/probe_qat.py`` (``fit_probe_qat``, ``probe --export_tflite
--qat_epochs``).  It does not use the grid of this file: the head's forward sees the symmetric int8 weights the exporter
writes (``conversion.quantize.quantize_weights``) and the logit grid of the exported tensor, so that the trained weights are the exported ones.
"""

from __future__ import annotations

import numpy as np


def fake_quantize_weights(w: np.ndarray, num_bits: int = 8, per_channel: bool = True, channel_axis: int = -1) -> np.ndarray:
    """Quantise-dequantise ``w`` on a ``[min, max]`` grid with ``2**num_bits - 1`` steps (per channel along ``channel_axis``)."""
    qmax = (1 << num_bits) - 1
    w = np.asarray(w)
    if per_channel and w.ndim > 1:
        axes = tuple(i for i in range(w.ndim) if i != channel_axis % w.ndim)
        lo = w.min(axis=axes, keepdims=True)
        hi = w.max(axis=axes, keepdims=True)
    else:
        lo, hi = w.min(), w.max()
    scale = np.maximum((hi - lo) / qmax, 1e-10)
    return (np.round((w - lo) / scale) * scale + lo).astype(np.float32)
