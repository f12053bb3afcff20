"""The float32 STFT kernel's memory side (``csrc/bn_stft.hip``: 8-byte sample loads, 16-byte stores of the tile-major spectrogram, short
guard records read by ``stft_minmax_exact_kernel``) must change no result.

* Guarded INT8 path from audio against the oracle (float64 STFT -> QUANTIZE -> the C port of the TFLite kernels): every quantised input byte
  and every score, no tolerance, at three geometries — T = 72000 (hop 281), T = 66150 (hop 258, even) and T = 8448 (hop 33).  The last is the
  smallest that can go wrong: its odd frames 1, 3, 5, 7 hold a sample pair that straddles samples -1 / 0, frames 249, 251, 253, 255 one that
  straddles the chunk's last sample, and every frame from 249 on runs past the end.  Six chunks each (``stft_minmax_exact_kernel`` takes four
  per workgroup: one full, one partial): three tone + noise, silence, one scaled by 1e-3, one stationary pure tone whose candidate counts
  run into the record's cap.  The same under ``stft_minint=0`` (chunks with overflowing records as whole float64 spectrograms).
* The plain float32 results against the digests of the commit before the change (``tests/golden/stft_stores_parent.json``): the input bytes
  under ``stft_exact=0`` (no settling pass: any changed float flips bytes), ``stft_device(normalize=False)`` and
  ``mel_spectrograms_device`` — the three instantiations share the sample loads.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, TFLITE_PATH, synth_chunks

pytestmark = pytest.mark.gpu

SHAPES = {72000: 24000, 66150: 22050, 8448: 24000}   # T -> sample rate of the synthetic chunks it is cut from
PARENT = os.path.join(GOLDEN, "stft_stores_parent.json")


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


def chunks_for(T: int) -> np.ndarray:
    """Six chunks of T samples: 0-2 tone + noise, 3 silence, 4 quiet, 5 a stationary pure tone."""
    sr = SHAPES[T]
    x = synth_chunks(6, sr=sr, seed=91)[:, :T].copy()
    assert x.shape == (6, T)
    x[3] = 0.0
    x[4] *= 1e-3
    x[5] = np.sin(2 * np.pi * 440.0 * np.arange(T) / sr).astype(np.float32)
    return x


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def runner(torch_mod):
    from birdnet_stm32.models.runners import load_model_runner

    r = load_model_runner(TFLITE_PATH, max_batch=6)
    yield r
    r.close()


_oracle_cache: dict = {}


def oracle_for(T: int):
    """(input bytes [6, 257 * 256], scores) of the reference arithmetic; computed once per geometry."""
    if T not in _oracle_cache:
        from birdnet_stm32.models._tflite_reader import load_tflite
        from oracle import cport, stft

        if not (os.path.isfile(cport.I8_LIB) and os.path.isfile(cport.CPU_LIB)):
            pytest.fail("oracle/_build is missing: run __graft_entry__.build() (the checker of this test is the C port of the oracle)")
        model = load_tflite(TFLITE_PATH)
        S = np.stack([stft.hybrid_spectrogram(a, 512, 256) for a in chunks_for(T)])[..., None].astype(np.float32)
        assert S.shape == (6, 257, 256, 1)
        scores, env = cport.CpuInt8Program(model).invoke(S, return_all=True)
        _oracle_cache[T] = (env[model.ops[0].outputs[0]].reshape(6, -1).copy(), scores.copy())
    return _oracle_cache[T]


@pytest.mark.parametrize("T", list(SHAPES))
def test_guarded_path_gives_the_oracles_bytes_and_scores(torch_mod, runner, T):
    from birdnet_stm32 import _hip

    ref_q, ref_scores = oracle_for(T)
    audio = torch_mod.from_numpy(chunks_for(T)).cuda()
    for minint in (1, 0):
        with _hip.options(stft_minint=minint):
            scores = runner.infer_audio_device(audio).cpu().numpy()
            q = runner.input_bytes(6).reshape(6, -1)
            st = runner.guard_stats(6)
        bad = np.argwhere(q != ref_q)
        print(f"T={T} stft_minint={minint}: {len(bad)} differing input bytes, guard stats {st}")
        first = [(int(b), int(e) // 256, int(e) % 256) for b, e in bad[:8]]
        assert len(bad) == 0, f"T={T} stft_minint={minint}: {len(bad)} quantised input bytes differ from the oracle's, first (chunk, bin, frame) {first}"
        assert np.array_equal(scores, ref_scores), f"T={T} stft_minint={minint}: scores differ"
        if minint == 0:   # the pure tone's records overflow: with the interval minimum off it must have gone the whole-chunk way
            assert st["whole_minmax"] >= 1 and st["interval_min"] == 0


def parent_digests() -> dict:
    with open(PARENT) as fh:
        return json.load(fh)["sha256"]


def plain_float32_digests(torch_mod, runner, which: str, T: int) -> str:
    """The digests the golden file holds (tools of this test and of the script that recorded them on the parent build)."""
    from birdnet_stm32 import _hip
    from birdnet_stm32.audio.spectrogram import mel_spectrograms_device
    from birdnet_stm32.models.runners import stft_device

    x = chunks_for(T)
    if which == "input_bytes":
        with _hip.options(stft_exact=0):
            runner.infer_audio_device(torch_mod.from_numpy(x).cuda())
            return digest(runner.input_bytes(6))
    d = torch_mod.from_numpy(x[:3].copy()).cuda()
    if which == "stft":
        return digest(stft_device(runner.ctx, d, normalize=False).cpu().numpy())
    return digest(mel_spectrograms_device(runner.ctx, d).cpu().numpy())


DIGEST_CASES = [("input_bytes", T) for T in SHAPES] + [(w, T) for w in ("stft", "mel") for T in (8448, 72000)]


@pytest.mark.parametrize("which,T", DIGEST_CASES)
def test_plain_float32_results_are_the_parents(torch_mod, runner, which, T):
    want = parent_digests()[f"{which}_{T}"]
    got = plain_float32_digests(torch_mod, runner, which, T)
    assert got == want, f"{which} at T={T}: sha256 {got}, the parent build gave {want}"
