"""``analyze`` on the GPU: span resampling of windows the one-shot resampler refuses, streamed files through ``detect_files`` against
the host path, streaming against the grouped path, and the CLI end to end.  Every file is synthesised into ``tmp_path``."""

from __future__ import annotations

import csv
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 22050


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; there is no CPU fallback to fall back to")
    return torch


def _write_wav(path, x, sr, bits=16, code=1):
    """``x`` [n, ch] integers (PCM) or floats (code 3) as a RIFF/WAVE file."""
    ch = x.shape[1]
    if code == 3:
        payload = x.astype("<f4").tobytes()
    elif bits == 24:
        v = x.astype(np.int32)
        payload = np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=-1).astype(np.uint8).tobytes()
    else:
        payload = x.astype("<i2").tobytes()
    fmt = struct.pack("<4sIHHIIHH", b"fmt ", 16, code, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4sI4s", b"RIFF", 36 + len(payload), b"WAVE") + fmt + struct.pack("<4sI", b"data", len(payload)) + payload)


def _field_signal(n, sr, seed):
    """Chirps, tones, noise and silence, in [-1, 1)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = np.zeros(n)
    seg = max(1, n // 8)
    for k in range(8):
        a, b = k * seg, min(n, (k + 1) * seg)
        tt = t[a:b] - t[a]
        kind = k % 4
        if kind == 0:
            x[a:b] = 0.5 * np.sin(2 * np.pi * (1500 + 3000 * tt / max(tt[-1], 1e-9)) * tt)   # chirp
        elif kind == 1:
            x[a:b] = 0.3 * np.sin(2 * np.pi * 3100 * tt) + 0.2 * np.sin(2 * np.pi * 5200 * tt)
        elif kind == 2:
            x[a:b] = 0.2 * rng.standard_normal(b - a)
        # kind 3: silence
    x[: n // 50] += 0.05 * rng.standard_normal(n // 50)
    return np.clip(x, -0.99, 0.99)


def _host_scores(runner, paths, torch):
    from birdnet_stm32.audio import io

    parts = []
    for p in paths:
        chunks = io.load_audio_file(p, SR, 0, 3.0)
        if len(chunks):
            parts.append(runner.infer_audio_device(torch.from_numpy(np.asarray(chunks, np.float32)).cuda()).cpu().numpy())
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def twelve_minutes(tmp_path_factory):
    """12 minutes of 48 kHz mono PCM16: bn_ingest_resample refuses the window (its 32-bit polyphase index)."""
    n = 12 * 60 * 48000
    pcm = np.clip(np.rint(_field_signal(n, 48000, 12) * 32767), -32768, 32767).astype(np.int16)
    p = tmp_path_factory.mktemp("long") / "twelve.wav"
    _write_wav(str(p), pcm[:, None], 48000)
    return str(p), pcm


def test_span_resampling_of_a_window_the_one_shot_path_refuses(torch_mod, twelve_minutes):
    from scipy.signal import resample_poly

    from birdnet_stm32 import _hip
    from birdnet_stm32.audio.ingest import polyphase_filter, resampled_length
    from birdnet_stm32.audio.pipeline import filter_geometry, plan_segments

    torch = torch_mod
    _path, pcm = twelve_minutes
    ctx = _hip.Context(0, 64)
    lib = ctx.lib
    up, down, hpp, pre = filter_geometry(48000, SR)
    taps = polyphase_filter(up, down)[0]
    n_in = pcm.shape[0]
    n_out = resampled_length(n_in, up, down)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_taps = torch.from_numpy(taps).cuda()
    mono = torch.full((n_out,), float("nan"), dtype=torch.float32, device="cuda")
    peak = torch.zeros(1, dtype=torch.float32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_off = torch.tensor([0, n_in], dtype=torch.int64, device="cuda")
    d_out = torch.tensor([0, n_out], dtype=torch.int64, device="cuda")
    rc = lib.bn_ingest_resample(ctx.handle, d_pcm.data_ptr(), 0, 1, d_off.data_ptr(), d_out.data_ptr(), 1, n_in, n_out, d_taps.data_ptr(), up, down,
                                hpp, pre, mono.data_ptr(), peak.data_ptr(), stream)
    assert rc != 0, "the one-shot resampler took a window past its 32-bit index"
    segs = plan_segments(n_in, n_out, up, down, hpp, pre, 2, 9 << 20)
    assert len(segs) >= 6
    o0, o1, s0, s1 = segs[2]
    # staged frames that miss the filter's halo are refused with BN_ERR_ARG, nothing launched
    assert lib.bn_ingest_resample_span(ctx.handle, d_pcm.data_ptr() + 2 * (s0 + 1), 0, 1, s0 + 1, s1 - s0 - 1, n_in, o0, o1, d_taps.data_ptr(), up, down,
                                       hpp, pre, mono.data_ptr(), peak.data_ptr(), stream) == -1
    assert b"need input frames" in lib.bn_last_error()
    for o0, o1, s0, s1 in segs:
        _hip.check(lib.bn_ingest_resample_span(ctx.handle, d_pcm.data_ptr() + 2 * s0, 0, 1, s0, s1 - s0, n_in, o0, o1, d_taps.data_ptr(), up, down,
                                               hpp, pre, mono.data_ptr(), peak.data_ptr(), stream))
    torch.cuda.synchronize()
    want = resample_poly(pcm.astype(np.float32) / np.float32(32768.0), up, down).astype(np.float32)
    got = mono.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert peak.cpu().numpy()[0] == np.abs(want).max()
    ctx.close()


@pytest.mark.parametrize("model_path", [TFLITE_PATH, KERAS_PATH])
def test_detect_files_on_twelve_minutes_equals_host_ingest(torch_mod, twelve_minutes, model_path):
    from birdnet_stm32.evaluation.detections import detect_files
    from birdnet_stm32.models.runners import load_model_runner

    path, _pcm = twelve_minutes
    runner = load_model_runner(model_path, max_batch=128)
    det = detect_files(runner, [path], min_conf=0.0, return_scores=True, sample_rate=SR, chunk_duration=3.0)
    want = _host_scores(runner, [path], torch_mod)
    assert det.scores.shape == want.shape == (240, runner.num_classes)
    assert np.array_equal(det.scores, want)
    assert det.chunks_per_file.tolist() == [240] and det.duration_s[0] == pytest.approx(720.0)
    assert len(det) == 240 * runner.num_classes   # min_conf 0: every score is a detection
    runner.close()


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """Files that a 1-4 MiB slab mostly streams, in an order that interleaves streamed and grouped files."""
    import flac_writer as fw

    d = tmp_path_factory.mktemp("mixed")
    paths = []

    def add(name, sr, seconds, ch=1, bits=16, code=1, seed=0):
        n = int(sr * seconds)
        x = np.stack([_field_signal(n, sr, seed + c) for c in range(ch)], axis=1)
        if code == 3:
            data = x.astype(np.float32)
        else:
            data = np.clip(np.rint(x * (2 ** (bits - 1) - 1)), -(2 ** (bits - 1)), 2 ** (bits - 1) - 1).astype(np.int32)
        p = str(d / name)
        _write_wav(p, data, sr, bits, code)
        paths.append(p)

    add("stereo44k_5min.wav", 44100, 300, ch=2, seed=1)    # decimate kernel (44.1 -> 22.05 kHz)
    add("short.wav", 48000, 1.2, seed=2)                   # shorter than one chunk
    add("s24_48k.wav", 48000, 40, ch=2, bits=24, seed=3)   # generic kernel
    add("same_rate.wav", SR, 70, seed=4)                   # no resampling
    bad = d / "broken.wav"
    bad.write_bytes(b"RIFF\x10\x00\x00\x00WAVEjunkjunk")
    paths.append(str(bad))
    add("f32_32k.wav", 32000, 60, code=3, bits=32, seed=5)
    add("phase_11k.wav", 11025, 100, seed=6)               # phase kernel (up 2, 21 taps per phase)
    add("r96k.wav", 96000, 12, seed=7)                      # generic kernel, 147/640
    n = 16000 * 40
    x = np.clip(np.rint(_field_signal(n, 16000, 8) * 20000), -32768, 32767).astype(np.int64)[:, None]
    frames = [{"n": 4096, "mode": "indep", "sub": [dict(kind="fixed", order=2, po=3)]} for _ in range(n // 4096)]
    frames.append({"n": n % 4096, "mode": "indep", "sub": [dict(kind="fixed", order=1, po=0)]})
    (d / "mono16k.flac").write_bytes(fw.encode(x, 16000, 16, frames))
    paths.append(str(d / "mono16k.flac"))
    add("tail.wav", 24000, 9.5, seed=9)
    return paths


def test_streaming_does_not_change_scores(torch_mod, mixed):
    from birdnet_stm32.audio.pipeline import long_files, plan_files
    from birdnet_stm32.evaluation.detections import detect_files
    from birdnet_stm32.models.runners import load_model_runner

    runner = load_model_runner(TFLITE_PATH, max_batch=96)
    tab = plan_files(mixed, SR, 3.0, 0.0, 0)
    assert long_files(tab, SR, 1 << 20).sum() >= 6 and not long_files(tab, SR, 256 << 20).any()
    base = detect_files(runner, mixed, min_conf=0.1, return_scores=True)
    assert base.skipped == [mixed[4]] and base.chunks_per_file[4] == 0 and base.chunks_per_file[1] == 1
    for opts in (dict(slab_bytes=1 << 20, readers=3), dict(slab_bytes=3 << 20, group_chunks=50), dict(slab_bytes=4 << 20, pinned_slabs=2)):
        got = detect_files(runner, mixed, min_conf=0.1, return_scores=True, pipeline_options=opts)
        assert got.chunks_per_file.tolist() == base.chunks_per_file.tolist()
        assert np.array_equal(got.scores, base.scores), opts
        assert np.array_equal(got.class_index, base.class_index) and np.array_equal(got.score, base.score)
    want = _host_scores(runner, mixed, torch_mod)
    assert np.array_equal(base.scores, want)
    runner.close()


def test_mono_budget_refuses_before_reading(torch_mod, twelve_minutes):
    from birdnet_stm32.evaluation.detections import detect_files
    from birdnet_stm32.models.runners import load_model_runner

    runner = load_model_runner(TFLITE_PATH, max_batch=32)
    with pytest.raises(ValueError, match="budget"):
        detect_files(runner, [twelve_minutes[0]], pipeline_options=dict(mono_budget_bytes=1 << 20))
    runner.close()


def test_analyze_cli_outputs_agree_with_its_npz(torch_mod, mixed, tmp_path):
    from birdnet_stm32.evaluation import detections as D
    from birdnet_stm32.training.config import ModelConfig

    names = ModelConfig.load(CONFIG_PATH).to_dict()["class_names"]
    inputs = [mixed[1], mixed[2], mixed[4], mixed[8]]
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "birdnet-stm32_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "analyze", "--model_path", TFLITE_PATH, "--input", *inputs, "--output", str(out),
                        "--format", "csv", "raven", "npz", "--min_conf", "0.05", "--top_k", "3", "--max_batch", "256"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "detections.npz")
    assert z["paths"].tolist() == inputs and z["class_names"].tolist() == names
    rows, cls = D.select(z["scores"], np.full(len(names), 0.05, np.float32), 3)
    want = [(inputs[int(z["file_index"][i])], float(z["start_s"][i]), float(z["end_s"][i]), int(c), np.float32(z["scores"][i, c])) for i, c in zip(rows, cls)]
    assert want
    table = list(csv.reader(open(out / "detections.csv")))[1:]
    assert len(table) == len(want)
    for row, (p, a, b, c, s) in zip(table, want):
        assert row[0] == p and int(row[5]) == c and np.float32(float(row[6])) == s
        assert float(row[1]) == pytest.approx(a, abs=1e-6) and float(row[2]) == pytest.approx(b, abs=1e-6)
        assert (row[3], row[4]) == D.split_name(names[c])
    tables = sorted(os.listdir(out / "raven"))
    assert len(tables) == 3   # one per analysed file (the broken one has none)
    raven = []
    for t in D.raven_table_names([inputs[0], inputs[1], inputs[3]]):
        lines = open(out / "raven" / t).read().splitlines()
        assert lines[0].split("\t") == list(D.RAVEN_COLUMNS)
        raven += [ln.split("\t") for ln in lines[1:]]
    assert [(r_[10], float(r_[3]), r_[9]) for r_ in raven] == [(p, pytest.approx(a, abs=1e-6), row[6]) for (p, a, _b, _c, _s), row in zip(want, table)]
