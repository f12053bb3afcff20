"""GPU: embeddings (the pooled vector in front of the classifier head) from every entry path, against the oracles.

INT8: the bytes equal the oracle's MEAN tensor (t127 of the shipped model) bit for bit, the float32 form equals numpy's
(q - zero_point) * scale in float32, and requesting embeddings leaves every score bit-identical.  Float32: within the float parity bars.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import KERAS_PATH, REPO, TFLITE_PATH, fixture_signals, synth_chunks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; there is no CPU fallback to fall back to")
    return torch


@pytest.fixture(scope="module")
def audio24():
    sig = fixture_signals(24000)
    return np.concatenate([synth_chunks(5), np.stack([sig["sine"], sig["noise"], sig["chirp"]])]).astype(np.float32)


@pytest.fixture(scope="module")
def oracle_specs(audio24):
    from oracle import stft

    return np.stack([stft.hybrid_spectrogram(a) for a in audio24])


@pytest.fixture(scope="module")
def oracle_i8(oracle_specs):
    from birdnet_stm32.models._tflite_reader import load_tflite
    from oracle.int8_graph import Int8Interpreter

    model = load_tflite(TFLITE_PATH)
    ref, env = Int8Interpreter(model).invoke(oracle_specs[..., None], return_all=True)
    t = model.tensors[127]
    return ref, env[127].reshape(len(oracle_specs), -1).astype(np.int8), float(np.float32(t.scale[0])), int(t.zero_point[0])


def _dequant(q, scale, zp):
    return (q.astype(np.int32) - np.int32(zp)).astype(np.float32) * np.float32(scale)


I8_FORMS = {"tail2": dict(), "tail1": dict(i8_tail_mfdw=0), "unfused_mean": dict(i8_tail=0)}


@pytest.mark.parametrize("form", list(I8_FORMS) + ["fuse_false"])
def test_i8_shipped_embeddings_bit_exact(torch_mod, audio24, oracle_specs, oracle_i8, form):
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.models.runners import load_model_runner

    ref_scores, ref_q, scale, zp = oracle_i8
    runner = load_model_runner(TFLITE_PATH, max_batch=16, fuse=form != "fuse_false")
    info = runner.embedding_info()
    assert info == {"dim": 256, "dtype": "int8", "scale": scale, "zero_point": zp}
    B = audio24.shape[0]
    audio = torch.from_numpy(audio24).cuda()
    spec = torch.from_numpy(oracle_specs.reshape(B, -1)).cuda()
    with _hip.options(**I8_FORMS.get(form, {})):
        for name, call, arg in (("audio", runner.infer_audio_device, audio), ("spectrogram", runner.predict_device, spec)):
            plain = call(arg).cpu().numpy()
            s8, e8 = call(arg, return_embeddings=True, emb_dtype="int8")
            s32, l32, e32 = call(arg, return_logits=True, return_embeddings=True)
            s8, e8, s32, e32 = s8.cpu().numpy(), e8.cpu().numpy(), s32.cpu().numpy(), e32.cpu().numpy()
            assert e8.dtype == np.int8 and e8.shape == (B, 256) and e32.dtype == np.float32
            assert np.array_equal(e8, ref_q), f"{form}/{name}: {int((e8 != ref_q).sum())} embedding bytes differ from the oracle's tensor 127"
            assert np.array_equal(e32, _dequant(ref_q, scale, zp)), f"{form}/{name}: float32 form"
            assert np.array_equal(plain, ref_scores) and np.array_equal(s8, plain) and np.array_equal(s32, plain), f"{form}/{name}: scores changed"
    runner.close()


@pytest.mark.parametrize("B", [1, 3, 5])
def test_i8_embeddings_ragged_groups(torch_mod, audio24, oracle_i8, B):
    torch = torch_mod
    from birdnet_stm32.models.runners import load_model_runner

    _ref, ref_q, _s, _z = oracle_i8
    runner = load_model_runner(TFLITE_PATH, max_batch=16)
    for off in (0, 8 - B):
        _scores, e8 = runner.infer_audio_device(torch.from_numpy(audio24[off : off + B]).cuda(), return_embeddings=True, emb_dtype="int8")
        assert np.array_equal(e8.cpu().numpy(), ref_q[off : off + B])
    runner.close()


def test_i8_embeddings_large_batches_and_host_slicing(torch_mod, audio24, oracle_i8):
    """4096 chunks in one call (the fused tail's groups over many workgroups) and a call above max_batch (the runner slices on the host)."""
    torch = torch_mod
    from birdnet_stm32.models.runners import load_model_runner

    _ref, ref_q, scale, zp = oracle_i8
    runner = load_model_runner(TFLITE_PATH, max_batch=4096)
    big = torch.from_numpy(audio24).cuda().repeat(512, 1)
    s, e = runner.infer_audio_device(big, return_embeddings=True)
    plain = runner.infer_audio_device(big)
    assert torch.equal(s, plain)
    assert np.array_equal(e.cpu().numpy(), np.tile(_dequant(ref_q, scale, zp), (512, 1)))
    runner.close()
    small = load_model_runner(TFLITE_PATH, max_batch=16)
    x = torch.from_numpy(audio24).cuda().repeat(5, 1)[:37]
    _s, e8 = small.infer_audio_device(x, return_embeddings=True, emb_dtype="int8")
    assert np.array_equal(e8.cpu().numpy(), np.tile(ref_q, (5, 1))[:37])
    small.close()


def test_host_embed_matches_device(torch_mod, oracle_specs, oracle_i8):
    from birdnet_stm32.models.runners import load_model_runner

    _ref, ref_q, scale, zp = oracle_i8
    runner = load_model_runner(TFLITE_PATH, max_batch=3)   # (8 chunks: three host slices)
    assert np.array_equal(runner.embed(oracle_specs[..., None], dtype="int8"), ref_q)
    assert np.array_equal(runner.embed(oracle_specs[..., None]), _dequant(ref_q, scale, zp))
    runner.close()


def test_f32_shipped_embeddings(torch_mod, oracle_specs):
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.models._keras_loader import load_keras_archive
    from birdnet_stm32.models.runners import load_model_runner
    from oracle import float_graph

    x = oracle_specs[..., None]
    B = x.shape[0]
    _s, _l, acts = float_graph.forward(load_keras_archive(KERAS_PATH), x, np.float64, return_all=True, return_logits=True)
    ref = acts["gap"].reshape(B, -1)
    fused = load_model_runner(KERAS_PATH, max_batch=16)
    plain = load_model_runner(KERAS_PATH, max_batch=16, fuse=False)
    d = torch.from_numpy(x.reshape(B, -1)).cuda()
    sf, ef = fused.predict_device(d, return_embeddings=True)
    sp, ep = plain.predict_device(d, return_embeddings=True)
    assert torch.equal(sf, fused.predict_device(d)) and torch.equal(sp, plain.predict_device(d))
    ef, ep = ef.cpu().numpy(), ep.cpu().numpy()
    assert ef.shape == (B, 256)
    for e in (ef, ep):
        assert np.abs(e - ref).max() / np.abs(ref).max() < 1e-5
    assert np.abs(ef - ep).max() / np.abs(ep).max() < 1e-5   # the fused kernel's GAP against the unfused plan's GAP slot
    with pytest.raises(_hip.HipError):
        fused.predict_device(d, return_embeddings=True, emb_dtype="int8")   # BN_ERR_ARG: float32 plans give float32
    fused.close()
    plain.close()


@pytest.mark.parametrize("kw", [dict(use_inverted_residual=False, use_se=True, embeddings_size=128, use_attention_pooling=True, class_activation="sigmoid"),
                                dict(use_se=True, embeddings_size=96)], ids=["ds_se_attnpool_emb", "ir_se_emb"])
def test_f32_topologies_against_the_oracle(torch_mod, oracle_specs, kw):
    from birdnet_stm32.models import build_model
    from birdnet_stm32.models._lower_f32 import lower_f32
    from birdnet_stm32.models.runners import HipRunner
    from oracle import float_graph

    args = dict(num_mels=64, spec_width=256, sample_rate=24000, chunk_duration=3, embeddings_size=256, num_classes=10, randomize_bn=True, seed=7)
    args.update(kw)
    spec = build_model("dscnn", **args)
    x = oracle_specs[:4, ..., None]
    _s, _l, acts = float_graph.forward(spec, x, np.float64, return_all=True, return_logits=True)
    plain = lower_f32(spec, fuse=False)
    ref = acts[plain.ops[plain.embedding.ops["input"]].name].reshape(4, -1)   # the pooling layer's output (GAP / attention pooling)
    for fuse in (True, False):
        runner = HipRunner(lower_f32(spec, fuse=fuse), max_batch=4)
        got = runner.embed(x)
        assert got.shape == (4, args["embeddings_size"]) == ref.shape
        assert np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12) < 5e-4
        runner.close()


@pytest.mark.parametrize("name", ["ds_se_emb_sigmoid", "ds_attnpool_sigmoid", "raw_pcen_ir_se"])
def test_own_int8_exports_against_the_oracle(torch_mod, name):
    from test_conversion import EXPORT_TOPOLOGIES, _export

    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models.runners import HipRunner
    from oracle.int8_graph import Int8Interpreter

    _spec, model, _raw, x = _export(EXPORT_TOPOLOGIES[name])
    ref, env = Int8Interpreter(model).invoke(x, return_all=True)
    B = x.shape[0]
    for fuse in (True, False):
        plan = lower_i8(model, fuse=fuse)
        e = plan.embedding
        mi = [i for i in e.marked if plan.ops[i].name.startswith("t")][0]
        want = env[int(plan.ops[mi].name[1:])].reshape(B, -1)
        runner = HipRunner(plan, max_batch=8)
        assert np.array_equal(runner.embed(x, dtype="int8"), want)
        assert np.array_equal(runner.embed(x), _dequant(want, e.scale, e.zero_point))
        runner.close()


def _write_flac(path, pcm, sr):
    import flac_writer as fw  # the tests' own encoder (RFC 9639)

    n, ch = pcm.shape
    frames = [{"n": 4096, "mode": "indep", "sub": [dict(kind="fixed", order=2, po=3)] * ch} for _ in range(n // 4096)]
    if n % 4096:
        frames.append({"n": n % 4096, "mode": "indep", "sub": [dict(kind="fixed", order=1, po=0)] * ch})
    with open(path, "wb") as f:
        f.write(fw.encode(pcm.astype(np.int64), sr, 16, frames))


def test_embed_files_and_cli(torch_mod, tmp_path):
    torch = torch_mod
    import wave

    from birdnet_stm32.audio.io import load_audio_file
    from birdnet_stm32.audio.pipeline import plan_files
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner

    rng = np.random.default_rng(3)
    specs = [("a.wav", 24000, 1, 7.5), ("b.wav", 48000, 2, 4.0), ("c.flac", 22050, 1, 5.2), ("d.wav", 16000, 1, 1.2), ("e.flac", 24000, 2, 9.0)]
    paths = []
    for name, sr, ch, sec in specs:
        n = int(sr * sec)
        t = np.arange(n) / sr
        x = 0.3 * np.sin(2 * np.pi * (800 + 300 * rng.random()) * t)[:, None] + 0.05 * rng.standard_normal((n, ch))
        pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
        p = str(tmp_path / name)
        if name.endswith(".wav"):
            with wave.open(p, "wb") as w:
                w.setnchannels(ch)
                w.setsampwidth(2)
                w.setframerate(sr)
                w.writeframes(pcm.tobytes())
        else:
            _write_flac(p, pcm, sr)
        paths.append(p)
    runner = load_model_runner(TFLITE_PATH, max_batch=64)
    sr, cd = 22050, 3.0   # (the shipped model's config)
    for ov in (0.0, 1.5):
        tab = plan_files(paths, sr, cd, ov)
        res = embed_files(runner, paths, chunk_overlap=ov, dtype="int8", sample_rate=sr, chunk_duration=cd)
        assert res.chunks_per_file.tolist() == tab.n_chunks.tolist() and res.embeddings.shape == (int(tab.n_chunks.sum()), 256)
        rows = []
        for p in paths:
            chunks = load_audio_file(p, sample_rate=sr, max_duration=60, chunk_duration=cd, chunk_overlap=ov)
            rows.append(runner.infer_audio_device(torch.from_numpy(np.stack(chunks).astype(np.float32)).cuda(), return_embeddings=True,
                                                  emb_dtype="int8")[1].cpu().numpy())
        assert np.array_equal(res.embeddings, np.concatenate(rows))
        assert np.array_equal(res.file_index, np.repeat(np.arange(len(paths)), tab.n_chunks))
        f32 = embed_files(runner, paths, chunk_overlap=ov, sample_rate=sr, chunk_duration=cd).embeddings
        assert np.array_equal(f32, _dequant(res.embeddings, res.scale, res.zero_point))
        for pooling, fn in (("avg", np.mean), ("max", np.max)):
            pooled = embed_files(runner, paths, chunk_overlap=ov, pooling=pooling, sample_rate=sr, chunk_duration=cd, budget_bytes=4 * 256 * 3)
            want = np.stack([fn(_dequant(r, res.scale, res.zero_point), axis=0) for r in rows])
            assert pooled.embeddings.shape == (len(paths), 256)
            assert np.array_equal(pooled.embeddings, want.astype(np.float32)), pooling
    with pytest.raises(ValueError):
        embed_files(runner, paths, pooling="lme", sample_rate=sr, chunk_duration=cd)
    runner.close()
    # the CLI in a child process: a readable npz
    ckpt = tmp_path / "m.tflite"
    ckpt.write_bytes(open(TFLITE_PATH, "rb").read())
    cfg = open(os.path.splitext(TFLITE_PATH)[0] + "_model_config.json").read()
    (tmp_path / "m_model_config.json").write_text(cfg)
    out = tmp_path / "e.npz"
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "birdnet-stm32_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "embed", "--model_path", str(ckpt), "--input", *paths, "--output", str(out),
                        "--dtype", "int8", "--max_batch", "256"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert z["embeddings"].dtype == np.int8 and z["embeddings"].shape[1] == 256 and z["embeddings"].shape[0] == int(z["chunks_per_file"].sum())
    assert len(z["paths"]) == len(paths) and float(z["scale"]) > 0 and int(z["zero_point"]) == -128
