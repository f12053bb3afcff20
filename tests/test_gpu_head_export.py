"""GPU tests of the head export: ``bn_head_i8_forward`` (csrc/bn_head_i8.hip) against the numpy specification
(``conversion.head_export.head_scores_i8_reference``) bit for bit over every shape at which the kernel takes another path; an exported model
against ``QuantizedHead.predict_device`` and the interpreter; ``probe --export_tflite`` -> ``evaluate`` end to end."""
from __future__ import annotations

import json
import os
import wave

import numpy as np
import pytest

import i8_mutants as im
import i8_variants as iv
from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of float32


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


def make_head(D, C, activation="sigmoid", spread=0.1, seed=0):
    from birdnet_stm32.training.linear_probe import ProbeHead

    rng = np.random.default_rng([seed, D, C])
    return ProbeHead(rng.normal(0.0, spread, (D, C)), rng.normal(0.0, 1.0, C), activation, [f"class{j}" for j in range(C)])


def float_logits(head, rows, s_in, z_in):
    return ((rows.astype(np.float64) - z_in) * float(np.float32(s_in))) @ head.W.astype(np.float64) + head.b.astype(np.float64)


def quantized(head, rows, s_in, z_in, per_tensor=False, shrink=1.0):
    """``shrink`` < 1 narrows the logit range the quantiser is told, so that logits fall outside it and both clamps fire."""
    from birdnet_stm32.conversion.head_export import quantize_head

    z = float_logits(head, rows, s_in, z_in)
    return quantize_head(head, s_in, z_in, shrink * float(z.min()), shrink * float(z.max()), per_tensor)


def byte_rows(n, D, seed):
    """Rows over all 256 byte values; -128 and 127 are in every row that is long enough, at both ends of the row."""
    rows = np.random.default_rng([seed, n, D]).integers(-128, 128, (n, D)).astype(np.int8)
    if n and D >= 4:
        rows[:, 0], rows[:, 1], rows[:, -1], rows[:, -2] = -128, 127, -128, 127
    return rows


def on_device(torch, rows, offset=0):
    """The rows on the device, their base pointer ``offset`` bytes behind an allocation's (256-byte aligned) start."""
    n, D = rows.shape
    buf = torch.empty(n * D + offset, dtype=torch.int8, device="cuda")
    view = buf[offset:].view(n, D)
    view.copy_(torch.from_numpy(rows))
    assert n == 0 or view.data_ptr() % 256 == offset
    return view


def check(torch, ctx, qh, rows, offset=0, what=""):
    from birdnet_stm32.conversion.head_export import head_scores_i8_reference

    scores, logit = qh.predict_device(on_device(torch, rows, offset), ctx, return_logit_bytes=True)
    torch.cuda.synchronize()
    want_bytes, want_scores = head_scores_i8_reference(qh, rows)
    got_bytes, got_scores = logit.cpu().numpy(), scores.cpu().numpy()
    assert got_bytes.shape == want_bytes.shape and got_scores.shape == want_scores.shape
    bad = int((got_bytes != want_bytes).sum())
    assert bad == 0, f"{what}: {bad} of {want_bytes.size} logit bytes differ"
    if qh.activation == "sigmoid":
        assert np.array_equal(got_scores, want_scores), what
    return got_bytes, got_scores, want_scores


CLASS_COUNTS = (1, 15, 16, 17, 50, 100, 129)   # 1, 2, 4 and 8 class tiles per pass over a step's rows (50: the only count here that takes 4); 129: two groups of 8
ROW_COUNTS = (1, 63, 64, 65)


@pytest.mark.parametrize("D", [16, 50, 80, 256, 320])
def test_kernel_equals_the_specification(torch_mod, ctx, D):
    """D = 50: rows off the 16-byte grid and a padded last chunk; 80: a padded second chunk; 320: five chunks, more than the streamer's
    group of four in flight.  Per-channel weights put +-127 into every class row."""
    for C in CLASS_COUNTS:
        for n in ROW_COUNTS:
            rows = byte_rows(n, D, seed=C)
            qh = quantized(make_head(D, C, seed=n), rows, 0.0159, -128, per_tensor=(C + n) % 2 == 1)
            assert np.abs(qh.w.astype(np.int32)).max() == 127 and (D < 4 or (rows.min(), rows.max()) == (-128, 127))
            check(torch_mod, ctx, qh, rows, what=f"D={D} C={C} n={n}")
            qh.close()


def test_kernel_edges(torch_mod, ctx):
    """The shapes and values at which something else happens, each against the specification bit for bit."""
    from birdnet_stm32 import _hip

    torch = torch_mod
    # -- no rows: success without a launch, whatever the pointers
    qh = quantized(make_head(80, 17), byte_rows(8, 80, 0), 0.02, -128)
    scores, logit = qh.predict_device(torch.empty((0, 80), dtype=torch.int8, device="cuda"), ctx, return_logit_bytes=True)
    assert tuple(scores.shape) == (0, 17) and tuple(logit.shape) == (0, 17)
    # -- a row base pointer off the 16-byte boundary (D a multiple of 16: only the pointer decides) and another zero point
    for off in (1, 4, 15):
        rows = byte_rows(65, 80, off)
        check(torch, ctx, quantized(make_head(80, 17, seed=off), rows, 0.02, 37), rows, offset=off, what=f"offset {off}")
    # -- two workgroups with a ragged last step: split_rows gives a workgroup at least BN_HEAD_I8_MIN_WG_STEPS = 8 steps of 64 rows, so
    #    581 rows = 10 steps (the last of 5 rows) go to ceil(10 / 8) = 2 workgroups of 5 steps
    n = 581
    steps = -(-n // _hip.HEAD_I8_STEP_ROWS)
    assert (steps, -(-steps // _hip.HEAD_I8_MIN_WG_STEPS), n % _hip.HEAD_I8_STEP_ROWS) == (10, 2, 5)
    rows = byte_rows(n, 50, 1)
    check(torch, ctx, quantized(make_head(50, 17), rows, 0.0159, -128), rows, what="two workgroups")
    # -- a second pass over the classes.  The LDS plan (head_i8_geometry): a class tile takes 16 * (D rounded up to 64, + 16) + 192 bytes
    #    of the 160 KB less the table's 256.  D = 2048: 33216 bytes, 4 tiles = 64 classes per pass, so C = 65 is the first count with two
    #    passes; D = 320: 5568 bytes, 29 tiles fit, 24 = three groups of 8 are taken = 384 classes per pass, so C = 400 takes two passes
    #    whose second holds one real tile
    for D, C, per_pass in ((2048, 64, 64), (2048, 65, 64), (320, 400, 384)):
        assert _hip.head_i8_pass_classes(D, C) == per_pass
        rows = byte_rows(70, D, C)
        check(torch, ctx, quantized(make_head(D, C, spread=0.02), rows, 0.0159, -128, per_tensor=C == 65), rows, what=f"D={D} C={C}")
    # -- a range narrow enough that both clamps fire
    rows = byte_rows(65, 256, 9)
    qh = quantized(make_head(256, 100, spread=0.5), rows, 0.0159, -128, shrink=0.05)
    got, _, _ = check(torch, ctx, qh, rows, what="clamps")
    assert (got == -128).mean() > 0.05 and (got == 127).mean() > 0.05
    # -- D = 1: one byte per row
    rows = np.arange(-128, 128, dtype=np.int64).astype(np.int8).reshape(256, 1)
    check(torch, ctx, quantized(make_head(1, 3, spread=0.5), rows, 0.05, -128), rows, what="D=1")


def softmax_bound(P, z, C):
    """|dP| <= P (8 u a + (C + 6) u), a = the row's largest |z| (test_softmax_head derives it); one denormal step for scores that underflow."""
    return P.astype(np.float64) * (8 * U * np.abs(z).max(axis=1, keepdims=True) + (C + 6) * U) + 2.0 ** -149


def test_softmax_head(torch_mod, ctx):
    """The kernel writes the logit bytes, the model's own softmax kernel the scores: bytes bit for bit; scores against the float32
    specification within the float32 roundings of a softmax.  With a = the row's largest |z|: the exponent's argument z - max is off by at
    most 2 u a (the device may fuse the dequantising product into the subtraction, for the element and for the maximum), so every term and
    their sum by a factor within 2 u a + u (expf within 1 ulp), the sum of C terms in another order by C u more and the division by u:
    |dP| <= P (8 u a + (C + 6) u)."""
    for D, C, n in ((80, 1, 5), (256, 17, 65), (320, 129, 70)):
        rows = byte_rows(n, D, C)
        qh = quantized(make_head(D, C, "softmax", spread=0.3), rows, 0.0159, -128)
        got_bytes, got, want = check(torch_mod, ctx, qh, rows, what=f"softmax D={D} C={C}")
        z = (got_bytes.astype(np.float64) - qh.z_out) * qh.s_out
        bound = softmax_bound(want, z, C)
        err = np.abs(got.astype(np.float64) - want)
        print(f"softmax D={D} C={C}: max err / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound) and np.allclose(got.sum(axis=1), 1.0, atol=1e-5)


def test_refused_calls(torch_mod, ctx):
    torch = torch_mod
    lib = ctx.lib
    err = lambda: lib.bn_last_error().decode()  # noqa: E731
    rows = torch.zeros((8, 64), dtype=torch.int8, device="cuda")
    w = torch.zeros((4, 64), dtype=torch.int8, device="cuda")
    i32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    lut = torch.zeros(256, dtype=torch.int8, device="cuda")
    out = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    byt = torch.zeros((8, 4), dtype=torch.int8, device="cuda")

    def call(rows_p=rows.data_ptr(), n=8, D=64, w_p=w.data_ptr(), C=4, zp=0, lut_p=lut.data_ptr(), act=0, logit_p=byt.data_ptr(), out_p=out.data_ptr()):
        return lib.bn_head_i8_forward(ctx.handle, rows_p, n, D, w_p, i32.data_ptr(), i32.data_ptr(), i32.data_ptr(), C, zp, lut_p, act, 1.0, logit_p, out_p, None)

    assert call() == 0
    assert call(rows_p=None) == -1 and "null" in err()
    assert call(out_p=None) == -1 and "null" in err()
    assert call(D=0) == -1 and "D=0" in err()
    assert call(D=2049) == -1 and call(C=0) == -1 and call(C=4097) == -1 and call(n=-1) == -1 and call(act=2) == -1
    assert call(zp=128) == -1 and "zero point" in err()
    assert call(lut_p=None) == -1 and "table" in err()                 # sigmoid without its table
    assert call(act=1) == -1 and "table" in err()                      # softmax with one
    assert call(act=1, lut_p=None, logit_p=None) == -1 and "d_logit_bytes" in err()
    assert call(w_p=w.data_ptr() + 4) == -1 and "aligned" in err()
    assert call(act=1, lut_p=None) == 0 and call(logit_p=None) == 0 and call(n=0, rows_p=None) == 0
    torch.cuda.synchronize()
    assert lib.bn_head_i8_pass_classes(0, 4) == -1 and lib.bn_head_i8_pass_classes(64, 4097) == -1 and lib.bn_head_i8_pass_classes(64, 4) == 16


def test_softmax_rows_past_one_launch(torch_mod, ctx):
    """A softmax head's scores come from a kernel of one 64-thread workgroup per row, launched in slices of 2^24 rows (a launch holds fewer
    than 2^32 threads): 2^26 + 5 rows of one byte and one class.  The logit bytes of the first and last rows and of the rows around every
    slice border equal the specification, and every score is the softmax of one class: 1 within ``softmax_bound``."""
    from birdnet_stm32.conversion.head_export import head_scores_i8_reference

    torch = torch_mod
    n = (1 << 26) + 5
    g = torch.Generator(device="cuda").manual_seed(4)
    rows = torch.randint(-128, 128, (n, 1), device="cuda", generator=g, dtype=torch.int8)
    qh = quantized(make_head(1, 1, "softmax", spread=0.5), np.arange(-128, 128, dtype=np.int64).astype(np.int8).reshape(256, 1), 0.05, -128)
    scores, logit = qh.predict_device(rows, ctx, return_logit_bytes=True)
    torch.cuda.synchronize()
    a = max(abs(-128 - qh.z_out), abs(127 - qh.z_out)) * qh.s_out   # the largest |z| a byte can mean: softmax_bound with P = 1, C = 1
    worst = float((scores - 1.0).abs().max())
    assert worst <= 8 * U * a + 7 * U, worst
    for r0 in [0, n - 300] + [k * (1 << 24) - 150 for k in range(1, 5)]:
        want, _ = head_scores_i8_reference(qh, rows[r0 : r0 + 300].cpu().numpy())
        assert np.array_equal(logit[r0 : r0 + 300].cpu().numpy(), want), r0
    qh.close()


# -- an exported model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,activation", [(7, "sigmoid"), (129, "sigmoid"), (7, "softmax"), (129, "softmax")])
def test_exported_model_equals_predict_device_and_the_interpreter(torch_mod, tmp_path, C, activation):
    """The 16 shared spectrograms through the exported file's runner, and through the backbone's int8 embeddings and the head kernel: the
    same scores, and the interpreter's on the exported graph (sigmoid: bit for bit; softmax: the bytes it is computed from are, the float32
    softmax within ``softmax_bound``)."""
    import shutil

    from birdnet_stm32.conversion.head_export import find_classifier, graft_head
    from birdnet_stm32.models._tflite_reader import load_tflite
    from birdnet_stm32.models._tflite_writer import write_tflite
    from birdnet_stm32.models.runners import load_model_runner

    torch = torch_mod
    S = iv.inputs()
    backbone = load_model_runner(TFLITE_PATH, max_batch=iv.N_INPUTS)
    try:
        info = backbone.embedding_info()
        rows = backbone.embed(S.reshape(iv.N_INPUTS, -1), dtype="int8")
        assert rows.dtype == np.int8 and rows.shape == (iv.N_INPUTS, 256)
        qh = quantized(make_head(256, C, activation, seed=C), rows, info["scale"], info["zero_point"])
        stem = str(tmp_path / "exported")
        with open(stem + ".tflite", "wb") as fh:
            fh.write(write_tflite(graft_head(im.shipped(), qh)))
        shutil.copy(CONFIG_PATH, stem + "_model_config.json")
        runner = load_model_runner(stem + ".tflite", max_batch=iv.N_INPUTS)
        try:
            assert runner.num_classes == C
            got = runner.predict(S.reshape(iv.N_INPUTS, -1))
        finally:
            runner.close()
        own = qh.predict_device(torch.from_numpy(rows).cuda(), backbone.ctx).cpu().numpy()
        qh.close()
    finally:
        backbone.close()
    assert np.array_equal(got, own)
    grafted = load_tflite(stem + ".tflite")
    want, env = iv.oracle(grafted, S)
    assert np.array_equal(env[127].reshape(iv.N_INPUTS, -1), rows)
    if activation == "sigmoid":
        assert np.array_equal(got, want)
    else:
        q = env[grafted.ops[find_classifier(grafted)["fc"]].outputs[0]].reshape(iv.N_INPUTS, C).astype(np.float64)
        z = (q - qh.z_out) * qh.s_out
        assert np.all(np.abs(got.astype(np.float64) - want) <= softmax_bound(want, z, C))


# -- end to end -----------------------------------------------------------------------------------------------------------------------
SR = 22050


def _tone_file(path, f0, seed):
    """3 s of a tone with two harmonics and a slow tremolo, a little noise under it."""
    rng = np.random.default_rng(seed)
    t = np.arange(3 * SR) / SR
    f = f0 * (1 + 0.05 * rng.uniform(-1, 1))
    x = sum(a * np.sin(2 * np.pi * k * f * t + rng.uniform(0, 6.28)) for k, a in ((1, 1.0), (2, 0.4), (3, 0.2)))
    x = x * (0.7 + 0.3 * np.sin(2 * np.pi * rng.uniform(2, 6) * t)) + 0.01 * rng.standard_normal(t.size)
    pcm = np.clip(np.round(0.8 * x / np.abs(x).max() * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def test_probe_export_then_evaluate(torch_mod, tmp_path):
    from birdnet_stm32.cli import evaluate as evaluate_cli
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.evaluation.detections import detect_files
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead

    data = tmp_path / "data"
    files = []
    for kind, f0 in (("high_tone", 2800.0), ("low_tone", 500.0)):
        os.makedirs(data / kind)
        for i in range(8):
            _tone_file(data / kind / f"{i:02d}.wav", f0, seed=int(f0) + i)
            files.append(str(data / kind / f"{i:02d}.wav"))
    # a float backbone is refused before any file is read: neither the data folder nor the output's folder exists
    with pytest.raises(SystemExit, match="INT8 .tflite"):
        probe_cli.main(["--model_path", KERAS_PATH, "--data_path_train", str(tmp_path / "nowhere"), "--output", str(tmp_path / "no" / "head"), "--export_tflite"])
    assert not os.path.exists(tmp_path / "no")

    out = str(tmp_path / "tones")
    runner = load_model_runner(TFLITE_PATH, max_batch=64, prepare_pipeline=True)
    try:
        head = probe_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(data), "--output", out, "--epochs", "3",
                               "--learning_rate", "0.01", "--export_tflite"], runner=runner)
        for suffix in (".npz", ".tflite", "_export.json", "_labels.txt", "_model_config.json"):
            assert os.path.isfile(out + suffix), suffix
        rep = json.load(open(out + "_export.json"))
        assert rep["classes"] == 2 and rep["rows"] == 16 and rep["report_rows"] == 4 and rep["cosine_mean"] >= 0.95   # 16 files of one chunk, 4 of them validate
        assert rep["logit_range"][0] < rep["logit_range"][1] and 0.0 <= rep["clipped_share"] <= 1.0 and np.isfinite([rep["loss_float"], rep["loss_int8"]]).all()
        emb = embed_files(runner, files, max_duration=30, sample_rate=22050, chunk_duration=3.0)
        want = ProbeHead.load(out + ".npz").predict(emb.embeddings, runner.ctx).astype(np.float64)
        info = runner.embedding_info()
    finally:
        runner.close()

    metrics = evaluate_cli.main(["--model_path", out + ".tflite", "--data_path_test", str(data)])
    assert len(metrics["ap_per_class"]) == 2 and all(np.isfinite(a) for a in metrics["ap_per_class"])

    exported = load_model_runner(out + ".tflite", max_batch=64, prepare_pipeline=True)
    try:
        assert exported.num_classes == 2
        det = detect_files(exported, files, sample_rate=22050, chunk_duration=3.0, return_scores=True, max_duration=30)
    finally:
        exported.close()
    assert det.scores.shape == want.shape == (16, 2)
    # the roundings bound of INT8 against float head, per element; x = the dequantised embedding, the scales are the
    # exported file's own
    from birdnet_stm32.conversion.head_export import find_classifier
    from birdnet_stm32.models._tflite_reader import load_tflite

    written = load_tflite(out + ".tflite")
    fc = written.ops[find_classifier(written)["fc"]]
    s_w = written.tensors[fc.inputs[1]].scale.astype(np.float64)
    s_out = float(written.tensors[fc.outputs[0]].scale[0])
    assert s_w.shape == (2,) and s_out == rep["logit_scale"] and float(written.tensors[fc.inputs[0]].scale[0]) == info["scale"]
    s_in = info["scale"]
    x_abs = np.abs(emb.embeddings.astype(np.float64)).sum(axis=1)[:, None]
    bound = 0.25 * (x_abs * s_w[None, :] / 2 + s_in * s_w[None, :] / 2 + 1.01 * s_out / 2 + s_out * 2.0 ** -7) + 1.0 / 256
    err = np.abs(det.scores.astype(np.float64) - want)
    print(f"exported model vs float head: max err {err.max():.4f}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
