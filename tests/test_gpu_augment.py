"""GPU tests of the probe augmentation: bn_augment_inputs (csrc/bn_augment.hip) against training.augment.augment_reference bit for bit,
guard rows, refused calls, the augmented fit (identity = the plain fit, determinism), model_inputs_device, embed_files(keep_inputs=True)
and probe with the new flags end to end."""

import ctypes
import os

import numpy as np
import pytest

from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

N_ROWS = 9
SHAPES = [(1, 1001), (1, 1002), (1, 1004), (3, 8), (20, 44), (64, 256), (257, 256)]
GUARD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]   # a NaN with a payload: any write shows


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


def _inputs(F, W, seed=0):
    """Nine rows with negative values, -0.0, subnormals; row 7 holds values around 1e-12 (a gain of 1e-27 makes its products subnormal)."""
    rng = np.random.default_rng(1000 * F + W + seed)
    E = F * W
    x = rng.standard_normal((N_ROWS, E)).astype(np.float32)
    x[rng.random((N_ROWS, E)) < 0.08] = -0.0
    sub = rng.random((N_ROWS, E)) < 0.08
    x[sub] = (rng.standard_normal(int(sub.sum())) * 1e-40).astype(np.float32)
    x[7] = (rng.standard_normal(E) * 1e-12).astype(np.float32)
    return x


def _mask_tables(F, W):
    """(fmask, tmask) [9, 2, 2] for the nine source rows: width 0, start 0, ending exactly at the edge, reaching past it, wholly outside,
    overlapping, time starts at 1, 2, 3 (mod 4), and row 8 with every frequency row masked."""
    f = np.zeros((N_ROWS, 2, 2), np.int32)
    t = np.zeros((N_ROWS, 2, 2), np.int32)
    f[0], t[0] = [[0, 0], [0, 2]], [[1, 3], [max(W - 2, 0), 2]]
    f[1], t[1] = [[F - 1, 1], [0, 0]], [[2, 5], [3, 2]]
    f[2], t[2] = [[F - 1, 5], [F + 3, 2]], [[W - 1, 9], [0, 0]]
    f[3], t[3] = [[1, 2], [2, 2]], [[6, 1], [7, 3]]
    f[5], t[5] = [[0, 1], [5, 0]], [[5, 0], [W // 2, 0]]
    t[6] = [[0, 1], [W // 2 + 3, 6]]
    f[8] = [[0, F], [0, 0]]
    return f, t


RECIPES = [   # (nsrc, sources, gains or None for a Dirichlet draw)
    (3, (0, 1, 2), None),
    (1, (1, 1, 1), (1.0, 0.0, 0.0)),
    (2, (2, 2, 2), (0.25, 0.75, 0.0)),              # the partner is the row itself
    (3, (3, 4, 4), None),                           # the same source twice
    (2, (4, 7, 4), (1.0, 1e-27, 0.0)),              # a gain of 1.0; 1e-27 x 1e-12: subnormal products
    (1, (8, 8, 8), (1.0, 0.0, 0.0)),                # every frequency row masked: all +0.0
    (2, (6, 1, 6), None),                           # rows of different parity: different misalignment at W = 1002
    (3, (7, 0, 5), (1e-27, 1e-27, 1e-27)),
    (1, (3, 3, 3), (1.0, 0.0, 0.0)),
    (2, (0, 8, 0), None),
    (1, (7, 7, 7), (1.0, 0.0, 0.0)),                # a copy of subnormal-heavy values
]


def _hand_plan(m, F, W, fmask=True, tmask=True):
    from birdnet_stm32.training.augment import AugmentPlan

    rng = np.random.default_rng(m)
    nsrc, src, gain = np.zeros(m, np.int32), np.zeros((m, 3), np.int32), np.zeros((m, 3), np.float32)
    for r in range(m):
        k, s, g = RECIPES[r % len(RECIPES)]
        shift = r // len(RECIPES)   # later cycles move to other rows: other alignments of output against sources
        nsrc[r], src[r] = k, [(v + shift) % N_ROWS for v in s]
        gain[r, :k] = rng.dirichlet([0.2] * k).astype(np.float32) if g is None else np.asarray(g[:k], np.float32)
    f, t = _mask_tables(F, W)
    return AugmentPlan(nsrc, src, gain, f if fmask else None, t if tmask else None, F, W)


def _call(torch, ctx, d_x, n_rows, F, W, tabs, nf, nt, m, d_out):
    """The raw C call (no Python-side checks): the return code."""
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return ctx.lib.bn_augment_inputs(ctx.handle, p(d_x), n_rows, F, W, p(tabs[0]), p(tabs[1]), p(tabs[2]), p(tabs[3]), nf, p(tabs[4]), nt, m, p(d_out),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _device_augment(torch, ctx, x, plan):
    """bn_augment_inputs on ``x`` with ``plan``: the output rows; asserts the guard rows around them and ``d_x`` are untouched."""
    from birdnet_stm32 import _hip

    m, E = plan.rows, x.shape[1]
    d_x = torch.from_numpy(x).cuda()
    full = torch.full((m + 2, E), float("nan"), dtype=torch.float32, device="cuda")
    full.view(torch.int32).fill_(int(GUARD.view(np.int32)))
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tabs = [up(a) for a in (plan.nsrc, plan.src, plan.gain, plan.fmask, plan.tmask)]
    nf, nt = (0 if a is None else a.shape[1] for a in (plan.fmask, plan.tmask))
    _hip.check(_call(torch, ctx, d_x, x.shape[0], plan.F, plan.W, tabs, nf, nt, m, full[1:]))
    torch.cuda.synchronize()
    got = full.cpu().numpy().view(np.int32)
    guard = int(GUARD.view(np.int32))
    assert (got[0] == guard).all() and (got[-1] == guard).all(), "a row outside the plan's output was written"
    assert np.array_equal(d_x.cpu().numpy().view(np.int32), x.view(np.int32)), "d_x changed"
    return got[1:-1]


@pytest.mark.parametrize("m", [1, 5, 70])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_specification_bit_for_bit(torch_mod, ctx, shape, m):
    from birdnet_stm32.training.augment import augment_reference

    F, W = shape
    x = _inputs(F, W)
    plan = _hand_plan(m, F, W)
    want = augment_reference(x, plan).view(np.int32)
    got = _device_augment(torch_mod, ctx, x, plan)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (row, element) {bad[0].tolist()}: nsrc {plan.nsrc[bad[0][0]]} src {plan.src[bad[0][0]].tolist()}"
    if m >= 6:
        assert (want[5] == 0).all()   # the all-masked source really gave +0.0 everywhere
    if m == 70:
        ref = want.view(np.float32)
        assert (np.abs(ref[ref != 0]) < np.finfo(np.float32).tiny).any() and np.signbit(ref[ref == 0]).any()   # subnormals and -0.0 reached the output


@pytest.mark.parametrize("shape", [(1, 1001), (20, 44)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("tables", ["time_only", "freq_only", "none"])
def test_kernel_with_one_mask_table_or_none(torch_mod, ctx, shape, tables):
    from birdnet_stm32.training.augment import augment_reference

    F, W = shape
    x = _inputs(F, W, seed=1)
    plan = _hand_plan(23, F, W, fmask=tables == "freq_only", tmask=tables == "time_only")
    assert np.array_equal(_device_augment(torch_mod, ctx, x, plan), augment_reference(x, plan).view(np.int32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kernel_on_plans_at_the_reference_defaults(torch_mod, ctx, seed):
    from birdnet_stm32.training.augment import ProbeAugmentation, augment_plan, augment_reference

    aug = ProbeAugmentation(mixup_alpha=0.2, mixup_probability=0.25, spec_augment=True)
    for F, W in ((64, 256), (257, 256), (1, 66150)):
        x = _inputs(F, W, seed=seed)
        plan = augment_plan(N_ROWS, F, W, aug, seed, 4)
        assert int((plan.nsrc > 1).sum()) == 2
        assert np.array_equal(_device_augment(torch_mod, ctx, x, plan), augment_reference(x, plan).view(np.int32)), (F, W)


def test_refused_calls_return_err_arg_and_launch_nothing(torch_mod, ctx):
    torch = torch_mod
    from birdnet_stm32 import _hip

    F, W, m = 20, 44, 5
    x = _inputs(F, W)
    plan = _hand_plan(m, F, W)
    d_x = torch.from_numpy(x).cuda()
    out = torch.zeros((m, F * W), dtype=torch.float32, device="cuda")
    tabs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (plan.nsrc, plan.src, plan.gain, plan.fmask, plan.tmask)]
    wide = torch.zeros((N_ROWS, _hip.AUGMENT_MAX_MASKS + 1, 2), dtype=torch.int32, device="cuda")
    ok = dict(d_x=d_x, n_rows=N_ROWS, F=F, W=W, tabs=tabs, nf=2, nt=2, m=m, d_out=out)

    def rc(**kw):
        a = dict(ok, **kw)
        return _call(torch, ctx, a["d_x"], a["n_rows"], a["F"], a["W"], a["tabs"], a["nf"], a["nt"], a["m"], a["d_out"])

    def without(i):
        return [None if j == i else t for j, t in enumerate(tabs)]

    bad = [dict(d_x=None), dict(d_out=None), dict(tabs=without(0)), dict(tabs=without(1)), dict(tabs=without(2)),
           dict(tabs=tabs[:3] + [wide, tabs[4]], nf=_hip.AUGMENT_MAX_MASKS + 1), dict(tabs=tabs[:4] + [wide], nt=_hip.AUGMENT_MAX_MASKS + 1),
           dict(nf=-1), dict(nt=-1),
           dict(tabs=without(3)), dict(tabs=without(4)),                    # counts without their tables
           dict(nf=0), dict(nt=0),                                          # tables without their counts
           dict(d_out=d_x), dict(d_out=d_x[N_ROWS - 1 :]), dict(d_x=out[m - 1 :], n_rows=1),   # overlap, whole or by one row
           dict(n_rows=0), dict(m=-1), dict(F=0), dict(W=0), dict(F=1 << 20, W=1 << 20)]
    for kw in bad:
        assert rc(**kw) == -1, kw   # BN_ERR_ARG
        assert b"" != ctx.lib.bn_last_error()
    torch.cuda.synchronize()
    assert not out.any() and np.array_equal(d_x.cpu().numpy().view(np.int32), x.view(np.int32))   # nothing ran
    assert rc(m=0) == 0 and not out.any()
    assert rc() == 0
    torch.cuda.synchronize()
    assert out.any()


# -- the fit ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def i8_probe_data(torch_mod):
    """The shipped INT8 model (slices of 16), model inputs of 40 synthetic chunks, their embeddings and targets of three classes."""
    from birdnet_stm32.models.runners import load_model_runner

    from conftest import synth_chunks

    runner = load_model_runner(TFLITE_PATH, max_batch=16)
    audio = torch_mod.from_numpy(synth_chunks(40, seed=5)).cuda()
    inputs = torch_mod.cat([runner.model_inputs_device(audio[b : b + 16]) for b in range(0, 40, 16)]).contiguous()
    _, emb = runner.predict_device(inputs, return_embeddings=True)
    rng = np.random.default_rng(0)
    Y = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 40)]
    Y[::9] = 0.0
    yield runner, inputs, emb.clone(), Y
    runner.close()


FIT = dict(epochs=3, batch_size=8, learning_rate=0.01)


def test_identity_augmentation_is_the_plain_fit(torch_mod, i8_probe_data):
    from birdnet_stm32.training.augment import ProbeAugmentation
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_augmented

    runner, inputs, emb, Y = i8_probe_data
    before = inputs.clone()
    ident = ProbeAugmentation(mixup_probability=0.0, spec_augment=True, freq_mask_max=1, time_mask_max=1)
    plain = fit_probe(runner, emb[:32], Y[:32], emb[32:], Y[32:], seed=7, **FIT)
    aug = fit_probe_augmented(runner, inputs[:32].contiguous(), Y[:32], emb[32:], Y[32:], augment=ident, input_shape=runner.input_shape(), seed=7, **FIT)
    assert np.array_equal(plain.W.view(np.int32), aug.W.view(np.int32)) and np.array_equal(plain.b.view(np.int32), aug.b.view(np.int32))
    assert plain.history["loss"] == aug.history["loss"] and plain.history["val_loss"] == aug.history["val_loss"]
    assert len(aug.history["augment_seconds"]) == 3 and torch_mod.equal(inputs, before)


def test_augmented_fit_is_deterministic_and_follows_its_seed(torch_mod, i8_probe_data):
    from birdnet_stm32.training.augment import ProbeAugmentation
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_augmented

    runner, inputs, emb, Y = i8_probe_data
    on = ProbeAugmentation(mixup_alpha=0.2, mixup_probability=0.25, spec_augment=True)
    kw = dict(augment=on, input_shape=runner.input_shape(), **FIT)
    a, b, c = (fit_probe_augmented(runner, inputs, Y, seed=s, **kw) for s in (7, 7, 8))
    assert np.array_equal(a.W.view(np.int32), b.W.view(np.int32)) and np.array_equal(a.b.view(np.int32), b.b.view(np.int32))
    assert a.history["loss"] == b.history["loss"]
    assert not np.array_equal(a.W, c.W)
    assert not np.array_equal(a.W, fit_probe(runner, emb, Y, seed=7, **FIT).W)   # the augmentation really changed the rows
    assert np.isfinite(a.W).all() and np.isfinite(a.history["loss"]).all()


def test_an_epochs_embeddings_differ_in_the_rows_the_plan_touches(torch_mod, i8_probe_data):
    """Without SpecAugment the plan touches the mixed rows only.  The gains are drawn at alpha = 50 (near-equal shares), so that every mix
    with a partner other than the row itself moves the input by tens of percent; a row mixed only with itself is g0 v + g1 v, v up to
    rounding, and may or may not move its embedding: it is left out of the comparison."""
    from birdnet_stm32.training.augment import ProbeAugmentation, augment_plan
    from birdnet_stm32.training.linear_probe import augmented_embeddings

    runner, inputs, emb, _Y = i8_probe_data
    F, W = runner.input_shape()
    plan = augment_plan(40, F, W, ProbeAugmentation(mixup_alpha=50.0, mixup_probability=0.25), 3, 0)
    got = augmented_embeddings(runner, inputs, plan)
    differs = (got != emb).any(dim=1).cpu().numpy()
    others = np.array([any(plan.src[r, s] != r for s in range(1, plan.nsrc[r])) for r in range(40)])
    only_self = (plan.nsrc > 1) & ~others
    assert others.sum() >= 8 and np.array_equal(differs[~only_self], others[~only_self])
    assert np.array_equal(plan.touched(), plan.nsrc > 1)
    assert torch_mod.equal(augmented_embeddings(runner, inputs, plan), got)


# -- model inputs -----------------------------------------------------------------------------------------------------------------------
def test_model_inputs_then_predict_is_infer_audio(torch_mod):
    torch = torch_mod
    from birdnet_stm32.models import build_model
    from birdnet_stm32.models._lower_f32 import lower_f32
    from birdnet_stm32.models.runners import HipRunner, load_model_runner

    from conftest import synth_chunks

    common = dict(num_mels=64, spec_width=256, sample_rate=24000, chunk_duration=3, embeddings_size=64, num_classes=7, use_se=False,
                  use_inverted_residual=False, randomize_bn=True, seed=3)
    audio = torch.from_numpy(synth_chunks(5)).cuda()
    raw = HipRunner(lower_f32(build_model("dscnn", audio_frontend="raw", mag_scale="pwl", raw_length_limit=None, **common)), max_batch=4)
    mel = HipRunner(lower_f32(build_model("dscnn", audio_frontend="librosa", mag_scale="pwl", **common)), max_batch=4)
    mel.configure_precomputed("librosa", 24000, "pwl", 512, 64, 20)
    for r, shape in ((raw, (1, 72000)), (mel, (64, 256))):
        x = r.model_inputs_device(audio)
        assert tuple(x.shape) == (5, r.input_elems) and r.input_shape() == shape
        s, e = r.infer_audio_device(audio, return_embeddings=True)
        s2, e2 = r.predict_device(x, return_embeddings=True)
        assert torch.equal(s, s2) and torch.equal(e, e2)
        r.close()
    # hybrid float32: the fused audio path and stft_device + predict_device round differently; the bound is the one
    # tests/test_gpu_sweeps.py already sets for this pair (infer_audio_device against predict_device(stft_device(audio)): < 1e-5)
    hyb = load_model_runner(KERAS_PATH, max_batch=4)
    x = hyb.model_inputs_device(audio)
    assert tuple(x.shape) == (5, 257 * 256) and hyb.input_shape() == (257, 256)
    assert torch.equal(x.view(5, 257, 256), hyb.stft_device(audio, normalize=True))
    d = (hyb.predict_device(x) - hyb.infer_audio_device(audio)).abs().max().item()
    print(f"hybrid float32: max |scores(model_inputs -> predict) - scores(infer_audio)| = {d:.3e}")
    assert d < 1e-5
    hyb.close()


# -- files ------------------------------------------------------------------------------------------------------------------------------
SR = 24000


def _write_wav(path, x):
    import wave

    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def _tone_folders(root, per_class=6, seed=0):
    """Two tone classes plus a noise folder of 3 s and 6 s WAVs; returns the paths in folder order."""
    rng = np.random.default_rng(seed)
    paths = []
    for kind, f0 in (("low_tone", 700.0), ("high_tone", 3100.0), ("noise", 0.0)):
        os.makedirs(root / kind)
        for i in range(per_class):
            n = SR * (6 if i % 3 == 0 else 3)
            t = np.arange(n) / SR
            x = 0.05 * rng.standard_normal(n)
            if f0:
                x = x + 0.6 * np.sin(2 * np.pi * (f0 + 40.0 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
            else:
                x = 6.0 * x
            _write_wav(root / kind / f"{i:02d}.wav", x)
            paths.append(str(root / kind / f"{i:02d}.wav"))
    return paths


def test_embed_files_keeps_the_model_inputs(torch_mod, tmp_path, monkeypatch):
    torch = torch_mod
    from birdnet_stm32.audio import pipeline as pl
    from birdnet_stm32.audio.io import load_audio_window
    from birdnet_stm32.audio.pipeline import ChunkSelection
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner

    paths = _tone_folders(tmp_path, per_class=3)
    runner = load_model_runner(TFLITE_PATH, max_batch=8, prepare_pipeline=True)
    kw = dict(max_duration=30, sample_rate=22050, chunk_duration=3.0, pipeline_options=dict(group_chunks=5))
    size = 66150
    try:
        for select in (None, ChunkSelection(1)):
            plain = embed_files(runner, paths, select=select, **kw)
            # (embedding blocks of at most four rows: the kept inputs of several blocks land in one buffer)
            kept = embed_files(runner, paths, select=select, keep_inputs=True, budget_bytes=4 * 256 * 4, **kw)
            assert plain.inputs is None and kept.inputs.is_cuda and tuple(kept.inputs.shape) == (kept.embeddings.shape[0], runner.input_elems)
            assert np.array_equal(plain.embeddings, kept.embeddings) and np.array_equal(plain.file_index, kept.file_index)
            assert np.array_equal(plain.start_s, kept.start_s)
            assert kept.embeddings.shape[0] == len(paths) if select is not None else kept.embeddings.shape[0] > len(paths)
            # the rows are model_inputs_device of the same chunks: cut them again from the files, as the pipeline's host twin does
            chunks = []
            for f, s0 in zip(kept.file_index, kept.start_s):
                y = load_audio_window(paths[int(f)], sample_rate=22050, max_duration=30, chunk_duration=3.0)
                a = int(round(float(s0) * 22050))
                c = np.zeros(size, np.float32)
                c[: min(size, len(y) - a)] = y[a : a + size]
                chunks.append(c)
            want = torch.cat([runner.model_inputs_device(torch.from_numpy(np.stack(chunks[b : b + 8])).cuda()) for b in range(0, len(chunks), 8)])
            assert torch.equal(kept.inputs, want)   # (the device ingest's samples are the host loader's: tests/test_gpu_activity.py compares the same way)
        # the budget refusal fires before any file is read
        monkeypatch.setattr(pl.EvaluatePipeline, "run", lambda *a, **k: pytest.fail("a file was read"))
        with pytest.raises(ValueError, match=r"\b3 rows would fit"):
            embed_files(runner, paths, keep_inputs=True, inputs_budget_bytes=3 * runner.input_elems * 4 + 100, **kw)
        with pytest.raises(ValueError, match="pooling"):
            embed_files(runner, paths, keep_inputs=True, pooling="avg", **kw)
    finally:
        runner.close()
        pl.release_pinned_slabs()


def test_probe_with_augmentation_end_to_end(torch_mod, tmp_path, capsys):
    from birdnet_stm32.cli import analyze as analyze_cli
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead

    train = tmp_path / "train"
    os.makedirs(train)
    paths = _tone_folders(train, per_class=6)
    runner = load_model_runner(TFLITE_PATH, max_batch=16, prepare_pipeline=True)
    base = ["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(train), "--epochs", "12", "--batch_size", "8",
            "--learning_rate", "0.02", "--seed", "3"]
    try:
        out = str(tmp_path / "aug")
        head = probe_cli.main(base + ["--output", out, "--mixup_probability", "0.25", "--spec_augment"], runner=runner)
        for suffix in (".npz", "_labels.txt", "_model_config.json", "_history.csv"):
            assert os.path.isfile(out + suffix), suffix
        said = capsys.readouterr().out
        assert "augment + re-embed" in said and "ms per epoch" in said
        loss = head.history["loss"]
        print(f"augmented probe: loss per epoch {[round(v, 4) for v in loss]}")
        assert len(loss) >= 2 and loss[-1] < loss[0] and np.isfinite(loss).all()   # it trained to a lower loss than its first epoch's
        loaded = ProbeHead.load(out + ".npz")
        assert loaded.class_names == ["high_tone", "low_tone"] and np.array_equal(loaded.W, head.W)
        det = analyze_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--head", out + ".npz", "--input", *paths[:8],
                                "--output", str(tmp_path / "det.csv"), "--min_conf", "0.0", "--top_k", "1"], runner=runner)
        assert len(det) > 0 and set(int(c) for c in det.class_index) <= {0, 1} and os.path.isfile(tmp_path / "det.csv")
        # with a selection too
        head_sel = probe_cli.main(base + ["--output", str(tmp_path / "augsel"), "--mixup_probability", "0.25", "--spec_augment", "--max_chunks_per_file", "1"],
                                  runner=runner)
        assert np.isfinite(head_sel.W).all() and os.path.isfile(str(tmp_path / "augsel.npz"))
        # the new flags at their off values: the bytes of a run without them
        probe_cli.main(base + ["--output", str(tmp_path / "plain")], runner=runner)
        probe_cli.main(base + ["--output", str(tmp_path / "off"), "--mixup_probability", "0", "--mixup_alpha", "0.2", "--freq_mask_max", "8",
                               "--time_mask_max", "25"], runner=runner)
        with np.load(tmp_path / "plain.npz") as a, np.load(tmp_path / "off.npz") as b:   # (the archives' zip headers carry the time of writing)
            assert a.files == b.files and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a.files)
        for suffix in ("_labels.txt", "_model_config.json", "_history.csv"):
            assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "off") + suffix, "rb").read()
        assert not np.array_equal(ProbeHead.load(str(tmp_path / "plain.npz")).W, head.W)
    finally:
        runner.close()
        from birdnet_stm32.audio import pipeline as pl

        pl.release_pinned_slabs()
