"""Probe augmentation on the host: plans, the numpy specification of bn_augment_inputs, the reference fit, refusals, the parser (no GPU)."""

import argparse

import numpy as np
import pytest

from birdnet_stm32.training import augment as A
from birdnet_stm32.training import linear_probe as lp

DEFAULTS = A.ProbeAugmentation(mixup_alpha=0.2, mixup_probability=0.25, spec_augment=True)   # the reference CLI's settings


def _ulp_sum_error(g: np.ndarray) -> float:
    """|sum - 1| of one gain row in units of the float32 ulp at 1 (exact sum in float64: three float32 values add exactly there)."""
    return abs(float(g.astype(np.float64).sum()) - 1.0) / float(np.spacing(np.float32(1.0)))


def test_plan_properties_over_200_seed_epoch_pairs():
    n, F, W = 37, 64, 256
    n_mixed = int(n * 0.25)
    for i in range(200):
        seed, epoch = 1000 + i // 10, i % 10
        p = A.augment_plan(n, F, W, DEFAULTS, seed, epoch)
        assert p.nsrc.shape == (n,) and p.nsrc.dtype == np.int32
        assert p.src.shape == (n, 3) and p.src.dtype == np.int32
        assert p.gain.shape == (n, 3) and p.gain.dtype == np.float32
        assert p.fmask.shape == (n, 2, 2) and p.fmask.dtype == np.int32
        assert p.tmask.shape == (n, 2, 2) and p.tmask.dtype == np.int32
        assert set(np.unique(p.nsrc)) <= {1, 2, 3}
        assert int((p.nsrc > 1).sum()) == n_mixed
        assert np.array_equal(p.src[:, 0], np.arange(n))
        assert p.src.min() >= 0 and p.src.max() < n
        for r in np.flatnonzero(p.nsrc == 3):
            assert p.src[r, 1] != p.src[r, 2]   # partners are distinct from each other (either may be the row itself)
        for r in range(n):
            k = int(p.nsrc[r])
            g = p.gain[r]
            assert np.all(np.isfinite(g[:k])) and np.all(g[:k] > 0) and np.all(g[k:] == 0)
            if k == 1:
                assert g[0] == 1.0
            else:
                assert _ulp_sum_error(g[:k]) <= 2.0
        for tab, mx, size in ((p.fmask, 8, F), (p.tmask, 25, W)):
            start, width = tab[..., 0], tab[..., 1]
            assert width.min() >= 0 and width.max() < max(1, min(mx, size))
            assert start.min() >= 0 and np.all(start < np.maximum(1, size - width))
        A.check_plan(p, n)
    # F = 1 (the raw frontend) gets no masks; a narrow map bounds the widths by its size
    raw = A.augment_plan(n, 1, 66150, DEFAULTS, 5, 0)
    assert raw.fmask is None and raw.tmask is None and int((raw.nsrc > 1).sum()) == n_mixed
    small = A.augment_plan(n, 3, 8, DEFAULTS, 5, 0)
    assert small.fmask[..., 1].max() < 3 and small.tmask[..., 1].max() < 8
    assert np.all(small.fmask[..., 0] + small.fmask[..., 1] <= 3) and np.all(small.tmask[..., 0] + small.tmask[..., 1] <= 8)
    # the same (seed, epoch) gives the same plan, another epoch or seed another
    a, b, c, d = (A.augment_plan(n, F, W, DEFAULTS, s, e) for s, e in ((9, 4), (9, 4), (9, 5), (10, 4)))
    same = lambda x, y: all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("nsrc", "src", "gain", "fmask", "tmask"))  # noqa: E731
    assert same(a, b) and not same(a, c) and not same(a, d)
    # mixup alone draws no masks, SpecAugment alone mixes nothing
    assert A.augment_plan(n, F, W, A.ProbeAugmentation(mixup_probability=0.25), 1, 0).fmask is None
    only_masks = A.augment_plan(n, F, W, A.ProbeAugmentation(spec_augment=True), 1, 0)
    assert np.all(only_masks.nsrc == 1) and np.all(only_masks.gain == np.array([1, 0, 0], np.float32))
    assert int((A.augment_plan(3, F, W, A.ProbeAugmentation(mixup_probability=0.25), 1, 0).nsrc > 1).sum()) == 0   # int(3 * 0.25) == 0
    one = A.augment_plan(1, F, W, A.ProbeAugmentation(mixup_probability=1.0), 1, 0)   # one row: its only partner is itself
    assert one.nsrc[0] == 2 and one.src[0].tolist() == [0, 0, 0]


def _awkward_rows(rng, n_rows, E):
    x = rng.standard_normal((n_rows, E)).astype(np.float32)
    x[rng.random((n_rows, E)) < 0.1] = -0.0
    sub = rng.random((n_rows, E)) < 0.1
    x[sub] = (rng.standard_normal(int(sub.sum())) * 1e-40).astype(np.float32)   # subnormals
    x[rng.random((n_rows, E)) < 0.1] *= np.float32(1e-12)
    return x


def test_augment_reference_is_the_literal_numpy_expressions():
    rng = np.random.default_rng(11)
    n_rows, F, W = 9, 20, 44
    x = _awkward_rows(rng, n_rows, F * W)
    assert np.signbit(x[x == 0]).any() and (np.abs(x[x != 0]) < np.finfo(np.float32).tiny).any()
    plan = A.augment_plan(n_rows, F, W, A.ProbeAugmentation(mixup_probability=0.7, spec_augment=True), 3, 1)
    two, three = np.flatnonzero(plan.nsrc > 1)[:2]   # one row of each kind with gains of 1e-27: subnormal products
    plan.nsrc[two], plan.src[two], plan.gain[two] = 2, (two, 5, two), (np.float32(1e-27), np.float32(1.0), 0)
    plan.nsrc[three], plan.src[three], plan.gain[three] = 3, (three, 0, three), np.float32(1e-27)
    assert set(plan.nsrc.tolist()) == {1, 2, 3}
    plan.fmask[0] = [[18, 5], [0, 0]]   # past the edge: clipped, as slicing clips
    got = A.augment_reference(x, plan)
    assert got.dtype == np.float32 and got.shape == (n_rows, F * W)
    masked = x.reshape(n_rows, F, W).copy()
    for s in range(n_rows):
        for f0, w in plan.fmask[s]:
            masked[s, f0 : f0 + w, :] = 0.0
        for t0, w in plan.tmask[s]:
            masked[s, :, t0 : t0 + w] = 0.0
    for r in range(n_rows):
        k = int(plan.nsrc[r])
        if k == 1:
            want = masked[plan.src[r, 0]]
        else:
            want = np.sum(plan.gain[r, :k].reshape(k, 1, 1) * masked[plan.src[r, :k]], axis=0)
        assert want.dtype == np.float32
        assert np.array_equal(got[r].view(np.int32), want.reshape(-1).view(np.int32)), r
    assert (np.abs(got[got != 0]) < np.finfo(np.float32).tiny).any()   # subnormal results were kept
    # an identity plan returns the rows bit for bit (-0.0 included)
    ident = A.augment_plan(n_rows, F, W, A.ProbeAugmentation(spec_augment=True, freq_mask_max=1, time_mask_max=1), 3, 1)
    assert not ident.touched().any()
    assert np.array_equal(A.augment_reference(x, ident).view(np.int32), x.view(np.int32))
    assert plan.touched().any()


def test_mixed_targets_is_maximum_reduce():
    rng = np.random.default_rng(2)
    n, C = 50, 7
    Y = (rng.random((n, C)) < 0.2).astype(np.float32)
    plan = A.augment_plan(n, 1, 10, A.ProbeAugmentation(mixup_probability=0.5), 4, 2)
    got = A.mixed_targets(Y, plan)
    for r in range(n):
        assert np.array_equal(got[r], np.maximum.reduce(Y[plan.src[r, : plan.nsrc[r]]]))
    assert got.dtype == Y.dtype and not np.array_equal(got, Y)


def _embed(proj):
    return lambda x: np.tanh(x @ proj).astype(np.float32)


def test_reference_fit_with_an_identity_plan_is_the_plain_reference_fit():
    rng = np.random.default_rng(5)
    n, F, W, D, C = 41, 4, 6, 16, 3
    x = rng.standard_normal((n, F * W)).astype(np.float32)
    Y = np.eye(C, dtype=np.float32)[rng.integers(0, C, n)]
    embed = _embed(rng.standard_normal((F * W, D)).astype(np.float32))
    ident = A.ProbeAugmentation(mixup_probability=0.0, spec_augment=True, freq_mask_max=1, time_mask_max=1)
    kw = dict(epochs=4, batch_size=8, learning_rate=0.01, seed=7, dtype=np.float32)
    Xv, Yv = embed(x[:9]), Y[:9]
    plain = lp.fit_probe_reference(embed(x), Y, Xv, Yv, **kw)
    aug = lp.fit_probe_augmented_reference(embed, x, Y, Xv, Yv, augment=ident, input_shape=(F, W), **kw)
    assert np.array_equal(plain.W.view(np.int32), aug.W.view(np.int32)) and np.array_equal(plain.b.view(np.int32), aug.b.view(np.int32))
    assert plain.history["loss"] == aug.history["loss"] and plain.history["val_loss"] == aug.history["val_loss"]
    # with the augmentation on the fit is deterministic and differs from the plain one
    on = A.ProbeAugmentation(mixup_probability=0.25, spec_augment=True, freq_mask_max=2, time_mask_max=3)
    a, b = (lp.fit_probe_augmented_reference(embed, x, Y, Xv, Yv, augment=on, input_shape=(F, W), **kw) for _ in range(2))
    assert np.array_equal(a.W, b.W) and not np.array_equal(a.W, plain.W)


class _NoModel:
    """Stands where a runner would: any use is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the refusal")


def test_refusals_fire_before_a_model_is_loaded(tmp_path):
    with pytest.raises(ValueError, match="mixup_alpha"):
        A.ProbeAugmentation(mixup_alpha=0.005, mixup_probability=0.25)
    A.ProbeAugmentation(mixup_alpha=0.0)   # (alpha is not looked at while mixup is off)
    for bad in (dict(mixup_probability=-0.1), dict(mixup_probability=1.5), dict(freq_mask_max=-1), dict(time_mask_max=-1), dict(num_freq_masks=-1),
                dict(num_time_masks=A.MAX_MASKS + 1), dict(num_freq_masks=A.MAX_MASKS + 1)):
        with pytest.raises(ValueError):
            A.ProbeAugmentation(**bad)
    x, Y = np.zeros((4, 12), np.float32), np.zeros((4, 2), np.float32)
    off, mix = A.ProbeAugmentation(), A.ProbeAugmentation(mixup_probability=0.5)
    assert not off.active and mix.active and A.ProbeAugmentation(spec_augment=True).active
    for fit, first in ((lp.fit_probe_augmented, _NoModel()), (lp.fit_probe_augmented_reference, lambda v: v)):
        with pytest.raises(ValueError, match="fit_probe"):
            fit(first, x, Y, augment=off, input_shape=(3, 4))
        with pytest.raises(ValueError, match="sigmoid"):
            fit(first, x, Y, augment=mix, input_shape=(3, 4), activation="softmax")
        with pytest.raises(ValueError, match="input_shape"):
            fit(first, x, Y, augment=mix, input_shape=(5, 4))
    # a bad plan is refused on the host: the device cannot see its tables
    plan = A.augment_plan(4, 3, 4, mix, 1, 0)
    for field, value in (("nsrc", 4), ("nsrc", 0), ("src", 4), ("src", -1)):
        broken = A.AugmentPlan(plan.nsrc.copy(), plan.src.copy(), plan.gain, None, None, 3, 4)
        getattr(broken, field)[1] = value
        with pytest.raises(ValueError):
            A.augment_reference(x, broken)
    with pytest.raises(ValueError):
        A.augment_reference(x, A.AugmentPlan(plan.nsrc, plan.src, plan.gain, np.full((4, 1, 2), -1, np.int32), None, 3, 4))
    with pytest.raises(ValueError):
        A.augment_reference(x, A.AugmentPlan(plan.nsrc, plan.src, plan.gain, np.zeros((4, A.MAX_MASKS + 1, 2), np.int32), None, 3, 4))
    # the command: bad flags end it before the model path is even looked at
    from birdnet_stm32.cli import probe as probe_cli

    base = ["--model_path", str(tmp_path / "missing.tflite"), "--data_path_train", str(tmp_path), "--output", str(tmp_path / "h")]
    for flags, word in ((["--mixup_probability", "0.25", "--mixup_alpha", "0.001"], "mixup_alpha"), (["--mixup_probability", "2"], "mixup_probability"),
                        (["--spec_augment", "--freq_mask_max", "-3"], "freq_mask_max"),
                        (["--mixup_probability", "0.25", "--activation", "softmax"], "sigmoid")):
        with pytest.raises(SystemExit, match=word):
            probe_cli.main(base + flags, runner=_NoModel())
    with pytest.raises(SystemExit, match="not found"):   # good flags get as far as the missing model
        probe_cli.main(base + ["--mixup_probability", "0.25", "--spec_augment"], runner=_NoModel())


def test_keep_inputs_refusals_need_no_device():
    from birdnet_stm32.audio.pipeline import check_inputs_budget

    check_inputs_budget(10, 257 * 256, 32 << 30)
    with pytest.raises(ValueError, match=r"\b15 rows would fit"):
        check_inputs_budget(100, 257 * 256, 15 * 257 * 256 * 4 + 5)
    with pytest.raises(ValueError, match="stream_long"):
        check_inputs_budget(1, 8, 1 << 20, stream_long=True)
    with pytest.raises(ValueError, match="measure_latency"):
        check_inputs_budget(1, 8, 1 << 20, measure_latency=True)


def test_probe_parser_without_the_new_flags_builds_the_old_namespace():
    from birdnet_stm32.cli import probe as probe_cli

    args = probe_cli.build_parser().parse_args(["--model_path", "m", "--data_path_train", "d", "--output", "o"])
    assert (args.mixup_alpha, args.mixup_probability, args.spec_augment, args.freq_mask_max, args.time_mask_max) == (0.2, 0.0, False, 8, 25)
    assert lp.augmentation_from_args(args) is None   # everything off: run_linear_probe takes the path it always took
    old = {k: v for k, v in vars(args).items() if k not in ("mixup_alpha", "mixup_probability", "spec_augment", "freq_mask_max", "time_mask_max")}
    assert lp.augmentation_from_args(argparse.Namespace(**old)) is None   # a namespace from before the flags existed
    assert old["activation"] == "sigmoid" and old["epochs"] == 50 and old["max_chunks_per_file"] == 0 and old["seed"] == 42
    on = probe_cli.build_parser().parse_args(["--model_path", "m", "--data_path_train", "d", "--output", "o", "--mixup_probability", "0.25", "--spec_augment"])
    assert lp.augmentation_from_args(on) == A.ProbeAugmentation(mixup_probability=0.25, spec_augment=True)


def test_the_binding_declares_the_entry_point():
    from birdnet_stm32 import _hip

    assert "bn_augment_inputs" in _hip.EXPORTS and _hip.AUGMENT_MAX_MASKS == A.MAX_MASKS
