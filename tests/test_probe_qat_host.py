"""Host tests of the quantisation-aware fine-tune of a probe head (birdnet_stm32/training/probe_qat.py): the fake-quantised weights are the
exporter's, the fake-quantised logits are the exported head's bytes to within one code, the clamp mask, the numpy fit, the export's range
override and the command line's refusals.  No GPU."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

from conftest import TFLITE_PATH

HEAD_DIMS = (1, 16, 50, 256, 320)
HEAD_CLASSES = (1, 7, 100, 129)
S_IN, Z_IN = 0.0235, -128   # int8 embeddings of a ReLU backbone: all of the range above the zero point


def make_head(D, C, activation="sigmoid", spread=0.1, seed=0):
    from birdnet_stm32.training.linear_probe import ProbeHead

    rng = np.random.default_rng([seed, D, C])
    return ProbeHead(rng.normal(0.0, spread, (D, C)), rng.normal(0.0, 1.0, C), activation, [f"class{j}" for j in range(C)])


def _clusters(n, D, C, seed):
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    return np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32), np.eye(C, dtype=np.float32)[lab]


@pytest.mark.parametrize("per_tensor", [False, True], ids=["per_class", "per_tensor"])
def test_fake_quantized_weights_are_the_exporters(per_tensor):
    """``q * s_w`` of ``quantize_weights`` itself; an all-zero class takes the 5e-7 floor, and a value exactly half way between two codes
    (63.5 steps of a class whose largest weight is 127 steps: 0.5 and 1.0 are exact) rounds to the even one."""
    from birdnet_stm32.conversion.quantize import quantize_weights
    from birdnet_stm32.training.probe_qat import fake_quantize_head_weights

    W = np.random.default_rng(3).normal(0.0, 0.2, (50, 9)).astype(np.float32)
    W[:, 2] = 0.0
    W[:, 4] = np.clip(W[:, 4], -0.9, 0.9)
    W[0, 4], W[1, 4], W[2, 4] = 1.0, 0.5, -0.5
    got = fake_quantize_head_weights(W, per_tensor)
    q, s_w = quantize_weights(W.T, 0, per_tensor)
    assert got.shape == W.shape and got.dtype == np.float32 and got.flags.c_contiguous
    assert np.array_equal(got, (q.astype(np.float32) * s_w[:, None]).T)
    assert np.all(got[:, 2] == 0.0) and not np.signbit(got[:, 2]).any()
    if per_tensor:
        assert len(set(s_w.tolist())) == 1
    else:
        assert s_w[2] == np.float32(5e-7 / 127.0) and (q[4, 1], q[4, 2]) == (64, -64)   # 63.5 -> 64: half to even
        assert np.all(np.abs(got - W) <= s_w[None, :].astype(np.float64) / 2 * (1 + 2.0 ** -22))


def _logit_codes(head, qh, rows):
    """The fine-tune's forward over dequantised int8 rows: weights ``q * s_w``, float32 logits, the logit grid of ``qh``."""
    from birdnet_stm32.training.probe_qat import fake_quantize_head_weights, fake_quantize_logits

    x = ((rows.astype(np.float32) - np.float32(Z_IN)) * np.float32(S_IN)).astype(np.float32)
    z = (x @ fake_quantize_head_weights(head.W, qh.per_tensor) + head.b).astype(np.float32)
    return fake_quantize_logits(z, qh.s_out, qh.z_out)


def test_fake_quantized_logits_are_the_exported_bytes_to_one_code():
    """40 seeded heads, every second one told half its logit range so that both clamps fire.  The bias grid (s_in s_w), the Q31 multiplier
    (2^-31 relative) and the float32 logit (D 2^-24 relative) each move the value in front of the rounding by far less than one code, so the
    codes differ by at most 1, and only where that value lies next to a rounding boundary.  The share that differs is printed."""
    from birdnet_stm32.conversion.head_export import head_scores_i8_reference, quantize_head

    differ = total = 0
    low = high = 0
    for D in HEAD_DIMS:
        for C in HEAD_CLASSES:
            for shrink in (1.0, 0.5):
                head = make_head(D, C, seed=int(10 * shrink))
                rows = np.random.default_rng([D, C]).integers(-128, 128, (96, D)).astype(np.int8)
                z = ((rows.astype(np.float64) - Z_IN) * float(np.float32(S_IN))) @ head.W.astype(np.float64) + head.b
                qh = quantize_head(head, S_IN, Z_IN, shrink * float(z.min()), shrink * float(z.max()), per_tensor=bool((D + C) % 2))
                want, _ = head_scores_i8_reference(qh, rows)
                zq, codes, ok = _logit_codes(head, qh, rows)
                d = np.abs(codes.astype(np.int32) - want.astype(np.int32))
                assert d.max() <= 1, f"D={D} C={C} shrink={shrink}: codes {int(d.max())} apart"
                assert zq.dtype == np.float32 and codes.dtype == np.int8 and ok.dtype == bool
                assert np.array_equal(zq, ((codes.astype(np.float32) - np.float32(qh.z_out)) * np.float32(qh.s_out)).astype(np.float32))
                differ, total = differ + int((d != 0).sum()), total + d.size
                if shrink < 1:
                    low, high = low + int((~ok & (codes == -128)).sum()), high + int((~ok & (codes == 127)).sum())
    print(f"{differ} of {total} logit codes differ from the exported head's bytes ({100.0 * differ / total:.3f} %); clamped low {low}, high {high}")
    assert low > 0 and high > 0


def test_pass_is_false_exactly_where_the_code_leaves_the_int8_range():
    """Against the unclamped code in integers: the float32 quotient is the float64 quotient rounded once more (innocuous for a division of
    float32 operands), its rounding to an integer is exact, and so is adding the zero point."""
    from birdnet_stm32.training.probe_qat import fake_quantize_logits

    s, zp = np.float32(0.0371), -23
    on_grid = (np.arange(-140, 141, dtype=np.float32) - np.float32(zp)) * s          # codes -140 .. 140, the clamps' last and first among them
    z = np.concatenate([on_grid, np.random.default_rng(0).normal(0.0, 4.0, 4000).astype(np.float32), np.float32([1e6, -1e6, 0.0])])
    zq, codes, ok = fake_quantize_logits(z, s, zp)
    k = np.rint((z.astype(np.float64) / np.float64(s)).astype(np.float32)).astype(np.int64) + zp
    assert np.array_equal(ok, (k >= -128) & (k <= 127)) and ok.any() and (~ok).any()
    assert np.array_equal(codes, np.clip(k, -128, 127).astype(np.int8))
    assert ok[k == 127].all() and ok[k == -128].all() and not ok[k == 128].any() and not ok[k == -129].any()
    assert (k == 127).any() and (k == -128).any() and (k == 128).any() and (k == -129).any()


def test_reference_fit_is_deterministic_and_lowers_its_loss():
    from birdnet_stm32.conversion.quantize import choose_activation_params
    from birdnet_stm32.training.linear_probe import fit_probe_reference, head_scores
    from birdnet_stm32.training.probe_qat import fit_probe_qat_reference

    X, Y = _clusters(600, 32, 5, seed=1)
    Xv, Yv = _clusters(100, 32, 5, seed=2)
    head = fit_probe_reference(X, Y, epochs=2, dropout=0.0, seed=3, class_names=list("abcde"))
    z = X.astype(np.float64) @ head.W + head.b
    rng = (float(z.min()), float(z.max()))
    kw = dict(head=head, logit_range=rng, epochs=4, learning_rate=1e-3, dropout=0.0, seed=3)
    a = fit_probe_qat_reference(X, Y, Xv, Yv, **kw)
    b = fit_probe_qat_reference(X, Y, Xv, Yv, **kw)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.b, b.b) and a.history["loss"] == b.history["loss"]
    assert not np.array_equal(a.W, head.W) and a.class_names == list("abcde") and a.activation == head.activation
    print("QAT training loss per epoch", [round(v, 5) for v in a.history["loss"]], "val", [round(v, 5) for v in a.history["val_loss"]])
    assert a.history["loss"][-1] < a.history["loss"][0]
    s_out, z_out = choose_activation_params(*rng)
    assert a.history["qat"] == {"logit_range": list(rng), "logit_scale": s_out, "logit_zero_point": z_out, "per_tensor": False, "quantize_logits": True,
                                "epochs": 4}
    # the first step's loss is the loss of the fake-quantised forward of the head it starts from
    from birdnet_stm32.training.linear_probe import epoch_permutation, probe_loss
    from birdnet_stm32.training.probe_qat import _fake_quantize_logits, fake_quantize_head_weights

    idx = epoch_permutation(3, 0, 600)[:32]
    z0 = X[idx].astype(np.float64) @ fake_quantize_head_weights(head.W).astype(np.float64) + head.b.astype(np.float64)
    zq = _fake_quantize_logits(z0, s_out, z_out, np.float64)[0]
    assert a.history["step_loss"][0] == pytest.approx(float(probe_loss(1.0 / (1.0 + np.exp(-zq)), Y[idx].astype(np.float64), "sigmoid")), rel=1e-9)
    assert head_scores(X[:4].astype(np.float64), a.W.astype(np.float64), a.b.astype(np.float64), "sigmoid").shape == (4, 5)


def test_what_is_no_part_of_the_qat_phase_is_refused_by_name():
    from birdnet_stm32.training.probe_qat import fit_probe_qat_reference

    X, Y = _clusters(40, 8, 3, seed=1)
    head = make_head(8, 3)
    with pytest.raises(ValueError, match="label_smoothing"):
        fit_probe_qat_reference(X, Y, head=head, logit_range=(-1.0, 1.0), label_smoothing=0.1)
    with pytest.raises(ValueError, match="augment"):
        fit_probe_qat_reference(X, Y, head=head, logit_range=(-1.0, 1.0), augment=object())
    with pytest.raises(ValueError, match="logit range"):
        fit_probe_qat_reference(X, Y, head=head, logit_range=(2.0, 1.0))
    with pytest.raises(ValueError, match=r"\[8, 3\]"):
        fit_probe_qat_reference(X[:, :5], Y, head=head, logit_range=(-1.0, 1.0))


def test_the_exports_range_override_sets_the_logit_parameters():
    """``export_head_tflite(..., logit_range=)`` hands the range to ``quantize_head`` in place of the observed one (the device call itself
    is tested on the GPU): the logit parameters are ``choose_activation_params`` of that range, whatever the head's own logits are."""
    from birdnet_stm32.conversion.head_export import export_head_tflite, quantize_head
    from birdnet_stm32.conversion.quantize import choose_activation_params

    assert inspect.signature(export_head_tflite).parameters["logit_range"].default is None
    head = make_head(64, 7)
    for rng in ((-3.25, 9.5), (-0.001, 40.0), (0.5, 2.0)):
        qh = quantize_head(head, S_IN, Z_IN, *rng)
        assert (qh.s_out, qh.z_out) == choose_activation_params(*rng)


def test_cli_refusals(tmp_path):
    """Before a model is loaded or a file read: neither the data folder nor the output's folder exists."""
    from birdnet_stm32.cli import probe as probe_cli

    base = ["--model_path", TFLITE_PATH, "--data_path_train", str(tmp_path / "nowhere"), "--output", str(tmp_path / "no" / "head")]
    with pytest.raises(SystemExit, match="--qat_epochs needs --export_tflite"):
        probe_cli.main(base + ["--qat_epochs", "2"])
    with pytest.raises(SystemExit, match="--qat_epochs must be >= 0"):
        probe_cli.main(base + ["--export_tflite", "--qat_epochs", "-1"])
    with pytest.raises(SystemExit, match="--qat_learning_rate must be finite and > 0"):
        probe_cli.main(base + ["--export_tflite", "--qat_epochs", "2", "--qat_learning_rate", "0"])
    assert not (tmp_path / "no").exists()
    args = probe_cli.build_parser().parse_args(base)
    assert args.qat_epochs == 0 and args.qat_learning_rate == 1e-4
