"""The device bootstrap (bn_bootstrap_*, birdnet_stm32/evaluation/bootstrap.py) on a real MI355X: multiplicities against
``np.bincount(rng.integers(...))`` exactly, average precisions against scikit-learn resample by resample within
``2 n 2^-53`` (the terms are bit-equal, only the order of the sum differs), and ``bootstrap_ap_ci_device`` / the evaluate
command against ``metrics.bootstrap_ap_ci``."""

import json
import warnings

import numpy as np
import pytest

from conftest import CONFIG_PATH, TFLITE_PATH, synth_chunks

pytestmark = pytest.mark.gpu

NAN_I32 = 0x7FC0BEEF
NAN_I64 = 0x7FF8DEADBEEF0001


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; there is no CPU fallback to fall back to")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bs():
    from birdnet_stm32.evaluation import bootstrap

    return bootstrap


def _numpy_counts(seed, n, B, skip_draws=0):
    g = np.random.default_rng(seed)
    if skip_draws:
        g.integers(0, n, size=skip_draws)
    return np.stack([np.bincount(g.integers(0, n, size=n), minlength=n) for _ in range(B)])


def _device_counts(torch, ctx, bs, seed, n, B, skip_draws=0):
    state, inc = bs.generator_state(seed)
    start = bs.bounded_draws_reference(state, inc, n, skip_draws)[1] if skip_draws else 0
    ranges = bs.device_ranges(ctx, state, inc, n, B, start)
    out = torch.full((B, n), NAN_I32, dtype=torch.int32, device="cuda")
    got = bs.bootstrap_counts_device(ctx, state, inc, n, ranges, out=out)
    return got, ranges


# (4097, 8) starts behind 3 * 4097 accepted draws: an odd offset, as the second consuming class of a run finds it
@pytest.mark.parametrize("n,B,skip", [(1, 3, 0), (2, 5, 0), (60, 25, 0), (255, 4, 0), (256, 4, 0), (257, 4, 0), (4097, 8, 3 * 4097), (32768, 2, 0)])
def test_counts_equal_numpy_bincount(torch_mod, ctx, bs, n, B, skip):
    assert n <= bs.MAX_N == 32768
    got, ranges = _device_counts(torch_mod, ctx, bs, 42, n, B, skip)
    want = _numpy_counts(42, n, B, skip)
    assert got.dtype == np.uint32 and got.shape == (B, n)
    assert (got.sum(axis=1) == n).all()
    assert np.array_equal(got, want)
    assert (ranges[:, 1] - ranges[:, 0] >= n).all()


def test_counts_across_rejections_24576_by_128(torch_mod, ctx, bs):
    n, B = 24576, 128
    state, inc = bs.generator_state(42)
    # from the numpy specification, before any device output is looked at: the tested stream holds rejections (one slip misplaces every
    # later resample)
    want_rej = bs.rejected_positions_reference(state, inc, n, 0, n * B + 14)
    assert want_rej.size == 14 and want_rej.size >= 1
    assert bs.bounded_draws_reference(state, inc, n, n * B)[1] == n * B + 14
    got_rej = bs.rejected_positions_device(ctx, state, inc, n, 0, n * B + 14)
    assert np.array_equal(got_rej, want_rej)
    got, ranges = _device_counts(torch_mod, ctx, bs, 42, n, B)
    assert np.array_equal(ranges, bs.resample_ranges(want_rej, n, B)) and int(ranges[-1, 1]) == n * B + 14
    assert np.array_equal(got, _numpy_counts(42, n, B))
    # the list does not truncate: too small a capacity is an error that names the count
    from birdnet_stm32 import _hip

    with pytest.raises(_hip.HipError, match="14 rejected positions"):
        bs.rejected_positions_device(ctx, state, inc, n, 0, n * B + 14, capacity=5)
    # a small call after the large one (the workspace is reused), twice for the same bits
    small, _ = _device_counts(torch_mod, ctx, bs, 42, 60, 25)
    again, _ = _device_counts(torch_mod, ctx, bs, 42, 60, 25)
    assert np.array_equal(small, _numpy_counts(42, 60, 25)) and np.array_equal(small, again)


def _lattice(rng, n):
    return (np.floor(rng.random(n) ** 3 * 256) / 256).astype(np.float32)  # the INT8 model's scores: multiples of 1/256, long runs of equal ones


def _ap_cases():
    rng = np.random.default_rng(11)
    cases = {}
    n = 1000
    s = np.stack([_lattice(rng, n), np.full(n, 0.25, np.float32), rng.permutation(n).astype(np.float32) / np.float32(n)], axis=1)
    t = (rng.random((n, 3)) < 0.1).astype(np.uint8)
    cases["lattice_equal_distinct_1000"] = (s, t)
    s3 = np.array([[0.5], [0.25], [0.25]], np.float32)
    cases["n3_one_positive"] = (s3, np.array([[1], [0], [0]], np.uint8))
    n = 257
    t257 = np.ones((n, 2), np.uint8)
    t257[100, 0] = 0
    t257[0, 1] = 0
    cases["n257_256_positives"] = (np.stack([_lattice(rng, n), rng.permutation(n).astype(np.float32)], axis=1), t257)
    return cases


_AP_CASES = _ap_cases()


def _sklearn_aps(seed, s, t, ids, B):
    """The reference's loop (metrics.bootstrap_ap_ci), keeping every resample: NaN where it drops one."""
    from sklearn.metrics import average_precision_score

    g = np.random.default_rng(seed)
    n = s.shape[0]
    out = np.full((len(ids), B), np.nan)
    for i, c in enumerate(ids):
        for b in range(B):
            pick = g.integers(0, n, size=n)
            k = int(t[pick, c].sum())
            if 0 < k < n:
                out[i, b] = average_precision_score(t[pick, c], s[pick, c])
    return out


@pytest.mark.parametrize("case", sorted(_AP_CASES))
def test_ap_equals_sklearn_resample_by_resample(torch_mod, ctx, bs, case):
    s, t = _AP_CASES[case]
    n, C = s.shape
    B, seed = 48, 5
    ids = list(range(C))
    state, inc = bs.generator_state(seed)
    ranges = bs.device_ranges(ctx, state, inc, n, C * B)
    out = torch_mod.full((C, B), NAN_I64, dtype=torch_mod.int64, device="cuda").view(torch_mod.float64)
    got, cols = bs.bootstrap_ap_device(ctx, state, inc, s, t, ids, B, ranges, out=out)
    want = _sklearn_aps(seed, s, t, ids, B)
    dropped = np.isnan(want)
    print(case, "dropped", int(dropped.sum()), "of", dropped.size, "max |diff|", np.nanmax(np.abs(got - want)) if (~dropped).any() else None,
          "tolerance", bs.ap_tolerance(n))
    assert np.array_equal(np.isnan(got), dropped)
    assert (got.view(np.uint64)[dropped] == 0x7FF8000000000000).all()  # written, not the pattern the output was filled with
    assert (np.abs(got - want)[~dropped] <= bs.ap_tolerance(n)).all()
    if case == "n3_one_positive":
        assert 0.15 * B < dropped.sum() < 0.5 * B  # (2/3)^3 = 30 % of the resamples miss the positive
    if case == "n257_256_positives":
        assert dropped.any() and not dropped.all()  # (256/257)^257 = 37 % miss the negative
    # the same numbers from the numpy specification of the kernel's arithmetic, and the same bits from a second call
    counts = bs.bootstrap_counts_device(ctx, state, inc, n, ranges[:B])
    o = cols[0]
    for b in range(0, B, 7):
        ref = bs.ap_from_counts_reference(counts[b][o], t[o, 0], s[o, 0])
        assert (np.isnan(ref) and np.isnan(got[0, b])) or abs(ref - got[0, b]) <= bs.ap_tolerance(n)
    again, _ = bs.bootstrap_ap_device(ctx, state, inc, s, t, ids, B, ranges)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


def _check_rows(bs, got, want, n):
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert set(g) == set(w) == {"class", "ap", "ci_lower", "ci_upper", "n_positive", "n_total"}
        assert g["class"] == w["class"] and g["n_positive"] == w["n_positive"] and g["n_total"] == w["n_total"] == n
        assert g["ap"] == w["ap"] or (np.isnan(g["ap"]) and np.isnan(w["ap"]))
        for k in ("ci_lower", "ci_upper"):
            worst = max(worst, abs(g[k] - w[k]))
            assert abs(g[k] - w[k]) <= bs.ap_tolerance(n), (g, w)
    print("max |interval bound - host|", worst, "tolerance", bs.ap_tolerance(n))


def test_ci_device_matches_host_60_by_6_with_skipped_classes(ctx, bs):
    """The recipe of test_metric_helpers_match_their_definitions, the positive-free class in the MIDDLE column and an all-positive column
    added: neither consumes the generator, so the stream offsets of the classes behind them depend on the skips."""
    from birdnet_stm32.evaluation.metrics import bootstrap_ap_ci

    rng = np.random.default_rng(3)
    yt = (rng.random((60, 6)) < 0.3).astype(np.float32)
    yt[:, 2] = 0
    yt[:, 4] = 1
    ys = np.round(rng.random((60, 6)), 2).astype(np.float32)  # ties on purpose
    names = list("abcdef")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (no positives in a class: the library says so)
        want = bootstrap_ap_ci(yt, ys, names, n_bootstrap=25, seed=7)
        got = bs.bootstrap_ap_ci_device(yt, ys, names, n_bootstrap=25, seed=7, ctx=ctx)
        again = bs.bootstrap_ap_ci_device(yt, ys, names, n_bootstrap=25, seed=7, ctx=ctx)
    _check_rows(bs, got, want, 60)
    assert got == again
    assert got[2]["ci_lower"] == got[2]["ci_upper"] == got[2]["ap"] and got[4]["ci_lower"] == got[4]["ci_upper"] == got[4]["ap"]
    assert got[5]["ci_lower"] < got[5]["ci_upper"]


def test_ci_device_matches_host_1000_by_12(ctx, bs):
    from birdnet_stm32.evaluation.metrics import bootstrap_ap_ci

    rng = np.random.default_rng(21)
    n, C = 1000, 12
    yt = (rng.random((n, C)) < 0.05).astype(np.float32)
    ys = np.stack([_lattice(rng, n) for _ in range(C)], axis=1)
    names = [f"c{i}" for i in range(C)]
    want = bootstrap_ap_ci(yt, ys, names, n_bootstrap=50, confidence=0.9)
    got = bs.bootstrap_ap_ci_device(yt, ys, names, n_bootstrap=50, confidence=0.9, ctx=ctx)
    _check_rows(bs, got, want, n)


def test_fallbacks_return_the_host_result_with_a_warning(ctx, bs, monkeypatch):
    from birdnet_stm32.evaluation.metrics import bootstrap_ap_ci

    rng = np.random.default_rng(2)
    n = bs.MAX_N + 1
    yt = (rng.random((n, 2)) < 0.5).astype(np.float32)
    ys = _lattice(rng, 2 * n).reshape(n, 2)
    want = bootstrap_ap_ci(yt, ys, ["a", "b"], n_bootstrap=1)
    with pytest.warns(RuntimeWarning, match="exceed the device limit"):
        assert bs.bootstrap_ap_ci_device(yt, ys, ["a", "b"], n_bootstrap=1, ctx=ctx) == want
    yt, ys = yt[:500], ys[:500]
    want = bootstrap_ap_ci(yt, ys, ["a", "b"], n_bootstrap=10)
    with pytest.warns(RuntimeWarning, match="not finite float32"):
        assert bs.bootstrap_ap_ci_device(yt, ys.astype(np.float64), ["a", "b"], n_bootstrap=10, ctx=ctx) == want
    # numpy's stream is not the restated one (the comparison is forced to say so, numpy itself is untouched)
    monkeypatch.setattr(bs, "_guard_passed", None)
    monkeypatch.setattr(bs, "_counts_match", lambda a, b: False)
    with pytest.warns(RuntimeWarning, match="stream is not the one"):
        assert bs.bootstrap_ap_ci_device(yt, ys, ["a", "b"], n_bootstrap=10, ctx=ctx) == want


def test_cli_evaluate_species_report(torch_mod, bs, tmp_path, monkeypatch, capsys):
    """`evaluate --species_report --n_bootstrap 20` with the real runner: the device intervals against bootstrap_ap_ci on the y_true /
    y_scores the command computed; `--bootstrap_backend host` gives bootstrap_ap_ci's rows themselves."""
    import birdnet_stm32.cli.evaluate as cli
    import birdnet_stm32.evaluation.metrics as metrics
    from birdnet_stm32.audio.io import save_wav

    cfg = json.load(open(CONFIG_PATH))
    cfg.update(sample_rate=24000, hop_length=281)
    (tmp_path / "model_cfg.json").write_text(json.dumps(cfg))
    x = synth_chunks(16)
    for i in range(16):
        d = tmp_path / "data" / cfg["class_names"][i % 4]
        d.mkdir(parents=True, exist_ok=True)
        save_wav(x[i], str(d / f"c{i}.wav"), 24000)
    seen = {}
    real_evaluate, real_save = metrics.evaluate, cli.save_species_report_csv

    def evaluate_spy(*a, **kw):
        out = real_evaluate(*a, **kw)
        seen["y_true"], seen["y_scores"] = out[2], out[3]
        return out

    def save_spy(rows, path):
        seen["rows"] = rows
        return real_save(rows, path)

    monkeypatch.setattr(metrics, "evaluate", evaluate_spy)
    monkeypatch.setattr(cli, "save_species_report_csv", save_spy)
    argv = ["--model_path", TFLITE_PATH, "--model_config", str(tmp_path / "model_cfg.json"), "--data_path_test", str(tmp_path / "data"),
            "--species_report", str(tmp_path / "species.csv"), "--n_bootstrap", "20", "--max_batch", "16"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        cli.main(argv)
        assert "classes, device)" in capsys.readouterr().out
        want = metrics.bootstrap_ap_ci(seen["y_true"], seen["y_scores"], cfg["class_names"], n_bootstrap=20)
        assert seen["y_true"].shape == (16, 100) and sum(1 for r in want if r["ci_lower"] < r["ci_upper"]) >= 1
        _check_rows(bs, seen["rows"], want, 16)
        assert (tmp_path / "species.csv").read_text().count("\n") == 101
        cli.main(argv + ["--bootstrap_backend", "host"])
        assert "classes, host)" in capsys.readouterr().out
        assert seen["rows"] == metrics.bootstrap_ap_ci(seen["y_true"], seen["y_scores"], cfg["class_names"], n_bootstrap=20)
