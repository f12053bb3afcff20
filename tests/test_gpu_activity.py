"""bn_short_time_energy / bn_activity_counts and the selecting pipeline against audio/activity.py — for EQUALITY: the kernels repeat the float32
operation order that module spells out, so counts, stats and energies are compared bit for bit."""

from __future__ import annotations

import ctypes
import os
import wave

import numpy as np
import pytest

from conftest import KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

SR, CD, SIZE = 22050, 3.0, 66150   # the shipped model's config


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def activity():
    from birdnet_stm32.audio import activity

    return activity


def _device_counts(torch, ctx, x, k=2.0, subsample=512, want_stats=True):
    from birdnet_stm32 import _hip
    from birdnet_stm32.audio.activity import subsample_indices

    B, n = x.shape
    idx = subsample_indices(n, subsample).astype(np.int32)
    d_x, d_idx = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(idx).cuda()
    d_active = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    d_stats = torch.full((B + 1, 3), -7.0, dtype=torch.float32, device="cuda")
    _hip.check(ctx.lib.bn_activity_counts(ctx.handle, d_x.data_ptr(), B, n, d_idx.data_ptr(), idx.shape[0], k, d_active.data_ptr(),
                                          d_stats.data_ptr() if want_stats else None, None))
    torch.cuda.synchronize()
    active, stats = d_active.cpu().numpy(), d_stats.cpu().numpy()
    assert active[B] == -7 and np.all(stats[B] == -7.0)   # nothing past the last row
    return active[:B], stats[:B]


def _check_rows(torch, ctx, activity, x, k=2.0, subsample=512):
    active, stats = _device_counts(torch, ctx, x, k, subsample)
    for b in range(x.shape[0]):
        med, mad, thr, count = activity.activity_stats(x[b], k, subsample)
        want = np.array([med, mad, thr], np.float32)
        assert np.array_equal(stats[b].view(np.uint32), want.view(np.uint32)), (b, stats[b], want)
        assert int(active[b]) == count, (b, int(active[b]), count)
    return active, stats


N_SET = [1, 2, 3, 400, 511, 512, 513, 1027, 20 * 256, 65792, 66150, 72000]


@pytest.mark.parametrize("n", N_SET)
def test_activity_counts_shapes(torch_mod, ctx, activity, n):
    """Odd and even m, n = m and n = m + 1, rows that lose 16-byte alignment (n = 66150, 1027, 513, 3 with B = 3)."""
    rng = np.random.default_rng(n)
    for B in (1, 3):
        x = (rng.standard_normal((B, n)) * np.float32(10.0) ** rng.integers(-3, 3, (B, 1))).astype(np.float32)
        x[:, ::7] = np.abs(x[:, ::7]) ** 3   # a heavy tail, so that counts are neither 0 nor n
        _check_rows(torch_mod, ctx, activity, x)
    if n in (400, 65792):
        _device_counts(torch_mod, ctx, x, want_stats=False)   # d_stats may be NULL


@pytest.mark.parametrize("n", N_SET)
def test_activity_counts_more_rows_than_compute_units(torch_mod, ctx, activity, n):
    cus = torch_mod.cuda.get_device_properties(0).multi_processor_count
    x = np.random.default_rng(n + 1).standard_normal((2 * cus + 9, n)).astype(np.float32)
    x[:, 5::11] *= 6
    _check_rows(torch_mod, ctx, activity, x, k=1.5)


def test_activity_counts_1024_rows_of_65792(torch_mod, ctx, activity):
    x = np.random.default_rng(99).random((1024, 65792), dtype=np.float32)
    x[:, 3::13] **= 0.1
    _check_rows(torch_mod, ctx, activity, x)


@pytest.mark.parametrize("n", [400, 1027, 66150])
def test_activity_counts_data_cases(torch_mod, ctx, activity, n):
    rng = np.random.default_rng(7 + n)
    idx = set(activity.subsample_indices(n, 512).tolist())
    free = np.array([i for i in range(n) if i not in idx][:40]) if n > 512 else np.zeros(0, int)
    zeros = np.zeros(n, np.float32)
    const = np.full(n, 0.375, np.float32)
    half = rng.standard_normal(n).astype(np.float32)
    half[::2] = np.float32(np.median(np.abs(half)))          # half of the values tied at (about) the median
    neg = -np.abs(rng.standard_normal(n)).astype(np.float32)
    neg[::5] *= 9
    den = (rng.integers(0, 1 << 20, n).astype(np.uint32)).view(np.float32).copy()   # denormals only
    den[::3] = 0.0
    mix = den.copy()
    mix[1::4] = np.float32(1e-38)
    planted = rng.standard_normal(n).astype(np.float32)
    x = np.stack([zeros, const, half, neg, den, mix, planted])
    if free.size:   # elements equal to thresh exactly (strict >: not counted) and one ulp above (counted), outside the median's sample
        thr = activity.activity_stats(planted, 2.0, 512)[2]
        x[6, free[:20]] = thr
        x[6, free[20:30]] = -thr
        x[6, free[30:]] = np.nextafter(thr, np.float32(np.inf))
        assert activity.activity_stats(x[6], 2.0, 512)[2] == thr
    active, stats = _check_rows(torch_mod, ctx, activity, x)
    assert active[0] == 0 and stats[0].tolist() == [0.0, np.float32(1e-10), np.float32(np.float32(2.0) * np.float32(1e-10))]
    assert active[1] == 0 and stats[1, 0] == 0.375


def test_activity_counts_one_element_moves_one_count(torch_mod, ctx, activity):
    n = 66150
    x = np.random.default_rng(3).standard_normal((3, n)).astype(np.float32)
    base, stats = _check_rows(torch_mod, ctx, activity, x)
    idx = set(activity.subsample_indices(n, 512).tolist())
    j = next(i for i in range(n) if i not in idx and abs(x[1, i]) <= stats[1, 2])
    y = x.copy()
    y[1, j] = np.nextafter(stats[1, 2], np.float32(np.inf))
    moved, _ = _check_rows(torch_mod, ctx, activity, y)
    assert (moved - base).tolist() == [0, 1, 0]


def test_activity_counts_refusals(torch_mod, ctx):
    d = torch_mod.zeros(1024, device="cuda")
    di = torch_mod.zeros(1024, dtype=torch_mod.int32, device="cuda")
    f = ctx.lib.bn_activity_counts
    assert f(ctx.handle, d.data_ptr(), 1, 1024, di.data_ptr(), 513, 2.0, di.data_ptr(), None, None) == -1
    assert f(ctx.handle, d.data_ptr(), 1, 1024, di.data_ptr(), 0, 2.0, di.data_ptr(), None, None) == -1
    assert f(ctx.handle, d.data_ptr(), 1, 0, di.data_ptr(), 1, 2.0, di.data_ptr(), None, None) == -1
    assert f(ctx.handle, None, 1, 1024, di.data_ptr(), 512, 2.0, di.data_ptr(), None, None) == -1
    assert f(ctx.handle, None, 0, 1024, None, 512, 2.0, None, None, None) == 0


def test_short_time_energy(torch_mod, ctx, activity):
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.audio.pipeline import ste_frame_counts

    rng = np.random.default_rng(12)
    # the five named lengths each start at an ODD offset (even lengths keep the parity, odd ones flip it, odd pads flip it back);
    # the 66157-sample window is the one long enough (128 frames) for several passes per workgroup
    lens = np.array([901, 1024, 1536, 1535, 3001, 4097, 899, 66150 + 7, 20000])
    named = {1024: 1, 1536: 2, 1535: 3, 4097: 5, 66150 + 7: 7}
    index = np.array([0, 1, 2, 0, 4, 1, 0, 3, 2], np.int32)                        # windows 1 and 5 share a peak entry
    peaks = np.array([0.5, 0.37, 2.0, 0.731, 0.0], np.float32)                     # entry 4 (the 3001-sample window): peak 0, no division
    skip = np.array([False] * 8 + [True])                                          # the last window gets an empty slice of d_ste
    win_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for ln, w in named.items():
        assert lens[w] == ln and win_off[w] % 2 == 1, (ln, int(win_off[w]))
    mono = (rng.standard_normal(int(win_off[-1])) * 0.3).astype(np.float32)
    nf = ste_frame_counts(lens, ~skip)
    assert nf.tolist() == [0, 1, 2, 1, 4, 7, 0, 128, 0]
    frame_off = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
    total = int(frame_off[-1])
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(mono=mono, peak=peaks, win=win_off, idx=index, fo=frame_off).items()}
    d_ste = torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda")
    call = lambda fl, hop: ctx.lib.bn_short_time_energy(ctx.handle, d["mono"].data_ptr(), d["peak"].data_ptr(), d["win"].data_ptr(), d["idx"].data_ptr(),  # noqa: E731
                                                        d["fo"].data_ptr(), len(lens), fl, hop, d_ste.data_ptr(), None)
    assert call(512, 256) == -4 and call(1024, 256) == -4    # BN_ERR_UNSUPPORTED
    assert np.all(d_ste.cpu().numpy() == -7.0)
    _hip.check(call(1024, 512))
    torch.cuda.synchronize()
    got = d_ste.cpu().numpy()
    assert np.all(got[total:] == -7.0)
    for w in range(len(lens)):
        y = mono[win_off[w] : win_off[w + 1]]
        p = peaks[index[w]]
        if p > 0:
            y = y / p
        want = activity.short_time_energy(y)[: nf[w]] if nf[w] else np.zeros(0, np.float32)
        assert np.array_equal(got[frame_off[w] : frame_off[w + 1]].view(np.uint32), want.view(np.uint32)), w
        if nf[w]:
            assert np.array_equal(want, np.array([np.mean(y[f * 512 : f * 512 + 1024] ** 2) for f in range(nf[w])], np.float32))


# ------------------------------------------------------------------------------------------------------------------ end to end
def _band_burst(rng, m, lo=1500.0, hi=6500.0):
    b = rng.standard_normal(m)
    spec = np.fft.rfft(b)
    f = np.fft.rfftfreq(m, 1 / SR)
    spec[(f < lo) | (f > hi)] = 0
    b = np.fft.irfft(spec, m)
    return b / np.abs(b).max() * np.hanning(m) ** 0.25


def four_bursts(seed=4, sec=30.0, bursts=((2.0, 0.7, 0.5), (9.0, 1.3, 0.9), (16.0, 1.9, 0.35), (24.0, 2.5, 0.7))):
    """Band-limited noise bursts of different lengths in faint noise: candidate activity counts 25668 / 19552 / 15293 / 12205 / 9128 / 8593
    of 65792 with the float64 STFT (threshold 0.1 -> 6579.2): the smallest gap between neighbours is 535, to the threshold 2014."""
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.standard_normal(int(SR * sec))
    for at, dur, amp in bursts:
        a, m = int(at * SR), int(dur * SR)
        x[a : a + m] += amp * _band_burst(rng, m)
    return x


def _write_wav(path, x, sr=SR):
    x = np.atleast_2d(x.T).T
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    d = tmp_path_factory.mktemp("select")
    rng = np.random.default_rng(8)
    t = np.arange(44100 * 11) / 44100
    stereo = np.stack([0.4 * np.sin(2 * np.pi * 2100 * t) * (t % 4 < 1.5), 0.2 * np.sin(2 * np.pi * 900 * t) * (t > 6)], axis=1) + 0.01 * rng.standard_normal((t.size, 2))
    files = {"a_four.wav": (four_bursts(), SR), "b_grid.wav": (stereo, 44100), "c_short.wav": (0.3 * _band_burst(rng, int(1.2 * SR)), SR),
             "d_two.wav": (four_bursts(5, 24.0, ((3.0, 1.0, 0.6), (19.0, 2.2, 0.8))), SR), "e_silent.wav": (np.zeros(25 * SR), SR)}
    paths = []
    for name, (x, sr) in files.items():
        _write_wav(d / name, x, sr)
        paths.append(str(d / name))
    return paths


def host_selection(path, sel, features):
    """What the specification module selects from one file, on host-loaded audio: (start samples, chunks) in rank order."""
    from birdnet_stm32.audio import activity
    from birdnet_stm32.audio.io import estimate_num_chunks, load_audio_window
    from birdnet_stm32.audio.pipeline import chunk_table_arrays

    y = load_audio_window(path, sample_rate=SR, max_duration=60, chunk_duration=CD)
    if estimate_num_chunks(y.shape[0], SR, CD) > sel.candidate_chunks:
        starts = activity.smart_crop_starts(y, SR, CD, sel.candidate_chunks, sel.energy_percentile)
    else:
        starts = chunk_table_arrays(np.array([y.shape[0]]), SR, CD, 0.0)[0].tolist()
    chunks = []
    for s in starts:
        c = np.zeros(SIZE, np.float32)
        c[: min(SIZE, y.shape[0] - s)] = y[s : s + SIZE]
        chunks.append(c)
    ratios = [activity.get_activity_ratio(features(c), sel.k, sel.max_active, sel.subsample) for c in chunks]
    order = activity.rank_by_activity(ratios, sel.activity_threshold)[: sel.max_chunks_per_file]
    return [starts[i] for i in order], [chunks[i] for i in order], len(starts)


@pytest.mark.parametrize("model", ["int8", "float32"])
def test_embed_files_selects_what_the_specification_selects(torch_mod, recordings, model):
    """Rows, order, counts and start positions against the specification on host-loaded audio (features: oracle/stft.py).  The embedding
    rows are compared with ``runner.infer_audio_device`` on the host-cut float32 samples -- a proxy for "the row embed_files gives for the
    same samples cut directly": writing the cut samples to a file would quantise them, and embed_files on a file of exactly those samples
    ends in this same call (tests/test_gpu_embeddings.py::test_embed_files_and_cli pins that equality)."""
    torch = torch_mod
    from oracle import stft

    from birdnet_stm32.audio.pipeline import ChunkSelection
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner

    runner = load_model_runner(TFLITE_PATH if model == "int8" else KERAS_PATH, max_batch=8)   # (candidates take several STFT slices)
    kw = dict(sample_rate=SR, chunk_duration=CD, max_duration=60)
    plain = embed_files(runner, recordings, **kw)
    again = embed_files(runner, recordings, select=None, **kw)
    assert plain.embeddings.tobytes() == again.embeddings.tobytes() and np.array_equal(plain.start_s, again.start_s)
    assert plain.chunks_per_file.tolist() == [10, 4, 1, 8, 9] and plain.candidate_rows == 0
    sel = ChunkSelection(3, exact_stft=True)
    res = embed_files(runner, recordings, select=sel, pipeline_options=dict(group_chunks=16), **kw)   # (two groups)
    want_file, want_start, want_rows, n_cand = [], [], [], 0
    for i, p in enumerate(recordings):
        starts, chunks, cand = host_selection(p, sel, lambda c: stft.hybrid_spectrogram(c).astype(np.float32))
        n_cand += cand
        want_file += [i] * len(starts)
        want_start += starts
        want_rows.append(runner.infer_audio_device(torch.from_numpy(np.stack(chunks)).cuda(), return_embeddings=True)[1].cpu().numpy())
    assert res.file_index.tolist() == want_file
    assert np.array_equal(res.start_s, np.asarray(want_start, np.float64) / SR)
    assert res.chunks_per_file.tolist() == np.bincount(want_file, minlength=len(recordings)).tolist() and res.candidate_rows == n_cand
    assert res.chunks_per_file[0] == 3 and res.chunks_per_file[2] == 1 and res.chunks_per_file[4] == 1   # (silence: one chunk is always kept)
    assert any(s % SIZE for s in want_start)                                                            # smart-crop starts are off the grid
    assert np.array_equal(res.embeddings, np.concatenate(want_rows))
    pooled = embed_files(runner, recordings, select=sel, pooling="avg", **kw)
    assert pooled.embeddings.shape == (5, res.embeddings.shape[1])
    runner.close()


def test_fast_stft_gives_the_same_selection_on_separated_bursts(torch_mod, ctx, recordings, activity):
    """The default (float32 FFT) features may move a count by a few elements against the exact ones.  Measured here and printed; the
    recording's neighbouring candidate counts, and the last one and the threshold, lie at least ten times that apart (docs/testing.md)."""
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.audio.io import load_audio_window
    from birdnet_stm32.audio.pipeline import ChunkSelection
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner, stft_device

    sel = ChunkSelection(3)
    y = load_audio_window(recordings[0], sample_rate=SR, max_duration=60, chunk_duration=CD)
    starts = activity.smart_crop_starts(y, SR, CD, sel.candidate_chunks)
    d = torch.from_numpy(np.stack([y[s : s + SIZE] for s in starts])).cuda()
    counts = {}
    for exact in (False, True):
        spec = stft_device(ctx, d, 512, None, 256, True, exact=exact)
        counts[exact] = _device_counts(torch, ctx, spec.view(len(starts), -1).cpu().numpy())[0].astype(np.int64)
    moved = int(np.abs(counts[False] - counts[True]).max())
    ranked = np.sort(counts[True])[::-1]
    gaps = np.concatenate([ranked[:-1] - ranked[1:], [ranked[-1] - 0.1 * 257 * 256]])
    print(f"max |count_fast - count_exact| = {moved} over {len(starts)} candidates; exact counts {ranked.tolist()}, smallest gap {gaps.min():.1f}")
    assert gaps.min() >= 10 * moved and gaps.min() >= 500
    runner = load_model_runner(TFLITE_PATH, max_batch=64)
    kw = dict(sample_rate=SR, chunk_duration=CD, max_duration=60)
    fast = embed_files(runner, recordings[:1], select=sel, **kw)
    exact = embed_files(runner, recordings[:1], select=ChunkSelection(3, exact_stft=True), **kw)
    assert np.array_equal(fast.start_s, exact.start_s) and np.array_equal(fast.embeddings, exact.embeddings) and fast.chunks_per_file.tolist() == [3]
    runner.close()
    del _hip


def test_probe_trains_on_bursts_only(torch_mod, tmp_path, capsys):
    """Class folders whose files are 80 % silence: with --max_chunks_per_file 2 the probe trains on fewer rows, all of them over a burst.

    The overlap with a burst is checked on a separate ``embed_files(select=ChunkSelection(2))`` call over all eight files, not on the rows
    the probe trained on: the probe keeps no ``start_s``.  It is a proxy: the training files go through the same call with the same
    threshold (0.1); the two validation files use 0.5 in the probe, which can only drop rows of this set, never add one."""
    from birdnet_stm32.cli import probe
    from birdnet_stm32.audio.pipeline import ChunkSelection
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner

    sec, spans = 30.0, {}
    for c, cls in enumerate(("kiwi", "tui")):
        os.makedirs(tmp_path / "data" / cls)
        for i in range(4):
            at = 3.0 + 5.0 * i + c
            bursts = ((at, 2.5, 0.8), (at + 9.0 if at < 15 else at - 9.0, 2.5, 0.5))   # 5 of 30 seconds carry signal
            p = tmp_path / "data" / cls / f"{cls}{i}.wav"
            _write_wav(p, four_bursts(10 * c + i, sec, bursts))
            spans[str(p)] = [(b[0], b[0] + b[1]) for b in bursts]
    runner = load_model_runner(TFLITE_PATH, max_batch=128)
    base = ["--model_path", TFLITE_PATH, "--data_path_train", str(tmp_path / "data"), "--epochs", "2", "--val_split", "0.25", "--max_duration", "30"]
    probe.main(base + ["--output", str(tmp_path / "all")], runner=runner)
    out_all = capsys.readouterr().out
    probe.main(base + ["--output", str(tmp_path / "sel"), "--max_chunks_per_file", "2"], runner=runner)
    out_sel = capsys.readouterr().out
    rows = lambda out: int(out.split("[probe] ")[-1].split(" training rows")[0])  # noqa: E731
    assert "candidate rows ->" in out_sel and "candidate rows" not in out_all
    assert rows(out_all) == 6 * 10 and rows(out_sel) <= 6 * 2 and rows(out_sel) >= 6
    res = embed_files(runner, sorted(spans), select=ChunkSelection(2), sample_rate=SR, chunk_duration=CD, max_duration=30)
    assert len(res.start_s) >= 8
    for f, s in zip(res.file_index, res.start_s):
        assert any(s < b and s + CD > a for a, b in spans[res.paths[f]]), (res.paths[f], s)
    runner.close()
