"""audio/activity.py (the numpy specification of chunk selection) against recorded outputs of the reference's module
(tests/golden/reference_activity.json, written by tools/make_activity_fixture.py), and the host side of ChunkSelection."""

from __future__ import annotations

import json
import os
import re

import numpy as np
import pytest

import activity_cases as ac

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(REPO, "tests", "golden", "reference_activity.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def activity():
    from birdnet_stm32.audio import activity

    return activity


def _index_of(samples, got):
    return [next(i for i, s in enumerate(samples) if s is g) for g in got]


def test_smart_crop_matches_the_reference(golden, activity):
    names = {c["name"] for c in golden["crop"]}
    assert {"zeros", "short", "four_bursts", "close_bursts", "end_burst", "ties", "quantised"} <= names
    for c in golden["crop"]:
        x = ac.crop_signal(c["name"], c["seed"])
        chunks = activity.smart_crop(x, ac.SR, ac.CD, max_chunks=c["max_chunks"], energy_percentile=c["energy_percentile"])
        assert all(ch.dtype == np.float32 and ch.shape == (ac.CHUNK,) for ch in chunks)
        assert [ac.locate(ch, x) for ch in chunks] == c["starts"], c
        if c["name"] == "zeros":   # (every position of an all-zero recording matches the chunk: the centre crop is what the module documents)
            assert activity.smart_crop_starts(x, ac.SR, ac.CD) == [x.shape[0] // 2 - ac.CHUNK // 2]
        elif c["starts"][0] >= 0:
            assert activity.smart_crop_starts(x, ac.SR, ac.CD, c["max_chunks"], c["energy_percentile"]) == c["starts"]
    by = {(c["name"], c["max_chunks"]): c["starts"] for c in golden["crop"] if c["energy_percentile"] == 75.0}
    assert len(by[("four_bursts", 5)]) == 4                                 # four separated stretches
    assert by[("end_burst", 5)][0] == 10 * ac.SR - ac.CHUNK                 # clamped to n - chunk_size
    s = by[("close_bursts", 5)]
    assert all(abs(a - b) >= ac.CHUNK // 2 for i, a in enumerate(s) for b in s[:i])


def test_activity_ratio_matches_the_reference(golden, activity):
    by_name = {}
    for c in golden["activity"]:
        x = ac.activity_input(c["name"], c["seed"])
        got = activity.get_activity_ratio(x, k=c["k"], max_active=c["max_active"], subsample=c["subsample"])
        assert isinstance(got, float) and got == c["ratio"], c
        by_name.setdefault(c["name"], []).append(c)
        # activity_stats gives the count the ratio implies (a ratio that collapsed to 0.0 implies only "above max_active")
        med, mad, thr, count = activity.activity_stats(x, c["k"], c["subsample"])
        assert all(isinstance(v, np.float32) for v in (med, mad, thr))
        if c["ratio"] > 0.0:
            assert count == round(c["ratio"] * x.size) and float(count) / float(x.size) == c["ratio"]
        else:
            assert count == 0 or count / x.size > c["max_active"]
    assert by_name["broadband_map"][0]["ratio"] == 0.0 and by_name["zeros_map"][0]["ratio"] == 0.0
    med, mad, thr, count = activity.activity_stats(ac.activity_input("zeros_map", 11))
    assert (med, mad, count) == (0.0, np.float32(1e-10), 0) and thr == np.float32(np.float32(2.0) * np.float32(1e-10))
    assert activity.activity_stats(ac.activity_input("broadband_map", 13))[3] > 0.8 * 257 * 64


def test_sorts_and_random_picks_match_the_reference(golden, activity):
    for c in golden["sort"]:
        samples = ac.sort_samples(c["seed"], c["kind"])
        got = getattr(activity, c["fn"])(samples, threshold=c["threshold"])
        assert _index_of(samples, got) == c["order"], c
    samples = ac.sort_samples(21, "maps")
    for c in golden["random"]:
        np.random.seed(c["np_seed"])
        got = activity.pick_random_samples(samples, num_samples=c["num_samples"], pick_first=c["pick_first"])
        assert isinstance(got, list) == (min(c["num_samples"], len(samples)) > 1)
        assert _index_of(samples, got if isinstance(got, list) else [got]) == c["picked"], c
    assert activity.pick_random_samples([]) == []
    with pytest.raises(ValueError):
        activity.sort_by_s2n([np.zeros((2, 2, 2))])
    r = [0.3, 0.1, 0.3, 0.0]
    assert activity.rank_by_activity(r, 0.05) == [int(i) for i in np.argsort(np.array(r))[::-1] if r[i] >= 0.05]
    assert activity.rank_by_activity([0.0, 0.0], 0.5) == [int(np.argsort(np.zeros(2))[::-1][0])]


def test_short_time_energy_is_numpys_mean_bit_for_bit(golden, activity):
    for c in golden["ste"]:
        e = activity.short_time_energy(ac.ste_signal(c["seed"], c["n"]))
        assert e.dtype == np.float32 and e.view(np.uint32).tolist() == c["bits"]
    rng = np.random.default_rng(5)
    for decade in range(-4, 3):   # amplitudes 1e-4 .. 1e2: six decades
        x = (rng.standard_normal(1024 + 512 * 40) * 10.0**decade).astype(np.float32)
        want = np.array([np.mean(x[f * 512 : f * 512 + 1024] ** 2) for f in range(41)], np.float32)
        assert np.array_equal(activity.short_time_energy(x, 1024, 512).view(np.uint32), want.view(np.uint32)), decade
    x = rng.standard_normal(700).astype(np.float32)   # shorter than a frame: one (partial) frame, numpy's own mean
    assert activity.short_time_energy(x).tolist() == [np.float32(np.mean(x**2))]
    x = rng.standard_normal(3000).astype(np.float32)
    assert np.array_equal(activity.short_time_energy(x, 256, 128), np.array([np.mean(x[s : s + 256] ** 2) for s in range(0, 3000 - 255, 128)], np.float32))


def test_chunk_selection_planning():
    from birdnet_stm32.audio.pipeline import ChunkSelection, selection_from_args, ste_frame_counts

    s = ChunkSelection(3)
    assert (s.candidate_chunks, s.activity_threshold, s.k, s.max_active, s.subsample, s.energy_percentile, s.exact_stft) == (6, 0.1, 2.0, 0.8, 512, 75.0, False)
    assert [ChunkSelection(n).candidate_chunks for n in (1, 2, 3, 4, 9)] == [4, 4, 6, 8, 8]
    assert ChunkSelection(2, candidate_chunks=5).candidate_chunks == 5
    n_chunks = np.array([0, 1, 6, 7, 20])
    assert s.crops(n_chunks).tolist() == [False, False, False, True, True]          # more grid chunks than candidates
    assert s.candidate_counts(n_chunks).tolist() == [0, 1, 6, 6, 6]
    assert s.max_counts(n_chunks).tolist() == [0, 1, 3, 3, 3]                       # the planned count becomes an upper bound
    assert ste_frame_counts([500, 1024, 1535, 1536, 66157], [True] * 5).tolist() == [0, 1, 1, 2, 1 + (66157 - 1024) // 512]
    assert ste_frame_counts([66157, 66157], [False, True]).tolist() == [0, 128]
    for bad in (dict(max_chunks_per_file=0), dict(max_chunks_per_file=2, candidate_chunks=0), dict(max_chunks_per_file=2, subsample=513)):
        with pytest.raises(ValueError):
            ChunkSelection(**bad)

    class Args:
        max_chunks_per_file, activity_threshold, candidate_chunks = 2, 0.2, 0

    assert selection_from_args(Args) == ChunkSelection(2, 0.2) and selection_from_args(Args, 0.5).activity_threshold == 0.5
    Args.max_chunks_per_file = 0
    assert selection_from_args(Args) is None


def test_selection_refusals():
    from birdnet_stm32.audio.pipeline import ChunkSelection, EvaluatePipeline
    from birdnet_stm32.models import _pack as pk

    class Runner:
        ctx, device, max_batch, input_kind = None, "cpu", 64, pk.INPUT_SPECTROGRAM

    sel = ChunkSelection(2)
    with pytest.raises(ValueError, match="stream_long"):
        EvaluatePipeline(Runner, 22050, 3.0, select=sel, stream_long=True, numa_pin=False)
    with pytest.raises(ValueError, match="4096"):
        EvaluatePipeline(Runner, 8000, 0.5, select=sel, numa_pin=False)
    with pytest.raises(ValueError, match="overlap"):
        EvaluatePipeline(Runner, 22050, 3.0, 1.5, select=sel, numa_pin=False)
    Runner.input_kind = pk.INPUT_MEL
    with pytest.raises(ValueError, match="precomputed"):
        EvaluatePipeline(Runner, 22050, 3.0, select=sel, numa_pin=False)
    Runner.input_kind = pk.INPUT_WAVEFORM
    assert EvaluatePipeline(Runner, 22050, 3.0, select=sel, numa_pin=False).select is sel
    assert EvaluatePipeline(Runner, 22050, 3.0, numa_pin=False).select is None


def test_flags_parse_and_default_to_off():
    from birdnet_stm32.audio.pipeline import selection_from_args
    from birdnet_stm32.cli import embed, probe

    base = {probe: ["--model_path", "m", "--data_path_train", "d", "--output", "o"], embed: ["--model_path", "m", "--input", "i", "--output", "o"]}
    for mod, argv in base.items():
        a = mod.build_parser().parse_args(argv)
        assert (a.max_chunks_per_file, a.activity_threshold, a.candidate_chunks) == (0, 0.1, 0) and selection_from_args(a) is None
        a = mod.build_parser().parse_args(argv + ["--max_chunks_per_file", "3", "--activity_threshold", "0.2", "--candidate_chunks", "7"])
        s = selection_from_args(a)
        assert (s.max_chunks_per_file, s.activity_threshold, s.candidate_chunks) == (3, 0.2, 7)


def test_bad_selection_flags_end_in_an_error_message_in_both_commands():
    from birdnet_stm32.cli import embed, probe

    base = {probe: ["--model_path", "m", "--data_path_train", "d", "--output", "o"], embed: ["--model_path", "m", "--input", "i", "--output", "o"]}
    for mod, argv in base.items():
        for bad in (["--max_chunks_per_file", "-1"], ["--max_chunks_per_file", "2", "--candidate_chunks", "-3"]):
            with pytest.raises(SystemExit, match="error: --"):
                mod.main(argv + bad, runner=object())


def test_candidate_table_and_rank_rows():
    """The two host decisions of the selecting pipeline, on plain arrays."""
    from birdnet_stm32.audio import activity
    from birdnet_stm32.audio.pipeline import ChunkSelection, candidate_table, rank_rows

    sel = ChunkSelection(2, candidate_chunks=4)
    x = ac.crop_signal("four_bursts", 4)
    n_out = np.array([x.shape[0], 2 * ac.CHUNK + 100, 5000])
    start, valid, owner = candidate_table(n_out, [activity.short_time_energy(x), None, None], sel, ac.SR, ac.CD)
    assert start[owner == 0].tolist() == activity.smart_crop_starts(x, ac.SR, ac.CD, 4)                      # cropped: off the grid
    assert start[owner == 1].tolist() == [0, ac.CHUNK, ac.CHUNK + 100] and start[owner == 2].tolist() == [0]   # grid, tail chunk at n - size
    assert valid.tolist() == [ac.CHUNK] * 7 + [5000] and valid.dtype == np.int32
    active = np.array([100, 900, 900, 50, 7000, 10, 2000, 0])     # of 8000 elements: ratios .0125 .1125 .1125 .00625 | .875 -> 0 .00125 .25 | 0
    rows, kept = rank_rows(active, 8000, owner, 3, sel)
    assert kept.tolist() == [2, 1, 1]
    assert rows.tolist() == [2, 1, 6, 7]          # ties fall as np.argsort(r)[::-1]; above max_active counts as 0; one row is always kept
    assert candidate_table(np.zeros(0, np.int64), [], sel, ac.SR, ac.CD)[0].shape == (0,)


def test_header_and_binding_declare_the_entry_points():
    from birdnet_stm32 import _hip

    hdr = open(os.path.join(REPO, "include", "birdnet_hip.h")).read()
    for name in ("bn_short_time_energy", "bn_activity_counts"):
        assert re.search(r"BN_API int " + name + r"\(", hdr) and name in _hip.EXPORTS
    assert "audio/activity.py:12-30" in hdr and "audio/activity.py:188-209" in hdr   # the reference lines they replace
    assert len(_hip.OPTION_NAMES) == 30                                               # no run-time option was added
