"""Host-side tests of ``analyze``: the segment planner of streamed files, span resampling restated in numpy, detection selection,
times, merging and the CSV / Raven / npz writers.  No GPU."""

from __future__ import annotations

import csv
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "birdnet-stm32_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from birdnet_stm32.audio.ingest import polyphase_filter, resampled_length  # noqa: E402
from birdnet_stm32.audio.pipeline import FileTable, filter_geometry, long_files, plan_segments, span_inputs  # noqa: E402
from birdnet_stm32.evaluation import detections as D  # noqa: E402

RATES = (48000, 44100, 32000, 24000, 16000, 96000, 22050)
SR = 22050


def _geometry(sr0):
    up, down, hpp, pre = filter_geometry(sr0, SR)
    return up, down, hpp, pre


def _touched(n, n_in, up, down, hpp, pre):
    """Inputs output(s) n read, by the polyphase index formula (int64 numpy): [kmax - hpp + 1, kmax] clipped to the window."""
    if hpp == 0:
        return np.clip(n, 0, n_in), np.clip(n + 1, 0, n_in)
    kmax = (n + pre) * down // up
    return np.clip(kmax - (hpp - 1), 0, n_in), np.clip(kmax + 1, 0, n_in)


@pytest.mark.parametrize("sr0", RATES)
def test_segments_tile_and_stage_exactly_what_they_touch(sr0):
    rng = np.random.default_rng(sr0)
    up, down, hpp, pre = _geometry(sr0)
    for trial in range(3):
        n_in = int(rng.integers(1, 3 * 3600 * sr0))
        n_out = n_in if hpp == 0 else resampled_length(n_in, up, down)
        fb = int(rng.choice([2, 4, 6, 8]))
        budget = int(rng.integers((hpp + 64) * fb, 1 << 20)) if trial else 1 << 20
        segs = plan_segments(n_in, n_out, up, down, hpp, pre, fb, budget, max_out=int(rng.integers(1 << 16, 1 << 22)))
        o = np.array([s[:2] for s in segs], np.int64)
        assert o[0, 0] == 0 and o[-1, 1] == n_out
        assert np.all(o[1:, 0] == o[:-1, 1]) and np.all(o[:, 1] > o[:, 0])
        for o0, o1, s0, s1 in segs:
            assert (s1 - s0) * fb <= budget
        # staged frames = the union of what the segment's outputs touch (brute force over every output of a sample of segments)
        pick = rng.choice(len(segs), size=min(len(segs), 6), replace=False)
        for j in sorted(set(pick.tolist()) | {0, len(segs) - 1}):
            o0, o1, s0, s1 = segs[j]
            lo, hi = _touched(np.arange(o0, o1, dtype=np.int64), n_in, up, down, hpp, pre)
            nz = hi > lo
            assert nz.any()
            assert (int(lo[nz].min()), int(hi[nz].max())) == (s0, s1)
        if (n_out + pre + 4096) * down >= 1 << 32:   # past the 32-bit index: Python ints against numpy int64, no wrap-around
            o0, o1, s0, s1 = segs[-1]
            assert s1 == min(n_in, (o1 - 1 + pre) * down // up + 1) if hpp else s1 == o1


def test_segments_refuse_a_budget_below_one_output():
    up, down, hpp, pre = _geometry(48000)
    with pytest.raises(ValueError):
        plan_segments(10**6, resampled_length(10**6, up, down), up, down, hpp, pre, 2, 2 * (hpp - 1))


def test_span_inputs_clip_to_the_window():
    up, down, hpp, pre = _geometry(48000)
    assert span_inputs(0, 1, 1000, up, down, hpp, pre)[0] == 0
    n_out = resampled_length(1000, up, down)
    assert span_inputs(n_out - 5, n_out, 1000, up, down, hpp, pre)[1] == 1000
    assert span_inputs(3, 9, 100, 1, 1, 0, 0) == (3, 9)


def _span_resample(staged, s0, n_in, o0, o1, taps, up, down, hpp, pre):
    """Outputs [o0, o1) of a window of n_in frames from its staged frames [s0, s0 + len(staged)) only: the kernels' operations
    (float32 multiply, float32 add, oldest input first, zeros outside the window)."""
    n = np.arange(o0, o1, dtype=np.int64)
    if hpp == 0:
        return staged[n - s0].astype(np.float32)
    t = (n + pre) * down
    kmax, phase = t // up, t % up
    acc = np.zeros(n.shape[0], np.float32)
    for q in range(hpp):
        k = kmax - (hpp - 1) + q
        inside = (k >= 0) & (k < n_in)
        assert np.all((k[inside] >= s0) & (k[inside] < s0 + staged.shape[0])), "a segment read a frame it did not stage"
        xv = np.where(inside, staged[np.clip(k - s0, 0, staged.shape[0] - 1)], np.float32(0))
        acc = acc + xv * taps[phase, q]
    return acc


@pytest.mark.parametrize("sr0", RATES)
def test_span_resampling_equals_resample_poly(sr0):
    from scipy.signal import resample_poly

    rng = np.random.default_rng(7 + sr0)
    n_in = int(95.3 * sr0)
    t = np.arange(n_in) / sr0
    x = (0.4 * np.sin(2 * np.pi * (300 + 2000 * t / t[-1]) * t) + 0.05 * rng.standard_normal(n_in)).astype(np.float32)
    x[n_in // 3 : n_in // 3 + sr0] = 0.0
    up, down, hpp, pre = _geometry(sr0)
    if hpp:
        taps = polyphase_filter(up, down)[0]
        want = resample_poly(x, up, down).astype(np.float32)
    else:
        taps, want = None, x
    n_out = want.shape[0]
    segs = plan_segments(n_in, n_out, up, down, hpp, pre, 4, int(rng.integers(200_000, 900_000)))
    assert len(segs) > 3
    got = np.concatenate([_span_resample(x[s0:s1], s0, n_in, o0, o1, taps, up, down, hpp, pre) for o0, o1, s0, s1 in segs])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    peak = max(float(np.abs(got[o0:o1]).max()) for o0, o1, _, _ in segs)
    assert np.float32(peak) == np.abs(want).max()


def test_long_files_by_slab_and_by_index():
    n = 3
    tab = FileTable(["a.wav", "b.wav", "c.wav"], np.array([0, 0, -1], np.int32), np.zeros(n, np.int32), np.array([1, 1, 0]),
                    np.array([48000, 32000, 0]), np.array([48000 * 60, 32000 * 400, 0]), np.zeros(n, np.int64),
                    np.array([48000 * 60 * 2, 32000 * 400 * 2, 0]), np.zeros(n, np.int64), np.zeros(n, np.int64))
    tab.n_out = np.array([SR * 60, SR * 400, 0])
    assert long_files(tab, SR, 256 << 20).tolist() == [False, True, False]    # 400 s from 32 kHz: past the 32-bit index
    assert long_files(tab, SR, 1 << 20).tolist() == [True, True, False]
    sub = tab.sub(1, 3)
    assert sub.paths == ["b.wav", "c.wav"] and sub.frames.tolist() == [32000 * 400, 0]


# -- selection, times, merging ---------------------------------------------------------------------------------------------------------
def _scores():
    s = np.zeros((6, 4), np.float32)
    s[0] = [0.9, 0.1, 0.3, 0.9]
    s[1] = [0.2, 0.5, 0.5, 0.26]
    s[2] = [0.0, 0.0, 0.0, 0.0]
    s[3] = [0.3, 0.25, 0.1, 0.8]
    s[4] = [0.6, 0.0, 0.0, 0.0]
    s[5] = [0.7, 0.0, 0.4, 0.0]
    return s


def test_select_order_threshold_and_top_k():
    s = _scores()
    rows, cls = D.select(s, np.full(4, 0.25, np.float32))
    assert list(zip(rows.tolist(), cls.tolist())) == [(0, 0), (0, 3), (0, 2), (1, 1), (1, 2), (1, 3), (3, 3), (3, 0), (3, 1), (4, 0), (5, 0), (5, 2)]
    rows, cls = D.select(s, np.full(4, 0.25, np.float32), top_k=1)
    assert list(zip(rows.tolist(), cls.tolist())) == [(0, 0), (1, 1), (3, 3), (4, 0), (5, 0)]
    with pytest.raises(ValueError):
        D.select(s, np.zeros(4, np.float32), top_k=0)


def test_class_thresholds_and_unknown_names():
    names = ["A a_Aa", "B b_Bb", "C c_Cc", "D d_Dd"]
    thr = D.class_thresholds_vector(4, 0.25, {"D d_Dd": 0.85, "A a_Aa": 0.1}, names)
    assert thr.tolist() == pytest.approx([0.1, 0.25, 0.25, 0.85])
    rows, cls = D.select(_scores(), thr)
    assert (3, 3) not in set(zip(rows.tolist(), cls.tolist())) and (0, 3) in set(zip(rows.tolist(), cls.tolist()))
    assert (1, 0) in set(zip(rows.tolist(), cls.tolist()))
    with pytest.raises(ValueError, match="unknown"):
        D.class_thresholds_vector(4, 0.25, {"Nope_Nope": 0.5}, names)
    with pytest.raises(ValueError):
        D.class_thresholds_vector(4, 0.25, {"A a_Aa": 0.5}, None)


def test_times_last_chunk_alignment_and_end_clipping():
    size = SR * 3
    n_out = np.array([size * 2 + 1000, 500, 0, size])
    ct = D.chunk_table(n_out, SR, 3.0, 0.0)
    assert ct.file.tolist() == [0, 0, 0, 1, 3]
    assert ct.start.tolist() == [0, size, n_out[0] - size, 0, 0]          # the last chunk starts at n - size
    assert ct.end.tolist() == [size, 2 * size, n_out[0], 500, size]        # a short file's chunk ends at its end
    assert ct.end_s[3] == pytest.approx(500 / SR)
    ct = D.chunk_table(np.array([size + 1]), SR, 3.0, 1.5)
    assert ct.start.tolist() == [0, 1]


def test_detections_from_scores_and_merging():
    size = SR * 3
    n_out = np.array([size * 4, size * 2])     # file 0: chunks 0..3, file 1: chunks 4..5
    s = np.zeros((6, 3), np.float32)
    s[0, 1], s[1, 1], s[2, 1] = 0.5, 0.9, 0.4  # class 1 in chunks 0-2 of file 0 -> one event 0-9 s, score 0.9
    s[3, 1] = 0.3                              # ... chunk 3 as well (touching): still one event, 0-12 s
    s[1, 2] = 0.6                              # class 2 alone in chunk 1
    s[4, 1], s[5, 1] = 0.7, 0.8                # file 1: does not merge into file 0's event
    det = D.detections_from_scores(s, n_out, ["a", "b"], SR, 3.0, 0.0, min_conf=0.25)
    assert det.file_index.tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert det.class_index.tolist() == [1, 1, 2, 1, 1, 1, 1]
    assert det.start_s.tolist() == [0.0, 3.0, 3.0, 6.0, 9.0, 0.0, 3.0]
    assert det.score.dtype == np.float32 and det.score[1] == np.float32(0.9)
    m = D.detections_from_scores(s, n_out, ["a", "b"], SR, 3.0, 0.0, min_conf=0.25, merge=True)
    assert list(zip(m.file_index.tolist(), m.class_index.tolist(), m.start_s.tolist(), m.end_s.tolist())) == [
        (0, 1, 0.0, 12.0), (0, 2, 3.0, 6.0), (1, 1, 0.0, 6.0)]
    assert m.score.tolist() == [np.float32(0.9), np.float32(0.6), np.float32(0.8)]
    # a gap breaks an event; overlapping chunks merge
    s2 = np.zeros((6, 3), np.float32)
    s2[0, 0] = s2[2, 0] = 0.5
    m2 = D.detections_from_scores(s2, n_out, ["a", "b"], SR, 3.0, 0.0, merge=True)
    assert m2.start_s.tolist() == [0.0, 6.0]
    ov = D.detections_from_scores(np.full((3, 1), 0.5, np.float32), [size * 2], ["a"], SR, 3.0, 1.5, merge=True)
    assert (ov.start_s.tolist(), ov.end_s.tolist()) == ([0.0], [6.0])
    assert det.chunks_per_file.tolist() == [4, 2] and det.duration_s.tolist() == [12.0, 6.0]
    with pytest.raises(ValueError):
        D.detections_from_scores(s[:5], n_out, ["a", "b"], SR, 3.0)


# -- writers ----------------------------------------------------------------------------------------------------------------------------
NAMES = ["Actitis macularius_Spotted Sandpiper", "Plain", "Anas platyrhynchos_Mallard"]


def _det(tmp_path):
    size = SR * 3
    s = np.array([[0.91, 0.0, 0.3], [0.0, 0.26, 0.123456789], [0.5, 0.5, 0.0]], np.float32)
    paths = [str(tmp_path / "x" / "rec.wav"), str(tmp_path / "y" / "rec.wav"), str(tmp_path / "bad.wav")]
    return D.detections_from_scores(s, [size + 100, size, 0], paths, SR, 3.0, 0.0, min_conf=0.1, skipped=[paths[2]], return_scores=True), s


def test_csv_writer(tmp_path):
    det, _ = _det(tmp_path)
    out = tmp_path / "d.csv"
    D.write_csv(str(out), det, NAMES)
    rows = list(csv.reader(open(out)))
    assert tuple(rows[0]) == D.CSV_COLUMNS
    assert len(rows) == 1 + len(det)
    assert rows[1][3:6] == ["Actitis macularius", "Spotted Sandpiper", "0"]
    assert rows[3][0] == det.paths[0] and float(rows[3][1]) == pytest.approx(100 / SR, abs=1e-6) and float(rows[3][2]) == pytest.approx((SR * 3 + 100) / SR, abs=1e-6)
    assert [np.float32(float(r[6])) for r in rows[1:]] == det.score.tolist()
    assert rows[-1][3:5] == ["Plain", "Plain"] and rows[-1][0] == det.paths[1]


def test_raven_writer(tmp_path):
    det, _ = _det(tmp_path)
    written = D.write_raven(str(tmp_path / "raven"), det, NAMES)
    assert [os.path.basename(p) for p in written] == ["00000_rec.selections.txt", "00001_rec.selections.txt"]
    lines = open(written[0]).read().splitlines()
    assert lines[0].split("\t") == list(D.RAVEN_COLUMNS)
    first = lines[1].split("\t")
    assert first[:3] == ["1", "Spectrogram 1", "1"] and first[5:7] == ["0", f"{SR / 2:g}"] and first[-1] == det.paths[0]
    assert [ln.split("\t")[0] for ln in lines[1:]] == [str(i) for i in range(1, len(lines))]
    assert len(lines) - 1 == int((det.file_index == 0).sum())
    assert D.raven_table_names(["a/u.wav", "b/v.flac"]) == ["u.selections.txt", "v.selections.txt"]


def test_npz_writer_and_recomputed_selection(tmp_path):
    det, s = _det(tmp_path)
    D.write_npz(str(tmp_path / "d.npz"), det, NAMES)
    z = np.load(tmp_path / "d.npz")
    assert np.array_equal(z["scores"], s) and z["file_index"].tolist() == [0, 0, 1]
    assert z["start_s"].tolist() == [0.0, 100 / SR, 0.0] and z["chunks_per_file"].tolist() == [2, 1, 0]
    assert z["class_names"].tolist() == NAMES and z["paths"].tolist() == det.paths
    rows, cls = D.select(z["scores"], np.full(3, 0.1, np.float32))
    assert np.array_equal(z["file_index"][rows], det.file_index) and np.array_equal(cls, det.class_index)
    det.scores = None
    with pytest.raises(ValueError):
        D.write_npz(str(tmp_path / "e.npz"), det, NAMES)


def test_cli_parser_and_outputs(tmp_path):
    from birdnet_stm32 import __main__ as m
    from birdnet_stm32.cli import analyze

    assert "analyze" in m.USAGE
    a = analyze.build_parser().parse_args(["--model_path", "m.tflite", "--input", "x", "--output", "o", "--format", "csv", "npz", "--top_k", "3"])
    assert a.max_duration == 0 and a.format == ["csv", "npz"] and a.top_k == 3
    outs = analyze.output_paths(str(tmp_path / "out"), ["csv", "raven", "npz"])
    assert os.path.isdir(tmp_path / "out") and outs["raven"].endswith("raven")
    assert analyze.output_paths("f.csv", ["csv"]) == {"csv": "f.csv"}
    assert analyze.load_thresholds('{"A_B": 0.5}') == {"A_B": 0.5}
    p = tmp_path / "t.json"
    p.write_text('{"A_B": 0.7}')
    assert analyze.load_thresholds(str(p)) == {"A_B": 0.7}
