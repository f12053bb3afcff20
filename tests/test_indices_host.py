"""Host tests of indices (evaluation/indices.py, cli/indices.py): the specification against values worked by hand and against the known
answers of synthetic audio, scale invariance, band-to-bin conversion at the edges, the windows of ``aggregate``, every refusal of
``IndexParams`` and the command line, the PNG encoder against a zlib decode, and the agreement of parser, dispatcher, module doc,
header and bindings.  No device."""

import json
import math
import os
import re
import struct
import zlib

import numpy as np
import pytest

import indices_cases as cases
from birdnet_stm32.cli import indices as cli
from birdnet_stm32.evaluation import indices as IX

SR = cases.SAMPLE_RATE


def _col(name):
    return IX.INDEX_COLUMNS.index(name)


def test_columns_and_limits():
    assert IX.INDEX_COLUMNS == ("aci", "hf", "ht", "h", "ndsi", "bi", "adi", "aei") and IX.SPECTRAL_COLUMNS == ("aci", "ent", "cvr")
    assert cli.CSV_COLUMNS == ("file", "start_s", "end_s", "chunks") + IX.INDEX_COLUMNS
    assert (IX.N_BINS, IX.N_SCALARS, IX.MAX_BANDS, IX.MIN_WIDTH, IX.MAX_WIDTH) == (257, 8, 16, 2, 1024)
    p = IX.IndexParams()
    assert (p.anthro, p.bio, p.db, p.band_hz, p.max_hz) == ((1000.0, 2000.0), (2000.0, 8000.0), -50.0, 1000.0, 10000.0)


def test_spot_values_by_hand():
    """257 x 4: bin 30 (1292 Hz, anthrophony) holds 1 1 1 1, bin 100 (4307 Hz, biophony) holds 2 0 2 0, everything else 0."""
    S = np.zeros((257, 4), np.float32)
    S[30], S[100] = [1, 1, 1, 1], [2, 0, 2, 0]
    scalars, bins = IX.indices_reference(S, SR)
    ln = math.log
    # r = 4, 4; |dS| = 0, 6; p = 4, 8; e = 5 1 5 1
    assert bins[0, 30] == 0.0 and bins[0, 100] == 1.5 and np.count_nonzero(bins[0]) == 1
    assert scalars[_col("aci")] == 1.5
    hf = -(1 / 3 * ln(1 / 3) + 2 / 3 * ln(2 / 3)) / ln(257)
    ht = -(2 * 5 / 12 * ln(5 / 12) + 2 * 1 / 12 * ln(1 / 12)) / ln(4)
    assert scalars[_col("hf")] == pytest.approx(hf, rel=1e-14) and scalars[_col("ht")] == pytest.approx(ht, rel=1e-14)
    assert scalars[_col("h")] == pytest.approx(hf * ht, rel=1e-14)
    assert scalars[_col("ndsi")] == pytest.approx((8 - 4) / 12, rel=1e-15)
    # biophony: bins 47 .. 185; L_100 = 10 log10(8 / 4), every other bin sits on the floor 10 log10(1e-12 * 2^2)
    assert IX.band_bins(2000, 8000, SR) == (47, 186) and IX.band_bins(1000, 2000, SR) == (24, 47)
    bi = (10 * math.log10(2.0) - 10 * math.log10(4e-12)) * (SR / 512 / 1000)
    assert scalars[_col("bi")] == pytest.approx(bi, rel=1e-13)
    # cover: thr = 2 * 10^-2.5; bin 30 has 4 cells above it, bin 100 has 2; bands of 1 kHz: band 1 = bins 24 .. 46, band 4 = bins 93 .. 116
    assert IX.diversity_edges(IX.IndexParams(), SR).tolist() == [0, 24, 47, 70, 93, 117, 140, 163, 186, 209, 233]
    assert bins[2, 30] == 1.0 and bins[2, 100] == 0.5 and np.count_nonzero(bins[2]) == 2
    c1, c4 = 4 / (23 * 4), 2 / (24 * 4)
    q1, q4 = c1 / (c1 + c4), c4 / (c1 + c4)
    assert scalars[_col("adi")] == pytest.approx(-(q1 * ln(q1) + q4 * ln(q4)), rel=1e-14)
    assert scalars[_col("aei")] == pytest.approx(2 * (9 * c4 + 10 * c1) / (10 * (c1 + c4)) - 11 / 10, rel=1e-14)
    # 1 - H(1 1 1 1) = 0; 1 - H(4 0 4 0) = 1 - ln 2 / ln 4
    assert bins[1, 30] == pytest.approx(0.0, abs=1e-15) and bins[1, 100] == pytest.approx(0.5, rel=1e-15) and np.count_nonzero(bins[1]) <= 2
    per_bin, per_band = IX.cover_counts(S, SR, IX.IndexParams())
    assert per_bin[30] == 4 and per_bin[100] == 2 and per_band.tolist() == [0, 4, 0, 0, 2, 0, 0, 0, 0, 0]
    # the float32 restatement agrees where everything is exact
    s32, b32 = IX.indices_reference_f32(S, SR)
    assert s32.dtype == np.float32 and b32.dtype == np.float32
    assert s32[_col("aci")] == 1.5 and s32[_col("ndsi")] == np.float32(4) / np.float32(12) and np.array_equal(b32[2], bins[2].astype(np.float32))


def _family(key: str):
    """``indices_reference`` of one signal family at W = 256."""
    name, keys = {"tone3k": ("tones_noise_w256", 0), "noise": ("tones_noise_w256", 2), "zeros": ("chirps_zeros_tone_w256", 1),
                  "tone1k5": ("chirps_zeros_tone_w256", 2)}[key]
    s, b = cases.reference("float", name)
    return s[keys], b[keys]


def test_known_answers_on_synthetic_audio():
    s, _ = _family("tone3k")
    assert s[_col("ndsi")] > 0.999
    s, _ = _family("tone1k5")
    assert s[_col("ndsi")] < -0.999
    s, _ = _family("noise")
    assert s[_col("hf")] > 0.99 and abs(s[_col("adi")] - math.log(10)) < 1e-3 and s[_col("aei")] < 0.01
    s, b = _family("zeros")
    assert not s.any() and not b.any()
    s32, b32 = cases.reference_f32("float", "chirps_zeros_tone_w256")
    assert not s32[1].any() and not b32[1].any()
    for kind, group in (("float", cases.float_cases()), ("int", cases.integer_cases())):
        for name, S in group:
            s, b = cases.reference(kind, name)
            assert S.shape == (cases.BATCH, 257, int(name.rsplit("w", 1)[1])) and np.isfinite(s).all() and np.isfinite(b).all(), name
            if kind == "int":
                assert np.array_equal(S, np.rint(S)) and S.min() >= 0 and S.max() <= 15
    zeros = dict(cases.integer_cases())["zeros_w6"]
    assert not zeros[1].any() and not zeros[2, :256].any() and zeros[2, 256].all() and not zeros[0, [0, 5, 46, 47, 100, 255]].any()
    edges = dict(cases.integer_cases())["edges_w6"][0]
    assert np.flatnonzero(edges.any(axis=1)).tolist() == cases.band_edge_bins()


def test_yardstick_constants_cover_the_measurement():
    rel, ab = cases.measure_yardstick()
    assert cases.YARDSTICK_REL / 4 <= rel <= cases.YARDSTICK_REL, rel
    assert cases.YARDSTICK_ABS / 4 <= ab <= cases.YARDSTICK_ABS, ab
    assert cases.RTOL == 8 * cases.YARDSTICK_REL and cases.ATOL == 8 * cases.YARDSTICK_ABS


def test_scale_invariance():
    """x 0.37 moves nothing by more than 1e-6 relative: every scalar relative to its own value, every per-bin channel relative to the
    channel's largest value.  (The scaled magnitudes are rounded to float32 again, 6e-8 per cell; ``ACI_f`` of a steady tone's bin is a sum
    of differences of nearly equal cells, 5e-5 in all, and amplifies that rounding to 1e-4 of its own value — 1e-8 of the channel's
    scale.  Measured: scalars within 4e-8, channels within 3e-8 of their largest value.)"""
    for name, S in cases.float_cases():
        if "w256" not in name:
            continue
        for i in range(S.shape[0]):
            a, fa = IX.indices_reference(S[i], SR)
            b, fb = IX.indices_reference(S[i] * np.float32(0.37), SR)
            assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(np.abs(a), np.abs(b))), (name, i, a, b)
            assert np.all(np.abs(fa - fb) <= 1e-6 * np.abs(fa).max(axis=1, keepdims=True)), (name, i)
            assert np.array_equal(fa[2], fb[2]), "the cover counts of these inputs do not move at all"


def test_band_to_bin_conversion_at_the_edges():
    f = IX.bin_frequencies(SR)
    assert f[1] == SR / 512 and f[256] == SR / 2
    # a band edge exactly on a bin: lo is inside, hi is outside
    assert IX.band_bins(f[10], f[20], SR) == (10, 20)
    assert IX.band_bins(np.nextafter(f[10], 0), np.nextafter(f[20], 1e9), SR) == (10, 21)
    assert IX.band_bins(np.nextafter(f[10], 1e9), np.nextafter(f[20], 0), SR) == (11, 20)
    assert IX.band_bins(0, SR / 2, SR) == (0, 256) and IX.band_bins(0, 1e9, SR) == (0, 257)
    for lo, hi in ((1000, 2000), (2000, 8000)):
        k0, k1 = IX.band_bins(lo, hi, SR)
        assert f[k0] >= lo > f[k0 - 1] and f[k1 - 1] < hi <= f[k1]
    assert cases.band_edge_bins() == [24, 46, 47, 185]
    # 48 kHz: bins are 93.75 Hz apart, 1000 Hz is not on a bin, 3000 Hz is
    assert IX.band_bins(1000, 3000, 48000) == (11, 32)
    dp = IX.device_params(IX.IndexParams(), SR)
    assert (dp.anthro_k0, dp.anthro_k1, dp.bio_k0, dp.bio_k1, dp.n_bands) == (24, 47, 47, 186, 10)
    assert list(dp.band_edge) == [0, 24, 47, 70, 93, 117, 140, 163, 186, 209, 233] + [233] * 6
    assert np.float32(dp.cover_ratio) == np.float32(10.0 ** -2.5) and np.float32(dp.df_khz) == np.float32(SR / 512 / 1000)
    assert IX.device_params(IX.IndexParams(max_hz=20000.0), SR).n_bands == 11   # clipped at Nyquist, whole bands only


def test_aggregate_by_hand():
    rows = np.array([[1.0, 10.0], [3.0, 30.0], [5.0, 50.0], [9.0, 70.0], [2.0, 4.0]], np.float32)
    file = np.array([0, 0, 0, 0, 1])
    start = np.array([0.0, 3.0, 6.0, 7.0, 0.0])   # file 0 is 10 s long: its last chunk starts at n - size = 7
    end = start + 3.0
    t = IX.aggregate(rows, file, start, 5.0, end)
    assert t.file_index.tolist() == [0, 0, 1] and t.start_s.tolist() == [0.0, 5.0, 0.0] and t.end_s.tolist() == [6.0, 10.0, 3.0]
    assert t.chunks.tolist() == [2, 2, 1] and t.values.tolist() == [[2.0, 20.0], [7.0, 60.0], [2.0, 4.0]] and len(t) == 3
    # the default window holds everything of a file; order does not matter
    perm = np.array([4, 2, 0, 3, 1])
    t = IX.aggregate(rows[perm], file[perm], start[perm])
    assert t.file_index.tolist() == [0, 1] and t.chunks.tolist() == [4, 1] and t.values.tolist() == [[4.5, 40.0], [2.0, 4.0]]
    assert t.end_s.tolist() == [7.0, 0.0]   # (no chunk ends given: the start of the last chunk)
    # window_s = 0: one row per chunk, as given
    t = IX.aggregate(rows, file, start, 0.0, end)
    assert t.chunks.tolist() == [1] * 5 and np.array_equal(t.values, rows) and t.start_s.tolist() == start.tolist() and t.end_s.tolist() == end.tolist()
    assert len(IX.aggregate(np.zeros((0, 8)), [], [], 60.0)) == 0
    with pytest.raises(ValueError, match="window_s"):
        IX.aggregate(rows, file, start, -1.0)
    with pytest.raises(ValueError, match="5 rows need"):
        IX.aggregate(rows, file[:4], start)


def test_index_params_refusals():
    ok = IX.IndexParams()
    assert ok.validate(SR) is ok and ok.validate(48000) is ok
    for kw, sr, match in ((dict(bio=(2000.0, 12000.0)), SR, "bio band 2000-12000 Hz does not fit below 11025"),
                          (dict(), 12000, "bio band 2000-8000 Hz does not fit below 6000"),
                          (dict(anthro=(2000.0, 1000.0)), SR, "anthro band"),
                          (dict(anthro=(-5.0, 1000.0)), SR, "anthro band"),
                          (dict(anthro=(1000.0, 1001.0)), SR, "holds no bin"),
                          (dict(bio=(2000.0, float("nan"))), SR, "two frequencies"),
                          (dict(db=3.0), SR, "db threshold"),
                          (dict(db=float("-inf")), SR, "db threshold"),
                          (dict(band_hz=0.0), SR, "band_hz"),
                          (dict(band_hz=10.0), SR, "at most 16"),
                          (dict(band_hz=20000.0), SR, "no whole band"),
                          (dict(max_hz=-1.0), SR, "max_hz"),
                          (dict(), 0, "sample_rate")):
        with pytest.raises(ValueError, match=match):
            IX.IndexParams(**kw).validate(sr)
    with pytest.raises(ValueError, match="magnitudes"):
        IX.indices_reference(np.zeros((256, 8), np.float32), SR)
    with pytest.raises(ValueError, match="magnitudes"):
        IX.indices_reference(np.zeros((257, 1), np.float32), SR)


def _decode_png(data: bytes) -> np.ndarray:
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos : pos + 4])
        kind, body = data[pos + 4 : pos + 8], data[pos + 8 : pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n : pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


def test_png_decodes_back(tmp_path):
    rng = np.random.default_rng(1)
    for shape in ((257, 7, 3), (1, 1, 3), (5, 300, 3)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        assert np.array_equal(_decode_png(cli.encode_png(img)), img)
    with pytest.raises(ValueError):
        cli.encode_png(np.zeros((4, 4), np.uint8))
    # the map: time along x, frequency upwards, channels scaled between LDFC_BOUNDS
    assert cli.LDFC_BOUNDS == {"aci": (0.4, 0.7), "ent": (0.0, 0.6), "cvr": (0.0, 1.0)}
    aci = np.zeros((2, 257))
    ent, cvr = aci.copy(), aci.copy()
    aci[1, 256], aci[0, 0], ent[0, 3], cvr[1, 5] = 0.7, 0.55, 0.9, 0.25
    img = cli.ldfc_image(aci, ent, cvr)
    assert img.shape == (257, 2, 3) and img.dtype == np.uint8
    assert img[0, 1].tolist() == [255, 0, 0] and img[256, 0].tolist() == [128, 0, 0] and img[253, 0].tolist() == [0, 255, 0] and img[251, 1].tolist() == [0, 0, 64]
    assert cli.ldfc_paths("m.png", 1) == ["m.png"] and cli.ldfc_paths("d/m.png", 3) == ["d/m_0.png", "d/m_1.png", "d/m_2.png"]
    # the writers, from a hand-made table
    values = np.zeros((3, 8 + 3 * 257))
    values[:, :8] = np.arange(24).reshape(3, 8) / 7.0
    values[2, 8 + 256] = 0.7
    table = IX.IndexTable(np.array([0, 0, 2]), np.array([0.0, 60.0, 0.0]), np.array([60.0, 63.0, 9.0]), np.array([20, 1, 3]), values)
    paths = ["a.wav", "b.wav", "c.wav"]
    out = tmp_path / "i.csv"
    assert cli.write_indices_csv(str(out), table, paths) == 3
    lines = out.read_text().splitlines()
    assert lines[0] == "file,start_s,end_s,chunks,aci,hf,ht,h,ndsi,bi,adi,aei" and len(lines) == 4
    assert lines[2].split(",")[:5] == ["a.wav", "60.000", "63.000", "1", f"{8 / 7:.7g}"] and lines[3].startswith("c.wav,0.000,9.000,3,")
    cli.write_spectral_npz(str(tmp_path / "s.npz"), table, paths, SR)
    with np.load(tmp_path / "s.npz") as z:
        assert sorted(z.files) == ["aci", "cvr", "ent", "file_index", "freqs_hz", "paths", "start_s"]
        assert z["aci"].shape == z["ent"].shape == z["cvr"].shape == (3, 257) and z["aci"].dtype == np.float32 and z["aci"][2, 256] == np.float32(0.7)
        assert z["file_index"].tolist() == [0, 0, 2] and z["start_s"].tolist() == [0.0, 60.0, 0.0] and z["paths"].tolist() == paths
        assert np.array_equal(z["freqs_hz"], IX.bin_frequencies(SR))
    written = cli.write_ldfc(str(tmp_path / "map.png"), table, 3)
    assert written == [str(tmp_path / "map_0.png"), str(tmp_path / "map_2.png")]
    img = _decode_png(open(written[0], "rb").read())
    assert img.shape == (257, 2, 3)
    assert _decode_png(open(written[1], "rb").read())[0, 0].tolist() == [255, 0, 0]


def test_command_line_refusals(tmp_path):
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    base = ["--input", str(wav), "--output", str(tmp_path / "o.csv")]
    args = cli.build_parser().parse_args(base)
    assert (args.window_s, args.sample_rate, args.chunk_duration, args.spec_width, args.overlap, args.max_duration) == (60.0, 22050, 3.0, 256, 0.0, 0)
    assert (args.anthro, args.bio, args.db_threshold, args.band_hz, args.max_hz, args.device, args.max_batch) == (
        [1000.0, 2000.0], [2000.0, 8000.0], -50.0, 1000.0, 10000.0, 0, 4096)
    sr, cd, width, ov, params = cli.resolve_args(args)
    assert (sr, cd, width, ov) == (22050, 3.0, 256, 0.0) and params == IX.IndexParams()
    cfg = tmp_path / "m.json"
    cfg.write_text(json.dumps({"sample_rate": 24000, "chunk_duration": 3.0, "spec_width": 240}))
    assert cli.resolve_args(cli.build_parser().parse_args(base + ["--model_config", str(cfg)]))[:3] == (24000, 3.0, 240)
    for extra, match in ((["--bio", "2000", "12000"], "error: bio band 2000-12000 Hz does not fit"),
                         (["--sample_rate", "8000"], "error: bio band"),
                         (["--spec_width", "1"], "error: --spec_width 1"),
                         (["--spec_width", "2048"], "error: --spec_width 2048"),
                         (["--window_s=-1"], "error: --window_s"),
                         (["--overlap", "3"], "error: --overlap"),
                         (["--max_duration=-2"], "error: --max_duration"),
                         (["--db_threshold", "5"], "error: db threshold"),
                         (["--band_hz", "10"], "error: 1000 bands of 10 Hz"),
                         (["--max_batch", "0"], "error: --max_batch"),
                         (["--chunk_duration", "0.001", "--sample_rate", "22050"], "error: chunks of 22 samples"),
                         (["--model_config", str(tmp_path / "none.json")], "error: model config not found")):
        with pytest.raises(SystemExit, match=match):
            cli.main(base + extra)
    with pytest.raises(SystemExit, match="error: input not found"):
        cli.main(["--input", str(tmp_path / "missing"), "--output", str(tmp_path / "o.csv")])
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit, match="error: no audio files found"):
        cli.main(["--input", str(tmp_path / "empty"), "--output", str(tmp_path / "o.csv")])
    assert not (tmp_path / "o.csv").exists()


def test_dispatcher_doc_header_and_bindings_agree():
    import birdnet_stm32.__main__ as m
    from birdnet_stm32 import _hip

    assert "indices" in m.USAGE.split("{")[1].split(",") and "``indices``" in m.__doc__
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    assert flags == {"--input", "--output", "--window_s", "--sample_rate", "--chunk_duration", "--spec_width", "--model_config", "--overlap",
                     "--max_duration", "--anthro", "--bio", "--db_threshold", "--band_hz", "--max_hz", "--spectral_out", "--ldfc_png", "--device",
                     "--max_batch"}
    for word in ("--window_s", "--spectral_out", "--ldfc_png", "--model_config", "LDFC_BOUNDS", "MEAN"):
        assert word in cli.__doc__, word
    assert ", ".join(IX.INDEX_COLUMNS) in cli.__doc__
    for i, name in enumerate(IX.INDEX_COLUMNS):
        assert re.search(rf"^{i + 1}\. ``{name}``", IX.__doc__, re.M), name
    for word in ("Hilbert", "peak-normalises", "not indices of the whole minute", "chunk's own maximum"):
        assert word in IX.__doc__, word
    root = os.path.join(os.path.dirname(_hip.LIB_PATH), "..", "..")
    with open(os.path.join(root, "include", "birdnet_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"BN_API int bn_acoustic_indices\(bn_ctx\* ctx, const float\* d_spec, const float\* d_minmax, int B, int F, int W,", hdr)
    assert "bn_acoustic_indices" in _hip.EXPORTS
    for macro, value in (("SCALARS", IX.N_SCALARS), ("BINS", IX.N_BINS), ("MIN_W", IX.MIN_WIDTH), ("MAX_W", IX.MAX_WIDTH), ("MAX_BANDS", IX.MAX_BANDS)):
        assert int(re.search(rf"#define BN_INDICES_{macro} (\d+)", hdr).group(1)) == value
    assert "{ aci, hf, ht, h, ndsi, bi, adi, aei }" in hdr
    # the ctypes struct is the header's: five int32, 17 edges, two floats
    body = re.search(r"typedef struct bn_indices_params \{(.*?)\} bn_indices_params;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[[^\]]*\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [n for n, _ in IX.DeviceParams._fields_]
    import ctypes

    assert ctypes.sizeof(IX.DeviceParams) == 4 * (5 + 17 + 2)
    if os.path.isfile(_hip.LIB_PATH):
        assert "acoustic_indices_kernel" in _hip.load_library().bn_kernel_names().decode().split("\n")
    with open(os.path.join(root, "birdnet-stm32_amd", "csrc", "Makefile")) as f:
        assert "bn_indices.hip" in f.read()
    for doc, words in (("README.md", ("birdnet_stm32 indices", "bn_acoustic_indices", "§5r")), ("DESIGN.md", ("5r", "bn_acoustic_indices", "Hilbert")),
                       ("INTEGRATION.md", ("bn_acoustic_indices", "aci, hf, ht, h, ndsi, bi, adi, aei"))):
        with open(os.path.join(root, doc)) as f:
            text = f.read()
        for w in words:
            assert w in text, (doc, w)
