"""GPU tests of indices (csrc/bn_indices.hip, evaluation/indices.py, cli/indices.py) against the numpy specification.

Integer-valued spectrograms (tests/indices_cases.py) have one float32 value for ``ACI_f``, ``CVR_f``, the band counts and NDSI, and
``bn_acoustic_indices`` is held to it bit for bit.  Float-valued ones are held to ``indices_reference`` (float64) within
``ATOL + RTOL * |value|``, eight times the measured error of the float32 numpy restatement over the same inputs, and their cover counts
bit for bit.  Every case is also read through a view one float off a 16-byte boundary (the guarded scalar loads), which must give the
same bits as the wide loads.  ``indices_files``, ``aggregate`` and the command run end to end on three small WAV files."""

import csv
import math
import wave

import numpy as np
import pytest

import indices_cases as cases
from birdnet_stm32.evaluation import indices as IX

pytestmark = pytest.mark.gpu

SR = cases.SAMPLE_RATE
NAN_BITS = 0x7FC0BEEF
GUARD = 8
COL = {name: i for i, name in enumerate(IX.INDEX_COLUMNS)}


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


def _guarded(torch, shape):
    """A float32 tensor of ``shape`` filled with a NaN pattern between guard elements of the same pattern: (whole buffer as int32, view)."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    return flat, flat[GUARD : GUARD + n].view(torch.float32).view(*shape)


def _guards_intact(flat):
    b = flat.cpu().numpy()
    return bool(np.all(b[:GUARD] == NAN_BITS) and np.all(b[-GUARD:] == NAN_BITS))


def _device_spec(torch, S, offset: bool):
    """``S [B, 257, W]`` on the device, 16-byte aligned or (``offset``) one float behind a 16-byte boundary, with its min / max."""
    n = S.size
    flat = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    view = flat[1 : 1 + n] if offset else flat[:n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(S).reshape(-1)))
    spec = view.view(*S.shape)
    assert spec.data_ptr() % 16 == (4 if offset else 0) and spec.is_contiguous()
    minmax = torch.stack([spec.amin(dim=(1, 2)), spec.amax(dim=(1, 2))], dim=1).contiguous()
    return spec, minmax


def _run(torch, ctx, S, offset=False, spectral=True, params=None):
    """``(scalars [B, 8], per-bin [B, 3, 257] or None)`` as numpy; outputs lie between guards that must survive."""
    spec, minmax = _device_spec(torch, S, offset)
    B = S.shape[0]
    flat_o, out = _guarded(torch, (B, IX.N_SCALARS))
    flat_s, bins = _guarded(torch, (B, 3, IX.N_BINS))
    before = spec.clone()
    got_o, got_s = IX.acoustic_indices_device(ctx, spec, minmax, SR, params or cases.PARAMS, spectral, out, bins if spectral else None)
    torch.cuda.synchronize()
    assert _guards_intact(flat_o) and _guards_intact(flat_s) and torch.equal(spec, before)
    assert got_o.data_ptr() == out.data_ptr() and (got_s is None) == (not spectral)
    if not spectral:
        assert np.all(flat_s.cpu().numpy() == NAN_BITS), "nothing is written without d_spectral"
    return out.cpu().numpy(), (bins.cpu().numpy() if spectral else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _band_counts(cvr, W):
    """Band counts recovered from ``CVR_f = count / W`` (exact: the count is the nearest integer to ``CVR_f * W``)."""
    per_bin = np.rint(cvr.astype(np.float64) * W).astype(np.int64)
    edges = IX.diversity_edges(cases.PARAMS, SR)
    return per_bin, np.array([per_bin[edges[b] : edges[b + 1]].sum() for b in range(len(edges) - 1)], np.int64)


@pytest.mark.parametrize("name", [n for n, _ in cases.integer_cases()])
def test_integer_cases_bit_equal(torch_mod, ctx, name):
    S = dict(cases.integer_cases())[name]
    W = S.shape[2]
    s32, b32 = cases.reference_f32("int", name)
    s64, b64 = cases.reference("int", name)
    got_s, got_b = _run(torch_mod, ctx, S)
    off_s, off_b = _run(torch_mod, ctx, S, offset=True)
    assert np.array_equal(_bits(got_s), _bits(off_s)) and np.array_equal(_bits(got_b), _bits(off_b)), "wide and scalar loads give the same bits"
    assert np.array_equal(_bits(got_b[:, 0]), _bits(b32[:, 0])), "ACI_f"
    assert np.array_equal(_bits(got_b[:, 2]), _bits(b32[:, 2])), "CVR_f"
    assert np.array_equal(_bits(got_s[:, COL["ndsi"]]), _bits(s32[:, COL["ndsi"]])), "NDSI"
    for i in range(S.shape[0]):
        per_bin, per_band = IX.cover_counts(S[i], SR, cases.PARAMS)
        g_bin, g_band = _band_counts(got_b[i, 2], W)
        assert np.array_equal(g_bin, per_bin) and np.array_equal(g_band, per_band), (name, i)
    assert cases.within(got_s, s64).all() and cases.within(got_b, b64).all()
    if name.startswith("zeros"):
        assert not got_s[1].any() and not got_b[1].any(), "an all-zero chunk gives zeros everywhere"
        assert np.count_nonzero(got_b[2, 0]) == np.count_nonzero(got_b[2, 2]) == 1 and got_b[2, 2, 256] == 1.0, "energy only in bin 256"
        assert got_s[2, COL["ndsi"]] == 0.0 and got_s[2, COL["bi"]] == 0.0 and got_s[2, COL["adi"]] == 0.0 and got_s[2, COL["aei"]] == 0.0


@pytest.mark.parametrize("name", [n for n, _ in cases.float_cases()])
def test_float_cases_within_tolerance(torch_mod, ctx, name):
    S = dict(cases.float_cases())[name]
    W = S.shape[2]
    s64, b64 = cases.reference("float", name)
    got_s, got_b = _run(torch_mod, ctx, S)
    off_s, off_b = _run(torch_mod, ctx, S, offset=True)
    assert np.array_equal(_bits(got_s), _bits(off_s)) and np.array_equal(_bits(got_b), _bits(off_b)), "wide and scalar loads give the same bits"
    err_s, err_b = np.abs(got_s - s64), np.abs(got_b - b64)
    print(f"{name}: scalars worst |err| / (ATOL + RTOL |v|) = {(err_s / (cases.ATOL + cases.RTOL * np.abs(s64))).max(axis=0).round(4).tolist()}, "
          f"per-bin worst |err| = {err_b.max(axis=(0, 2)).tolist()} (ATOL {cases.ATOL:.3g}, RTOL {cases.RTOL:.3g})")
    assert cases.within(got_s, s64).all(), (name, got_s, s64)
    assert cases.within(got_b, b64).all(), (name, err_b.max(axis=(0, 2)))
    # cover: counts, bit for bit
    assert np.array_equal(_bits(got_b[:, 2]), _bits(b64[:, 2].astype(np.float32))), "CVR_f"
    for i in range(S.shape[0]):
        per_bin, per_band = IX.cover_counts(S[i], SR, cases.PARAMS)
        g_bin, g_band = _band_counts(got_b[i, 2], W)
        assert np.array_equal(g_bin, per_bin) and np.array_equal(g_band, per_band), (name, i)
    if name == "tones_noise_w256":
        assert got_s[0, COL["ndsi"]] > 0.999
        assert got_s[2, COL["hf"]] > 0.99 and abs(got_s[2, COL["adi"]] - math.log(10)) < 1e-3 and got_s[2, COL["aei"]] < 0.01
    if name == "chirps_zeros_tone_w256":
        assert got_s[2, COL["ndsi"]] < -0.999 and not got_s[1].any() and not got_b[1].any()


def test_scalars_without_spectral_and_repeat_runs(torch_mod, ctx):
    for group, name in ((cases.float_cases(), "tones_noise_w260"), (cases.float_cases(), "chirps_zeros_tone_w6"), (cases.integer_cases(), "edges_w256")):
        S = dict(group)[name]
        a_s, a_b = _run(torch_mod, ctx, S)
        b_s, b_b = _run(torch_mod, ctx, S)
        assert np.array_equal(_bits(a_s), _bits(b_s)) and np.array_equal(_bits(a_b), _bits(b_b)), "two runs give identical bits"
        for offset in (False, True):
            n_s, none = _run(torch_mod, ctx, S, offset=offset, spectral=False)
            assert none is None and np.array_equal(_bits(n_s), _bits(a_s)), "d_spectral = NULL gives the same scalars"


def test_other_bands_and_thresholds(torch_mod, ctx):
    """Parameters other than the defaults reach the kernel: narrow bands at the spectrum's ends, 16 diversity bands, another threshold."""
    params = IX.IndexParams(anthro=(0.0, 500.0), bio=(9000.0, 11025.0), db=-20.0, band_hz=600.0, max_hz=9600.0)
    assert IX.device_params(params, SR).n_bands == 16 and IX.band_bins(9000.0, 11025.0, SR) == (209, 256)
    S = dict(cases.float_cases())["tones_noise_w256"]
    got_s, got_b = _run(torch_mod, ctx, S, params=params)
    for i in range(S.shape[0]):
        s64, b64 = IX.indices_reference(S[i], SR, params)
        assert cases.within(got_s[i], s64).all() and cases.within(got_b[i], b64).all(), (i, got_s[i], s64)
        assert np.array_equal(_bits(got_b[i, 2]), _bits(b64[2].astype(np.float32)))


def test_refusals_without_a_launch(torch_mod, ctx):
    import ctypes

    torch = torch_mod
    lib, h = ctx.lib, ctx.handle
    spec = torch.ones((2, 257, 8), dtype=torch.float32, device="cuda")
    minmax = torch.ones((2, 2), dtype=torch.float32, device="cuda")
    flat_o, out = _guarded(torch, (2, IX.N_SCALARS))
    flat_s, bins = _guarded(torch, (2, 3, IX.N_BINS))
    good = IX.device_params(cases.PARAMS, SR)

    def call(B=2, F=257, W=8, dp=good, d_spec=spec.data_ptr(), d_out=out.data_ptr()):
        rc = lib.bn_acoustic_indices(h, d_spec, minmax.data_ptr(), B, F, W, ctypes.byref(dp) if dp is not None else None, d_out, bins.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    def changed(**kw):
        dp = IX.device_params(cases.PARAMS, SR)
        for k, v in kw.items():
            if k == "edge":
                dp.band_edge[v[0]] = v[1]
            else:
                setattr(dp, k, v)
        return dp

    UNSUPPORTED, ARG = -4, -1
    assert call(F=256) == UNSUPPORTED and call(F=513) == UNSUPPORTED and "257" in lib.bn_last_error().decode()
    assert call(W=1) == ARG and call(W=1025) == ARG and call(B=-1) == ARG
    assert call(dp=changed(bio_k1=258)) == ARG and "biophony" in lib.bn_last_error().decode()
    assert call(dp=changed(anthro_k0=50, anthro_k1=40)) == ARG and call(dp=changed(anthro_k0=-1)) == ARG
    assert call(dp=changed(n_bands=17)) == ARG and call(dp=changed(edge=(10, 258))) == ARG and call(dp=changed(edge=(3, 10))) == ARG
    assert call(dp=changed(cover_ratio=float("nan"))) == ARG and call(dp=changed(df_khz=-1.0)) == ARG
    assert call(dp=None) == ARG and call(d_spec=None) == ARG and call(d_out=None) == ARG and call(d_spec=spec.data_ptr() + 2) == ARG
    assert np.all(flat_o.cpu().numpy() == NAN_BITS) and np.all(flat_s.cpu().numpy() == NAN_BITS), "a refused call writes nothing"
    assert call(B=0) == 0 and np.all(flat_o.cpu().numpy() == NAN_BITS)
    assert call() == 0 and not np.any(flat_o.cpu().numpy()[GUARD:-GUARD] == NAN_BITS) and _guards_intact(flat_o) and _guards_intact(flat_s)
    with pytest.raises(ValueError, match="contiguous float32 CUDA tensor"):
        IX.acoustic_indices_device(ctx, spec[:, :, ::2], minmax, SR)
    with pytest.raises(ValueError, match="minmax"):
        IX.acoustic_indices_device(ctx, spec, minmax[:1], SR)
    assert "acoustic_indices_kernel" in lib.bn_kernel_names().decode().split("\n")


# -- end to end --------------------------------------------------------------------------------------------------------------------------
def _write_wav(path, frames, sr):
    pcm = np.clip(np.rint(np.asarray(frames, np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def wav_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("indices_wav")
    rng = np.random.default_rng(5)
    t = np.arange(7 * 22050) / 22050.0
    paths = [d / "tone.wav", d / "noise.wav", d / "zeros.wav"]
    _write_wav(paths[0], 0.8 * np.sin(2 * np.pi * 3000.0 * t), 22050)
    _write_wav(paths[1], np.clip(0.2 * rng.standard_normal((7 * 48000, 2)), -1, 1), 48000)
    _write_wav(paths[2], np.zeros(22050), 22050)
    return [str(p) for p in paths]


@pytest.fixture(scope="module")
def file_result(torch_mod, wav_files):
    return IX.indices_files(wav_files, max_batch=2)   # (slices of 2: the 3-chunk groups take two launches)


def test_files_end_to_end(torch_mod, ctx, wav_files, file_result):
    from birdnet_stm32.audio import ingest
    from birdnet_stm32.models.runners import stft_device

    res = file_result
    assert res.chunks_per_file.tolist() == [3, 3, 1] and len(res) == 7 and res.skipped == [] and res.paths == wav_files
    assert res.scalars.shape == (7, 8) and res.spectral.shape == (7, 3, 257) and res.scalars.dtype == res.spectral.dtype == np.float32
    assert res.chunk_file.tolist() == [0, 0, 0, 1, 1, 1, 2]
    assert res.chunk_start_s.tolist() == [0.0, 3.0, 4.0, 0.0, 3.0, 4.0, 0.0] and res.chunk_end_s.tolist() == [3.0, 6.0, 7.0, 3.0, 6.0, 7.0, 1.0]
    assert res.duration_s.tolist() == [7.0, 7.0, 1.0]
    # the same chunks by the stand-alone ingest, the STFT and the kernel: bit for bit
    wins = [ingest.read_pcm_window(p, max_duration=None, chunk_duration=3.0) for p in wav_files]
    chunks, counts = ingest.ingest_windows_device(ctx, wins, SR, 3.0, 0.0)
    assert list(counts) == [3, 3, 1]
    spec, minmax = stft_device(ctx, chunks, 512, None, 256, False, return_minmax=True)
    scalars, bins = IX.acoustic_indices_device(ctx, spec, minmax, SR)
    assert np.array_equal(_bits(scalars.cpu().numpy()), _bits(res.scalars)) and np.array_equal(_bits(bins.cpu().numpy()), _bits(res.spectral))
    assert torch_mod.equal(minmax[:, 1], spec.amax(dim=(1, 2))), "the STFT's maximum is the spectrogram's"
    # the known answers hold on the device values
    s = res.scalars
    assert (s[0:3, COL["ndsi"]] > 0.999).all()
    assert (s[3:6, COL["hf"]] > 0.99).all() and (np.abs(s[3:6, COL["adi"]] - math.log(10)) < 1e-3).all() and (s[3:6, COL["aei"]] < 0.01).all()
    assert not s[6].any() and not res.spectral[6].any()
    # ... and against the specification on the device's own spectrograms
    host = spec.cpu().numpy()
    for i in range(7):
        s64, b64 = IX.indices_reference(host[i], SR)
        assert cases.within(s[i], s64).all() and cases.within(res.spectral[i], b64).all(), i
    # windows
    rows = np.concatenate([res.scalars, res.spectral.reshape(7, -1)], axis=1)
    table = IX.aggregate(rows, res.chunk_file, res.chunk_start_s, 60.0, res.chunk_end_s)
    assert table.file_index.tolist() == [0, 1, 2] and table.chunks.tolist() == [3, 3, 1] and table.start_s.tolist() == [0.0, 0.0, 0.0]
    assert table.end_s.tolist() == [7.0, 7.0, 1.0] and table.values.shape == (3, 8 + 3 * 257)
    assert np.allclose(table.values[0], rows[0:3].astype(np.float64).sum(axis=0) / 3, rtol=1e-14, atol=0) and np.array_equal(table.values[2], rows[6].astype(np.float64))
    table = IX.aggregate(rows, res.chunk_file, res.chunk_start_s, 4.0)
    assert table.chunks.tolist() == [2, 1, 2, 1, 1] and table.start_s.tolist() == [0.0, 4.0, 0.0, 4.0, 0.0], "the last chunk starts at n - size = 4 s"


def test_files_without_spectral(torch_mod, wav_files, file_result):
    res = IX.indices_files(wav_files[:1], spectral=False)
    assert res.spectral is None and np.array_equal(_bits(res.scalars), _bits(file_result.scalars[:3]))


def test_command_line_writes_all_outputs(torch_mod, wav_files, file_result, tmp_path, capsys):
    import struct
    import zlib

    from birdnet_stm32.cli import indices as cli

    out, npz, png = tmp_path / "indices.csv", tmp_path / "s.npz", tmp_path / "map.png"
    table = cli.main(["--input"] + wav_files + ["--output", str(out), "--window_s", "4", "--spectral_out", str(npz), "--ldfc_png", str(png)])
    assert "Indices of 3 files (0.00 h, 7 chunks) in 5 windows" in capsys.readouterr().out and len(table) == 5
    with open(out, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == list(cli.CSV_COLUMNS) and len(lines) == 6
    assert [ln[:4] for ln in lines[1:]] == [[wav_files[0], "0.000", "6.000", "2"], [wav_files[0], "4.000", "7.000", "1"],
                                            [wav_files[1], "0.000", "6.000", "2"], [wav_files[1], "4.000", "7.000", "1"], [wav_files[2], "0.000", "1.000", "1"]]
    want = file_result.scalars[0:2].astype(np.float64).mean(axis=0)
    assert lines[1][4:] == [f"{v:.7g}" for v in want] and lines[5][4:] == ["0"] * 8
    with np.load(npz) as z:
        assert z["aci"].shape == z["ent"].shape == z["cvr"].shape == (5, 257) and z["file_index"].tolist() == [0, 0, 1, 1, 2]
        assert z["start_s"].tolist() == [0.0, 4.0, 0.0, 4.0, 0.0] and z["paths"].tolist() == wav_files and z["freqs_hz"][256] == SR / 2
        assert np.array_equal(z["cvr"][1], file_result.spectral[2, 2])
    for i, width in enumerate((2, 2, 1)):
        data = (tmp_path / f"map_{i}.png").read_bytes()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (width, 257)
        n = struct.unpack(">I", data[33:37])[0]
        assert len(zlib.decompress(data[41 : 41 + n])) == 257 * (1 + 3 * width)
    # one line per chunk
    cli.main(["--input", wav_files[0], "--output", str(out), "--window_s", "0"])
    with open(out, newline="") as f:
        lines = list(csv.reader(f))
    assert len(lines) == 4 and [ln[1] for ln in lines[1:]] == ["0.000", "3.000", "4.000"] and lines[3][4:] == [f"{v:.7g}" for v in file_result.scalars[2]]
