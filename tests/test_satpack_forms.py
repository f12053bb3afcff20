"""The algebra of the packed shift-and-saturate epilogues (``csrc/bn_requant.h``: ``sat_pack_2x4``, ``sat_pack_quads`` / ``sat_pack_quad``;
``csrc/bn_i8_tail2.hip``: SAT) on the CPU: a numpy emulation of the instruction sequences against the definitions they replace —
``pack4(med3(h >> e1, -128, 127))`` per position — over random ``h`` within +-2^28 and every shift 0..30, dead-channel constants included;
the byte selectors are read from the header.  And the choice of the form through the host library (``tail2_satpack_ok`` behind
``tail2_plan``): the full int8 range in every block selects the new form, ONE narrower bound anywhere does not.

What the emulation assumes of the instruction itself is held to the hardware by tests/test_gpu_satpack.py."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import satpack_cases as sc
from conftest import PKG, REPO

CSRC = os.path.join(PKG, "csrc")
N = 20000


def _selectors() -> tuple[int, int]:
    src = open(os.path.join(CSRC, "bn_requant.h")).read()
    m = re.search(r"kSatSelA = (0x[0-9a-fA-F]+)u, kSatSelB = (0x[0-9a-fA-F]+)u", src)
    assert m, "bn_requant.h no longer defines the byte selectors"
    return int(m.group(1), 16), int(m.group(2), 16)


def pack4(q) -> np.ndarray:
    """bn_requant.h: the low bytes of four values as one dword."""
    q = np.asarray(q, np.int64) & 0xFF
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)


def old_form(h, e1, lo=-128, hi=127) -> np.ndarray:
    """pack4(med3(h >> e1, lo, hi)) — h [..., 4], e1 [..., 4] or scalar."""
    return pack4(np.clip(h >> e1, lo, hi))


def _cases(rng):
    """h of two positions x four channels, per-channel shifts: every shift 0..30 in every channel slot, h within +-2^28 with the values
    around both saturation edges of the shifted result mixed in."""
    e1 = rng.integers(0, 31, (N, 4))
    e1[:31 * 4] = np.repeat(np.arange(31), 4)[:, None]          # every shift, four rows each, in all four slots at once
    h = rng.integers(-(1 << 28), (1 << 28) + 1, (N, 2, 4))
    edge = rng.choice(np.array([-130, -129, -128, -127, -1, 0, 1, 126, 127, 128, 129]), (N // 2, 2, 4))
    near = (edge << e1[: N // 2, None, :]) + rng.integers(-1, 2, (N // 2, 2, 4))
    h[: N // 2] = np.where(np.abs(near) <= 1 << 28, near, h[: N // 2])
    return h, e1


def test_two_positions_of_four_channels_sat_pack_2x4():
    """ra = (a0 b0 a1 b1), rb = (a2 b2 a3 b3), shifts taken from the packed-bytes word as the kernels do (the word itself for channel 0, the word
    >> 8, 16, 24 for the others: the instruction reads five bits); perm(rb, ra, kSatSelA / kSatSelB) = the two positions' dwords."""
    sel_a, sel_b = _selectors()
    h, e1 = _cases(np.random.default_rng(31))
    packed = (e1[:, 0] | (e1[:, 1] << 8) | (e1[:, 2] << 16) | (e1[:, 3] << 24)).astype(np.int32).astype(np.int64)
    se = [packed >> (8 * e) for e in range(4)]
    a, b = h[:, 0], h[:, 1]
    ra = sc.ashr_pk(a[:, 0], b[:, 0], se[0]) | (sc.ashr_pk(a[:, 1], b[:, 1], se[1]) << 16)
    rb = sc.ashr_pk(a[:, 2], b[:, 2], se[2]) | (sc.ashr_pk(a[:, 3], b[:, 3], se[3]) << 16)
    assert np.array_equal(sc.perm(rb, ra, sel_a), old_form(a, e1)), "position a"
    assert np.array_equal(sc.perm(rb, ra, sel_b), old_form(b, e1)), "position b"
    got = set((sc.perm(rb, ra, sel_a) & 0xFF).tolist())
    assert {0x80, 0x7F, 0x81, 0x7E, 0x00, 0xFF} <= got, "the cases reach both saturation ends and their neighbours"


def test_dead_channel_constants():
    """A dead channel (multiplier 0, e = 1, c1 = 1 + 2 q: models/_lower_i8.py) gives h = hi32(C) = q for every accumulator and shift 0."""
    rng = np.random.default_rng(32)
    sel_a, sel_b = _selectors()
    q = rng.integers(-128, 128, (N, 4))
    c1 = 1 + 2 * q
    C = (c1 << 31) + (1 << 30)                                  # bn_requant.h: rq64
    x = rng.integers(-(1 << 30), 1 << 30, (N, 2, 4))
    h = (x * 0 + C[:, None, :]) >> 32                           # rq_h with multiplier 0
    assert np.array_equal(h[:, 0], q) and np.array_equal(h[:, 1], q)
    live = rng.integers(0, 31, (N, 4))                          # mixed into quads whose other channels are live
    dead = rng.random((N, 4)) < 0.5
    e1 = np.where(dead, 0, live)
    hh = np.where(dead[:, None, :], h, rng.integers(-(1 << 28), 1 << 28, (N, 2, 4)))
    a, b = hh[:, 0], hh[:, 1]
    ra = sc.ashr_pk(a[:, 0], b[:, 0], e1[:, 0]) | (sc.ashr_pk(a[:, 1], b[:, 1], e1[:, 1]) << 16)
    rb = sc.ashr_pk(a[:, 2], b[:, 2], e1[:, 2]) | (sc.ashr_pk(a[:, 3], b[:, 3], e1[:, 3]) << 16)
    assert np.array_equal(sc.perm(rb, ra, sel_a), old_form(a, e1)) and np.array_equal(sc.perm(rb, ra, sel_b), old_form(b, e1))
    assert np.array_equal(np.where(dead, (sc.perm(rb, ra, sel_a)[:, None] >> (8 * np.arange(4))) & 0xFF, 0), np.where(dead, q & 0xFF, 0))


def test_add_output_pairs_adjacent_channels_behind_the_layers_shift():
    """The ADD's output rescale has ONE shift per layer: channels (0, 1) go to the low half, (2, 3) to the high half of the stored dword."""
    rng = np.random.default_rng(33)
    h = rng.integers(-(1 << 28), (1 << 28) + 1, (N, 4))
    s = rng.integers(0, 31, N)
    s[:31] = np.arange(31)
    edge = rng.choice(np.array([-129, -128, -127, 126, 127, 128]), (N // 2, 4))
    h[: N // 2] = np.where(np.abs(edge << s[: N // 2, None]) <= 1 << 28, (edge << s[: N // 2, None]) + rng.integers(-1, 2, (N // 2, 4)), h[: N // 2])
    d = sc.ashr_pk(h[:, 0], h[:, 1], s) | (sc.ashr_pk(h[:, 2], h[:, 3], s) << 16)
    assert np.array_equal(d, old_form(h, s[:, None]))


def test_stem_window_dword_of_three_columns():
    """i8_front_strip_kernel's stem rows (sat_window_lo / sat_window_hi): columns (0, 1) of a channel into bytes 0-1, column 2 into the high
    half — against deposit_column's definition, byte j = low byte of (clamp(h_j, lo << e1, ((hi + 1) << e1) - 1) >> e1) with (lo, hi) =
    (-128, 127).  Byte 3 is a don't-care (the depthwise window's fourth tap weight is 0: front_strip_constants): here it repeats column 2."""
    rng = np.random.default_rng(34)
    e1 = rng.integers(0, 31, N)
    e1[:31] = np.arange(31)
    h = rng.integers(-(1 << 28), (1 << 28) + 1, (N, 3))
    edge = rng.choice(np.array([-130, -129, -128, -127, -1, 0, 126, 127, 128, 129]), (N // 2, 3))
    near = (edge << e1[: N // 2, None]) + rng.integers(-1, 2, (N // 2, 3))
    h[: N // 2] = np.where(np.abs(near) <= 1 << 28, near, h[: N // 2])
    blo, bhi = -128 << e1, (128 << e1) - 1                       # bn_requant.h: shifted_bounds
    old = (np.clip(h, blo[:, None], bhi[:, None]) >> e1[:, None]) & 0xFF
    t = sc.ashr_pk(h[:, 0], h[:, 1], e1) | (sc.ashr_pk(h[:, 2], h[:, 2], e1) << 16)
    assert np.array_equal(t & 0xFFFFFF, old[:, 0] | (old[:, 1] << 8) | (old[:, 2] << 16))
    assert np.array_equal(t >> 24, old[:, 2])


def test_front_strip_selection_is_the_int8_range_of_the_stem():
    """The launcher's predicate (csrc/bn_kernels.h: front_strip_satpack_ok) as the source states it, and the shipped stem's clamp."""
    import i8_mutants as im

    src = open(os.path.join(CSRC, "bn_kernels.h")).read()
    assert "inline bool front_strip_satpack_ok(int st_lo, int st_hi) { return st_lo == -128 && st_hi == 127; }" in src
    m = im.shipped()
    stem, _ = im.backbone(m)
    assert im.act_bounds(m, stem) == (-128, 127)


# ------------------------------------------------------------------------------------------------ which form the library picks
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("satpack") / "satpack_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(REPO, "tests", "host", "satpack_main.cpp"), os.path.join(CSRC, "bn_chain_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _forms(prog, form, n_layers, nc, words, edits=()) -> list[int]:
    path = prog + ".words.bin"
    np.asarray(words, dtype="<i4").tofile(path)
    args = [prog, form, str(n_layers), str(nc), path]
    if len(edits):
        np.asarray(edits, dtype="<i4").reshape(-1).tofile(prog + ".edits.bin")
        args.append(prog + ".edits.bin")
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-4000:]
    return [int(v) for v in r.stdout.split()]


def _tables(plan) -> dict:
    from birdnet_stm32.models import _pack as pk

    out = {}
    for o in plan.ops:
        words = lambda name: plan.tensors[o.get(name)].reshape(-1).astype(np.int32)   # noqa: E731
        if o.kind == pk.I8_TAIL and o.get("desc2") >= 0 and o.get("cst2") >= 0:
            out["tail2"] = (o.get("n_layers"), o.get("n_classes"), words("desc2"))
        elif o.kind == pk.I8_MID:
            out["mid"] = (o.get("n_layers"), 0, words("desc"))
    return out


def test_full_range_selects_the_new_form_and_any_narrower_bound_does_not(prog):
    """On the shipped tables: the new form; then every bound word the predicate reads, in every block, moved inwards by one (lower bound + 1,
    upper bound - 1): the old form, each time.  The pointwise bounds of a block with the ADD are not stored bytes' bounds (the own term is
    unclamped): moving them changes nothing."""
    import i8_mutants as im
    from birdnet_stm32.models._lower_i8 import lower_i8

    tables = _tables(lower_i8(im.shipped()))
    assert set(tables) == {"mid", "tail2"}
    for form, (nl, nc, words) in tables.items():
        edits, expect = [], []
        for i in range(nl):
            row = words[32 * i: 32 * i + 32]
            add = bool(row[9])
            for w, delta, counts in ((11, 1, True), (12, -1, True), (13, 1, not add), (14, -1, not add), (18, 1, add), (19, -1, add)):
                edits.append((32 * i + w, int(row[w]) + delta))
                expect.append(0 if counts else 1)
        got = _forms(prog, form, nl, nc, words, edits)
        assert got[0] == 1, f"{form}: the shipped chain must select the new form"
        assert got[1:] == expect, f"{form}: {[(e, g) for e, g, x in zip(edits, got[1:], expect) if g != x]}"


@pytest.mark.parametrize("which,want", [("narrow_relu6", {"mid": 0, "tail2": 0}), ("add_zero_point", {"mid": 1, "tail2": 0})])
def test_models_with_a_narrower_clamp_keep_their_chains_fused_and_the_old_form(prog, which, want):
    import i8_mutants as im
    from birdnet_stm32.models._lower_i8 import lower_i8

    plan = lower_i8(getattr(sc, which)())
    forms = im.plan_forms(plan)
    assert forms["mid"] == 1 and forms["tail2"], "the lowering keeps both chains fused"
    bounds = sc.chain_bounds(plan)
    for form, (nl, nc, words) in _tables(plan).items():
        assert _forms(prog, form, nl, nc, words) == [want[form]], form
        assert sc.bounds_full(bounds[form]) == bool(want[form])
