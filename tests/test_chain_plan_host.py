"""The host-side LDS planners of the fused INT8 chains (``csrc/bn_chain_plan.cpp``: ``tail_plan``, ``tail2_plan``, ``tail2_plan_resident``
and their companions) without a device: ``tests/host/chain_plan_main.cpp`` is compiled ONCE, together with the planners, by the system
C++ compiler under the address and undefined-behaviour sanitizers, and run on the descriptor tables the lowering writes — which form each
shape variant is given, every accepted plan against ``tests/golden/chain_plans.json``, the resident stage-2 placement, why the 8-block
chain is refused, hostile tables, and every single word of the shipped tables set to an extreme value."""
from __future__ import annotations

import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import i8_variants as iv
from conftest import PKG, REPO, TFLITE_PATH

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
if CXX is None:
    pytest.skip("no C++ compiler on this machine", allow_module_level=True)

CSRC = os.path.join(PKG, "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "chain_plans.json")
LDS_CAP = 160 * 1024
FORMS = ("tail", "tail2", "mid", "mid-resident")
I32_MIN, I32_MAX = -(2**31), 2**31 - 1


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """The program, built once.  The sanitizer runtimes are linked statically where the compiler has them: the program then needs nothing
    preloaded and does not care what else the process environment loads in front of it."""
    exe = str(tmp_path_factory.mktemp("chain_plan") / "chain_plan_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(REPO, "tests", "host", "chain_plan_main.cpp"), os.path.join(CSRC, "bn_chain_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(prog, form, n_layers, nc, words, sweep=False) -> list[str]:
    path = prog + ".words.bin"
    np.asarray(words, dtype="<i4").tofile(path)
    r = subprocess.run([prog, form, str(n_layers), str(nc), path] + (["sweep"] if sweep else []), capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, f"{form}, {n_layers} blocks, NC {nc}: exit status {r.returncode}\n{r.stderr[-4000:]}"
    return r.stdout.splitlines()


def _parse(form: str, ints: list[int]) -> dict | None:
    """The program's line of integers -> None (refused) or the plan by field."""
    if ints == [0]:
        return None
    assert ints[0] == 1
    per = 7 if form == "tail" else 5
    plan = dict(zip(("lds_bytes", "const_words", "mean_off", "fcw_off", "bar_off", "resident"), ints[1:7]))
    rest = ints[7:]
    nl = len(rest) // per if not form.startswith("mid") else (len(rest) - 5) // (per + 6)
    plan["layers"] = [rest[per * i: per * (i + 1)] for i in range(nl)]
    plan["dump"] = rest[per * nl:]
    assert len(plan["dump"]) == (5 + 6 * nl if form.startswith("mid") else 0)
    return plan


def plan_of(prog, form, n_layers, nc, words):
    (line,) = _run(prog, form, n_layers, nc, words)
    return [int(v) for v in line.split()]


def tables(plan) -> dict:
    """form -> (n_layers, NC, descriptor words) of every fused chain in a lowered plan."""
    from birdnet_stm32.models import _pack as pk

    out = {}
    for o in plan.ops:
        words = lambda name: plan.tensors[o.get(name)].reshape(-1).astype(np.int32)   # noqa: E731
        if o.kind == pk.I8_TAIL:
            out["tail"] = (o.get("n_layers"), o.get("n_classes"), words("desc"))
            if o.get("desc2") >= 0 and o.get("cst2") >= 0:
                out["tail2"] = (o.get("n_layers"), o.get("n_classes"), words("desc2"))
        elif o.kind == pk.I8_MID:
            out["mid"] = out["mid-resident"] = (o.get("n_layers"), 0, words("desc"))
    return out


def variant_tables(name: str) -> dict:
    return tables(iv.plan(name))   # (models, oracle runs and plans are shared with tests/test_i8_variants_host.py: built once per session)


@functools.lru_cache(maxsize=1)
def shipped_tables() -> dict:
    from birdnet_stm32.models.runners import lower_model_file

    t = tables(lower_model_file(TFLITE_PATH))
    assert set(t) == set(FORMS) and [t[f][0] for f in FORMS] == [6, 6, 3, 3] and t["tail"][1] == 100
    return t


def all_plans(prog) -> dict:
    """'variant/form' -> the program's integers, for every chain of every variant and of the shipped model (what the golden file holds)."""
    out = {}
    for name in ["shipped"] + list(iv.VARIANTS):
        for form, (nl, nc, words) in (shipped_tables() if name == "shipped" else variant_tables(name)).items():
            out[f"{name}/{form}"] = plan_of(prog, form, nl, nc, words)
    return out


# ------------------------------------------------------------------------------------------------ what the planners make of the real tables
def test_constants_are_the_lowering_s(prog):
    from birdnet_stm32.models import _lower_i8 as lw

    r = subprocess.run([prog], capture_output=True, text=True, check=True)
    assert [int(v) for v in r.stdout.split()] == [lw.TAIL_LAYER_WORDS, lw.TAIL_HEAD_WORDS, lw.TAIL2_LAYER_WORDS, lw.TAIL_G, 2]


@pytest.mark.parametrize("name", iv.GPU_VARIANTS)
def test_variant_is_given_the_form_the_device_test_expects(prog, name):
    """``runner.tail_form()[0]`` as the library derives it: 0 where ``tail_plan`` refuses, 2 where ``tail2_plan`` accepts too (it only runs
    where the first form could), else 1; the stage-2 chain is the same in every variant and takes its resident placement."""
    t = variant_tables(name)
    ok = {form: _parse(form, plan_of(prog, form, *t[form])) is not None for form in t}
    form = 0 if not ok.get("tail") else 2 if ok.get("tail2") else 1
    assert form == iv.TAIL_FORM[name], (name, ok)
    assert ok["mid"] and ok["mid-resident"]


def test_every_plan_equals_the_recorded_one(prog):
    """Byte offsets, LDS sizes and constant-block words of every chain: recorded from the planners as they stood in the two kernel files,
    before they were moved and de-duplicated."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = all_plans(prog)
    assert sorted(got) == sorted(want)
    assert sum(v != [0] for v in want.values()) >= 60   # (the file is not a list of refusals)
    for key in want:
        assert got[key] == want[key], key


def test_why_the_eight_block_chain_is_refused(prog):
    """The cause ``i8_variants.TAIL_FORM`` names, as numbers: with an even number of res128 blocks in front of it the 128 -> 256 block
    reads its input at 0 and first fit puts its output map (4 chunks x 4 x 8 positions x 260 bytes) at 67584; the first res256 block then has
    its input there, its output at 0, and its 64 KB of pointwise weights fit neither between the maps nor above them."""
    from birdnet_stm32.models import _lower_i8 as lw

    nl, nc, words = variant_tables("chain8")["tail"]
    assert nl == 8 and _parse("tail", plan_of(prog, "tail", nl, nc, words)) is None
    head = words[24 * nl:]

    def prefix(n):   # the first n blocks under the same head (the last three blocks all end on 4 x 8 positions of 256 channels)
        return _parse("tail", plan_of(prog, "tail", n, nc, np.concatenate([words[: 24 * n], head])))

    p6 = prefix(6)
    assert p6 is not None and prefix(7) is None
    x_off, y_off = p6["layers"][5][:2]
    out_map = lw.TAIL_G * 4 * 8 * (256 + 4)
    assert (x_off, y_off, out_map, y_off + out_map) == (0, 67584, 33280, 100864)
    assert y_off - out_map < 256 * 256 and y_off + out_map + 256 * 256 > LDS_CAP and 100864 + 65536 > LDS_CAP


def test_resident_stage2_plan_of_the_shipped_model(prog):
    """What tests/test_gpu_mid_split.py asserts of ``runner.mid_plan()``, on the CPU."""
    nl, nc, words = shipped_tables()["mid-resident"]
    p = _parse("mid-resident", plan_of(prog, "mid-resident", nl, nc, words))
    assert p is not None and p["resident"] == 1
    resident, lds_bytes, map_bytes, bar_off, blocks = p["dump"][:5]
    assert (resident, lds_bytes, bar_off, blocks) == (1, p["lds_bytes"], p["bar_off"], 3)
    parts = [(p["dump"][5 + 6 * i + 2 * j], p["dump"][5 + 6 * i + 2 * j + 1]) for i in range(blocks) for j in range(3)]
    parts = [(o, n) for o, n in parts if n > 0]
    assert len(parts) == 3 + 3 + 2
    assert [(o) for o, _ in parts] == [v for i, L in enumerate(p["layers"]) for v in (L[2:5] if i else L[2:4])]   # dw_off, pw_off, zp_off
    assert map_bytes == 2 * 16 * 32 * (64 + 16)
    spans = [(0, map_bytes), (bar_off, bar_off + 16)] + [(o, o + n) for o, n in parts]
    for b, e in spans:
        assert 0 <= b < e <= lds_bytes <= LDS_CAP and b % 16 == 0, (b, e, p)
    spans.sort()
    for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
        assert e0 <= b1, f"[{b0}, {e0}) overlaps [{b1}, {e1})"
    assert sum(n for _, n in parts) == 50592   # 7168 + 5376, then twice 13568 + 5376 + 80


# ------------------------------------------------------------------------------------------------ tables the planners must refuse
def _hostile():
    """(form, n_layers or None = the table's own, mutation of the word list) -> refused.  The first four are the mutations of
    test_gpu_sweeps.py::test_hostile_tail_descriptor_falls_back_to_the_block_kernels."""
    def put(word, value):
        def f(w):
            w = w.copy()
            w[word] = value if not callable(value) else value(int(w[word]))
            return w
        return f

    cases = [("tail", None, put(21, -4), "g_dwc of block 0 negative"), ("tail", None, put(13, -300), "pw_lo of block 0 below int8"),
             ("tail", None, put(24 + 19, 400), "add_hi of block 1 above int8"), ("tail", None, put(24 * 6 + 7, -8), "g_fcw negative")]
    for form in ("tail2", "mid", "mid-resident"):
        cases += [(form, None, put(24, -4), "g_cst of block 0 negative"), (form, None, put(32 + 24, lambda v: v + 2), "g_cst of block 1 unaligned"),
                  (form, None, put(11, -300), "dw_lo of block 0 below int8"), (form, None, put(32 + 12, 200), "dw_hi of block 1 above int8"),
                  (form, None, put(32 + 23, 2), "res_k of block 1 below 3"), (form, None, put(32 + 23, 20), "res_k of block 1 above 19")]
    cases += [("tail2", None, put(13, -300), "pw_lo of block 0 below int8"), ("tail2", None, put(32 + 19, 400), "add_hi of block 1 above int8"),
              ("tail2", None, put(32 * 6 + 7, -8), "g_fcw negative")]
    for form, lw in (("tail", 24), ("tail2", 32), ("mid", 32), ("mid-resident", 32)):
        cases += [(form, None, lambda w: np.append(w, 0), "one word too many"), (form, None, lambda w: w[:-1], "one word too few"),
                  # no blocks / nine blocks, in tables of exactly the size those counts call for (the args structs hold eight)
                  (form, 0, lambda w, lw=lw: w[lw * (len(w) // lw):], "n_layers 0"),
                  (form, 9, lambda w, lw=lw: np.concatenate([w[:lw]] + [w[lw: 2 * lw]] * 8 + [w[lw * (len(w) // lw):]]), "n_layers 9"),   # (block 1 is residual: it chains)
                  (form, 0, lambda w: w, "n_layers 0, the table as it is"), (form, 9, lambda w: w, "n_layers 9, the table as it is")]
    return cases


@pytest.mark.parametrize("form,n_layers,mutate,what", _hostile(), ids=[f"{c[0]}: {c[3]}" for c in _hostile()])
def test_hostile_table_is_refused(prog, form, n_layers, mutate, what):
    nl, nc, words = shipped_tables()[form]
    assert _parse(form, plan_of(prog, form, nl, nc, words)) is not None   # (the table is refused for the mutation, not for what it was)
    bad = mutate(words)
    if n_layers in (0, 9) and "as it is" not in what:
        lw, hw = (24 if form == "tail" else 32), (0 if form.startswith("mid") else 16)
        assert len(bad) == lw * n_layers + hw, "the table must have the size the block count calls for"
    assert plan_of(prog, form, nl if n_layers is None else n_layers, nc, bad) == [0], f"{form}: {what} was accepted"


@pytest.mark.parametrize("form", FORMS)
def test_single_word_sweep_of_the_shipped_tables(prog, form):
    """Every word of the table in turn = INT32_MIN, -1, INT32_MAX: no sanitizer report (the program would end with a non-zero status), and
    the planner either refuses or returns a plan it could run under — every LDS offset within [0, lds_bytes], lds_bytes within 160 KB, a
    constant-block size that is not negative.  -1 stands for "not in LDS" in exactly three fields and is allowed there only: the first
    block's ``x_off`` (its input map is in memory), ``fcw_off`` (the classifier is read from memory), ``bar_off`` (no barrier counters)."""
    nl, nc, words = shipped_tables()[form]
    lines = _run(prog, form, nl, nc, words, sweep=True)
    assert len(lines) == 3 * len(words)
    accepted = 0
    for k, line in enumerate(lines):
        v = [int(t) for t in line.split()]
        assert v[:2] == [k // 3, (I32_MIN, -1, I32_MAX)[k % 3]]
        p = _parse(form, v[2:])
        if p is None:
            continue
        accepted += 1
        assert 0 <= p["lds_bytes"] <= LDS_CAP and p["const_words"] >= 0, (v[:2], p)
        offs = [p["mean_off"]] + [o for L in p["layers"][1:] for o in L] + p["layers"][0][1:]
        offs += [o for o in (p["fcw_off"], p["bar_off"], p["layers"][0][0]) if o != -1]
        assert all(0 <= o <= p["lds_bytes"] for o in offs), (v[:2], p)
    print(f"\n{form}: {accepted} of {len(lines)} single-word mutations accepted")
    assert 0 < accepted < len(lines)   # (values that place nothing — zero points, multipliers — are not the planner's to judge)
