"""The fused INT8 chains' epilogues (option ``i8_satpack`` bit 0; ``csrc/bn_i8_tail2.hip``: SAT) and the front strip's stem rows (bit 1;
``csrc/bn_i8_strip.hip``) as the packed shift-and-saturate instruction against the clamp-shift-pack forms they replace, on the device: scores, pre-sigmoid outputs, int8 embeddings and the stage-2 output
map for ``i8_satpack`` = 0, 1, 2, 3 — the same bytes for all four, and the numpy interpreter's — on the shipped model and one model per
family of ``tests/i8_mutants.py``, at a batch that leaves the pair and the group of four ragged and one that makes the persistent kernels
loop.  A perturbed shift constant must be reported; a chain with one narrower clamp must keep the old form and the oracle's bytes.

Models, oracle runs and inputs are those of tests/test_gpu_i8_mutants.py (its module-level cache: each oracle run happens once per session)."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import i8_mutants as im
import satpack_cases as sc
from test_gpu_i8_mutants import _case, _diff, _inputs, _production, _run, _section

pytestmark = pytest.mark.gpu

BATCHES = (5, 37)
MODELS = [("shipped", 0)] + [(f, seeds[0]) for f, seeds in im.FAMILIES.items()]


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


def _four_ways(torch, runner, mid_op, x, nb):
    """The four tensors of one forward under i8_satpack = 0, 1, 2, 3."""
    from birdnet_stm32 import _hip

    out = {}
    for v in (0, 1, 2, 3):
        with _hip.options(i8_satpack=v):
            out[v] = _run(torch, runner, x[:nb], mid_op)
    return out


@pytest.mark.parametrize("family,seed", MODELS)
def test_old_and_new_epilogue_forms_give_the_oracles_bytes(torch_mod, family, seed):
    torch = torch_mod
    from birdnet_stm32 import _hip

    assert _hip.get_option("i8_satpack") == 3 and "i8_satpack" in _hip.SCHEDULING_OPTION_NAMES
    case = _case(family, seed)
    runner, mid_op = _production(case, max(BATCHES))
    # every stored clamp of these models' chains is the int8 range: the new form is what runs by default (dense: no matrix-core tail)
    assert runner.satpack_form() == (1, -1 if family == "dense" else 1, 1)
    x = torch.from_numpy(_inputs()[: max(BATCHES)].reshape(max(BATCHES), -1)).cuda()
    for nb in BATCHES:
        got = _four_ways(torch, runner, mid_op, x, nb)
        for v, tensors in got.items():
            d = _diff(tensors, case, np.arange(nb))
            print(f"{family}/{seed} batch {nb} i8_satpack {v}: differing from the oracle {d}")
            assert not any(d.values()), f"{family}/{seed}, batch {nb}, i8_satpack = {v}: differing elements {d}"
            for name, a, b in zip(("scores", "logits", "emb", "mid"), tensors, got[0]):
                assert a.dtype == b.dtype and np.array_equal(a, b), f"{family}/{seed}, batch {nb}: {name} under i8_satpack = {v} differs from = 0"
    assert runner.mid_split_giveups() == 0
    runner.close()


def test_a_perturbed_shift_is_reported_by_the_new_form(torch_mod):
    """One more on the shift of ONE live depthwise channel of stage 2's last block — channel 1 of a quad, whose shift the new form takes
    from byte 1 of the packed word with an instruction of its own — in the packed plan of the shipped model: the comparison above must see it."""
    torch = torch_mod
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8

    case = _case("shipped", 0)
    plan = lower_i8(case["model"])
    op = next(o for o in plan.ops if o.kind == pk.I8_MID)
    desc = plan.tensors[op.get("desc")].reshape(-1)
    _, blocks = im.backbone(case["model"])
    dw = [b for b in blocks if b["stage"] == "stage2"][2]["dw"]
    e = -im.fixed_point(case["model"], dw)[1].astype(np.int64)
    c = next(int(k) for k in np.nonzero(e <= 20)[0] if k % 4 == 1)
    w = _section(desc, 2)["dwc"] + ((c // 16) * 5 + 4) * 16 + ((c % 16) // 4) * 4
    x = torch.from_numpy(_inputs()[:37].reshape(37, -1)).cuda()

    def run(delta: int) -> dict:
        bad = copy.deepcopy(plan)
        cst = bad.tensors[op.get("cst")].copy()
        word = int(cst.reshape(-1)[w])
        assert (word >> 8) & 0xFF == e[c] - 1, "byte 1 of the packed word = the channel's shift - 1"
        cst.reshape(-1)[w] = word + (delta << 8)
        bad.tensors[op.get("cst")] = cst
        runner, mid_op = _production(case, 37, plan=bad)
        assert runner.satpack_form()[0] == 1
        d = _diff(_run(torch, runner, x, mid_op), case, np.arange(37))
        runner.close()
        return d

    assert not any(run(0).values()), "the unperturbed plan must agree"
    d = run(1)
    print(f"shift of depthwise channel {c} of stage 2's last block + 1: differing {d}")
    assert d["mid"] > 0, "a wrong shift went unnoticed: the comparison cannot fail"


@pytest.mark.parametrize("which", ["narrow_relu6", "add_zero_point"])
def test_a_narrower_clamp_keeps_the_old_form_and_the_oracles_bytes(torch_mod, which):
    """``narrow_relu6``: a ReLU6 output of stage 2 and one of stage 3 with an upper bound below 127 — both chains keep the old form.
    ``add_zero_point``: two ADD outputs of the tail with zero point -120 — the tail keeps the old form, stage 2 (untouched) runs the new one.
    Both plans keep their chains fused.  (No family of ``i8_mutants.FAMILIES`` has a narrower bound on a chain layer: the first test asserts
    the new form for every one of them.)"""
    torch = torch_mod
    from oracle.int8_graph import Int8Interpreter

    model = getattr(sc, which)()
    S = _inputs()[:37]
    scores, env = Int8Interpreter(model).invoke(S, return_all=True)
    fc = next(o for o in model.ops if o.name == "FULLY_CONNECTED")
    s, z = im.qp(model, fc.outputs[0])
    _, blocks = im.backbone(model)
    case = dict(model=model, scores=scores, env=env, emb=env[fc.inputs[0]].reshape(len(S), -1),
                logits=(env[fc.outputs[0]].astype(np.float32) - z) * np.float32(s), mid=env[[b for b in blocks if b["stage"] == "stage2"][-1]["out"]])
    runner, mid_op = _production(case, 37)
    assert runner.mid_form()[0] == 1 and runner.tail_form()[0] == 2, "the chains stay fused"
    assert runner.satpack_form() == ((0, 0, 1) if which == "narrow_relu6" else (1, 0, 1))
    lo_hi = [(int(env[b["out"]].min()), int(env[b["out"]].max())) for b in blocks]
    print(f"{which}: (min, max) of the blocks' output maps {lo_hi}")
    x = torch.from_numpy(S.reshape(37, -1)).cuda()
    for nb in BATCHES:
        for v, tensors in _four_ways(torch, runner, mid_op, x, nb).items():
            d = _diff(tensors, case, np.arange(nb))
            assert not any(d.values()), f"{which}, batch {nb}, i8_satpack = {v}: differing elements {d}"
    runner.close()
