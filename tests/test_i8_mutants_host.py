"""Coverage ledger of the INT8 weight families of ``tests/i8_mutants.py`` (CPU only): which kernel forms the lowering picks for each family
and which of the special requantisation forms one oracle run actually reaches — so that a GPU comparison on a family (tests/
test_gpu_i8_mutants.py) is known to exercise the form it is meant to.  The shipped checkpoint's own row is printed beside them; the table
in docs/testing.md is this test's output."""
from __future__ import annotations

import numpy as np
import pytest

import i8_mutants as im

# forms every family must keep: the fused stage-2 operator, the fused tail, the constant blocks of the front and strip kernels; only ``dense``
# loses the matrix-core constants of the tail (and so runs i8_tail_kernel)
WANT_FORMS = {f: dict(mid=1, tail=1, tail2=f != "dense", front_strip=True, strip=[True]) for f in im.FAMILIES}
RESIDUAL_CHAIN_BLOCKS = (3, 4, 6, 7, 8, 10)   # residual blocks of i8_mid2_kernel and of the fused tail (the rescale form R, the signed form)


@pytest.fixture(scope="module")
def ledgers():
    from birdnet_stm32.models._lower_i8 import lower_i8

    S = im.boundary_inputs(8)
    out = {}
    for name, model in [("shipped", im.shipped())] + [(f"{f}/{s}", im.mutant(f, s)) for f, s in im.all_mutants()]:
        forms = im.plan_forms(lower_i8(model))
        out[name] = (forms, im.ledger(model, S))
    print()
    for name, (forms, led) in out.items():
        print(im.format_ledger(name, forms, led))
    return out


def test_every_family_lowers_to_the_forms_it_is_meant_to_reach(ledgers):
    assert ledgers["shipped"][0] == dict(mid=1, tail=1, tail2=True, front_strip=True, strip=[True])
    for f, seed in im.all_mutants():
        assert ledgers[f"{f}/{seed}"][0] == WANT_FORMS[f], (f, seed, ledgers[f"{f}/{seed}"][0])


def test_families_are_deterministic_and_leave_the_frontend_alone():
    base = im.shipped()
    stem, _ = im.backbone(base)
    first = stem.inputs[1]
    for f in im.FAMILIES:
        a, b = im.mutant(f, 0), im.mutant(f, 0)
        changed = 0
        for ta, tb, t0 in zip(a.tensors, b.tensors, base.tensors):
            assert np.array_equal(ta.scale, tb.scale) and np.array_equal(ta.zero_point, tb.zero_point)
            assert (ta.data is None) == (tb.data is None) and (ta.data is None or np.array_equal(ta.data, tb.data))
            same = np.array_equal(ta.scale, t0.scale) and np.array_equal(ta.zero_point, t0.zero_point) and (ta.data is None or np.array_equal(ta.data, t0.data))
            changed += not same
            if t0.data is not None and t0.index not in {t for op in im.conv_ops(base, with_fc=True) for t in op.inputs[1:]}:
                assert same, f"{f}: constant tensor {t0.index} outside the backbone changed"
        assert changed > 20, f
    assert first == 59   # (the shipped graph's stem weights: the walk starts where it should)


def test_dead_channels_in_every_stage_kind_and_block(ledgers):
    """``dead``: at least three dead channels MORE than shipped in the stem and in the depthwise and the pointwise stage of every block — stage 1, 2
    and 3-4, pointwise with and without ADD, the first block of each chain kernel and the later ones."""
    _, led = ledgers["dead/0"]
    _, base = ledgers["shipped"]
    assert led["dead"][("stage1", "stem")] >= 3 and base["dead"][("stage1", "stem")] == 0
    for row, row0 in zip(led["blocks"], base["blocks"]):
        assert row["dead_dw"] >= row0["dead_dw"] + 3 and row["dead_pw"] >= row0["dead_pw"] + 3, row
    for stage in im.STAGES:
        for kind in ("dw", "pw", "pw+add"):
            assert led["dead"][(stage, kind)] > base["dead"][(stage, kind)], (stage, kind)
    assert {(r["stage"], r["first"]) for r in led["blocks"]} >= {("stage2", True), ("stage2", False), ("stage3-4", True), ("stage3-4", False)}


def test_edge_family_reaches_both_clamps_unclamped_own_terms_and_the_accumulator_bound(ledgers):
    _, led = ledgers["edge/0"]
    for i, row in enumerate(led["blocks"]):
        assert row["at_lo"] > 0.05 and row["at_hi"] > 0.05, (i, row)
        assert row["dw_pos"][1] > 0.5 and row["dw_ratio"] > 0.5, (i, row)   # accumulators in the upper half of [lo_dw, hi_dw]
        if row["add"]:
            assert row["own_outside"] > 0.05 and 0.05 < row["own_negative"] < 0.95 and row["v_max"] > 0.2, (i, row)


def test_scale_family_reaches_the_ends_of_the_accepted_shifts(ledgers):
    """e1 = 2 .. 16 in both chain kernels, output shifts 1 and 22; e1 = 0 and e1 = 1 are NOT reachable with a fused plan: the lowering refuses them
    (checked here on the plan, so the statement in the family's docstring and in docs/testing.md stays true)."""
    from birdnet_stm32.models._lower_i8 import lower_i8

    _, led = ledgers["scale/0"]
    assert led["e1"] == [4, 2, 16, 2, 6, 10, 16] and led["shifts"] == (1, 22)
    assert all(e >= 2 for _, l in ledgers.values() for e in l["e1"])
    for ratio in (1.0, 2.0):   # own scale = residual scale (e1 = 0) and twice it (e1 = 1), own zero point 0
        m = im.shipped()
        _, blocks = im.backbone(m)
        for blk in (blocks[3], blocks[6]):
            own = m.tensors[blk["pw"].outputs[0]]
            mult = im.get_mult(m, blk["pw"])
            res = next(t for t in blk["add"].inputs if t != blk["pw"].outputs[0])
            own.scale = np.asarray([np.float32(im.qp(m, res)[0] * ratio)], np.float32)
            own.zero_point = np.asarray([0], np.int64)
            im.set_mult(m, blk["pw"], mult)
            assert -im.add_params(m, blk).sh1 == (0 if ratio == 1.0 else 1)
        forms = im.plan_forms(lower_i8(m))
        assert forms["mid"] == 0 and not forms["tail2"], (ratio, forms)


def test_every_special_form_is_hit_by_some_family(ledgers):
    """The forms of the fused kernels that hold only for proven weights, each reached by at least one family in the blocks of the two chain
    kernels: the signed form with negative AND positive own terms, dead channels, own terms beyond the int8 clamp, every accepted residual
    rescale shift class, depthwise accumulators at their bound, |v| within a factor of two of 2^11."""
    fam = {k: v[1] for k, v in ledgers.items() if k != "shipped"}
    for i in RESIDUAL_CHAIN_BLOCKS:
        assert any(0.05 < l["blocks"][i]["own_negative"] < 0.95 for l in fam.values()), i
        assert any(l["blocks"][i]["own_outside"] > 0.05 for l in fam.values()), i
    assert max(r["v_max"] for l in fam.values() for r in l["blocks"] if r["add"]) > 0.5
    assert {e for l in fam.values() for e in l["e1"]} >= {2, 3, 4, 6, 10, 16}
    assert all(any(l["blocks"][i]["dw_ratio"] > 0.99 for l in fam.values()) for i in range(11))
    assert all(any(l["blocks"][i]["dead_pw"] > 0 for l in fam.values()) for i in range(11))
