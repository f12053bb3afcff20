"""The shape variants of ``tests/i8_variants.py`` on the CPU: what the lowering makes of each (fused stage 2, fused tail, matrix-core
constants, blocks in the tail operator), that the oracle runs it and its outputs are spread enough for a byte comparison to mean
something, and that the embedding mark still sits on the MEAN — so a builder that quietly yields an unfused or flat model fails here,
before tests/test_gpu_i8_variants.py spends device time on it."""
from __future__ import annotations

import numpy as np
import pytest

import i8_mutants as im
import i8_variants as iv


def _plan(name):
    return iv.plan(name)   # (lowered once for this module and tests/test_chain_plan_host.py)


@pytest.mark.parametrize("name", list(iv.VARIANTS))
def test_variant_lowers_to_the_expected_forms_and_is_not_flat(name):
    from birdnet_stm32.models import _pack as pk

    want, c = iv.VARIANTS[name], iv.case(name)
    model, plan = c["model"], _plan(name)
    # -- the graph is what the name says
    h = iv.head_ops(model)
    assert len(iv.tail_chain(model)) == want["layers"] and (h["logistic"] is not None) == want["table"]
    assert c["scores"].shape == c["logits"].shape == (iv.N_INPUTS, want["nc"]) and c["scores"].dtype == np.float32
    # -- the forms
    forms = im.plan_forms(plan)
    tail = [o for o in plan.ops if o.kind == pk.I8_TAIL]
    got = dict(mid=forms["mid"], tail=forms["tail"], tail2=forms["tail2"], layers=tail[0].get("n_layers") if tail else None, nc=tail[0].get("n_classes") if tail else None)
    assert got == dict(mid=1, tail=want["tail"], tail2=want["tail2"], layers=want["layers"] if want["tail"] else None, nc=want["nc"] if want["tail"] else None), got
    if want["tail"]:
        desc = plan.tensors[tail[0].get("desc")].reshape(-1)
        assert (desc[24 * want["layers"] + 11] >= 0) == want["table"], "head word g_hlut: -1 exactly where no table follows the classifier"
    else:   # the per-block operators run: none of them may be left tagged as covered
        assert not any(o.p[pk.TAIL_TAG] in (pk.TAIL_COVERED, pk.TAIL_OP) for o in plan.ops)
        assert sum(o.kind == pk.I8_FC for o in plan.ops) == 1 and sum(o.kind == pk.I8_HEAD for o in plan.ops) == 1
    # -- the conditions on the inputs
    s = iv.spread(c)
    print(f"\n{name}: NC {want['nc']} layers {want['layers']} table {int(want['table'])} | {got} | {s}")
    if want["nc"] == 1:   # 16 bytes in all: the figure stated for this model
        assert s["fc_min_per_class"] >= 4, s
    else:
        assert s["fc_distinct"] >= 24 and s["fc_min_per_class"] >= 2, s
    assert s["fc_saturated"] <= 0.10, s
    if want["table"]:
        assert s["score_distinct"] >= 8, s
        assert np.array_equal(c["scores"], (c["score_bytes"].astype(np.float32) + 128.0) / np.float32(256.0))
    else:
        assert np.array_equal(c["scores"], c["logits"])
    for cls in {0, want["nc"] // 2, want["nc"] - 1}:   # one unit of a classifier weight is visible (what the perturbation test on the device relies on)
        assert iv.weight_flips(c, cls).max() >= 1, cls
    if want["chain"]:
        assert s["emb_distinct"] >= 32 and s["emb_rows_distinct"] >= 12, s
    # -- the embedding mark: the MEAN, and the fused tail beside it where the plan has one
    e, mean_t = plan.embedding, model.tensors[h["mean"].outputs[0]]
    assert e is not None and (e.dim, e.dtype) == (256, "int8")
    assert e.scale == float(np.float32(mean_t.scale[0])) and e.zero_point == int(mean_t.zero_point[0])
    kinds = sorted(plan.ops[i].kind for i in e.marked)
    assert kinds == ([pk.I8_MEAN, pk.I8_TAIL] if want["tail"] else [pk.I8_MEAN])
    mean_op = next(plan.ops[i] for i in e.marked if plan.ops[i].kind == pk.I8_MEAN)
    assert mean_op.name == f"t{h['mean'].outputs[0]}"
    for path in ("input", "audio"):
        assert plan.ops[e.ops[path]].kind == (pk.I8_TAIL if want["tail"] else pk.I8_MEAN)


def test_the_table_covers_what_the_issue_lists():
    v = iv.VARIANTS
    assert {v[f"nc{n}"]["nc"] for n in iv.CLASS_COUNTS} == {1, 15, 16, 17, 100, 128, 129, 252, 253, 256, 257, 1000}
    assert {v[n]["layers"] for n in iv.CHAIN_VARIANTS} | {v["nc100"]["layers"]} == {2, 4, 5, 6, 8, 9}
    assert (v["chain2_nc252"]["layers"], v["chain2_nc17"]["layers"], v["chain8_nc128"]["nc"], v["chain8_nc129"]["nc"]) == (2, 2, 128, 129)
    assert not v["nolog100"]["table"] and not v["nolog17"]["table"] and v["chain9"]["tail"] == 0 and not v["chain9"]["gpu"]
    # the 5-layer chain ends on the stride-2 block, the 2-layer chain is the two stride-2 blocks
    strides = lambda n: [b["dw"].options["stride_w"] for b in iv.tail_chain(iv.case(n)["model"])]   # noqa: E731
    assert strides("chain5") == [2, 1, 1, 1, 2] and strides("chain2") == [2, 2] and strides("chain4") == [2, 1, 2, 1]
    assert strides("chain8") == [2, 1, 1, 1, 1, 2, 1, 1] and strides("chain9") == [2, 1, 1, 1, 1, 1, 2, 1, 1]


def test_shared_front_oracle_equals_a_plain_run():
    """``i8_variants.oracle`` resumes the interpreter behind stage 2: the same bytes as ``Int8Interpreter(model).invoke`` from the input."""
    from oracle.int8_graph import Int8Interpreter

    c = iv.case("chain4")
    scores, env = Int8Interpreter(c["model"]).invoke(iv.inputs()[[0, 9, 10, 15]], return_all=True)
    assert np.array_equal(scores, c["scores"][[0, 9, 10, 15]])
    for t, v in c["env"].items():
        assert np.array_equal(env[t], v[[0, 9, 10, 15]]), t


def test_builders_are_deterministic_and_touch_only_the_back_half():
    base = im.shipped()
    first = iv.tail_chain(base)[0]["dw"].index
    for name in ("nc17", "nolog17", "chain5", "chain8_nc129"):
        a, b = iv.build(name), iv.build(name)
        assert [(o.index, o.name, o.inputs, o.outputs) for o in a.ops] == [(o.index, o.name, o.inputs, o.outputs) for o in b.ops]
        assert [o.index for o in a.ops] == list(range(len(a.ops)))
        for ta, tb in zip(a.tensors, b.tensors):
            assert ta.shape == tb.shape and np.array_equal(ta.scale, tb.scale) and (ta.data is None or np.array_equal(ta.data, tb.data))
        assert [(o.name, o.inputs, o.outputs) for o in a.ops[:first]] == [(o.name, o.inputs, o.outputs) for o in base.ops[:first]]
        fc = iv.head_ops(a)["fc"]
        for t0, ta in zip(base.tensors, a.tensors):   # constants other than the classifier's: as shipped
            if t0.data is not None and t0.index not in fc.inputs[1:]:
                assert np.array_equal(t0.data, ta.data) and np.array_equal(t0.scale, ta.scale), t0.index


def test_repeated_blocks_share_their_originals_constants():
    m = iv.case("chain8")["model"]
    chain = iv.tail_chain(m)
    for orig, copy_ in ((chain[3], chain[4]), (chain[6], chain[7])):
        for k in ("dw", "pw"):
            assert orig[k].inputs[1:] == copy_[k].inputs[1:] and copy_[k].outputs != orig[k].outputs
            assert im.qp(m, orig[k].outputs[0]) == im.qp(m, copy_[k].outputs[0])
        assert copy_["dw"].inputs[0] == orig["out"] and orig["out"] in copy_["add"].inputs
    assert iv.head_ops(m)["mean"].inputs[0] == chain[7]["out"]
