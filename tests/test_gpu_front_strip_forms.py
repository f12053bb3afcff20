"""``i8_front_strip_kernel`` with clamp bounds strictly inside int8 and shifts at both ends of what the strip form takes.

The kernel clamps in front of the requantisation's shift, against bounds shifted per channel, and lets the shift write its byte where it
is read next (csrc/bn_requant.h: ``shifted_bounds``, ``deposit_column``; the identity itself: tests/test_front_strip_forms.py).  The shipped
checkpoint has zero points of -128 and ReLU6 ends at 127 in the front block, i.e. clamp bounds that an int8 saturation would give as
well.  The model here, built in memory with the helpers of tests/i8_mutants.py, moves the output quantisation of the stem, of the
stage1_ds1 depthwise and of the stage1_ds1 pointwise convolution so that BOTH bounds lie strictly inside int8, and gives channels of all
three the shifts 1, 18 and 22.  Three results must agree bit for bit on the front block's output map and on the scores: the strip kernel,
the generic ``i8_front_kernel`` (option ``i8_strip`` = 0) and the numpy interpreter — once with the launcher's own rows per wave and once
with ``i8_strip_th`` = 5 (ragged row blocks, the last of two rows: the bottom padding row lands inside a block)."""
from __future__ import annotations

import numpy as np
import pytest

import i8_mutants as im

pytestmark = pytest.mark.gpu

B = 3
# (zero point, ReLU6 end above it) of the three moved tensors: lower bound = zero point > -128, upper bound = zero point + end < 127
DESIGN = {"stem": (-100, 200), "dw": (-90, 180), "pw": (-110, 230)}
_cache: dict = {}


def front_model():
    """The shipped model with the front block's three output quantisations moved inside int8 and shifts 1 / 18 / 22 among the channels."""
    m = im.shipped()
    stem, blocks = im.backbone(m)
    ds1 = blocks[0]
    assert ds1["first"] and ds1["stage"] == "stage1" and ds1["add"] is None
    layers = {"stem": stem, "dw": ds1["dw"], "pw": ds1["pw"]}
    for k, op in layers.items():   # the weight scales stay: the real-valued function is the shipped one, quantised more coarsely
        zp, end = DESIGN[k]
        t = m.tensors[op.outputs[0]]
        t.scale = np.asarray([6.0 / end], np.float32)
        t.zero_point = np.asarray([zp], np.int64)
    for op in layers.values():
        mult = im.get_mult(m, op)
        live = np.nonzero(mult >= 2.0**-23)[0]   # (channels dead as shipped carry biases beyond 2^30: they stay dead)
        assert live.size >= 8
        mult[live[1::6]] = 0.3                   # shift 1, the smallest a strip form takes
        mult[live[3::6]] = 0.75 * 2.0**-22       # shift 22, the largest that is not dead
        mult[live[5::6]] = 0.6 * 2.0**-18        # shift 18
        im.set_mult(m, op, mult)
    return m, layers


def _case() -> dict:
    if not _cache:
        from oracle.int8_graph import Int8Interpreter

        model, layers = front_model()
        S = im.boundary_inputs(8)[[0, 3, 7]]   # a synthetic chunk's spectrogram, all ones, uniform noise
        assert S.shape[0] == B
        scores, env = Int8Interpreter(model).invoke(S, return_all=True)
        _cache.update(model=model, layers=layers, S=S, scores=scores, env=env)
    return _cache


def test_the_model_is_what_the_test_needs():
    """Bounds strictly inside int8, both reached by the oracle's tensors; shifts 1, 18 and 22 present in all three stages."""
    c = _case()
    for k, op in c["layers"].items():
        lo, hi = im.act_bounds(c["model"], op)
        assert -128 < lo < hi < 127, (k, lo, hi)
        assert (lo, hi) == (DESIGN[k][0], DESIGN[k][0] + DESIGN[k][1])
        t = c["env"][op.outputs[0]]
        assert t.min() == lo and t.max() == hi, f"{k}: the inputs reach [{t.min()}, {t.max()}] of [{lo}, {hi}]"
        e = -im.fixed_point(c["model"], op)[1].astype(np.int64)
        assert {1, 18, 22} <= set(e.tolist()), (k, sorted(set(e.tolist())))


@pytest.mark.parametrize("th", [0, 5])
def test_strip_kernel_generic_kernel_and_oracle_agree(th):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    from birdnet_stm32 import _hip
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models.runners import HipRunner

    c = _case()
    want_map = c["env"][c["layers"]["pw"].outputs[0]]
    results = {}
    # keep_all: every operator keeps its own buffer, so the front block's map can be read back; the production plan gives the scores too
    for name, plan in (("keep_all", lower_i8(c["model"], keep_all=True)), ("production", lower_i8(c["model"]))):
        assert im.plan_forms(plan)["front_strip"], f"{name} plan: the front block did not take the strip form"
        runner = HipRunner(plan, max_batch=B)
        front = [i for i, o in enumerate(plan.ops) if o.kind == pk.I8_FRONT]
        assert len(front) == 1
        if th:
            assert want_map.shape[1] % th == 2, "rows per wave of 5 should leave a last block of two rows"
        for strip in (1, 0):
            with _hip.options(i8_strip=strip, i8_strip_th=th):
                scores = runner.predict(c["S"])
                fmap = runner.op_output(front[0], B) if name == "keep_all" else None
            results[(name, strip)] = (scores, fmap)
        runner.close()
    for (name, strip), (scores, fmap) in results.items():
        kern = "strip kernel" if strip else "generic kernel"
        bad = int((scores != c["scores"]).sum())
        print(f"th {th}, {name} plan, {kern}: {bad} differing scores", end="")
        assert bad == 0, f"{name} plan, {kern}, i8_strip_th = {th}: {bad} scores differ from the oracle"
        if fmap is not None:
            badm = int((fmap.reshape(want_map.shape) != want_map).sum())
            print(f", {badm} of {want_map.size} differing map bytes")
            assert badm == 0, f"{name} plan, {kern}, i8_strip_th = {th}: {badm} of {want_map.size} bytes of the front block's map differ from the oracle"
        else:
            print()
    assert np.array_equal(results[("keep_all", 1)][1], results[("keep_all", 0)][1])
    assert np.array_equal(results[("keep_all", 1)][0], results[("keep_all", 0)][0])
