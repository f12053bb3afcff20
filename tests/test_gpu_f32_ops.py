"""Every float32 plan operator on the device against the float64 plan reference, element by element, under the rounding bound derived in
tests/f32_plan_ref.py (no tolerance here comes from device output).

After one forward call every operator with an output is compared.  Its reference input is the DEVICE's own output of the operator in
front (the model input for the first), so the bound is one operator's own arithmetic; an operator that works in place (MEL -> MAG) or
whose input a fused kernel kept on chip (``bn_debug_op_output`` answers BN_ERR_UNSUPPORTED) is folded with its neighbour into one composite
with a chained bound.  Scores and logits are compared the same way.  No element, channel or operator is left out.

Models and inputs: tests/f32_plan_cases.py (seeded models with their BatchNorm betas adjusted until the inputs reach every channel).
Forms: the default options, each float32 launcher switch, the ``fuse=False`` plan, and a keep-everything plan that carries the pair tags
(``lower_f32(tag_pairs=True)``), so that ``f32_front2_kernel``, ``f32_pwdw_kernel`` and the stem inside a PWDW pair run and are held as
composites.  Batches of 6, 1 and 67 (the six inputs repeated; compared at chunks 0, 3, 4, 63, 64, 66: first, borders of four-chunk and
64-position workgroups, last), for every form.  The audio entry (``infer_audio_device``) of every hybrid model is run on two chunks, silence
and a click: the fused STFT + mixer against the float64 STFT under the per-frame bound docs/exactness.md proves; the finalisation from the
device's mel energies and the device's own minimum and maximum, within a few u; everything behind it as on the input path.
"""

import numpy as np
import pytest

import f32_plan_cases as fc
import f32_plan_ref as fr

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},
    "strip0": dict(f32_strip=0),
    "strip_th1": dict(f32_strip_th=1),
    "strip_th5": dict(f32_strip_th=5),
    "wave_dwpw0": dict(wave_dwpw=0),
    "pw_ws0": dict(f32_pw_ws=0),
    "front_staged0": dict(f32_front_staged=0),
    "tile_slice1": dict(f32_tile_slice=1),
    "unfused": "fuse=False",
    "pairs": "tag_pairs=True",  # f32_pwdw at its default, 2: the pair kernel also hands row-block channel sums to the gate behind it
    "pairs_pwdw1": dict(f32_pwdw=1),  # the same plan, gates pool the maps themselves
}
ROWS67 = [0, 3, 4, 63, 64, 66]
CASES = [(m, f) for m in fc.MODELS for f in FORMS if m not in fc.BATCH3_ONLY or f in ("default", "pw_ws0")]
BATCH_CASES = [(m, f) for m in fc.MODELS if m not in fc.BATCH3_ONLY for f in FORMS]
AUDIO_MODELS = [m for m, (args, _) in fc.MODELS.items() if args is None or args.get("audio_frontend") != "raw"]  # every hybrid model


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; there is no CPU fallback to fall back to")
    return torch


def lower(name: str, form: str):
    from birdnet_stm32.models._lower_f32 import lower_f32

    spec, x = fc.case(name)
    if name in fc.BATCH3_ONLY:
        x = x[[0, 4, 5]]
    plan = lower_f32(spec, keep_all=True, fuse=form != "unfused", tag_pairs=True if form.startswith("pairs") else None)
    return plan, x, (FORMS[form] if isinstance(FORMS[form], dict) else {})


def fetcher(runner, B, rows=None):
    from birdnet_stm32 import _hip

    def fetch(oi):
        try:
            a = runner.op_output(oi, B)
        except _hip.HipError as e:
            if "did not write its output" not in str(e):
                raise
            return None  # a fused kernel kept the map on chip: the walker chains the reference into the next operator
        return a if rows is None else a[rows]

    return fetch


def compare(plan, x, fetch, scores, logits, what, mode=None, minmax=None, tagged=False):
    """Walk the plan; every observed operator within its bound.  An operator may be unreadable (held as a composite with the one behind
    it) only where that is expected: the MEL that MAG overwrites in place and, on a plan with pair tags (``tagged``), the head of a tagged
    pair.  Every other operator on the path is compared: the count is asserted.  Returns {kind: worst error / bound}, the composites."""
    from birdnet_stm32.models import _pack as pk

    mode = pk.PATH_INPUT if mode is None else mode
    worst, composites, checked = {}, [], 0
    for oi, op, r, got in fr.walk_plan(plan, x, fetch, mode=mode, minmax=minmax):
        kn = pk.KIND_NAMES[op.kind]
        assert r is not None, f"{what}: operator {oi} ({kn} {op.name}) has no reference"
        if op.out < 0:
            pairs = [("scores", scores, r["out"]), ("logits", logits, r["logits"])]
        elif got is None:
            assert op.kind == pk.F32_MEL or (tagged and op.p[pk.TAIL_TAG] in (pk.FRONT2_HEAD, pk.PWDW_HEAD, pk.PWDW_STEM)), \
                f"{what}: operator {oi} ({kn} {op.name}) reports its output unwritten"
            composites.append(f"{kn} {op.name}")
            continue
        else:
            pairs = [("output", got, r["out"])]
        for label, g, v in pairs:
            assert np.all(np.isfinite(g)), f"{what}: operator {oi} ({kn} {op.name}) {label}: non-finite values"
            ok, ratio, where = fr.check(g, v)
            worst[kn] = max(worst.get(kn, 0.0), ratio)
            assert ok, f"{what}: operator {oi} ({kn} {op.name}) {label}: {ratio:.2f} bounds from the float64 reference at {where}"
            checked += 1
    assert checked == len(fr.path_ops(plan, mode)) - len(composites) + 1  # (the head is compared twice: scores and logits)
    print(f"{what}: worst error / bound per kind: { {k: round(v, 3) for k, v in worst.items()} }; composites: {composites}")
    return worst, composites


def run(torch, runner, x, opts):
    from birdnet_stm32 import _hip

    xt = torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1))).cuda()
    with _hip.options(**opts):
        scores, logits = runner.predict_device(xt, return_logits=True)
        torch.cuda.synchronize()
    return scores.cpu().numpy(), logits.cpu().numpy()


@pytest.mark.parametrize("name,form", CASES)
def test_every_operator_within_its_bound(torch_mod, name, form):
    from birdnet_stm32.models.runners import HipRunner

    plan, x, opts = lower(name, form)
    B = x.shape[0]
    runner = HipRunner(plan, max_batch=B)
    try:
        scores, logits = run(torch_mod, runner, x, opts)
        compare(plan, x, fetcher(runner, B), scores, logits, f"{name} {form} B={B}", tagged=form.startswith("pairs"))
    finally:
        runner.close()


@pytest.mark.parametrize("name,form", BATCH_CASES)
def test_batches_of_1_and_67(torch_mod, name, form):
    from birdnet_stm32.models.runners import HipRunner

    plan, x, opts = lower(name, form)
    x67 = np.ascontiguousarray(np.tile(x, (12,) + (1,) * (x.ndim - 1))[:67])
    runner = HipRunner(plan, max_batch=67)
    try:
        scores, logits = run(torch_mod, runner, x67, opts)
        compare(plan, x67[ROWS67], fetcher(runner, 67, ROWS67), scores[ROWS67], logits[ROWS67], f"{name} {form} B=67", tagged=form.startswith("pairs"))
        for row in (1, 4):  # a synthetic chunk, the spikes
            scores, logits = run(torch_mod, runner, x[row : row + 1], opts)
            compare(plan, x[row : row + 1], fetcher(runner, 1), scores, logits, f"{name} {form} B=1 (input {row})", tagged=form.startswith("pairs"))
    finally:
        runner.close()


@pytest.mark.parametrize("name", AUDIO_MODELS)
def test_audio_entry(torch_mod, name):
    """``infer_audio_device``: STFTMEL from the audio under the proven STFT bound; MELFIN / the finalising front block from the device's
    own mel energies and the device's own minimum and maximum of the chunk (``bn_stft_mag`` returns them: the same kernel's arithmetic
    on the same audio), observed like every other input, so their bound is a few u; every operator behind them from the device's outputs."""
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_f32 import lower_f32
    from birdnet_stm32.models.runners import HipRunner, stft_device

    spec, _ = fc.case(name)
    audio = fc.click_and_silence(spec)
    for tag in (None, True):
        plan = lower_f32(spec, keep_all=True, tag_pairs=tag)
        assert any(o.p[pk.OP_PATH] == pk.PATH_AUDIO for o in plan.ops)
        runner = HipRunner(plan, max_batch=4)
        try:
            d_audio = torch_mod.from_numpy(audio).cuda()
            scores, logits = runner.infer_audio_device(d_audio, return_logits=True)
            _, minmax = stft_device(runner.ctx, d_audio, spec_width=plan.spec_width, normalize=False, return_minmax=True)
            torch_mod.cuda.synchronize()
            compare(plan, audio, fetcher(runner, 4), scores.cpu().numpy(), logits.cpu().numpy(), f"{name} audio entry tag_pairs={tag}", mode=pk.PATH_AUDIO,
                    minmax=minmax.cpu().numpy(), tagged=bool(tag))
        finally:
            runner.close()


def test_pair_tags_run_the_pair_kernels(torch_mod):
    """With the tags on a keep-everything plan the covered maps are reported unwritten (the pair kernels ran): the front block's map in the
    shipped model (``f32_front2_kernel``), expanded maps of inverted-residual blocks (``f32_pwdw_kernel``) and the stem's map inside a
    PWDW pair in the seed-7 model."""
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models.runners import HipRunner

    seen = {}
    for name in ("shipped", "ir_se_default"):
        plan, x, opts = lower(name, "pairs")
        runner = HipRunner(plan, max_batch=x.shape[0])
        try:
            run(torch_mod, runner, x, opts)
            fetch = fetcher(runner, x.shape[0])
            for oi in fr.path_ops(plan):
                op = plan.ops[oi]
                if op.out >= 0 and op.kind != pk.F32_MEL and fetch(oi) is None:
                    seen.setdefault(name, []).append((pk.KIND_NAMES[op.kind], op.p[pk.TAIL_TAG]))
        finally:
            runner.close()
    print("maps kept on chip:", seen)
    assert ("f32_front", pk.FRONT2_HEAD) in seen.get("shipped", [])
    assert ("f32_dwpw", pk.PWDW_HEAD) in seen.get("ir_se_default", [])
    assert ("f32_stem", pk.PWDW_STEM) in seen.get("ir_se_default", [])


def test_altered_plans_exceed_the_bound_and_pass_the_old_check(torch_mod):
    """The device runs a plan with ONE constant altered (tests/f32_plan_cases.py: mutants); the reference keeps the original.  The altered
    operator must leave its bound somewhere — and the relative-to-peak check of tests/test_gpu_parity.py (5e-4 against the oracle's
    activation, peak over the whole map) must still pass: the gap this file closes."""
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_f32 import lower_f32
    from birdnet_stm32.models.runners import HipRunner
    from oracle import float_graph

    spec, x = fc.case("ir_se_default")
    plan = lower_f32(spec, keep_all=True)
    _, acts = float_graph.forward(spec, x, np.float64, return_all=True)
    B = x.shape[0]
    for name, (mplan, oi, shown, what) in fc.mutants(plan, fc.reference_run(plan, x)).items():
        runner = HipRunner(mplan, max_batch=B)
        try:
            run(torch_mod, runner, x, {})
            fetch = fetcher(runner, B)
            over = None
            for oj, op, r, got in fr.walk_plan(plan, x, fetch):  # (the ORIGINAL plan's constants)
                if oj == shown:
                    ok, ratio, where = fr.check(got, r["out"])
                    over = ratio
                    assert not ok, f"{name} ({what}): operator {oj} stays within the bound (worst {ratio:.2f})"
                elif got is not None and op.out >= 0:
                    assert fr.check(got, r["out"])[0], f"{name}: unaltered operator {oj} ({op.name}) left its bound"
            old = 0.0
            for oj in fr.path_ops(plan):
                op = plan.ops[oj]
                if op.out < 0 or op.name not in acts:
                    continue
                a = runner.op_output(oj, B)
                ref = acts[op.name].reshape(a.shape)
                old = max(old, float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-12)))
            print(f"{name}: {what}: {over:.1f} bounds; old relative-to-peak check: worst {old:.2e} (passes below 5e-4)")
            assert old < 5e-4
        finally:
            runner.close()
