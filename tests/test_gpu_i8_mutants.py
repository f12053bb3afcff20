"""The fused INT8 kernels on weight sets other than the shipped checkpoint's (tests/i8_mutants.py; what each family reaches is asserted on
the CPU in tests/test_i8_mutants_host.py).  For every mutant: first the one-kernel-per-operator plan against the numpy interpreter, every int8
tensor bit for bit — so that a later mismatch belongs to the fused kernels — then the production plan against the same oracle: scores,
pre-sigmoid outputs, int8 embeddings and the stage-2 output map, at batch sizes that leave the pair (stage 2) and the group of four (tail)
ragged and at one that makes the persistent kernels loop.  Scheduling / fallback switches, a second model in the process and inference
from audio must give the same bytes; perturbed constants must NOT (the comparison can fail)."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import i8_mutants as im
from conftest import synth_chunks

pytestmark = pytest.mark.gpu

N_UNIQUE = 40                 # distinct spectrograms per mutant (numpy interpreter: ~0.1 s each)
BATCHES = (1, 2, 3, 5, 37)
OPTIONS = ("i8_mid_split", "i8_mid", "i8_tail", "i8_tail_mfdw", "i8_strip_mfdw")
ONE_PER_FAMILY = [(f, seeds[0]) for f, seeds in im.FAMILIES.items()]
_cache: dict = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


def _inputs() -> np.ndarray:
    if "S" not in _cache:
        _cache["S"] = im.boundary_inputs(N_UNIQUE)
    return _cache["S"]


def _case(family: str, seed: int) -> dict:
    """Model, oracle results on the shared inputs (every tensor) and the tensors compared: FC output (pre-sigmoid), pooled vector, stage-2 map."""
    key = (family, seed)
    if key not in _cache:
        from oracle.int8_graph import Int8Interpreter

        model = im.shipped() if family == "shipped" else im.mutant(family, seed)
        S = _inputs()
        scores, env = Int8Interpreter(model).invoke(S, return_all=True)
        fc = next(o for o in model.ops if o.name == "FULLY_CONNECTED")
        s, z = im.qp(model, fc.outputs[0])
        _, blocks = im.backbone(model)
        _cache[key] = dict(model=model, scores=scores, env=env, emb=env[fc.inputs[0]].reshape(len(S), -1),
                           logits=(env[fc.outputs[0]].astype(np.float32) - z) * np.float32(s),
                           mid=env[[b for b in blocks if b["stage"] == "stage2"][-1]["out"]])
    return _cache[key]


def _run(torch, runner, x, mid_op):
    """One production forward: (scores, pre-sigmoid outputs, int8 embeddings, stage-2 output map) as numpy arrays."""
    s, l, e = runner.predict_device(x, return_logits=True, return_embeddings=True, emb_dtype="int8")
    torch.cuda.synchronize()
    return s.cpu().numpy(), l.cpu().numpy(), e.cpu().numpy(), runner.op_output(mid_op, x.shape[0])


def _diff(got, case, idx) -> dict:
    """Differing elements per compared tensor against the oracle rows ``idx``."""
    want = (case["scores"][idx], case["logits"][idx], case["emb"][idx], case["mid"][idx])
    return {n: int((g.reshape(w.shape) != w).sum()) for n, g, w in zip(("scores", "logits", "emb", "mid"), got, want)}


def _production(case, max_batch, plan=None):
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models.runners import HipRunner

    runner = HipRunner(plan if plan is not None else lower_i8(case["model"]), max_batch=max_batch)
    mids = [i for i, o in enumerate(runner.plan.ops) if o.kind == pk.I8_MID]
    assert len(mids) == 1
    return runner, mids[0]


@pytest.mark.parametrize("family,seed", im.all_mutants())
def test_mutant_oracle_path_then_production_plan_bit_exact(torch_mod, family, seed):
    torch = torch_mod
    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models.runners import HipRunner

    case = _case(family, seed)
    S, env = _inputs(), case["env"]
    # 1. the generic kernels, tensor by tensor: synthetic spectrogram, noise, all ones, spike, silence
    pick = [0, N_UNIQUE - 1, N_UNIQUE - 6, N_UNIQUE - 5, N_UNIQUE - 7]
    base = HipRunner(lower_i8(case["model"], keep_all=True, fuse=False), max_batch=len(pick))
    got = base.predict(S[pick])
    for oi, op in enumerate(base.plan.ops):
        if op.out < 0:
            continue
        a = base.op_output(oi, len(pick))
        r = env[int(op.name[1:])][pick]
        if op.kind == 20:  # quantised, transposed, zero-padded spectrogram: compare the graph's 264 columns
            r = r.reshape(len(pick), a.shape[1], -1)
            a = a[:, :, : r.shape[2]]
        bad = int((a != r.reshape(a.shape)).sum())
        assert bad == 0, f"oracle path, tensor {op.name} (plan op {oi}): {bad} of {a.size} int8 values differ"
    assert np.array_equal(got, case["scores"][pick])
    base.close()
    # 2. the production plan
    n_big = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 9   # the persistent kernels loop, the last pair / group is ragged
    runner, mid_op = _production(case, n_big)
    assert runner.tail_form()[0] == (1 if family == "dense" else 2), "the tail form the host ledger expects"
    assert runner.mid_form()[0] == 1 and runner.mid_plan() is not None, "fused stage-2 chain with its constants resident"
    x = torch.from_numpy(S.reshape(N_UNIQUE, -1)).cuda()
    for nb in BATCHES:
        idx = np.arange(N_UNIQUE - nb, N_UNIQUE) if nb < 8 else np.arange(nb)   # (the small batches take the corner-case inputs)
        xb = x[torch.from_numpy(idx).cuda()].contiguous()
        for rep in range(2):
            d = _diff(_run(torch, runner, xb, mid_op), case, idx)
            print(f"{family}/{seed} batch {nb} launch {rep}: differing {d}")
            assert not any(d.values()), f"{family}/{seed}, batch {nb}, launch {rep}: differing elements {d}"
    idx = np.random.default_rng(5).integers(0, N_UNIQUE, n_big)
    xb = x[torch.from_numpy(idx).cuda()].contiguous()
    for rep in range(2):
        d = _diff(_run(torch, runner, xb, mid_op), case, idx)
        print(f"{family}/{seed} batch {n_big} launch {rep}: differing {d}")
        assert not any(d.values()), f"{family}/{seed}, batch {n_big}, launch {rep}: differing elements {d}"
    assert runner.mid_split_giveups() == 0
    runner.close()


@pytest.mark.parametrize("family,seed", ONE_PER_FAMILY)
def test_scheduling_and_fallback_options_give_the_same_bytes_on_mutants(torch_mod, family, seed):
    torch = torch_mod
    from birdnet_stm32 import _hip

    case = _case(family, seed)
    runner, mid_op = _production(case, 37)
    x = torch.from_numpy(_inputs()[:37].reshape(37, -1)).cuda()
    for nb in (37, 3):
        idx = np.arange(nb)
        for opt in OPTIONS:
            with _hip.options(**{opt: 0}):
                got = _run(torch, runner, x[:nb], mid_op - 1 if opt == "i8_mid" else mid_op)   # (i8_mid = 0: the last strip kernel writes the map)
            d = _diff(got, case, idx)
            assert not any(d.values()), f"{family}/{seed}, {opt} = 0, batch {nb}: differing elements {d}"
        with _hip.options(i8_mid=0, i8_tail=0):
            d = _diff(_run(torch, runner, x[:nb], mid_op - 1), case, idx)
        assert not any(d.values()), f"{family}/{seed}, block kernels only, batch {nb}: {d}"
    assert runner.mid_split_giveups() == 0
    runner.close()


@pytest.mark.parametrize("family", ["perm", "sign"])
def test_mutant_from_audio(torch_mod, family):
    torch = torch_mod
    from oracle import stft
    from oracle.int8_graph import Int8Interpreter

    case = _case(family, 0)
    audio = synth_chunks(11, seed=23)
    want = Int8Interpreter(case["model"]).invoke(np.stack([stft.hybrid_spectrogram(a) for a in audio])[..., None])
    runner, _ = _production(case, 11)
    for rep in range(2):
        got = runner.infer_audio_device(torch.from_numpy(audio).cuda()).cpu().numpy()
        assert np.array_equal(got, want), f"{family}/0 from audio, launch {rep}: {int((got != want).any(axis=1).sum())} of 11 chunks differ"
    runner.close()


def test_a_mutant_and_the_shipped_model_side_by_side(torch_mod):
    """Resident LDS constants and cached plans belong to a model: two models in one process, calls alternating, each its own oracle's bytes."""
    torch = torch_mod
    cases = [_case("edge", 0), _case("shipped", 0), _case("dead", 0)]
    runners = [_production(c, 37) for c in cases]
    x = torch.from_numpy(_inputs()[:37].reshape(37, -1)).cuda()
    for rep in range(3):
        for nb in (37, 2):
            for c, (r, mid_op) in zip(cases, runners):
                d = _diff(_run(torch, r, x[:nb], mid_op), c, np.arange(nb))
                assert not any(d.values()), f"round {rep}, batch {nb}: {d}"
    assert runners[0][0].mid_split_giveups() == 0
    for r, _ in runners:
        r.close()


# ------------------------------------------------------------------------------------------------ the comparison can fail
def _section(desc, i: int) -> dict:
    """Word offsets inside block ``i``'s run of the matrix-core constant tensor (``tail2_layer_section``): depthwise constants ``dwc`` [ct][kind][g][4]
    behind the depthwise fragments, pointwise constants ``pwc`` [nt][kind][g][4] behind the pointwise fragments."""
    row = desc[32 * i : 32 * i + 32]
    C, N, g_cst = int(row[2]), int(row[3]), int(row[24])
    nct, ks, nt, kinds = C // 16, (C + 63) // 64, N // 16, 8 if i == 0 else 5
    dwc = g_cst + nct * 3 * 256
    pwc = dwc + nct * kinds * 16 + nt * ks * 256
    return dict(dwc=dwc, pwc=pwc, kinds=kinds, add=bool(row[9]))


def _c1_flips(case, blk, n: int) -> np.ndarray:
    """Per channel of ``blk``'s depthwise stage: how many of its outputs on the first ``n`` inputs change when the channel's c1 grows by one —
    the sign-free form ``((x m + C) >> 32) >> (e - 1)``, C = (c1 << 31) + 2^30, evaluated in int64 numpy on the oracle's depthwise input (and
    checked against the oracle's depthwise output first).  Dead channels count 0."""
    model, env, dw = case["model"], case["env"], blk["dw"]
    acc = im.conv_acc(model, dw, env[dw.inputs[0]][:n])
    mu, sh = im.fixed_point(model, dw)
    mu, e = mu.astype(np.int64), -sh.astype(np.int64)
    _, z = im.qp(model, dw.outputs[0])
    lo, hi = im.act_bounds(model, dw)
    live = e <= 22
    c1 = (np.int64(1) << np.where(live, e - 1, 0)) + (np.int64(z) << np.where(live, e, 1))

    def form(c1):
        return np.clip(((acc * mu + (c1 << 31) + (1 << 30)) >> 32) >> np.where(live, e - 1, 0), lo, hi)

    base = form(c1)
    assert np.array_equal(base[..., live], env[dw.outputs[0]][:n].astype(np.int64)[..., live]), "the sign-free form as restated here differs from the oracle"
    return (base != form(c1 + 1)).reshape(-1, acc.shape[-1]).sum(axis=0) * live


def _perturbations(plan, case, n: int) -> dict:
    """name -> (constant tensor word, new value) in the stage-2 operator's constants, each an ARITHMETIC constant of a live channel:
    (a) the rounding addend C of a depthwise channel of the last block — the channel whose outputs one more unit of c1 changes most often on
    the tested inputs (``_c1_flips``: many channels of ``edge`` see only a few distinct accumulators, none of them on a rounding boundary),
    (b) the ``half`` term of a channel of residual block 2, (c) the right-border bias of a channel of the first block."""
    from birdnet_stm32.models import _pack as pk

    model = case["model"]
    op = next(o for o in plan.ops if o.kind == pk.I8_MID)
    cst, desc = plan.tensors[op.get("cst")].reshape(-1), plan.tensors[op.get("desc")].reshape(-1)
    _, blocks = im.backbone(model)
    mid = [b for b in blocks if b["stage"] == "stage2"]
    out = {}
    # (a) kind 2 holds (C low, C high) of r = 0, 1; kind 3 of r = 2, 3
    flips = _c1_flips(case, mid[2], n)
    c = int(np.argmax(flips))
    out["a_flips"] = int(flips[c])
    w = _section(desc, 2)["dwc"] + ((c // 16) * 5 + 2 + (c % 4) // 2) * 16 + ((c % 16) // 4) * 4 + 2 * (c % 2)
    lo = int(cst[w])
    assert lo & 0x3FFFFFFF == 0 and (lo >> 30) & 1, "C low dword = (c1 & 1) << 31 | 2^30"
    out["a_c_low_plus_1"] = (w, lo + 1)
    # one unit of c1 = bit 31 of the low dword: set it, or clear it and carry into the high dword
    out["a_c1_plus_1"] = {w: lo - (1 << 31)} if lo > 0 else {w: lo + (1 << 31), w + 1: int(cst[w + 1]) + 1}
    # (b) residual block 2: kind 2 / 3 hold (2^31, half) pairs
    e = -im.fixed_point(model, mid[2]["pw"])[1].astype(np.int64)
    c = int(np.argmin(np.where(e <= 22, e, 99)))
    w = _section(desc, 2)["pwc"] + ((c // 16) * 5 + 2 + (c % 4) // 2) * 16 + ((c % 16) // 4) * 4 + 2 * (c % 2) + 1
    assert int(cst[w]) == 1 << (int(e[c]) - 1) and int(cst[w - 1]) == -(1 << 31), "half term of the signed form"
    out["b_half_doubled"] = (w, 2 * int(cst[w]))
    # (c) first block: kind 5 = bias of the positions whose window leaves the map on the right; + four output steps
    mult = im.get_mult(model, mid[0]["dw"])
    c = int(np.argmax(np.where(mult < 0.4, mult, 0)))
    w = _section(desc, 0)["dwc"] + ((c // 16) * 8 + 5) * 16 + ((c % 16) // 4) * 4 + c % 4
    out["c_right_border_bias"] = (w, int(cst[w]) + int(round(4.0 / mult[c])))
    return out


@pytest.mark.parametrize("which", ["a_c1_plus_1", "b_half_doubled", "c_right_border_bias"])
def test_a_perturbed_constant_is_reported_as_a_mismatch(torch_mod, which):
    """One arithmetic constant of the fused stage-2 operator changed in the packed plan of the ``edge`` mutant (values only: ``bn_blob_check``
    still accepts the blob): the comparison of the first test must report differing bytes, i.e. the inputs reach that constant.

    (a) is the rounding addend C = (c1 << 31) + 2^30 of a depthwise channel.  ``C low dword + 1`` itself can never show: where a stage's input
    and output scales are equal (every depthwise stage of stage 2-4) the Q31 multiplier is a float32 mantissa << 7, so the low 7 bits of
    ``x m + C`` are zero for every x and an addend below 128 cannot carry into the high dword — the kernel's result is the same for EVERY
    input, not only for the tested ones (asserted below on the multipliers, and the perturbed plan is run and must still agree).  The smallest
    change of C that arithmetic can see is one unit of c1 (low dword + 2^31, carried into the high dword when bit 31 is set): that one is
    required to mismatch."""
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8

    case = _case("edge", 0)
    plan = lower_i8(case["model"])
    per = _perturbations(plan, case, 37)
    op = next(o for o in plan.ops if o.kind == pk.I8_MID)
    x = torch.from_numpy(_inputs()[:37].reshape(37, -1)).cuda()
    idx = np.arange(37)

    def run(words: dict) -> dict:
        bad = copy.deepcopy(plan)
        cst = bad.tensors[op.get("cst")].copy()
        for w, v in words.items():
            cst.reshape(-1)[w] = v
        bad.tensors[op.get("cst")] = cst
        blob = bad.to_blob()
        assert _hip.load_library().bn_blob_check(blob, len(blob)) == 0
        runner, mid_op = _production(case, 37, plan=bad)
        assert runner.mid_form()[0] == 1
        d = _diff(_run(torch, runner, x, mid_op), case, idx)
        runner.close()
        return d

    assert not any(run({}).values()), "the unperturbed plan must agree"
    if which == "a_c1_plus_1":
        _, blocks = im.backbone(case["model"])
        m, _ = im.fixed_point(case["model"], [b for b in blocks if b["stage"] == "stage2"][2]["dw"])
        assert (m.astype(np.int64) % 128 == 0).all()
        assert per["a_flips"] > 50, f"one more unit of c1 changes only {per['a_flips']} depthwise outputs of the best channel: the inputs are too weak"
        w, v = per["a_c_low_plus_1"]
        inert = run({w: v})
        print(f"C low dword + 1: differing {inert}")
        assert not any(inert.values()), "C low dword + 1 cannot carry (see the docstring), yet bytes differ"
        words = per[which]
    else:
        w, v = per[which]
        words = {w: v}
    d = run(words)
    print(f"{which}: differing {d}")
    assert d["mid"] > 0, f"{which}: the perturbed constant went unnoticed in the stage-2 map — the family does not reach it"
