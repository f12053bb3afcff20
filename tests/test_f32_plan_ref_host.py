"""The float64 plan reference (tests/f32_plan_ref.py) and the inputs of the float32 operator tests, checked without a GPU.

* packing round trips (matrix-core fragments with their zero rows, band-sparse mel mixer);
* lowering against the oracle by teacher forcing: every plan operator, fed the float64 oracle's layer outputs, must give the oracle's next
  output within the rounding of the folded constants alone (``Ref(fold=True)``: one u per folded weight and bias, chained through fused
  operators).  This pins BatchNorm folding, the band-sparse mixer, the fragment order and the gate / residual wiring on the CPU;
* the bound holds for float32 arithmetic in three summation orders and is not slack: weights cut to bfloat16 exceed it in every operator;
* the inputs reach the channels (>= 95 % of the channels behind every ReLU non-zero somewhere, none at the ReLU6 clamp everywhere);
* the four plan mutants of the sensitivity test move the float64 reference by more than four bounds;
* the audio entry's operators from audio against the oracle run on its own spectrograms.
"""

import copy

import numpy as np
import pytest

import f32_plan_cases as fc
import f32_plan_ref as fr
from birdnet_stm32.models import _pack as pk
from birdnet_stm32.models._lower_f32 import lower_f32, mel_bands, pack_pw_fragments

SEEDED = [n for n, (args, _) in fc.MODELS.items() if args is not None]


@pytest.fixture(scope="module")
def oracle_run():
    """{model: (scores, logits, acts)} of the float64 oracle on the model's inputs, computed once."""
    from oracle import float_graph

    cache = {}

    def run(name):
        if name not in cache:
            spec, x = fc.case(name)
            if name in fc.BATCH3_ONLY:
                x = x[[0, 4, 5]]
            cache[name] = (x, *float_graph.forward(spec, x, np.float64, return_all=True, return_logits=True))
        return cache[name]

    return run


@pytest.mark.parametrize("cin,cout", [(16, 16), (24, 48), (32, 32), (100, 16), (384, 192)])
def test_fragment_round_trip(cin, cout):
    w = np.random.default_rng(cin * 1000 + cout).standard_normal((cin, cout)).astype(np.float32)
    frag = pack_pw_fragments(w)
    assert frag.shape == (-(-cin // 16), cout // 16, 64, 4)
    assert np.array_equal(fr.unpack_pw_fragments(frag, cin), w)
    if cin % 16:  # the rows the packer added are zero, and a non-zero one is refused
        assert np.count_nonzero(frag) == np.count_nonzero(w)
        bad = frag.copy()
        bad[-1, 0, 63, 3] = 1.0  # lane q = 3, e = 3: row 16 j + 15
        with pytest.raises(AssertionError):
            fr.unpack_pw_fragments(bad, cin)


def test_mel_bands_round_trip():
    from birdnet_stm32.audio.melbank import hybrid_mel_mixer

    for sr, M in ((24000, 64), (16000, 32), (22050, 40)):
        mel = hybrid_mel_mixer(sr, 512, M)
        vals, bands = mel_bands(mel, 257)
        assert np.array_equal(fr.unpack_mel_bands(vals, bands, 257), mel[:257])
    dense = np.random.default_rng(0).standard_normal((264, 8)).astype(np.float32)
    dense[:, 3] = 0.0  # an empty band
    dense[5:9, 5] = 0.0  # zeros inside a band are kept
    vals, bands = mel_bands(dense, 257)
    assert bands[1, 3] == 0 and np.array_equal(fr.unpack_mel_bands(vals, bands, 257), dense[:257])


@pytest.mark.parametrize("name", list(fc.MODELS))
def test_lowering_matches_oracle_by_teacher_forcing(oracle_run, name):
    spec, _ = fc.case(name)
    x, scores, logits, acts = oracle_run(name)
    worst = {}
    for fuse in (True, False):
        plan = lower_f32(spec, keep_all=True, fuse=fuse)
        checked = 0
        for oi, op, r, got in fr.walk_plan(plan, x, lambda oi: acts.get(plan.ops[oi].name), ar=fr.Ref(fold=True)):
            pairs = [(scores, r["out"]), (logits, r["logits"])] if op.out < 0 else ([(got, r["out"])] if got is not None else [])
            for g, v in pairs:
                ok, ratio, where = fr.check(g, v)
                kn = pk.KIND_NAMES[op.kind]
                worst[kn] = max(worst.get(kn, 0.0), ratio)
                assert ok, f"{name} fuse={fuse}: operator {oi} ({kn} {op.name}) is {ratio:.2f} fold bounds from the oracle at {where}"
                checked += 1
        assert checked >= len(fr.path_ops(plan)) - 1  # (only an in-place MEL has no oracle layer of its own)
    print(f"{name}: worst distance / fold bound per kind:", {k: round(v, 3) for k, v in worst.items()})


EMU_MODELS = ["shipped", "ir_se_default", "ds_se_attnpool_emb", "raw_small_padded"]


@pytest.mark.parametrize("name", EMU_MODELS)
def test_bound_holds_for_float32_orders_and_sees_bfloat16_weights(oracle_run, name):
    """Every operator in numpy float32, summed forward, in reverse and pairwise, on the oracle's layer outputs (rounded to float32): within the bound everywhere.  With the linear stages' weights cut to bfloat16: outside it somewhere in every operator."""
    spec, _ = fc.case(name)
    x, _, _, acts = oracle_run(name)
    rows = list(range(x.shape[0]))
    worst = {}
    for fuse in (True, False):
        plan = lower_f32(spec, keep_all=True, fuse=fuse)

        def fetch(oi):
            a = acts.get(plan.ops[oi].name)
            return None if a is None else a[rows].astype(np.float32)

        for oi, op, r, _ in fr.walk_plan(plan, x, fetch):
            kn = pk.KIND_NAMES[op.kind]
            for order in ("forward", "reverse", "pairwise"):
                e = fr.eval_op(plan, op, r["in0"], r["in1"], r["gate"], ar=fr.Emu(order))
                for key in ("out", "logits"):
                    if key in e:
                        ok, ratio, where = fr.check(e[key].val, r[key])
                        worst[kn] = max(worst.get(kn, 0.0), ratio)
                        assert ok, f"{name}: operator {oi} ({kn} {op.name}) {order}: float32 is {ratio:.2f} bounds from float64 at {where}"
            if op.kind in fr.WEIGHT_FIELDS:
                e = fr.eval_op(plan, op, r["in0"], r["in1"], r["gate"], ar=fr.Emu("forward", trunc=True))
                # (a stage of its own where the operator's output hardly depends on the weights: the scores in front of attention pooling's softmax)
                seen = [fr.check(e[key].val, r[key]) for key in e if key == "out" or key.startswith("stage_")]
                ok, ratio = all(s[0] for s in seen), max(s[1] for s in seen)
                assert not ok, f"{name}: operator {oi} ({kn} {op.name}): bfloat16 weights stay within the bound (worst {ratio:.2f})"
    print(f"{name}: worst float32 emulation error / bound per kind:", {k: round(v, 3) for k, v in worst.items()})


HYBRID = [n for n, (args, _) in fc.MODELS.items() if args is None or args.get("audio_frontend") != "raw"]


@pytest.mark.parametrize("name", HYBRID)
def test_audio_entry_reference_against_oracle(name):
    """The audio entry's operators from audio (two chunks, silence, a click, dense noise whose minimum is far from zero).

    * Against the oracle run on its own spectrograms, with the oracle's minimum and maximum as the observed extremes: within the device
      bound (the un-normalised mel energies have no oracle layer, so the STFT's proven bound is carried into the finalisation here).  This
      pins ``wsum``, the band-sparse mixer and the finalisation's formula on the CPU.
    * The finalisation alone, from float32 mel energies and observed extremes (what the GPU test gives it): its bound is at most
      ``10 u (|raw| + |mn wsum|) / rng`` (+ ``u`` of the result for the front block's extra product); float32 in three orders stays within the
      operator's bound; with ``wsum`` alone cut to bfloat16, MELFIN and the finalising front block leave it."""
    from oracle import float_graph, stft

    spec, _ = fc.case(name)
    audio = fc.click_and_silence(spec)
    audio = np.concatenate([audio, np.random.default_rng(5).uniform(-1, 1, (1, audio.shape[1])).astype(np.float32)])
    W = int(spec.frontend.attrs["spec_width"])
    mags = [stft.stft_magnitude(a, 512, len(a) // W)[:, :W] for a in audio]
    minmax = np.array([[m.min(), m.max()] for m in mags], np.float32)
    S = np.stack([stft.minmax_normalize(m) for m in mags])[..., None]
    scores, logits, acts = float_graph.forward(spec, S, np.float64, return_all=True, return_logits=True)
    plan = lower_f32(spec, keep_all=True)
    seen = set()
    for oi, op, r, got in fr.walk_plan(plan, audio, lambda oi: acts.get(plan.ops[oi].name), mode=pk.PATH_AUDIO, minmax=minmax):
        assert r is not None
        kn = pk.KIND_NAMES[op.kind]
        for g, v in [(scores, r["out"]), (logits, r["logits"])] if op.out < 0 else ([(got, r["out"])] if got is not None else []):
            ok, ratio, where = fr.check(g, v)
            assert ok, f"{name}: operator {oi} ({kn} {op.name}) is {ratio:.2f} bounds from the oracle at {where}"
        if not (op.kind == pk.F32_MELFIN or (op.kind == pk.F32_FRONT and op.get("raw_mel"))):
            continue
        seen.add(kn)
        raw = fr.exact(r["in0"].val.astype(np.float32))
        mn, mx = r["minmax"]
        wsum = plan.tensors[op.get("wsum")]
        fin = fr.finalise(fr.REF, raw.reshape(len(audio), wsum.size, W), mn, mx, wsum, recip=op.kind == pk.F32_FRONT)
        scale = (np.abs(raw.val.reshape(fin.val.shape)) + np.abs(mn.val * wsum.reshape(1, -1, 1))) / ((mx.val - mn.val) + 1e-10)
        assert np.all(fin.err <= 10 * fr.U * scale + fr.U * fin.val + fr.FLOOR), f"{name}: {kn}: the finalisation's bound is not a few u"
        own = fr.eval_op(plan, op, raw, minmax=(mn, mx))
        worst = 0.0
        for order in ("forward", "reverse", "pairwise"):
            e = fr.eval_op(plan, op, raw, ar=fr.Emu(order), minmax=(mn, mx))
            ok, ratio, where = fr.check(e["out"].val, own["out"])
            worst = max(worst, ratio)
            assert ok, f"{name}: {kn} {order}: float32 is {ratio:.2f} bounds from float64 at {where}"
        # not slack: wsum alone cut to bfloat16 (every other constant intact), evaluated in float32, leaves the bound
        cut = copy.copy(plan)
        cut.tensors = list(plan.tensors)
        cut.tensors[op.get("wsum")] = fr.truncate_bf16(wsum)
        e = fr.eval_op(cut, op, raw, ar=fr.Emu("forward"), minmax=(mn, mx))
        seen_cut = [fr.check(e[key].val, own[key]) for key in e if key == "out" or key.startswith("stage_")]  # (the front block: its finalised map)
        ok, ratio = all(c[0] for c in seen_cut), max(c[1] for c in seen_cut)
        print(f"{name}: {kn} on the audio entry: float32 emulation {worst:.3f} of the bound; wsum cut to bfloat16: {ratio:.1f} bounds")
        assert not ok, f"{name}: {kn}: wsum cut to bfloat16 stays within the bound"
    assert seen


def test_inputs_reach_the_channels(oracle_run):
    for name in SEEDED:
        spec, _ = fc.case(name)
        _, _, _, acts = oracle_run(name)
        share = fc.live_share(spec, acts)
        live, total = sum(v[0] for v in share.values()), sum(v[1] for v in share.values())
        low = min(share.items(), key=lambda kv: kv[1][0] / kv[1][1])
        print(f"{name}: {live} of {total} channels behind a ReLU live ({live / total:.2%}); lowest layer {low[0]}: {low[1][0]} of {low[1][1]}")
        for layer, (n_live, n, n_top) in share.items():
            assert n_live >= 0.95 * n, f"{name}: {layer}: {n_live} of {n} channels live"
            assert n_top == 0, f"{name}: {layer}: {n_top} channels at the ReLU6 clamp everywhere"
    # the same models before the adjustment, for the record, and the shipped checkpoint (data: its dead channels stay)
    from oracle import float_graph

    spec = fc.raw_spec("ir_se_default")
    _, acts = float_graph.forward(spec, fc.model_inputs(spec), np.float64, return_all=True)
    share = fc.live_share(spec, acts)
    print(f"ir_se_default before the beta adjustment: {sum(v[0] for v in share.values())} of {sum(v[1] for v in share.values())} live")
    spec, _ = fc.case("shipped")
    _, _, _, acts = oracle_run("shipped")
    dead = {k: v[1] - v[0] for k, v in fc.live_share(spec, acts).items() if v[1] != v[0]}
    print(f"shipped checkpoint: dead channels per layer (of {sum(v[1] for v in fc.live_share(spec, acts).values())}): {dead}")


def test_mutants_are_visible_to_the_reference():
    spec, x = fc.case("ir_se_default")
    plan = lower_f32(spec, keep_all=True)
    ref = fc.reference_run(plan, x)
    muts = fc.mutants(plan, ref)
    assert set(muts) == {"pw_weight", "dw_corner_tap", "folded_bias", "mel_band_value"}
    for name, (mplan, oi, shown, what) in muts.items():
        mref = fc.reference_run(mplan, x)
        ok, ratio, where = fr.check(mref[shown]["out"].val, ref[shown]["out"])
        print(f"{name}: {what}: moves operator {shown} by {ratio:.1f} bounds at {where}")
        assert ratio > 4.0, f"{name}: the altered plan stays within four bounds ({ratio:.2f})"
        # and nothing in front of the altered operator moves
        assert all(np.array_equal(mref[oj]["out"].val, ref[oj]["out"].val) for oj in ref if oj < oi)
