"""The fused back half of the INT8 graph (``i8_tail2_kernel``, behind it ``i8_tail_kernel``, both with the MEAN -> FULLY_CONNECTED -> head
part) on shapes other than the shipped checkpoint's: class counts from 1 to 1000 across the tile edge (15 | 16 | 17), the edge between the
two kernels (128 | 129), the end of the classifier's LDS copy (252 | 253) and the end of the fused tail (256 | 257); a head without a
table; chains of 2, 4, 5 and 8 blocks.  tests/i8_variants.py builds the models, tests/test_i8_variants_host.py asserts on the CPU what
each reaches.  For every variant the production plan against the numpy interpreter, bit for bit: scores, pre-sigmoid outputs and
embeddings at batch sizes that leave the groups of four (tail) and the pairs (stage 2) ragged, under every form the options select, and
WHICH kernel ran.  Perturbed classifier constants must show up — in the one column and under the one form that reads them."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import i8_mutants as im
import i8_variants as iv

pytestmark = pytest.mark.gpu

BATCHES = (16, 1, 2, 3, 5, 9)
ALTERNATIVES = (dict(i8_tail=0), dict(i8_tail_mfdw=0), dict(i8_tail_fclds=0), dict(i8_tail_mfdw=0, i8_tail_fclds=0))
TAIL_FORM = iv.TAIL_FORM   # ``runner.tail_form()[0]`` per variant (tests/i8_variants.py says where the values come from)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


def _runner(model_or_plan):
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models.runners import HipRunner

    plan = model_or_plan if isinstance(model_or_plan, pk.Plan) else lower_i8(model_or_plan)
    return HipRunner(plan, max_batch=iv.N_INPUTS)


def _forward(torch, runner, x):
    """One production forward: (scores, pre-sigmoid outputs, int8 embeddings) as numpy arrays."""
    s, l, e = runner.predict_device(x, return_logits=True, return_embeddings=True, emb_dtype="int8")
    torch.cuda.synchronize()
    return s.cpu().numpy(), l.cpu().numpy(), e.cpu().numpy()


def _diff(got, c, nb) -> dict:
    want = (c["scores"][:nb], c["logits"][:nb], c["emb"][:nb])
    return {n: int((g != w).sum()) for n, g, w in zip(("scores", "logits", "emb"), got, want)}


def _launched(runner, x) -> dict:
    runner.profile(True)
    runner.predict_device(x)
    rows = {}
    for r in runner.profile_collect():
        if r["launches"]:
            rows[r["kind"]] = rows.get(r["kind"], 0) + r["launches"]
    runner.profile(False)
    return rows


@pytest.mark.parametrize("name", iv.GPU_VARIANTS)
def test_variant_bit_exact_under_every_form(torch_mod, name):
    torch = torch_mod
    from birdnet_stm32 import _hip

    c, S = iv.case(name), iv.inputs()
    runner = _runner(c["model"])
    form = runner.tail_form()
    print(f"\n{name}: tail_form {form}, expected {TAIL_FORM[name]}")
    x = torch.from_numpy(S.reshape(iv.N_INPUTS, -1)).cuda()
    # scores and pre-sigmoid outputs
    for nb in BATCHES:
        for rep in range(2):
            s, l = runner.predict_device(x[:nb], return_logits=True)
            torch.cuda.synchronize()
            s, l = s.cpu().numpy(), l.cpu().numpy()
            bad = (int((s != c["scores"][:nb]).sum()), int((l != c["logits"][:nb]).sum()))
            assert bad == (0, 0), f"{name}, batch {nb}, launch {rep}: {bad} differing (scores, logits) of {s.size}"
    # embeddings (the embedding instantiations of the tail kernels)
    for nb in (16, 3):
        e8, e32 = runner.embed(S[:nb], dtype="int8"), runner.embed(S[:nb])
        assert e8.dtype == np.int8 and np.array_equal(e8, c["emb"][:nb]), f"{name}, batch {nb}: {int((e8 != c['emb'][:nb]).sum())} int8 embedding bytes differ"
        assert e32.dtype == np.float32 and np.array_equal(e32, c["emb_f32"][:nb]), f"{name}, batch {nb}: float32 embeddings differ"
    # the other forms
    for nb in (16, 3):
        for alt in ALTERNATIVES:
            with _hip.options(**alt):
                d = _diff(_forward(torch, runner, x[:nb]), c, nb)
            assert not any(d.values()), f"{name}, {alt}, batch {nb}: differing elements {d}"
    # which kernel ran
    rows = _launched(runner, x)
    if TAIL_FORM[name]:
        assert rows.get("i8_tail") == 1 and "i8_mean" not in rows and "i8_fc" not in rows and "i8_head" not in rows, rows
    else:
        assert "i8_tail" not in rows and rows.get("i8_mean") == 1 and rows.get("i8_fc") == 1 and rows.get("i8_head") == 1, rows
    with _hip.options(i8_tail=0):
        rows = _launched(runner, x)
    assert "i8_tail" not in rows and rows.get("i8_mean") == 1 and rows.get("i8_fc") == 1, rows
    assert rows.get("i8_mid") == 1 and runner.mid_form()[0] == 1 and runner.mid_split_giveups() == 0
    runner.close()
    assert form[0] == TAIL_FORM[name], f"{name}: tail_form {form}, expected form {TAIL_FORM[name]}"


# ------------------------------------------------------------------------------------------------ the comparison can fail
def test_a_perturbed_classifier_weight_shows_in_its_column_under_the_form_that_reads_it(torch_mod):
    """NC = 17: class 16 is the only real row of the second class tile of ``i8_tail2_kernel``.  One of its weights + 1, (a) in the
    matrix-core fragments of the second form's constants, (b) in ``i8_tail_kernel``'s classifier section, (c) in a PADDED row (class 17 ..
    31) of the fragments.  (a) and (b) must give exactly the bytes of the oracle run on the model with that weight + 1 (and the bias that
    leaves the plan's folded bias word as it is) — differing from the
    unperturbed oracle in column 16 and nowhere else — under the form that reads the perturbed block, and the unperturbed bytes under
    the others; (c) must change nothing."""
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8

    c, S = iv.case("nc17"), iv.inputs()
    cls = 16
    flips = iv.weight_flips(c, cls)   # (resize_head puts one input of every class on a rounding boundary)
    k, flips = int(np.argmax(flips)), int(flips.max())
    assert flips >= 1, f"no weight of class {cls} changes the classifier byte on any input: the inputs are too weak"
    # the oracle on the model with W[16][k] + 1
    bad_model = copy.deepcopy(c["model"])
    fc = iv.head_ops(bad_model)["fc"]
    w = im.get_w(bad_model, fc)
    w[cls, k] += 1
    im.set_w(bad_model, fc, w)
    b = im.get_b(bad_model, fc)
    b[cls] += im.qp(bad_model, fc.inputs[0])[1]   # the plan stores b - zp sum(w): a weight + 1 with that word unchanged is this bias in the model
    im.set_b(bad_model, fc, b)
    bad_scores, env = iv.oracle(bad_model, S)
    s_fc, z_fc = im.qp(bad_model, fc.outputs[0])
    bad = dict(scores=bad_scores, logits=(env[fc.outputs[0]].astype(np.float32) - np.float32(z_fc)) * np.float32(s_fc), emb=c["emb"])
    cols = np.nonzero((bad["logits"] != c["logits"]).any(axis=0))[0].tolist()
    assert cols == [cls] and int((bad["logits"] != c["logits"]).sum()) == flips

    plan = lower_i8(c["model"])
    tail = next(o for o in plan.ops if o.kind == pk.I8_TAIL)
    n_layers = tail.get("n_layers")
    g_w1 = int(plan.tensors[tail.get("desc")].reshape(-1)[24 * n_layers + 7])
    g_w2 = int(plan.tensors[tail.get("desc2")].reshape(-1)[32 * n_layers + 7])
    ks, g, j = k // 64, (k % 64) // 16, k % 16    # fragments [class tile][ks][lane = 16 g + m][16 bytes]: byte j = W[16 ct + m][64 ks + 16 g + j]

    def frag_byte(row: int) -> int:
        return 4 * g_w2 + (((row // 16) * 4 + ks) * 64 + 16 * g + row % 16) * 16 + j

    cases = {"a_tail2_fragments": (2, frag_byte(cls)), "b_tail_section": (0, 4 * g_w1 + 256 * cls + k), "c_padded_row": (2, frag_byte(cls + 7))}
    reads = {"a_tail2_fragments": [dict(), dict(i8_tail_fclds=0)], "b_tail_section": [dict(i8_tail_mfdw=0), dict(i8_tail_mfdw=0, i8_tail_fclds=0)], "c_padded_row": []}
    x = torch.from_numpy(S.reshape(iv.N_INPUTS, -1)).cuda()
    for which, (ti, byte) in cases.items():
        p = copy.deepcopy(plan)
        cst = p.tensors[tail.t[ti]].copy()
        b8 = cst.reshape(-1).view(np.int8)
        want_old = 0 if which == "c_padded_row" else int(im.get_w(c["model"], iv.head_ops(c["model"])["fc"])[cls, k])
        assert int(b8[byte]) == want_old, f"{which}: the byte is not the weight it is taken for"
        b8[byte] += 1
        p.tensors[tail.t[ti]] = cst
        blob = p.to_blob()
        assert _hip.load_library().bn_blob_check(blob, len(blob)) == 0
        runner = _runner(p)
        assert runner.tail_form()[0] == 2
        for alt in (dict(),) + ALTERNATIVES:
            with _hip.options(**alt):
                got = _forward(torch, runner, x)
            want = bad if alt in reads[which] else c
            d = _diff(got, want, iv.N_INPUTS)
            print(f"{which} {alt}: differing from the {'perturbed' if want is bad else 'unperturbed'} oracle {d}")
            assert not any(d.values()), f"{which}, {alt}: {d} elements differ from the {'perturbed' if want is bad else 'unperturbed'} oracle"
            if want is bad:
                dc = np.nonzero((got[1] != c["logits"]).any(axis=0))[0].tolist()
                assert dc == [cls], f"{which}, {alt}: columns {dc} differ from the unperturbed oracle"
        runner.close()
