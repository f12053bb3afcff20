"""``i8_mid2_kernel`` with its constants resident in LDS and chunk-local barriers (option ``i8_mid_split``, the default) against the form
that stages every block's parts behind workgroup barriers (``i8_mid_split`` = 0): a scheduling change, so every byte must be the same."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import TFLITE_PATH, synth_chunks

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 255, 4096, 4097)   # one chunk, a full pair, a ragged pair, fewer groups than CUs, the benchmark's batch, ragged beyond it
LDS_CAP = 160 * 1024


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


def test_resident_plan_of_stage2_overlaps_nothing_and_fits_the_lds(torch_mod):
    """The placement the default form runs under: every block's depthwise part, pointwise part and zero-point row, the barrier counters
    and the maps are pairwise disjoint, and the whole stays within the 160 KB of a CU."""
    from birdnet_stm32 import _hip
    from birdnet_stm32.models.runners import load_model_runner

    assert _hip.get_option("i8_mid_split") == 1 and "i8_mid_split" in _hip.SCHEDULING_OPTION_NAMES
    runner = load_model_runner(TFLITE_PATH, max_batch=4)
    assert runner.mid_form()[0] == 1
    plan = runner.mid_plan()
    assert plan is not None, "the resident placement of the shipped stage-2 chain was refused: the default would silently be the staged form"
    assert plan["blocks"] == 3 and len(plan["parts"]) == 3 + 3 + 2
    assert plan["map_bytes"] == 2 * 16 * 32 * (64 + 16)
    spans = [(0, plan["map_bytes"]), (plan["bar_off"], plan["bar_off"] + 16)] + [(o, o + n) for o, n in plan["parts"]]
    for b, e in spans:
        assert 0 <= b < e <= plan["lds_bytes"] <= LDS_CAP and b % 16 == 0, (b, e, plan)
    spans.sort()
    for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
        assert e0 <= b1, f"[{b0}, {e0}) overlaps [{b1}, {e1})"
    assert sum(n for _, n in plan["parts"]) == 50592   # 7168 + 5376, then twice 13568 + 5376 + 80
    runner.close()


def test_mid_split_gives_the_bytes_of_the_staged_form(torch_mod):
    """Scores and the stage-2 output map (the tensor the tail kernel reads) from audio, ``i8_mid_split`` = 1 against = 0, ``torch.equal`` /
    byte equality at every batch size; once more through the embedding entry point (scores, int8 and float32 embeddings).  No chunk
    barrier may have given up waiting."""
    torch = torch_mod
    from birdnet_stm32 import _hip
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models.runners import load_model_runner

    nmax = max(BATCHES)
    audio = torch.from_numpy(synth_chunks(nmax, seed=61)).cuda()
    runner = load_model_runner(TFLITE_PATH, max_batch=nmax)
    mids = [i for i, o in enumerate(runner.plan.ops) if o.kind == pk.I8_MID]
    assert len(mids) == 1 and runner.mid_form()[0] == 1 and runner.mid_plan() is not None
    for nb in BATCHES:   # (small batches first: a broken barrier shows on one workgroup before it can on 256)
        with _hip.options(i8_mid_split=0):
            s0 = runner.infer_audio_device(audio[:nb]).clone()
            m0 = runner.op_output(mids[0], nb)
        for rep in range(2):
            with _hip.options(i8_mid_split=1):
                s1 = runner.infer_audio_device(audio[:nb])
                m1 = runner.op_output(mids[0], nb)
            assert torch.equal(s1, s0), f"scores, batch {nb}, launch {rep}"
            assert m1.dtype == np.int8 and np.array_equal(m1, m0), f"stage-2 output map, batch {nb}, launch {rep}"
        assert runner.mid_split_giveups() == 0, f"batch {nb}"
    for nb in (3, 4097):
        for dt in ("int8", "float32"):
            with _hip.options(i8_mid_split=0):
                s0, e0 = (t.clone() for t in runner.infer_audio_device(audio[:nb], return_embeddings=True, emb_dtype=dt))
            with _hip.options(i8_mid_split=1):
                s1, e1 = runner.infer_audio_device(audio[:nb], return_embeddings=True, emb_dtype=dt)
            assert torch.equal(s1, s0) and torch.equal(e1, e0), f"embedding entry point, batch {nb}, {dt}"
    assert runner.mid_split_giveups() == 0
    runner.close()
