"""Embeddings without a device: the plan mark lowering puts on the pooled vector in front of the classifier head, the blob and ABI
surface that carries it, the CLI's argument parsing, the npz writer and the chunk-start bookkeeping of ``embed_files``."""

import os

import numpy as np
import pytest

from conftest import KERAS_PATH, TFLITE_PATH


def _marked(plan):
    from birdnet_stm32.models import _pack as pk

    return [i for i, o in enumerate(plan.ops) if o.p[pk.EMB_TAG] == pk.EMB_OP]


def _head_input_op(plan):
    """Index of the operator whose output the classifier (I8_FC in front of I8_HEAD / F32_DENSE) reads: the last writer of its input slot
    in front of it (slots are recycled in plans other than keep_all ones)."""
    from birdnet_stm32.models import _pack as pk

    ops = plan.ops
    heads = [i for i, o in enumerate(ops) if o.kind in (pk.I8_HEAD, pk.F32_DENSE)]
    assert len(heads) == 1
    k = heads[0]
    if ops[k].kind == pk.I8_HEAD:
        k = max(i for i in range(k) if ops[i].out == ops[k].in0)
        assert ops[k].kind == pk.I8_FC
    return max(i for i in range(k) if ops[i].out == ops[k].in0)


def test_shipped_int8_model_marks_tensor_127():
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._tflite_reader import load_tflite
    from birdnet_stm32.models.runners import lower_model_file

    t = load_tflite(TFLITE_PATH).tensors[127]
    for kw in (dict(), dict(fuse=False), dict(keep_all=True)):
        plan = lower_model_file(TFLITE_PATH, **kw)
        e = plan.embedding
        assert e is not None and e.dim == 256 and e.dtype == "int8"
        assert e.scale == float(np.float32(t.scale[0])) and e.zero_point == int(t.zero_point[0]) == -128
        mean = [i for i in e.marked if plan.ops[i].kind == pk.I8_MEAN]
        assert len(mean) == 1 and plan.ops[mean[0]].name == "t127"
        # exactly one marked operator runs per entry path: the fused tail when the plan has one (it covers the MEAN), else the MEAN
        for path in ("input", "audio"):
            oi = e.ops[path]
            assert oi in e.marked
            if len(e.marked) == 2:
                assert plan.ops[oi].kind == pk.I8_TAIL and plan.ops[mean[0]].p[pk.TAIL_TAG] == pk.TAIL_COVERED
            else:
                assert oi == mean[0]
    assert len(lower_model_file(TFLITE_PATH).embedding.marked) == 2   # production plan: MEAN and the fused tail side by side
    assert _head_input_op(lower_model_file(TFLITE_PATH, keep_all=True)) == _marked(lower_model_file(TFLITE_PATH, keep_all=True))[0]


def test_shipped_float_model_marks_the_global_average_pool():
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models.runners import lower_model_file

    fused = lower_model_file(KERAS_PATH)
    assert [fused.ops[i].kind for i in _marked(fused)] == [pk.F32_GAPDENSE]
    plain = lower_model_file(KERAS_PATH, fuse=False)
    (gi,) = _marked(plain)
    assert plain.ops[gi].kind == pk.F32_GAP and gi == _head_input_op(plain)
    for plan in (fused, plain):
        e = plan.embedding
        assert (e.dim, e.dtype, e.scale, e.zero_point) == (256, "float32", 1.0, 0)
        assert e.ops["input"] == e.ops["audio"] == _marked(plan)[0]


TOPOLOGIES = {
    "gap_ir_se": dict(),
    "attnpool_emb_se": dict(use_inverted_residual=False, use_se=True, embeddings_size=128, use_attention_pooling=True, class_activation="sigmoid"),
    "ds_no_se": dict(use_inverted_residual=False, use_se=False, alpha=0.5),
    "ir_deep": dict(use_se=False, depth_multiplier=2, alpha=0.5, mag_scale="none"),
}


@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_build_model_topologies_mark_the_head_input(name):
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models import build_model
    from birdnet_stm32.models._lower_f32 import lower_f32

    args = dict(num_mels=64, spec_width=256, sample_rate=24000, chunk_duration=3, embeddings_size=256, num_classes=10, randomize_bn=True, seed=7)
    args.update(TOPOLOGIES[name])
    spec = build_model("dscnn", **args)
    want_d = args["embeddings_size"]
    for kw in (dict(fuse=False), dict(keep_all=True), dict()):
        plan = lower_f32(spec, **kw)
        marked = _marked(plan)
        assert len(marked) == 1, kw
        assert plan.embedding.dim == want_d
        if plan.ops[marked[0]].kind == pk.F32_GAPDENSE:
            assert not TOPOLOGIES[name].get("use_attention_pooling")
        else:
            assert marked[0] == _head_input_op(plan)
            assert plan.ops[marked[0]].kind == (pk.F32_ATTNPOOL if TOPOLOGIES[name].get("use_attention_pooling") else pk.F32_GAP)


@pytest.mark.parametrize("name", ["ir_se_softmax", "ds_se_emb_sigmoid", "ds_attnpool_sigmoid", "raw_pcen_ir_se"])
def test_exported_int8_graphs_mark_the_head_input(name):
    from test_conversion import EXPORT_TOPOLOGIES, _export

    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models._lower_i8 import lower_i8

    _spec, model, _raw, _x = _export(EXPORT_TOPOLOGIES[name])
    dbg = lower_i8(model, keep_all=True)
    (mi,) = _marked(dbg)
    assert mi == _head_input_op(dbg)
    ti = int(dbg.ops[mi].name[1:])
    t = model.tensors[ti]
    e = dbg.embedding
    assert e.scale == float(np.float32(t.scale[0])) and e.zero_point == int(t.zero_point[0]) and e.dim == dbg.ops[mi].out_shape[0]
    # squeeze-excite MEANs are never marked (the production plan fuses them with their gate layers)
    prod = lower_i8(model)
    for i, o in enumerate(prod.ops):
        if o.kind == pk.I8_MEAN and o.p[pk.TAIL_TAG] == pk.SEGATE_HEAD:
            assert i not in _marked(prod)
    assert all(prod.ops[i].kind in (pk.I8_MEAN, pk.I8_ATTNPOOL, pk.I8_TAIL) for i in _marked(prod))


def test_blobs_with_the_mark_pass_the_blob_check():
    from birdnet_stm32 import _hip
    from birdnet_stm32.models.runners import lower_model_file

    if not os.path.isfile(_hip.LIB_PATH):
        pytest.fail("libbirdnet_hip.so missing: run __graft_entry__.build()")
    for path in (TFLITE_PATH, KERAS_PATH):
        for kw in (dict(), dict(fuse=False)):
            _hip.blob_check(lower_model_file(path, **kw).to_blob())


def test_plan_without_a_mark_has_no_embedding():
    from birdnet_stm32.models import _pack as pk
    from birdnet_stm32.models.runners import lower_model_file

    plan = lower_model_file(TFLITE_PATH, fuse=False)
    for o in plan.ops:
        o.p[pk.EMB_TAG] = 0
    assert plan.embedding is None
    with pytest.raises(ValueError):
        pk.mark_embedding(plan.ops[0], 256)   # the first operator (QUANTIZE / mel mixer) cannot carry it


def test_abi_surface_lists_the_embedding_exports():
    from birdnet_stm32 import _hip

    for name in ("bn_forward_embed", "bn_infer_audio_embed", "bn_model_get_embedding_info"):
        assert name in _hip.EXPORTS
    assert "bn_set_option" in _hip.EXPORTS and (_hip.EMB_F32, _hip.EMB_I8) == (0, 1)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "birdnet_hip.h")).read()
    assert "#define BN_EMB_F32 0" in hdr and "#define BN_EMB_I8 1" in hdr


def test_cli_parses_its_arguments_and_collects_inputs(tmp_path):
    from birdnet_stm32.cli.embed import build_parser, collect_inputs

    a = build_parser().parse_args(["--model_path", "m.tflite", "--input", "d1", "f.wav", "--output", "o.npz", "--pooling", "max", "--dtype", "int8",
                                   "--overlap", "1.5", "--max_duration", "30", "--max_batch", "512", "--device", "1", "--skip_undecodable"])
    assert (a.model_path, a.input, a.output, a.pooling, a.dtype, a.overlap, a.max_duration, a.max_batch, a.device, a.skip_undecodable) == \
        ("m.tflite", ["d1", "f.wav"], "o.npz", "max", "int8", 1.5, 30.0, 512, 1, True)
    d = build_parser().parse_args(["--model_path", "m", "--input", "x", "--output", "o"])
    assert (d.pooling, d.dtype, d.overlap, d.max_duration) == ("none", "float32", 0.0, 60)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--model_path", "m", "--input", "x", "--output", "o", "--pooling", "lme"])
    (tmp_path / "b" / "c").mkdir(parents=True)
    for rel in ("a.wav", "b/x.FLAC", "b/c/y.ogg", "b/c/z.txt", "b/readme.md"):
        (tmp_path / rel).write_bytes(b"")
    got = [os.path.relpath(p, tmp_path) for p in collect_inputs([str(tmp_path)])]
    assert got == ["a.wav", os.path.join("b", "x.FLAC"), os.path.join("b", "c", "y.ogg")]
    with pytest.raises(FileNotFoundError):
        collect_inputs([str(tmp_path / "missing")])


def test_dispatcher_knows_embed():
    from birdnet_stm32 import __main__ as m

    assert "embed" in m.USAGE


@pytest.mark.parametrize("dtype", ["float32", "int8"])
def test_npz_writer_keys_and_shapes(tmp_path, dtype):
    from birdnet_stm32.evaluation.embeddings import FileEmbeddings, save_embeddings_npz

    emb = (np.arange(7 * 8) % 100).reshape(7, 8).astype(dtype)
    res = FileEmbeddings(emb, np.array([0, 0, 0, 2, 2, 2, 2]), np.arange(7) * 1.5, ["a.wav", "b.wav", "c.flac"], np.array([3, 0, 4]), "none", dtype,
                         0.0159, -128, ["b.wav"])
    out = tmp_path / "e.npz"
    save_embeddings_npz(str(out), res)
    z = np.load(out)
    keys = {"embeddings", "file_index", "start_s", "paths", "chunks_per_file"} | ({"scale", "zero_point"} if dtype == "int8" else set())
    assert set(z.files) == keys
    assert z["embeddings"].shape == (7, 8) and z["embeddings"].dtype == np.dtype(dtype) and np.array_equal(z["embeddings"], emb)
    assert z["file_index"].shape == (7,) and z["start_s"].shape == (7,) and list(z["paths"]) == ["a.wav", "b.wav", "c.flac"]
    assert z["chunks_per_file"].tolist() == [3, 0, 4]
    if dtype == "int8":
        assert float(z["scale"]) == np.float32(0.0159) and int(z["zero_point"]) == -128


@pytest.mark.parametrize("overlap", [0.0, 1.5])
def test_chunk_starts_follow_the_pipeline_chunk_table(overlap):
    from birdnet_stm32.audio.pipeline import chunk_table_arrays
    from birdnet_stm32.evaluation.embeddings import chunk_starts

    sr, cd = 24000, 3.0
    n_out = np.array([72000 * 3 + 5000, 1000, 0, 72000, 72000 * 20])
    fi, st = chunk_starts(n_out, sr, cd, overlap)
    start, _valid, owner, counts, _size = chunk_table_arrays(n_out, sr, cd, overlap)
    assert np.array_equal(fi, owner) and np.array_equal(st, start / sr)
    assert fi.shape[0] == int(counts.sum()) and np.all(np.diff(fi) >= 0)
    if overlap == 0.0:
        assert st[fi == 4].tolist() == [3.0 * k for k in range(20)]
    else:
        assert st[fi == 4][:3].tolist() == [0.0, 1.5, 3.0]
    assert st[fi == 1].tolist() == [0.0] and 2 not in fi


def test_embedding_blocks_respect_the_budget():
    from birdnet_stm32.evaluation.embeddings import embedding_blocks

    counts = np.array([10, 20, 0, 5, 100, 1])
    blocks = embedding_blocks(counts, 4, 25 * 4)
    assert blocks == [(0, 1), (1, 4), (4, 5), (5, 6)]
    assert embedding_blocks(counts, 4, 1 << 30) == [(0, 6)]
    assert embedding_blocks(np.zeros(0, np.int64), 4, 100) == []
