"""CPU tests of query by example: the numpy specification ``search_reference`` on hand-checked cases, the host side of
``EmbeddingIndex`` (archives, block merge) and the ``search`` command's parser, refusals and CSV writer."""

import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG


def _ref(*a, **kw):
    from birdnet_stm32.evaluation.search import search_reference

    return search_reference(*a, **kw)


def test_module_needs_no_torch_at_import():
    code = "import sys; import birdnet_stm32.evaluation.search; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_ties_are_broken_by_index():
    db = np.array([[1, 0], [0, 1], [2, 0], [1, 0], [1, 1]], np.float32)
    idx, score = _ref(db, np.array([[1, 0]], np.float32), 4, "cosine")
    assert idx.tolist() == [[0, 2, 3, 4]] and score[0, :3].tolist() == [1.0, 1.0, 1.0]   # rows 0, 2 and 3 all score 1: by index
    assert score[0, 3] == np.float32(np.float32(1.0) * np.float32(1.0) / np.sqrt(np.float32(2.0)))
    idx, score = _ref(db, np.array([[1, 0]], np.float32), 5, "dot")
    assert idx.tolist() == [[2, 0, 3, 4, 1]] and score.tolist() == [[2.0, 1.0, 1.0, 1.0, 0.0]]
    assert idx.dtype == np.int64 and score.dtype == np.float32


def test_zero_vectors_score_zero():
    db = np.array([[0, 0], [3, 4], [0, 0]], np.float32)
    idx, score = _ref(db, np.array([[3, 4], [0, 0]], np.float32), 3, "cosine")
    assert idx.tolist() == [[1, 0, 2], [0, 1, 2]]
    assert score[0].tolist() == [np.float32(np.float32(25 * np.float32(0.2)) * np.float32(0.2)), 0.0, 0.0] and score[1].tolist() == [0.0, 0.0, 0.0]


def test_k_beyond_the_rows_pads():
    db = np.array([[1, 0], [0, 1]], np.float32)
    idx, score = _ref(db, np.array([[0, 2]], np.float32), 4, "dot")
    assert idx.tolist() == [[1, 0, -1, -1]] and score[0, :2].tolist() == [2.0, 0.0] and np.isneginf(score[0, 2:]).all()
    with pytest.raises(ValueError):
        _ref(db, np.zeros((1, 3), np.float32), 1)
    with pytest.raises(ValueError):
        _ref(db, db, 1, "euclid")


def test_group_exclusion():
    db = np.array([[1, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    q = np.array([[1, 0], [0, 1]], np.float32)
    idx, score = _ref(db, q, 3, "cosine", db_group=[0, 1, 1, 2], query_group=[1, 2])
    assert idx.tolist() == [[0, 3, -1], [2, 0, 1]]   # query 0 loses rows 1 and 2, query 1 loses row 3
    assert score[0, 0] == 1.0 and np.isneginf(score[0, 2])
    assert _ref(db, q, 3, "cosine", db_group=[0, 1, 1, 2])[0].tolist() == _ref(db, q, 3, "cosine")[0].tolist()   # one side only: no exclusion


@pytest.mark.parametrize("zp", [-128, 0, 5])
def test_int8_equals_float_on_dequantised_rows_when_both_are_exact(zp):
    """Bytes within 16 of the zero point, D = 8: (byte - zp) are small integers, so every float32 product and sum is exact and the
    float path on the dequantised rows (scale 1) computes the same numbers as the integer path."""
    rng = np.random.default_rng(zp + 200)
    lo, hi = max(-128, zp - 16), min(127, zp + 16)
    db = rng.integers(lo, hi + 1, (200, 8)).astype(np.int8)
    db[5] = zp
    db[9] = db[3]
    q = db[[3, 5, 50, 77]]
    for metric in ("cosine", "dot"):
        ii, si = _ref(db, q, 12, metric, zero_point=zp)
        fi, sf = _ref((db.astype(np.int32) - zp).astype(np.float32), (q.astype(np.int32) - zp).astype(np.float32), 12, metric)
        assert np.array_equal(ii, fi) and np.array_equal(si.view(np.uint32), sf.view(np.uint32)), metric
    with pytest.raises(ValueError):
        _ref(db, q.astype(np.float32), 3)


def test_host_block_merge_equals_one_search():
    from birdnet_stm32.evaluation.search import merge_topk

    rng = np.random.default_rng(1)
    db = (rng.integers(0, 16, (300, 16)) / 16.0).astype(np.float32)
    db[100:120] = db[10:30]   # ties across blocks
    q = db[[10, 15, 200]]
    for k in (1, 7, 64):
        want = _ref(db, q, k, "cosine")
        bounds = [0, 64, 128, 150, 300]
        parts = [_ref(db[a:b], q, k, "cosine") for a, b in zip(bounds, bounds[1:])]
        idx = [np.where(p[0] >= 0, p[0] + a, -1) for p, a in zip(parts, bounds)]
        got = merge_topk(idx, [p[1] for p in parts], k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _file_embeddings(emb, file_index, start_s, paths, dtype="float32", scale=1.0, zp=0):
    from birdnet_stm32.evaluation.embeddings import FileEmbeddings

    counts = np.bincount(file_index, minlength=len(paths))
    return FileEmbeddings(emb, np.asarray(file_index), np.asarray(start_s, np.float64), list(paths), counts, "none", dtype, scale, zp)


def test_index_round_trips_archives_and_refuses_mismatches(tmp_path):
    from birdnet_stm32.evaluation.embeddings import save_embeddings_npz
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    rng = np.random.default_rng(2)
    a = _file_embeddings(rng.random((5, 8), np.float32), [0, 0, 1, 1, 1], [0, 3, 0, 3, 6], ["x.wav", "y.wav"])
    b = _file_embeddings(rng.random((2, 8), np.float32), [0, 1], [0, 0], ["z.wav", "w.wav"])   # (as a per-file pooled archive: one row per file)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    save_embeddings_npz(pa, a)
    save_embeddings_npz(pb, b)
    one = EmbeddingIndex.from_npz(pa)
    assert np.array_equal(one.embeddings, a.embeddings) and one.file_index.tolist() == [0, 0, 1, 1, 1] and one.start_s.tolist() == [0, 3, 0, 3, 6]
    assert one.paths == ["x.wav", "y.wav"] and one.dtype == "float32" and one.dim == 8 and len(one) == 5
    both = EmbeddingIndex.from_npz(pa, pb)
    assert len(both) == 7 and both.paths == ["x.wav", "y.wav", "z.wav", "w.wav"] and both.file_index.tolist() == [0, 0, 1, 1, 1, 2, 3]
    assert np.array_equal(both.embeddings, np.concatenate([a.embeddings, b.embeddings]))
    assert EmbeddingIndex(a.embeddings, a.file_index, a.start_s, a.paths, budget_bytes=2 * 8 * 4).block_ranges() == [(0, 2), (2, 4), (4, 5)]
    q8 = rng.integers(-128, 128, (3, 8)).astype(np.int8)
    pc, pd, pe, pf = (str(tmp_path / n) for n in ("c.npz", "d.npz", "e.npz", "f.npz"))
    save_embeddings_npz(pc, _file_embeddings(q8, [0, 0, 0], [0, 3, 6], ["i.wav"], "int8", 0.05, -128))
    save_embeddings_npz(pd, _file_embeddings(q8, [0, 0, 0], [0, 3, 6], ["j.wav"], "int8", 0.05, -127))
    save_embeddings_npz(pe, _file_embeddings(q8, [0, 0, 0], [0, 3, 6], ["k.wav"], "int8", 0.06, -128))
    save_embeddings_npz(pf, _file_embeddings(rng.random((2, 9), np.float32), [0, 0], [0, 3], ["l.wav"]))
    i8 = EmbeddingIndex.from_npz(pc, pc)
    assert i8.dtype == "int8" and i8.zero_point == -128 and np.float32(i8.scale) == np.float32(0.05) and len(i8) == 6
    assert i8.file_group.tolist() == [0, 0]   # the same file twice: one group
    for other, what in ((pa, "does not match"), (pd, "zero point"), (pe, "scale")):
        with pytest.raises(ValueError, match=what):
            EmbeddingIndex.from_npz(pc, other)
    with pytest.raises(ValueError, match="does not match"):
        EmbeddingIndex.from_npz(pa, pf)
    np.savez(str(tmp_path / "g.npz"), embeddings=a.embeddings)
    with pytest.raises(ValueError, match="not an archive"):
        EmbeddingIndex.from_npz(str(tmp_path / "g.npz"))
    with pytest.raises(ValueError):
        EmbeddingIndex(a.embeddings, [0, 0, 1, 1, 5], a.start_s, a.paths)
    with pytest.raises(ValueError, match="finite"):
        EmbeddingIndex(np.full((1, 8), np.nan, np.float32), [0], [0.0], ["x.wav"])


def test_same_file_index_compares_resolved_paths(tmp_path):
    from birdnet_stm32.evaluation.search import same_file_index

    (tmp_path / "d").mkdir()
    a = tmp_path / "d" / "a.wav"
    a.write_bytes(b"")
    got = same_file_index([str(a), str(tmp_path / "b.wav")], [str(tmp_path / "d" / ".." / "d" / "a.wav"), str(tmp_path / "c.wav"), str(tmp_path / "b.wav")])
    assert got.tolist() == [0, -1, 1]


def test_parser_defaults_and_refusals(tmp_path):
    from birdnet_stm32.cli.search import build_parser, main, validate_args

    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    base = ["--database", str(db), "--output", "hits.csv"]
    args = build_parser().parse_args(base + ["--model_path", "m.tflite", "--query", "q.wav"])
    assert (args.top_k, args.metric, args.query_pooling, args.min_score, args.exclude_same_file, args.overlap, args.max_duration, args.device) == (
        10, "cosine", "none", None, False, 0.0, 60, 0)
    validate_args(args)
    for extra, what in ((["--model_path", "m.tflite"], "either --query"), (["--query", "q.wav"], "needs --model_path"),
                        (["--model_path", "m.tflite", "--query", "q.wav", "--query_npz", str(db)], "either --query"),
                        (["--model_path", "m.tflite", "--query", "q.wav", "--top_k", "0"], "top_k"),
                        (["--model_path", "m.tflite", "--query", "q.wav", "--top_k", "129"], "top_k"),
                        (["--query_npz", str(db)], "chunk_duration"), (["--query_npz", str(db), "--chunk_duration", "3", "--query_pooling", "avg"], "query_pooling"),
                        (["--query_npz", str(tmp_path / "none.npz"), "--chunk_duration", "3"], "not found")):
        with pytest.raises(SystemExit, match=what):   # refused before any model or archive is read (m.tflite does not exist)
            main(base + extra)
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--metric", "euclid"])


def test_csv_writer_columns(tmp_path):
    from birdnet_stm32.cli.search import CSV_COLUMNS, write_hits_csv
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    index = EmbeddingIndex(np.eye(3, dtype=np.float32), [0, 0, 1], [0.0, 3.0, 1.5], ["a.wav", "b.wav"])
    res = index._result(np.array([[1, 2, -1], [2, 0, 1]]), np.array([[0.9, 0.5, -np.inf], [1.0, 0.25, 0.125]], np.float32), "cosine")
    out = str(tmp_path / "hits.csv")
    assert write_hits_csv(out, ["q.wav", "q.wav"], [0.0, 3.0], res, 3.0, min_score=0.2) == 4
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == CSV_COLUMNS == ("query_path", "query_start_s", "rank", "score", "match_path", "match_start_s", "match_end_s")
    assert rows[1:] == [["q.wav", "0.000", "1", "0.9", "a.wav", "3.000", "6.000"], ["q.wav", "0.000", "2", "0.5", "b.wav", "1.500", "4.500"],
                        ["q.wav", "3.000", "1", "1", "b.wav", "1.500", "4.500"], ["q.wav", "3.000", "2", "0.25", "a.wav", "0.000", "3.000"]]
    assert res.match_path[0][2] is None and np.isnan(res.match_start_s[0, 2])


def test_search_help_through_the_dispatcher():
    import birdnet_stm32.__main__ as m

    assert "search" in m.USAGE
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "search", "--help"], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "--database" in r.stdout and "--query_npz" in r.stdout and "--exclude_same_file" in r.stdout
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "no-such"], env=env, capture_output=True, text=True)
    assert r.returncode == 1 and "search" in r.stdout


def test_abi_constants_stay_in_step():
    import re

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import search

    hdr = open(os.path.join(os.path.dirname(PKG), "include", "birdnet_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (BN_SEARCH_\w+) (\d+)\n", hdr)}
    assert (val["BN_SEARCH_COSINE"], val["BN_SEARCH_DOT"]) == (_hip.SEARCH_METRICS["cosine"], _hip.SEARCH_METRICS["dot"])
    assert (val["BN_SEARCH_MAX_K"], val["BN_SEARCH_MAX_D"]) == (_hip.SEARCH_MAX_K, _hip.SEARCH_MAX_D) == (search.MAX_K, search.MAX_D)
    assert (val["BN_SEARCH_STEP_ROWS"], val["BN_SEARCH_MIN_WG_STEPS"], val["BN_SEARCH_MAX_WGS"]) == (_hip.SEARCH_STEP_ROWS, _hip.SEARCH_MIN_WG_STEPS, _hip.SEARCH_MAX_WGS)
    names = _hip.load_library().bn_kernel_names().decode().split("\n") if os.path.isfile(_hip.LIB_PATH) else None
    assert names is None or {"search_score_kernel", "search_merge_kernel", "search_inv_norms_kernel"} <= set(names)
