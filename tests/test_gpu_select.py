"""GPU tests of select (csrc/bn_select.hip, evaluation/select.py, cli/select.py) against the numpy specification.

On inputs whose dot products are exact in float32 in any order — lattice rows, unit rows of sixteen +-1/4, int8 bytes — the specification
has one value, and ``bn_select_run`` is held to ``run_reference`` bit for bit: picks, keys, the final ``m`` and ``nearest``, between guard
elements of a NaN pattern, with the inputs unchanged.  On real-valued float32 rows the traversal is compared teacher-forced, step by step,
against the float64 traversal under written-out bounds.  ``select_index`` and the CLI are run end to end."""

import csv
import functools

import numpy as np
import pytest

import select_cases as cases
from birdnet_stm32.evaluation import select as S

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF
GUARD = 4


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; there is no CPU fallback to fall back to")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


def _guarded(torch, values):
    """``values`` (float32 or int32) between guard elements of the fill pattern: (the whole buffer as int32, the view of the values)."""
    v = np.ascontiguousarray(values)
    flat = torch.full((v.size + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    flat[GUARD:GUARD + v.size] = torch.from_numpy(v.view(np.int32)).cuda()
    return flat, flat[GUARD:GUARD + v.size]


def _guards_intact(flat):
    b = flat.cpu().numpy()
    return np.all(b[:GUARD] == NAN_BITS) and np.all(b[-GUARD:] == NAN_BITS)


class Device:
    """The rows of a case on the device with their inverse norms; ``run`` is ``bn_select_run`` through the C ABI over a state on the host."""

    def __init__(self, torch, ctx, X, zp=0, weights=None, off=False):
        from birdnet_stm32 import _hip

        self.torch, self.ctx, self.hip, self.X, self.zp = torch, ctx, _hip, X, zp
        self.n, self.D = X.shape
        self.code = _hip.DTYPE_I8 if X.dtype == np.int8 else _hip.DTYPE_F32
        d = torch.from_numpy(np.ascontiguousarray(X)).cuda()
        if off:   # the same rows from element 1 of a flat buffer: +4 bytes for float32, +1 byte for int8
            flat = torch.empty(X.size + 1, dtype=d.dtype, device="cuda")
            flat[1:] = d.view(-1)
            d = flat[1:].view(X.shape)
            assert d.data_ptr() % 16 == X.itemsize
        self.d_rows = d
        self.d_inv = torch.empty(self.n, dtype=torch.float32, device="cuda")
        _hip.check(ctx.lib.bn_search_inv_norms(ctx.handle, d.data_ptr(), self.code, self.n, self.D, zp, self.d_inv.data_ptr(), None))
        self.weights = weights
        self.d_w = None if weights is None else torch.from_numpy(weights).cuda()
        self.inv = self.d_inv.cpu().numpy()

    def run(self, m, nearest, picked, forced, steps, expect=0):
        """``(picked, key, m, nearest, rc)`` after the call; the guards and the inputs are checked here.  ``key`` starts as the fill
        pattern, so an entry the call left alone still holds it."""
        torch = self.torch
        f_m, d_m = _guarded(torch, np.asarray(m, np.float32))
        f_n, d_n = _guarded(torch, np.asarray(nearest, np.int32))
        start = np.full(max(steps, 1), -1, np.int32)
        start[:forced] = np.asarray(picked, np.int32)[:forced]
        f_p, d_p = _guarded(torch, start)
        f_k, d_k = _guarded(torch, np.full(max(steps, 1), NAN_BITS, np.int32))
        rc = self.ctx.lib.bn_select_run(self.ctx.handle, self.d_rows.data_ptr(), self.code, self.n, self.D, self.zp, self.d_inv.data_ptr(),
                                        None if self.d_w is None else self.d_w.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), d_p.data_ptr(), forced, steps,
                                        d_k.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == expect, (rc, self.ctx.lib.bn_last_error())
        assert all(_guards_intact(f) for f in (f_m, f_n, f_p, f_k)), "a guard element was written"
        assert np.array_equal(self.d_rows.cpu().numpy(), self.X) and np.array_equal(self.d_inv.cpu().numpy().view(np.uint32), self.inv.view(np.uint32)), "an input changed"
        if self.d_w is not None:
            assert np.array_equal(self.d_w.cpu().numpy().view(np.uint32), self.weights.view(np.uint32)), "the weights changed"
        return (d_p.cpu().numpy()[:steps].copy(), d_k.cpu().numpy()[:steps].view(np.float32).copy(), d_m.cpu().numpy().view(np.float32).copy(),
                d_n.cpu().numpy().copy(), rc)


def _fresh(n):
    return np.full(n, -np.inf, np.float32), np.full(n, -1, np.int32)


def _same(got, want, forced, what):
    gp, gk, gm, gn = got[:4]
    wp, wk, wm, wn = want
    assert np.array_equal(gp, wp), f"{what}: picks differ: {gp.tolist()} / {wp.tolist()}"
    assert np.array_equal(gk[forced:].view(np.uint32), wk[forced:].view(np.uint32)), f"{what}: keys differ"
    assert np.all(gk[:forced].view(np.uint32) == NAN_BITS), f"{what}: the key of a forced entry was written"
    assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), f"{what}: m differs on {int((gm.view(np.uint32) != wm.view(np.uint32)).sum())} rows"
    assert np.array_equal(gn, wn), f"{what}: nearest differs"


def _reference(dev, forced_rows, steps):
    m, nearest = _fresh(dev.n)
    inv = S.inv_norms_reference(dev.X, dev.zp)
    assert np.array_equal(inv.view(np.uint32), dev.inv.view(np.uint32)), "the device's inverse norms are the specification's on these inputs"
    picked, key = S.run_reference(dev.X, inv, m, nearest, forced_rows, len(forced_rows), steps, dev.weights, dev.zp)
    return picked, key, m, nearest


def _check(torch, ctx, X, zp=0, weights=None, forced_rows=(), budget=64, off=False, what=""):
    dev = Device(torch, ctx, X, zp, weights, off)
    live = int((dev.inv != 0).sum())
    steps = len(forced_rows) + min(budget, live)
    want = _reference(dev, list(forced_rows), steps)
    m, nearest = _fresh(dev.n)
    got = dev.run(m, nearest, list(forced_rows), len(forced_rows), steps)
    _same(got, want, len(forced_rows), what)
    picks = got[0][len(forced_rows):]
    taken = picks[picks >= 0]
    assert np.unique(taken).size == taken.size and np.all(dev.inv[taken] != 0), f"{what}: picks are distinct live rows"
    keys = got[1][len(forced_rows):]
    assert np.all(keys[1:] <= keys[:-1]), f"{what}: the key sequence never increases"
    return dev, got


def _min_steps_n():
    from birdnet_stm32 import _hip

    assert _hip.SELECT_STEP_ROWS == 64
    return 64 * _hip.SELECT_MIN_WG_STEPS + 1


LATTICE_SHAPES = [(2, 8), (15, 1), (17, 96), (64, 255), (65, 256), ("min", 8), (1000, 96), (4099, 256), (1000, 255), (65, 1)]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("seeded", [False, True], ids=["unseeded", "seeded"])
@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=lambda s: "N{}-D{}".format(*s))
def test_lattice_runs_equal_the_specification_bit_for_bit(torch_mod, ctx, shape, seeded, weighted):
    """Lattice rows with duplicated rows and zero rows; with seeds the forced prefix holds a zero row, an entry out of range and a row
    twice, which are skipped or harmless; the weights hold zeros."""
    N, D = shape
    N = _min_steps_n() if N == "min" else N
    X = cases.lattice_rows(N, D, 11 + N + D)
    w = cases.weights(N, 5 + N) if weighted else None
    forced = [N - 1, N // 2 if N >= 15 else -3, N + 7, 0, N - 1] if seeded else [0]
    _check(torch_mod, ctx, X, 0, w, forced, 64, what=f"{N}x{D}")


@pytest.mark.parametrize("zp", [-128, 0, 3, 127])
@pytest.mark.parametrize("shape", [(17, 8), (65, 96), (1000, 255), (4099, 256), (2, 1), (64, 256)], ids=lambda s: "N{}-D{}".format(*s))
def test_int8_runs_equal_the_specification_bit_for_bit(torch_mod, ctx, shape, zp):
    N, D = shape
    X = cases.lattice_rows(N, D, 1000 + N + D + zp, int8_zp=zp)
    w = cases.weights(N, 9 + N) if (N + zp) % 2 else None
    _check(torch_mod, ctx, X, zp, w, [N // 3], 48, what=f"int8 {N}x{D} zp {zp}")


@pytest.mark.parametrize("N,D", [(1000, 96), (257, 255), (64, 17)])
def test_unit_rows_equal_the_specification_bit_for_bit(torch_mod, ctx, N, D):
    """Sixteen +-1/4 per row: many equal scores and equal keys, so the order among ties decides most picks."""
    _check(torch_mod, ctx, cases.unit_rows(N, D, 3 + N), 0, None, [], 64, what=f"unit {N}x{D}")


@pytest.mark.parametrize("case", ["f32-255", "f32-96", "i8-96", "i8-255"])
def test_rows_off_the_16_byte_boundary(torch_mod, ctx, case):
    """The rows start one element behind a 16-byte boundary: every load takes the streamer's slow path."""
    kind, D = case.split("-")
    X = cases.lattice_rows(130, int(D), 77, int8_zp=None if kind == "f32" else 3)
    _check(torch_mod, ctx, X, 0 if kind == "f32" else 3, cases.weights(130, 1), [5], 40, off=True, what=case)


def test_more_rows_than_the_workgroup_cap_deals_two_steps_to(torch_mod, ctx):
    """N above MAX_WGS * MIN_WG_STEPS * 64 at D = 8: the cap on the workgroups holds and every one streams more than the minimum."""
    from birdnet_stm32 import _hip

    N = _hip.SELECT_MAX_WGS * _hip.SELECT_MIN_WG_STEPS * _hip.SELECT_STEP_ROWS + 1
    X = cases.lattice_rows(N, 8, 4)
    dev, got = _check(torch_mod, ctx, X, 0, None, [], 3, what="cap")
    assert got[0].size == 3


def test_exhausting_the_rows_then_nothing_changes(torch_mod, ctx):
    X = cases.lattice_rows(17, 8, 21)
    dev = Device(torch_mod, ctx, X)
    live = int((dev.inv != 0).sum())
    assert live == 15
    want = _reference(dev, [], live + 4)
    got = dev.run(*_fresh(17), [], 0, live + 4)
    _same(got, want, 0, "exhaust")
    assert sorted(got[0][:live].tolist()) == np.flatnonzero(dev.inv != 0).tolist()
    assert np.all(got[0][live:] == -1) and np.all(got[1][live:] == -np.inf)
    again = dev.run(got[2], got[3], [], 0, 3)
    assert np.all(again[0] == -1) and np.all(again[1] == -np.inf)
    assert np.array_equal(again[2].view(np.uint32), got[2].view(np.uint32)) and np.array_equal(again[3], got[3]), "the state is untouched"


@pytest.mark.parametrize("kind", ["f32", "i8"])
def test_ten_steps_equal_four_then_six_and_two_runs_give_the_same_bits(torch_mod, ctx, kind):
    X = cases.lattice_rows(1000, 96, 8, int8_zp=None if kind == "f32" else -5)
    dev = Device(torch_mod, ctx, X, 0 if kind == "f32" else -5, cases.weights(1000, 2))
    whole = dev.run(*_fresh(1000), [7], 1, 10)
    twice = dev.run(*_fresh(1000), [7], 1, 10)
    for a, b in zip(whole[:4], twice[:4]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two runs differ"
    head = dev.run(*_fresh(1000), [7], 1, 4)
    tail = dev.run(head[2], head[3], [], 0, 6)
    assert np.array_equal(np.concatenate([head[0], tail[0]]), whole[0])
    assert np.array_equal(np.concatenate([head[1][1:], tail[1]]).view(np.uint32), whole[1][1:].view(np.uint32))
    assert np.array_equal(tail[2].view(np.uint32), whole[2].view(np.uint32)) and np.array_equal(tail[3], whole[3])
    _same(whole, _reference(dev, [7], 10), 1, "ten steps")


def test_refused_calls_write_nothing(torch_mod, ctx):
    from birdnet_stm32 import _hip

    X = cases.lattice_rows(65, 8, 1)
    dev = Device(torch_mod, ctx, X)
    m, nearest = _fresh(65)
    lib, h = ctx.lib, ctx.handle
    f_m, d_m = _guarded(torch_mod, m)
    f_n, d_n = _guarded(torch_mod, nearest)
    f_p, d_p = _guarded(torch_mod, np.full(4, 3, np.int32))
    f_k, d_k = _guarded(torch_mod, np.full(4, NAN_BITS, np.int32))
    before = [f.cpu().numpy().copy() for f in (f_m, f_n, f_p, f_k)]
    good = dict(rows=dev.d_rows.data_ptr(), code=dev.code, n=65, D=8, zp=0, inv=dev.d_inv.data_ptr(), w=None, m=d_m.data_ptr(), near=d_n.data_ptr(),
                picked=d_p.data_ptr(), forced=1, steps=4, key=d_k.data_ptr())
    bad = [dict(code=7), dict(n=-1), dict(n=1 << 31), dict(D=0), dict(D=2049), dict(forced=-1), dict(forced=5), dict(steps=-1), dict(rows=None),
           dict(inv=None), dict(m=None), dict(near=None), dict(picked=None), dict(key=None), dict(rows=dev.d_rows.data_ptr() + 2),
           dict(m=d_m.data_ptr() + 2), dict(inv=dev.d_inv.data_ptr() + 1), dict(w=dev.d_inv.data_ptr() + 2), dict(code=_hip.DTYPE_I8, zp=128)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.bn_select_run(h, a["rows"], a["code"], a["n"], a["D"], a["zp"], a["inv"], a["w"], a["m"], a["near"], a["picked"], a["forced"], a["steps"],
                               a["key"], None)
        assert rc != 0, f"{change} was accepted"
        torch_mod.cuda.synchronize()
        for f, b in zip((f_m, f_n, f_p, f_k), before):
            assert np.array_equal(f.cpu().numpy(), b), f"{change}: a refused call wrote"
    with pytest.raises(Exception):
        _hip.check(lib.bn_select_run(h, None, 0, 65, 8, 0, None, None, None, None, None, 0, 1, None, None))


def test_library_names_the_selection_kernel(ctx):
    names = ctx.lib.bn_kernel_names().decode().split("\n")
    assert "select_pass_kernel" in names


# ---------------------------------------------------------------------------------------------------------------------- bounded
BOUNDED = [(1000, 96, 8, 0.3, 42), (4099, 256, 16, 0.3, 5), (4099, 255, 12, 0.5, 42), (1000, 8, 4, 0.2, 42), (4099, 256, 16, 1.0, 42)]


@functools.lru_cache(maxsize=None)
def _trajectory(params, weighted):
    N, D, K, spread, seed = params
    X = cases.normal_clusters(N, D, K, spread, seed)
    w = np.random.default_rng(seed + 1).random(N).astype(np.float32) if weighted else None
    return X, w, cases.forced_trajectory(X, np.ones(N) if w is None else w.astype(np.float64), 64)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("params", BOUNDED, ids=lambda p: "N{}-D{}-K{}-s{}-seed{}".format(*p))
def test_teacher_forced_traversal_within_the_bounds(torch_mod, ctx, params, weighted):
    """Normal clusters, 64 steps of the float64 traversal from row 0.  At every step the device gets the reference's state rounded to
    float32 and picks once (forced = 0, steps = 1).  Its pick must lie among the rows whose float64 key plus bound reaches the best row's
    key minus bound (``select_cases.key_bound`` over ``select_cases.score_bound``), and must be the reference's where that leaves one row;
    its new ``m`` must lie within the score bound of the float64 state after taking the device's own pick.

    Clean shares of the 64 steps, computed on the CPU with this bound, plain / weighted, in the order of the parameters:
    93.8 % / 95.3 %, 87.5 % / 90.6 %, 92.2 % / 92.2 %, 98.4 % / 98.4 %, 98.4 % / 98.4 %.  The condition is 80 %."""
    X, w, steps = _trajectory(params, weighted)
    share = float(np.mean([s["clean"] for s in steps]))
    print(f"{params} weighted={weighted}: clean share {share:.4f}")
    assert share >= 0.80, "change the input, not the condition"
    dev = Device(torch_mod, ctx, X, 0, w)
    for t, s in enumerate(steps):
        picked, key, m, nearest, _ = dev.run(s["m32"], s["nearest"], [], 0, 1)
        c = int(picked[0])
        assert c in s["may"], f"step {t}: the device picked row {c}, which the bounds rule out"
        if s["clean"]:
            assert c == s["pick"], f"step {t}: a clean step, the device picked {c}, the reference {s['pick']}"
        S64, B = cases.score_bound(X, c)
        old = s["m64"]
        want = np.where(old == np.inf, np.inf, np.maximum(old, S64))
        want[c] = np.inf
        bound = np.maximum(cases.U * np.abs(np.where(np.isfinite(old), old, 0.0)), B)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(m), fin) and np.all(m[~fin] == np.inf)
        err = np.abs(m[fin].astype(np.float64) - want[fin])
        assert np.all(err <= bound[fin]), f"step {t}: largest error of m / bound {float((err / bound[fin]).max()):.3f}"
        assert nearest[c] == c


# ------------------------------------------------------------------------------------------------------------------- end to end
def _index(x, **kw):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = x.shape[0]
    return EmbeddingIndex(x, np.arange(n) // 7, (np.arange(n) % 7) * 3.0, [f"rec_{i}.wav" for i in range(n // 7 + 1)], **kw)


def _same_result(got, want):
    assert np.array_equal(got.picked, want.picked), (got.picked.tolist(), want.picked.tolist())
    assert np.array_equal(got.key.view(np.uint32), want.key.view(np.uint32))
    assert np.array_equal(got.nearest, want.nearest)
    assert np.array_equal(got.similarity.view(np.uint32), want.similarity.view(np.uint32))
    assert np.array_equal(got.seeds, want.seeds) and got.first == want.first and np.array_equal(got.nonzero, want.nonzero)


@pytest.mark.parametrize("kind", ["lattice", "int8"])
@pytest.mark.parametrize("start", ["seeds", "first"])
def test_select_index_equals_the_reference(torch_mod, ctx, kind, start):
    zp = 0 if kind == "lattice" else 5
    X = cases.lattice_rows(300, 96, 17, int8_zp=None if kind == "lattice" else zp)
    index = _index(X) if kind == "lattice" else _index(X, dtype="int8", scale=0.02, zero_point=zp)
    w = cases.weights(300, 6)
    kw = dict(seeds=[4, 150, 299, 17], weights=w) if start == "seeds" else dict(first=33)
    got = S.select_index(index, 40, min_key=-np.inf, ctx=ctx, **kw)
    want = S.select_reference(X, 40, min_key=-np.inf, zero_point=zp, **kw)
    _same_result(got, want)
    assert got.picked.size == 40 and np.isnan(got.similarity[150]) and got.nearest[150] == -1
    cut = S.select_index(index, 40, min_key=float(got.key[19]), ctx=ctx, **kw)
    _same_result(cut, S.select_reference(X, 40, min_key=float(got.key[19]), zero_point=zp, **kw))
    assert 1 <= cut.picked.size <= 40 and np.array_equal(cut.picked, got.picked[:cut.picked.size])


def test_select_index_computes_the_most_central_first(torch_mod, ctx):
    """Lattice rows, fewer than one segment of the update (256), so the sum of the normalised rows is added in the reference's order.  The
    most central row must be clear of the runner-up by more than the score bound of both, checked before the device is asked."""
    X = cases.lattice_rows(200, 96, 23)
    X[20] = 0.5   # (a lattice row in the middle of the others)
    live = np.flatnonzero(np.abs(X).sum(axis=1) > 0)
    X64 = X[live].astype(np.float64)
    T = X64 / np.sqrt((X64 * X64).sum(axis=1))[:, None]
    cosine = T @ (T.sum(axis=0) / np.linalg.norm(T.sum(axis=0)))
    order = np.argsort(-cosine)
    assert cosine[order[0]] - cosine[order[1]] > 4 * (96 + 10) * cases.U, "change the input: the most central row is not clear of the next"
    got = S.select_index(_index(X), 12, ctx=ctx)
    want = S.select_reference(X, 12)
    assert got.first == int(live[order[0]]) == want.first and got.picked[0] == got.first and got.key[0] == np.inf
    _same_result(got, want)


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cli_end_to_end(torch_mod, tmp_path, capsys):
    import birdnet_stm32.cli.select as cli

    X = cases.lattice_rows(120, 32, 31)
    db, out, cov, labels_csv, scores = (str(tmp_path / name) for name in ("db.npz", "select.csv", "cov.csv", "labels.csv", "f.npz"))
    file_index, start_s, paths = cases.synthetic_archive(db, X)
    rng = np.random.default_rng(0)
    F = rng.random((120, 3)).astype(np.float32)
    F[7] = 0
    F[60] = np.nan   # (row 60 is a zero row)
    names = ["alpha", "beta", "gamma"]
    with open(scores, "wb") as f:
        np.savez(f, F=F, labels=np.asarray(names), file_index=file_index, start_s=start_s, paths=np.asarray(paths))
    with open(labels_csv, "w") as f:
        f.write("path,start_s,label\nrec/file_0.wav,3.0,alpha\nrec/file_2.wav,0.0,beta\n")
    res = cli.main(["--database", db, "--budget", "10", "--output", out, "--labels", labels_csv, "--scores", scores, "--uncertainty", "entropy",
                    "--coverage_out", cov, "--min_key=-inf"])
    assert "Chose 10 of 120 rows" in capsys.readouterr().out
    w = S.uncertainty_reference(F, "entropy")
    seeds = [1, 60]   # file 0 holds rows 0..29, file 2 rows 60..89: row 60 is a zero row and is ignored
    want = S.select_reference(X, 10, seeds=seeds, weights=w, min_key=-np.inf)
    _same_result(res, want)
    assert want.seeds.tolist() == [1]
    rows = _read(out)
    assert tuple(rows[0]) == cli.CSV_COLUMNS and len(rows) == 11
    taken = np.zeros(120, int)
    taken[want.picked], taken[want.seeds] = 1, 2
    for rank, (line, row, key) in enumerate(zip(rows[1:], want.picked.tolist(), want.key.tolist())):
        covers = int(((want.nearest == row) & (taken == 0)).sum())
        guess = names[int(np.argmax(F[row]))]
        assert line == [str(rank), str(row), paths[file_index[row]], f"{start_s[row]:.3f}", f"{key:.7g}", f"{float(w[row]):.7g}", guess, str(covers)]
    lines = _read(cov)
    assert tuple(lines[0]) == cli.COVERAGE_COLUMNS and len(lines) == 121
    for i, line in enumerate(lines[1:]):
        sim = want.similarity[i]
        assert line == [str(i), paths[file_index[i]], f"{start_s[i]:.3f}", "" if want.nearest[i] < 0 else str(int(want.nearest[i])),
                        "" if np.isnan(sim) else f"{float(sim):.7g}", str(taken[i])]
    assert lines[61][3:] == ["", "", "0"] and lines[2][5] == "2"
    with pytest.raises(SystemExit):
        with open(scores, "wb") as f:
            np.savez(f, F=F[:100], labels=np.asarray(names), file_index=file_index[:100], start_s=start_s[:100], paths=np.asarray(paths))
        cli.main(["--database", db, "--budget", "10", "--output", out, "--scores", scores])
