"""The numpy specifications behind the device bootstrap (birdnet_stm32/evaluation/bootstrap.py) against numpy's generator and
scikit-learn: the PCG64 32-bit stream with its jump-ahead, Lemire's bounding with its rejections, the raw ranges of consecutive
resamples, and the average precision of a resample given as multiplicities.  No GPU."""

import os
import re

import numpy as np
import pytest

from conftest import REPO

from birdnet_stm32.evaluation import bootstrap as bs


def _state_of(g):
    st = g.bit_generator.state
    assert st["bit_generator"] == "PCG64" and st["has_uint32"] == 0
    return int(st["state"]["state"]), int(st["state"]["inc"])


def _halves(raw64):
    out = np.empty(2 * raw64.size, np.uint32)
    out[0::2] = raw64 & np.uint64(0xFFFFFFFF)
    out[1::2] = raw64 >> np.uint64(32)
    return out


def test_raw32_stream_is_random_raw_split_low_half_first():
    g = np.random.default_rng(42)
    state, inc = _state_of(g)
    want = _halves(np.random.default_rng(42).bit_generator.random_raw(600))
    assert np.array_equal(bs.pcg64_raw32_reference(state, inc, 0, 1200), want)
    for start, count in ((1, 7), (3, 400), (777, 1), (1198, 2), (5, 0)):  # odd starts: the first value is a high half
        assert np.array_equal(bs.pcg64_raw32_reference(state, inc, start, count), want[start:start + count]), (start, count)
        assert np.array_equal(bs._raw32_fast(state, inc, start, count), want[start:start + count])
    # a start beyond 2^33: the generator's own jump-ahead is the yardstick
    start = (1 << 33) + 12345
    bg = np.random.default_rng(42).bit_generator
    bg.advance(start >> 1)
    far = _halves(bg.random_raw(40))
    assert np.array_equal(bs.pcg64_raw32_reference(state, inc, start, 64), far[1:65])
    # a state taken after other draws (64-bit ones: they leave no spare half)
    g = np.random.default_rng(7)
    g.random(1001)
    g.integers(0, 1 << 40, size=13)
    state, inc = _state_of(g)
    want = _halves(g.bit_generator.random_raw(50))
    assert np.array_equal(bs.pcg64_raw32_reference(state, inc, 0, 100), want)
    assert np.array_equal(bs.pcg64_raw32_reference(state, inc, 31, 9), want[31:40])
    assert bs.pcg64_advance(state, inc, 0) == state


@pytest.mark.parametrize("bound,count", [(1, 50), (2, 5000), (60, 5000), (4096, 5000), (4097, 20001), (24576, 20001), (3 << 30, 200000)])
def test_bounded_draws_equal_generator_integers(bound, count):
    state, inc = bs.generator_state(42)
    want = np.random.default_rng(42).integers(0, bound, size=count)
    got, used = bs.bounded_draws_reference(state, inc, bound, count)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    thr = bs.lemire_threshold(bound)
    assert thr == ((1 << 32) - bound) % bound and (thr == 0) == (bound in (1, 2, 4096))
    rejected = bs.rejected_positions_reference(state, inc, bound, 0, used)
    assert used == (0 if bound == 1 else count + rejected.size)
    if bound == 3 << 30:
        assert rejected.size == 66535 and rejected.size >= 1  # a third of the raw values: the rejection path is exercised
    # consecutive calls read one stream: the spare half carries over (odd counts), so the second call starts where the first ended
    g = np.random.default_rng(42)
    first = g.integers(0, bound, size=count)
    second = g.integers(0, bound, size=77)
    assert np.array_equal(first, want)
    got2, _ = bs.bounded_draws_reference(state, inc, bound, 77, start=used)
    assert np.array_equal(got2, second)


def test_rejections_occur_in_the_tested_streams():
    state, inc = bs.generator_state(42)
    assert bs.rejected_positions_reference(state, inc, 24576, 0, 3145728 + 14).size == 14
    got, used = bs.bounded_draws_reference(state, inc, 24576, 3145728)
    assert used == 3145728 + 14


@pytest.mark.parametrize("n,B,start_draws", [(4097, 9, 0), (12289, 5, 4097), (33, 40, 0)])
def test_resample_ranges_hold_each_resamples_draws(n, B, start_draws):
    """Bound 3 * 2^30 rejects a third of the raw values; the resample length n is odd, so resamples start on either half."""
    bound = 3 << 30
    state, inc = bs.generator_state(42)
    g = np.random.default_rng(42)
    g.integers(0, bound, size=start_draws)
    want = [g.integers(0, bound, size=n) for _ in range(B)]
    _, start = bs.bounded_draws_reference(state, inc, bound, start_draws)
    scanned = start + 2 * n * B
    rejected = bs.rejected_positions_reference(state, inc, bound, start, scanned)
    assert rejected.size > n * B // 4
    ranges = bs.resample_ranges(rejected[::-1], n, B, start)  # (any order: the device appends as it finds them)
    assert ranges.shape == (B, 2) and ranges[-1, 1] <= scanned and (ranges[1:, 0] >= ranges[:-1, 1]).all()
    thr = bs.lemire_threshold(bound)
    for b in range(B):
        p0, p1 = map(int, ranges[b])
        m = bs.pcg64_raw32_reference(state, inc, p0, p1 - p0).astype(np.uint64) * np.uint64(bound)
        ok = (m & np.uint64(0xFFFFFFFF)) >= np.uint64(thr)
        assert ok[0] and ok[-1] and np.array_equal((m[ok] >> np.uint64(32)).astype(np.int64), want[b]), b
    # without rejections the ranges tile the stream
    assert bs.resample_ranges([], 5, 3, 7).tolist() == [[7, 12], [12, 17], [17, 22]]


def _score_sets(rng, n):
    return {
        "lattice": (np.floor(rng.random(n) ** 3 * 256) / 256).astype(np.float32),
        "equal": np.full(n, 0.25, np.float32),
        "distinct": rng.permutation(n).astype(np.float32) / np.float32(n),
    }


@pytest.mark.parametrize("n", [3, 60, 257, 1000])
def test_ap_from_counts_equals_average_precision_of_the_resample(n):
    from sklearn.metrics import average_precision_score

    rng = np.random.default_rng(n)
    tol = bs.ap_tolerance(n)
    assert tol == 2 * n * 2.0 ** -53
    checked = dropped = 0
    for kind, s in _score_sets(rng, n).items():
        for pos in sorted({1, n // 3 + 1, n - 1}):
            t = np.zeros(n, np.uint8)
            t[rng.permutation(n)[:pos]] = 1
            order = np.argsort(-s, kind="stable")
            for _ in range(12):
                idx = rng.integers(0, n, size=n)
                counts = np.bincount(idx, minlength=n)
                got = bs.ap_from_counts_reference(counts[order], t[order], s[order])
                k = int(t[idx].sum())
                if k == 0 or k == n:
                    assert np.isnan(got), (kind, pos)
                    dropped += 1
                else:
                    want = average_precision_score(t[idx], s[idx])
                    assert abs(got - want) <= tol, (kind, pos, got, want)
                    checked += 1
    assert checked > 30 and (dropped > 0 or n > 3)


def test_abi_declares_the_bootstrap_entry_points():
    from birdnet_stm32 import _hip

    hdr = open(os.path.join(REPO, "include", "birdnet_hip.h")).read()
    for name in ("bn_bootstrap_rejections", "bn_bootstrap_counts", "bn_bootstrap_ap"):
        assert re.search(r"BN_API int " + name + r"\(", hdr) and name in _hip.EXPORTS
    assert int(re.search(r"#define BN_BOOTSTRAP_MAX_N (\d+)\n", hdr).group(1)) == bs.MAX_N == _hip.BOOTSTRAP_MAX_N >= 32768
    if os.path.isfile(_hip.LIB_PATH):
        names = _hip.load_library().bn_kernel_names().decode().split("\n")
        assert {"bootstrap_table_kernel", "bootstrap_reject_kernel", "bootstrap_prepare_kernel", "bootstrap_resample_kernel"} <= set(names)
