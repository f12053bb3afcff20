"""The packed shift-and-saturate instruction the INT8 epilogues stand on (``csrc/bn_requant.h``: ``sat_pack2`` / ``sat_pack2_hi``, i.e.
``v_ashr_pk_i8_i32`` and its high-half form), run on arrays through ``bn_debug_satpack`` and held to numpy's ``clip(a >> s, -128, 127)``:
arithmetic shift by the low five bits of ``s``, SIGNED saturation of each value to 8 bits, byte 0 from ``a`` and byte 1 from ``b``, the
low form's other half zero, the high form's low half kept.  Every kernel form that uses the instruction assumes exactly this."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 5, 7, 8, 21, 30, 31)
KS = (-130, -129, -128, -127, -126, -1, 0, 1, 125, 126, 127, 128, 129)
I32_MIN, I32_MAX = -(2**31), 2**31 - 1


def cases() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, s): around every saturation edge at every shift ((k << s) + d where it fits an int32), the two ends of the int32 range, and
    4096 seeded random values with random shifts; b runs through the same values in another order so that the two bytes differ."""
    a, s = [], []
    for sh in SHIFTS:
        for k in KS:
            for d in (-1, 0, 1):
                v = (k << sh) + d
                if I32_MIN <= v <= I32_MAX:
                    a.append(v)
                    s.append(sh)
        a += [I32_MIN, I32_MAX]
        s += [sh, sh]
    rng = np.random.default_rng(20)
    a = np.concatenate([np.asarray(a, np.int64), rng.integers(I32_MIN, I32_MAX, 4096, endpoint=True)])
    s = np.concatenate([np.asarray(s, np.int64), rng.integers(0, 32, 4096)])
    order = np.argsort(s, kind="stable")
    a, s = a[order], s[order]
    b = a.copy()
    for sh in np.unique(s):   # (a rotation inside each shift: the pair shares its shift, as in the kernels)
        sel = np.nonzero(s == sh)[0]
        b[sel] = np.roll(a[sel], 7)
    return a.astype(np.int32), b.astype(np.int32), s.astype(np.int32)


def expected_half(a, b, s) -> np.ndarray:
    sat = lambda v: np.clip(v.astype(np.int64) >> (s.astype(np.int64) & 31), -128, 127) & 0xFF   # noqa: E731
    return (sat(a) | (sat(b) << 8)).astype(np.uint32)


@pytest.mark.parametrize("garbage_high_bits", [False, True])
def test_shift_saturate_pack_low_and_high_half(garbage_high_bits):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    from birdnet_stm32 import _hip

    a, b, s = cases()
    want = expected_half(a, b, s)
    assert {0x7F, 0x80, 0x00, 0xFF, 0x7E, 0x81} <= set((want & 0xFF).tolist()), "the cases must reach both saturation ends and their neighbours"
    s_dev = s | np.int32(0x5A5A5A40 & ~31) if garbage_high_bits else s   # the packed-shifts word of the kernels: only bits 4:0 count
    ctx = _hip.Context(0, max_batch=1)
    da, db, ds = (torch.from_numpy(v).cuda() for v in (a, b, s_dev.astype(np.int32)))
    out = torch.empty(len(a), dtype=torch.int32, device="cuda")
    for mode, name in ((0, "low half"), (1, "high half")):
        out.fill_(-1)
        _hip.check(ctx.lib.bn_debug_satpack(ctx.handle, da.data_ptr(), db.data_ptr(), ds.data_ptr(), len(a), mode, out.data_ptr(), None))
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        exp = want if mode == 0 else (want << 16) | np.uint32(0xBEEF)   # low: the other half zero; high: 0x1234 replaced, 0xBEEF kept
        bad = np.nonzero(got != exp)[0]
        print(f"{name}, garbage above bit 4 of the shift {garbage_high_bits}: {len(bad)} of {len(a)} differ")
        assert len(bad) == 0, (f"{name}: {len(bad)} of {len(a)} differ, first a={a[bad[0]]} b={b[bad[0]]} s={s[bad[0]]}: "
                               f"got {got[bad[0]]:#010x}, want {exp[bad[0]]:#010x}")
    ctx.close()
