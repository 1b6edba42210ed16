"""tests/fp8_reference.py against torch's CPU float8 casts and a direct scale-update loop: the model
the GPU tests (tests/test_gpu_fp8_edges.py) hold the kernels to must itself be right. No GPU needed."""
import math
import struct

import numpy as np
import pytest
import torch

from tests import fp8_reference as R

FMTS = pytest.mark.parametrize("fmt", [R.E4M3, R.E5M2], ids=["e4m3", "e5m2"])
TDT = {R.E4M3: torch.float8_e4m3fn, R.E5M2: torch.float8_e5m2}


def _torch_encode(v32: np.ndarray, fmt: int) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(v32)).clamp(-R.FMAX[fmt], R.FMAX[fmt])
    return t.to(TDT[fmt]).view(torch.uint8).numpy()


@FMTS
def test_decode_table_is_torch_decode(fmt):
    ref = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(TDT[fmt]).to(torch.float64).numpy()
    got = R.decode_table(fmt)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok], ref[ok])
    assert np.array_equal(np.signbit(got[ok]), np.signbit(ref[ok]))
    assert got[R.MAX_CODE[fmt]] == R.FMAX[fmt] and got[R.MAX_CODE[fmt] | 0x80] == -R.FMAX[fmt]
    assert np.array_equal(R.is_nan_code(np.arange(256), fmt), np.isnan(ref))


@FMTS
@pytest.mark.parametrize("qs", R.SCALES, ids=[f"{s:.4g}" for s in R.SCALES])
def test_encode_is_clamped_torch_cast(fmt, qs):
    """All 65280 finite bf16 patterns times the scale: every byte equals torch's cast of the clamped
    product. The set must reach both edges (saturated elements and zeros) at every scale."""
    x = R.bf16_to_f32(R.finite_bf16_patterns())
    with np.errstate(over="ignore"):
        prod = x * np.float32(qs)
    ref = _torch_encode(prod, fmt)
    got = R.encode(prod, fmt)
    assert int((got != ref).sum()) == 0
    assert np.array_equal(got, R.quant_reference(R.finite_bf16_patterns(), qs, fmt))
    sat = float(((got & 0x7F) == R.MAX_CODE[fmt]).mean())
    zeros = float(((got & 0x7F) == 0).mean())
    print(f"fmt{fmt} qs {qs:.4g}: saturated {sat:.4f} zero {zeros:.6f}")
    assert sat > 0 and zeros > 0


@FMTS
def test_encode_specials(fmt):
    v = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 3.4e38, -3.4e38, R.FMAX[fmt], -R.FMAX[fmt]], dtype=np.float32)
    got = R.encode(v, fmt)
    mx = R.MAX_CODE[fmt]
    assert R.is_nan_code(got[:2], fmt).all()
    assert np.isnan(R.decode_table(fmt)[got[:2]]).all()
    assert list(got[2:]) == [mx, mx | 0x80, 0x00, 0x80, mx, mx | 0x80, mx, mx | 0x80]
    # Inf and NaN inputs through the quantizer's product
    bits = np.array([0x7F80, 0xFF80, 0x7FC0, 0x0000, 0x8000], dtype=np.uint16)
    q = R.quant_reference(bits, 1e38, fmt)
    assert list(q[:2]) == [mx, mx | 0x80] and R.is_nan_code(q[2:3], fmt).all() and list(q[3:]) == [0x00, 0x80]


@FMTS
def test_encode_rounds_half_to_even_and_is_monotone(fmt):
    """Every midpoint between two adjacent codes goes to the even code, values a hair to either side go
    to their nearer neighbour, and the code is monotone in the magnitude."""
    tab = R.decode_table(fmt)
    mx = R.MAX_CODE[fmt]
    for c in range(mx):
        lo, hi = tab[c], tab[c + 1]
        mid = np.float32((lo + hi) / 2)  # exact: both have few mantissa bits
        assert float(mid) == (lo + hi) / 2
        even = c if c % 2 == 0 else c + 1
        below, above = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))
        assert list(R.encode(np.array([below, mid, above], dtype=np.float32), fmt)) == [c, even, c + 1]
    a = np.abs(np.random.default_rng(0).standard_normal(20000)).astype(np.float32) * np.float32(R.FMAX[fmt] / 2)
    a = np.sort(np.concatenate([a, a * np.float32(2.0 ** -12)]))
    assert (np.diff(R.encode(a, fmt).astype(np.int64)) >= 0).all()


@FMTS
@pytest.mark.parametrize("qs", [1.0, 37.5, 2.0 ** -10, 1e4, 448 / 0.37])
def test_bracket_contains_the_once_rounded_byte(fmt, qs):
    """Random fp32 v over many binades (subnormal bf16 results, exact powers of two and values just
    below them included) and y = bf16(v): encode(v * qs) lies inside bracket(y)."""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(200000) * np.exp2(rng.integers(-30, 12, 200000))).astype(np.float32)
    p2 = np.exp2(rng.integers(-20, 10, 2000)).astype(np.float32)
    v = np.concatenate([v, p2, np.nextafter(p2, np.float32(0)), -np.nextafter(p2, np.float32(np.inf)),
                        np.array([0.0, -0.0, 1e-40, -1e-40, 3e-39], dtype=np.float32)])
    y = R.f32_to_bf16_bits(v)
    assert torch.equal(torch.from_numpy(v).to(torch.bfloat16).view(torch.int16), torch.from_numpy(y.view(np.int16)))
    q = R.encode(v * np.float32(qs), fmt)
    d = R.bracket_distance(q, y, qs, fmt)
    assert int(d.max()) == 0, f"{int((d > 0).sum())} bytes outside their bracket, worst {int(d.max())}"
    lo, hi = R.bracket(y, qs, fmt)
    assert (lo <= hi).all() and int((hi - lo).max()) <= 2  # tight: bf16 carries 4-5 more bits than fp8
    # the bracket is not vacuous: a byte one code beyond either end is outside it
    assert (R.bracket_distance(np.minimum(hi + 1, 0x7F) | (y >> 15 << 7), y, qs, fmt)[hi < R.MAX_CODE[fmt]] > 0).all()
    sat = lo == R.MAX_CODE[fmt]
    if sat.any():
        assert ((q[sat] & 0x7F) == R.MAX_CODE[fmt]).all()


def _f32(x: float) -> float:
    try:
        return struct.unpack("f", struct.pack("f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _direct_scale_loop(seq, H, margin, fmax):
    """One slot, python floats rounded to float32 after every operation; returns per step
    (history oldest-last, qscale, dscale)."""
    hist, q, d, out = [0.0] * H, 1.0, 1.0, []
    for a in seq:
        if math.isfinite(a):
            hist = [a] + hist[:-1]
            m = max(hist)
            if m > 0:
                q = _f32(_f32(fmax / m) * 2.0 ** -margin)
                if math.isinf(q):
                    q = float(R.FLT_MAX)
            else:
                q = 1.0
            d = _f32(1.0 / q)
        out.append((list(hist), q, d))
    return out


AMAX_SEQ = [0.0, 9.183549615799121e-41, 0.5, 1e-37, 3.0, float("inf"), 2.0, float("nan"), 3e38, 0.0, 1.0, 1e-39, 0.25, 0.0, 0.0,
            0.0, 0.0, 0.125, 7.0, 0.0]


@FMTS
@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("H", [1, 2, 16])
def test_scale_model_against_direct_loop(fmt, H, margin):
    seq = [_f32(a) if math.isfinite(a) else a for a in AMAX_SEQ]
    want = _direct_scale_loop(seq, H, margin, R.FMAX[fmt])
    sm = R.ScaleModel(3, H, margin, R.FMAX[fmt])
    for a, (hist, q, d) in zip(seq, want):
        sm.amax[:] = np.array([a] * 3, dtype=np.float32).view(np.uint32)
        before = (sm.hist[0].copy(), sm.qscale[0], sm.dscale[0])
        sm.update(1, 3)
        # slot 0 is outside the range: untouched, amax word included
        assert np.array_equal(sm.hist[0], before[0]) and sm.qscale[0] == before[1] and sm.dscale[0] == before[2]
        assert sm.amax[0] == np.array([a], dtype=np.float32).view(np.uint32)[0] and sm.amax[1] == 0 and sm.amax[2] == 0
        for i in (1, 2):
            assert list(sm.hist[i].astype(np.float64)) == hist
            assert float(sm.qscale[i]) == q and float(sm.dscale[i]) == d
            assert np.isfinite(sm.qscale[i]) and sm.qscale[i] > 0 and np.isfinite(sm.dscale[i]) and sm.dscale[i] > 0


@FMTS
def test_scale_model_overflow_is_clamped(fmt):
    """A finite window maximum below fmax / FLT_MAX: the quotient overflows float32, qscale is the
    largest finite float, every element times it stays below fmax and zero stays zero."""
    m = np.float32(9.183549615799121e-41)  # the smallest bf16 subnormal
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(R.FMAX[fmt]) / m)
    sm = R.ScaleModel(1, 4, 0, R.FMAX[fmt])
    sm.amax[:] = np.array([m]).view(np.uint32)
    sm.update(0, 1)
    assert sm.qscale[0] == R.FLT_MAX and sm.dscale[0] > 0 and sm.hist[0, 0] == m
    bits = np.array([0x0000, 0x8000, 0x0001, 0x8001], dtype=np.uint16)
    q = R.quant_reference(bits, float(sm.qscale[0]), fmt)
    assert not R.is_nan_code(q, fmt).any() and list(q[:2]) == [0x00, 0x80]
    assert (np.abs(R.decode_table(fmt)[q]) < R.FMAX[fmt]).all()
