"""Independent model of the fp8 path's numerics, in numpy only (no torch float8 casts): the OCP
e4m3fn / e5m2 decode table, the quantizers' encode rule, the bracket a producer's byte must fall in
when it rounds an fp32 value once to fp8 and once to bf16, and the delayed-scaling update.

Every rounding step runs in float64, where it is exact: a float32 divided by a power of two, rounded
to an integer (half to even) and multiplied back loses nothing. tests/test_fp8_reference_cpu.py pins
this module against torch's CPU float8 casts; tests/test_gpu_fp8_edges.py holds the kernels to it.

Encode rule of the kernels (csrc/common.h pack2_fp8), spelled out:
  * round to nearest even on the format's grid (subnormal spacing 2^-9 for e4m3, 2^-16 for e5m2);
  * finite overflow and +-Inf saturate to +-max (0x7E / 0x7B plus the sign bit);
  * NaN gives a NaN code (its sign is not defined);
  * the sign of zero is kept.
"""
import numpy as np

E4M3, E5M2 = 0, 1
MBITS = {E4M3: 3, E5M2: 2}
BIAS = {E4M3: 7, E5M2: 15}
FMAX = {E4M3: 448.0, E5M2: 57344.0}
MAX_CODE = {E4M3: 0x7E, E5M2: 0x7B}
NAN_CODE = {E4M3: 0x7F, E5M2: 0x7F}
FLT_MAX = np.float32(3.4028234663852886e38)


def decode_table(fmt: int) -> np.ndarray:
    """The 256 values of a format as float64 (NaN / Inf where the format has them)."""
    mb, bias = MBITS[fmt], BIAS[fmt]
    out = np.empty(256, dtype=np.float64)
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e = (code & 0x7F) >> mb
        m = code & ((1 << mb) - 1)
        if fmt == E4M3 and (code & 0x7F) == 0x7F:
            v = np.nan
        elif fmt == E5M2 and e == 31:
            v = np.inf if m == 0 else np.nan
        elif e == 0:
            v = m * 2.0 ** (1 - bias - mb)
        else:
            v = (1.0 + m / float(1 << mb)) * 2.0 ** (e - bias)
        out[code] = sign * v
    return out


def encode_mag(a: np.ndarray, fmt: int) -> np.ndarray:
    """Magnitude code (0 .. MAX_CODE) of non-negative float64 values, +Inf included; no NaN."""
    mb, bias = MBITS[fmt], BIAS[fmt]
    emin = 1 - bias  # exponent of the smallest normal; subnormals share its spacing
    a = np.minimum(np.asarray(a, dtype=np.float64), FMAX[fmt])  # saturate (Inf too)
    _, ex = np.frexp(a)  # a = f * 2^ex, f in [0.5, 1): floor(log2 a) = ex - 1
    e = np.maximum(ex - 1, emin)
    k = np.rint(np.ldexp(a, -(e - mb)))  # integer multiples of the spacing 2^(e - mb), half to even
    # k in [0, 2^(mb+1)]: k == 2^(mb+1) is the next binade's first value; below 2^mb only for subnormals
    up = k >= (1 << (mb + 1))
    e = np.where(up, e + 1, e)
    k = np.where(up, 1 << mb, k)
    sub = k < (1 << mb)
    code = np.where(sub, k, ((e + bias).astype(np.int64) << mb) + (k.astype(np.int64) - (1 << mb)))
    return code.astype(np.int64)


def encode(v32: np.ndarray, fmt: int) -> np.ndarray:
    """float32 array -> fp8 bytes (uint8) by the kernels' rule."""
    v32 = np.asarray(v32, dtype=np.float32)
    nan = np.isnan(v32)
    a = np.abs(np.where(nan, np.float32(0), v32)).astype(np.float64)
    code = encode_mag(a, fmt)
    code = np.where(nan, NAN_CODE[fmt], code)
    sign = np.signbit(v32) & ~nan
    return (code | np.where(sign, 0x80, 0)).astype(np.uint8)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(v32: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even bf16 bit patterns of finite float32 values."""
    u = np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def quant_reference(x_bf16_bits: np.ndarray, qs: float, fmt: int) -> np.ndarray:
    """The stand-alone quantizers: the float32 product x * qs, rounded once to float32, then encode."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        prod = bf16_to_f32(x_bf16_bits) * np.float32(qs)
    return encode(prod, fmt)


def is_nan_code(b: np.ndarray, fmt: int) -> np.ndarray:
    m = np.asarray(b).astype(np.int64) & 0x7F
    return m == 0x7F if fmt == E4M3 else m > 0x7C


def bracket(y_bf16_bits: np.ndarray, qs: float, fmt: int):
    """(lo, hi) magnitude codes that bound the byte of a producer which rounds an fp32 value v once to
    fp8 (v * qs in float32) and once to the bf16 output y (finite).

    v lies within half a bf16 ulp of y: with |y| in [2^e, 2^(e+1)) the ulp is 2^(e-7) (2^-133 for
    bf16 subnormals), and a v below a power of two sits in the finer binade, which the same h covers.
    The float32 product adds at most 2^-24 relative; the ends are widened by 2^-20. encode is monotone
    in the magnitude, so the byte's magnitude code lies in [encode((|y| - h) qs), encode((|y| + h) qs)]
    and its sign is y's (for y == 0 either sign: v may be a tiny value of either sign). Where the lower
    end already saturates, lo == hi == MAX_CODE: the only allowed byte is +-max."""
    y = np.abs(bf16_to_f32(y_bf16_bits)).astype(np.float64)
    _, ex = np.frexp(y)
    e = np.where(y == 0, -126, np.maximum(ex - 1, -126))  # frexp(0) reports exponent 0
    h = np.ldexp(1.0, e - 8)  # half of 2^(e-7)
    q = float(np.float32(qs))
    lo = np.maximum(y - h, 0.0) * q * (1.0 - 2.0 ** -20)
    hi = (y + h) * q * (1.0 + 2.0 ** -20)
    return encode_mag(lo, fmt), encode_mag(hi, fmt)


def bracket_distance(q: np.ndarray, y_bf16_bits: np.ndarray, qs: float, fmt: int) -> np.ndarray:
    """Per element: how many codes the byte lies outside its bracket (0 inside). A NaN / Inf code or a
    wrong sign (y != 0) counts as 256."""
    lo, hi = bracket(y_bf16_bits, qs, fmt)
    q = np.asarray(q).astype(np.int64)
    mag = q & 0x7F
    d = np.maximum(lo - mag, 0) + np.maximum(mag - hi, 0)
    ybits = np.asarray(y_bf16_bits).astype(np.int64)
    wrong_sign = ((ybits & 0x7FFF) != 0) & ((q >> 7) != (ybits >> 15))
    return np.where((mag > MAX_CODE[fmt]) | wrong_sign, 256, d)


class ScaleModel:
    """fp8_scale_update in float32 numpy, step by step as ops/fp8.py's docstring defines it.

    A finite amax is pushed into the slot's history ring, a non-finite one is dropped (history and
    scales unchanged); either way the amax word of every slot in [s0, s1) becomes 0. With the window
    maximum m: qscale = fmax / m * 2^-margin for m > 0, else 1, clamped to the largest finite float
    when it overflows, and dscale = 1 / qscale. Slots outside [s0, s1) are untouched."""

    def __init__(self, n: int, history: int, margin: int, fmax):
        self.n, self.H = n, history
        self.hist = np.zeros((n, history), dtype=np.float32)
        self.amax = np.zeros(n, dtype=np.uint32)  # float32 bits, as on the device
        self.qscale = np.ones(n, dtype=np.float32)
        self.dscale = np.ones(n, dtype=np.float32)
        self.fmax = np.broadcast_to(np.asarray(fmax, dtype=np.float32), (n,)).copy()
        self.margin_mul = np.float32(2.0 ** -margin)

    def update(self, s0: int, s1: int) -> None:
        for i in range(s0, min(s1, self.n)):
            cur = self.amax[i:i + 1].view(np.float32)[0]
            self.amax[i] = 0
            if not np.isfinite(cur):
                continue
            self.hist[i, 1:] = self.hist[i, :-1].copy()
            self.hist[i, 0] = cur
            m = self.hist[i].max()
            q = np.float32(1.0)
            if m > 0:
                with np.errstate(over="ignore"):
                    q = np.float32(np.float32(self.fmax[i] / m) * self.margin_mul)
                if not np.isfinite(q):
                    q = FLT_MAX
            self.qscale[i] = q
            self.dscale[i] = np.float32(1.0) / q


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 ulps between positive finite float32 arrays (their bit patterns order
    like integers)."""
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


SCALES = (1.0, 7.0, 2.0 ** -10, 3e-5, 1e4, 2.0 ** 20, 448 / 0.37, 1e38)


def finite_bf16_patterns() -> np.ndarray:
    """All 65280 finite bf16 bit patterns (exponent field below 0xFF), both signs."""
    b = np.arange(65536, dtype=np.uint32)
    return b[(b & 0x7F80) != 0x7F80].astype(np.uint16)
