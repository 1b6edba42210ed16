"""The fp8 quantizers, the delayed-scaling update and the fp8-copy producers at the formats' edges,
against the independent numpy model of tests/fp8_reference.py (itself pinned to torch's CPU float8
casts by tests/test_fp8_reference_cpu.py).

(a) stand-alone quantizers: byte-exact (zero mismatches; a NaN must decode to NaN, its sign is free);
(b) fp8_scale_update against ScaleModel: copies exact, qscale / dscale within one ulp;
(c) producers whose input is already bf16 (column sums + copy): byte-exact, at three scales whose
    saturating share is set by construction (none, ~0.5 %: saturating and direct waves in one
    launch, ~30 %);
(d) producers that round an fp32 value once to fp8 and once to bf16: every byte inside the derived
    bracket of its bf16 output, at the same three settings.

Every test prints the figures it asserts on (lines starting with FP8EDGE)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fp8_reference as R  # noqa: E402

DEV = "cuda"
FMTS = pytest.mark.parametrize("fmt", [R.E4M3, R.E5M2], ids=["e4m3", "e5m2"])
SENTINEL = 0xA5
INF_WORD = 0x7F800000
QM_CHUNK = 256 * 16 * 4  # csrc/fp8.hip
# saturating share by construction: scale = fmax / (order statistic of |y|)
SETTINGS = (0.0, 0.005, 0.3)


def _ext():
    from pytorch_vit_paper_replication_amd import _ext as E

    return E.ext()


def _dev_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(DEV)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _word(am: torch.Tensor, i: int = 0) -> int:
    return int(am.cpu().numpy().view(np.uint32)[i])


def _f32(v) -> torch.Tensor:
    return torch.tensor([float(v)], dtype=torch.float32, device=DEV)


def _amax0(n: int = 1) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.int32, device=DEV)


def _guarded(rows: int, cols: int, guard: int = 64):
    flat = torch.full((rows * cols + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
    return flat, flat[:rows * cols].view(rows, cols)


_LUT = {}


def _lut(qs: float, fmt: int) -> np.ndarray:
    """quant_reference of all 65536 bf16 patterns at one scale: the reference bytes of any bf16 tensor
    are a table lookup (the quantizers read nothing but the element and the scale)."""
    key = (float(np.float32(qs)), fmt)
    if key not in _LUT:
        _LUT[key] = R.quant_reference(np.arange(65536, dtype=np.uint32).astype(np.uint16), key[0], fmt)
    return _LUT[key]


def _mismatches(got: np.ndarray, ref: np.ndarray, fmt: int) -> int:
    """Bytes that differ; where the reference is NaN the byte only has to decode to NaN."""
    rn, gn = R.is_nan_code(ref, fmt), R.is_nan_code(got, fmt)
    return int(((got != ref) & ~(rn & gn)).sum())


def _patterns(qs: float) -> np.ndarray:
    """The 65280 finite bf16 patterns; from 2^20 up the subnormal inputs are left out (replaced by a
    zero of their sign): their product depends on the denormal mode, which the project does not define."""
    bits = R.finite_bf16_patterns().copy()
    if qs >= 2.0 ** 20:
        sub = ((bits & 0x7F80) == 0) & ((bits & 0x007F) != 0)
        bits[sub] &= 0x8000
    return bits.reshape(4080, 16)


def _random_finite(shape, seed: int) -> np.ndarray:
    pat = R.finite_bf16_patterns()
    return pat[np.random.default_rng(seed).integers(0, pat.size, size=shape)]


def _exact_amax_word(bits: np.ndarray) -> int:
    return int((bits & 0x7FFF).max()) << 16


# ------------------------------------------------------------------------------------------------
# (a) stand-alone quantizers
@FMTS
@pytest.mark.parametrize("qs", R.SCALES, ids=[f"{s:.4g}" for s in R.SCALES])
def test_quant_all_finite_patterns(fmt, qs):
    bits = _patterns(qs)
    x = _dev_bf16(bits)
    flat, y = _guarded(4080, 16)
    am = _amax0()
    _ext().fp8_quant(x, y, _f32(qs), am, fmt)
    got, ref = y.cpu().numpy(), _lut(qs, fmt)[bits]
    bad = _mismatches(got, ref, fmt)
    zero_in = (bits & 0x7FFF) == 0
    sub_in = ((bits & 0x7F80) == 0) & ~zero_in
    print(f"FP8EDGE quant patterns fmt{fmt} qs {qs:.4g}: mismatches {bad} saturated {((got & 0x7F) == R.MAX_CODE[fmt]).mean():.4f} "
          f"zero bytes {((got & 0x7F) == 0).mean():.4f}")
    assert bad == 0
    assert (got[zero_in | sub_in] == (bits[zero_in | sub_in] >> 8 & 0x80)).all()  # +-0 with the sign kept
    assert _word(am) == 0x7F7F0000  # the largest finite bf16
    assert (flat[-64:] == SENTINEL).all().item()


@FMTS
def test_quant_inf_and_nan_element(fmt):
    bits = _patterns(7.0).copy()
    ref = _lut(7.0, fmt)[bits]
    for what, pattern in (("-inf", 0xFF80), ("+inf", 0x7F80), ("nan", 0x7FC0), ("-nan", 0xFFC1)):
        b = bits.copy()
        b[1234, 5] = pattern
        flat, y = _guarded(4080, 16)
        am = _amax0()
        _ext().fp8_quant(_dev_bf16(b), y, _f32(7.0), am, fmt)
        got = y.cpu().numpy()
        others = np.ones_like(got, dtype=bool)
        others[1234, 5] = False
        assert np.array_equal(got[others], ref[others]), what
        if "inf" in what:
            assert got[1234, 5] == (R.MAX_CODE[fmt] | (0x80 if what[0] == "-" else 0)), what
            assert _word(am) == INF_WORD, what
        else:
            assert R.is_nan_code(got[1234, 5], fmt) and np.isnan(R.decode_table(fmt)[got[1234, 5]]), what
            assert _word(am) > INF_WORD, what
        assert (flat[-64:] == SENTINEL).all().item()


@FMTS
def test_quant_strided_rows(fmt):
    bits = _random_finite((4080, 48), 3)
    big = _dev_bf16(bits)
    x = big[:, 16:32]  # ldx 48 > cols 16
    (f1, y1), (f2, y2) = _guarded(4080, 16), _guarded(4080, 16)
    a1, a2 = _amax0(), _amax0()
    _ext().fp8_quant(x, y1, _f32(7.0), a1, fmt)
    _ext().fp8_quant(x.contiguous(), y2, _f32(7.0), a2, fmt)
    assert torch.equal(y1, y2) and _word(a1) == _word(a2) == _exact_amax_word(bits[:, 16:32])
    assert _mismatches(y1.cpu().numpy(), _lut(7.0, fmt)[bits[:, 16:32]], fmt) == 0
    assert (f1[-64:] == SENTINEL).all().item() and (f2[-64:] == SENTINEL).all().item()


@pytest.mark.parametrize("rows,cols", [(1, 16), (1031, 2064), (4099, 2064)])
def test_quant_capped_grid(rows, cols):
    """512 blocks, 4 grid-stride steps per trip, loads clamped to the last group: one thread; a
    partial second step with steps 3 and 4 fully clamped; a second trip with a tail."""
    bits = _random_finite((rows, cols), rows)
    x = _dev_bf16(bits)
    for fmt in (R.E4M3, R.E5M2):
        flat, y = _guarded(rows, cols)
        am = _amax0()
        _ext().fp8_quant(x, y, _f32(7.0), am, fmt)
        assert _mismatches(y.cpu().numpy(), _lut(7.0, fmt)[bits], fmt) == 0
        assert _word(am) == _exact_amax_word(bits)
        assert (flat[-64:] == SENTINEL).all().item()
        am2 = _amax0()
        _ext().fp8_quant(x, None, None, am2, fmt)  # the calibration pass: amax only
        assert _word(am2) == _exact_amax_word(bits)


@FMTS
@pytest.mark.parametrize("dscale", [None, 0.37])
def test_dequant_all_codes(fmt, dscale):
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(DEV)
    got = _ext().fp8_dequant(codes, None if dscale is None else _f32(dscale), fmt).cpu().numpy()
    tab = R.decode_table(fmt).astype(np.float32)  # every fp8 value is a float32
    want = tab if dscale is None else tab * np.float32(dscale)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))  # bitwise: -0 and Inf too


@pytest.mark.parametrize("C", [16, 80])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_quant_t_and_transpose(T, C):
    bits = _random_finite((T, C + 32), 100 * T + C)  # ~45 % of these saturate at scale 7
    x = _dev_bf16(bits)[:, 16:16 + C]
    ld0 = (T + 63) // 64 * 64
    for fmt in (R.E4M3, R.E5M2):
        ref = _lut(7.0, fmt)[bits[:, 16:16 + C]]
        assert ((ref & 0x7F) == R.MAX_CODE[fmt]).any()
        x8 = torch.from_numpy(np.ascontiguousarray(_lut(7.0, fmt)[bits])).to(DEV)[:, 16:16 + C]
        for ldy in (ld0, (ld0 // 128 + 1) * 128):
            want = np.zeros((C, ldy), dtype=np.uint8)
            want[:, :T] = ref.T
            a = torch.full((C, ldy), SENTINEL, dtype=torch.uint8, device=DEV)
            b = torch.full((C, ldy), SENTINEL, dtype=torch.uint8, device=DEV)
            _ext().fp8_quant_t(x, a, _f32(7.0), fmt)
            _ext().fp8_transpose(x8, b)
            assert _mismatches(a.cpu().numpy(), want, fmt) == 0, (fmt, ldy)
            assert np.array_equal(b.cpu().numpy(), want), (fmt, ldy)


def _multi_case(lengths, slots, mags, seed):
    rng = np.random.default_rng(seed)
    srcs_bits = [R.f32_to_bf16_bits((rng.standard_normal(n) * m).astype(np.float32)) for n, m in zip(lengths, mags)]
    srcs = [_dev_bf16(b) for b in srcs_bits]
    dsts = [torch.full((n + 16,), SENTINEL, dtype=torch.uint8, device=DEV) for n in lengths]
    rows, chunk0 = [], 0
    for s, d, n, slot in zip(srcs, dsts, lengths, slots):
        rows.append([s.data_ptr(), d.data_ptr(), n, slot, chunk0])
        chunk0 += (n + QM_CHUNK - 1) // QM_CHUNK
    return srcs_bits, srcs, dsts, torch.tensor(rows, dtype=torch.int64, device=DEV), chunk0


@FMTS
def test_quant_multi_chunk_edges(fmt):
    lengths = [16, QM_CHUNK - 16, QM_CHUNK, QM_CHUNK + 16, 3 * QM_CHUNK + 48]
    slots = [3, 0, 4, 1, 2]
    bits, srcs, dsts, segs, nchunks = _multi_case(lengths, slots, [0.02, 3.0, 0.5, 40.0, 1.0], 11)
    assert nchunks == 1 + 1 + 1 + 2 + 4
    amax = _amax0(6)
    _ext().fp8_quant_multi(segs, nchunks, None, amax, fmt, True)
    words = amax.cpu().numpy().view(np.uint32)
    for b, slot in zip(bits, slots):
        assert int(words[slot]) == _exact_amax_word(b)
    assert words[5] == 0
    assert all((d == SENTINEL).all().item() for d in dsts)  # the amax pass writes no bytes
    # a different scale per slot; slot 1 (the QM_CHUNK + 16 segment) saturates about half its elements
    fmax = R.FMAX[fmt]
    qs = np.ones(6, dtype=np.float32)
    for b, slot, c in zip(bits, slots, [1.0, 0.5, 0.01, 1.0, 3.0]):
        qs[slot] = np.float32(fmax) / (words[slot:slot + 1].view(np.float32)[0]) * np.float32(c)
    qs[1] = np.float32(fmax / 40.0 * 1.5)
    _ext().fp8_quant_multi(segs, nchunks, torch.from_numpy(qs).to(DEV), amax, fmt, False)
    assert np.array_equal(amax.cpu().numpy().view(np.uint32), words)  # the quantize pass leaves amax alone
    for b, d, slot, n in zip(bits, dsts, slots, lengths):
        got = d.cpu().numpy()
        assert _mismatches(got[:n], _lut(qs[slot], fmt)[b], fmt) == 0, slot
        assert (got[n:] == SENTINEL).all(), slot
    sat = ((dsts[3].cpu().numpy()[:lengths[3]] & 0x7F) == R.MAX_CODE[fmt]).mean()
    print(f"FP8EDGE quant_multi fmt{fmt}: saturating slot share {sat:.3f}")
    assert 0.2 < sat < 0.8


def test_quant_multi_more_chunks_than_blocks():
    """8200 segments of 16 elements: nchunks exceeds the 8192-block grid, so blocks 0..7 take a second
    chunk (another segment, another slot)."""
    nseg = 8200
    rng = np.random.default_rng(12)
    bits = R.f32_to_bf16_bits((rng.standard_normal(nseg * 16) * np.exp2(rng.integers(-6, 6, nseg * 16))).astype(np.float32))
    src = _dev_bf16(bits)
    dst = torch.full((nseg * 16 + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    slot = (np.arange(nseg) * 37) % nseg  # a permutation: gcd(37, 8200) = 1
    i = np.arange(nseg, dtype=np.int64)
    segs = np.stack([src.data_ptr() + i * 32, dst.data_ptr() + i * 16, np.full(nseg, 16), slot, i], axis=1).astype(np.int64)
    segs = torch.from_numpy(segs).to(DEV)
    amax = _amax0(nseg)
    _ext().fp8_quant_multi(segs, nseg, None, amax, R.E4M3, True)
    want = np.zeros(nseg, dtype=np.uint32)
    want[slot] = (bits.reshape(nseg, 16) & 0x7FFF).max(axis=1).astype(np.uint32) << 16
    assert np.array_equal(amax.cpu().numpy().view(np.uint32), want)
    assert (dst == SENTINEL).all().item()
    scales = np.array([1.0, 30.0, 0.25, 2000.0], dtype=np.float32)  # 2000: most of a segment saturates
    qs = scales[np.arange(nseg) % 4]  # indexed by slot
    for fmt in (R.E4M3, R.E5M2):
        dst.fill_(SENTINEL)
        _ext().fp8_quant_multi(segs, nseg, torch.from_numpy(qs).to(DEV), amax, fmt, False)
        got = dst.cpu().numpy()
        ref = np.empty(nseg * 16, dtype=np.uint8)
        seg_scale = qs[slot]
        for s in scales:
            m = np.repeat(seg_scale == s, 16)
            ref[m] = _lut(s, fmt)[bits[m]]
        assert _mismatches(got[:-16], ref, fmt) == 0
        assert (got[-16:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------
# (b) fp8_scale_update against ScaleModel
BF16_SUBNORMAL = 2.0 ** -133
# the edge values, then a quiet stretch long enough for a 16-step window to forget them
AMAX_SEQ = np.array([0.0, BF16_SUBNORMAL, 1e-37, 0.5, 3.0, np.inf, 2.0, np.nan, 3e38, 0.0, 1.0, 0.25, 1e-39, 0.125, 7.0]
                    + [0.01 * (1 + k % 7) for k in range(40)], dtype=np.float32)
N_SLOTS = 70  # 64 threads per block: the full range launches two blocks
RANGES = [(0, N_SLOTS), (3, 5), (0, N_SLOTS), (64, 70), (0, N_SLOTS), (5, 5)]


@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("H", [1, 2, 16])
def test_scale_update_against_model(H, margin):
    """70 slots (e4m3 and e5m2 fmax alternating), every slot walking the amax sequence from its own
    offset: 0, a bf16 subnormal, 1e-37, ordinary values, 3e38, Inf, NaN, then 40 small ordinary values.
    72 steps, 36 of them over the full range, so even a 16-step window forgets its maximum.
    hist and amax words are copies: exact. qscale: one correctly rounded division and one product,
    within 1 ulp of the model. dscale: within 1 ulp of 1 / (the device's own qscale)."""
    ext = _ext()
    fmax = np.where(np.arange(N_SLOTS) % 2 == 0, 448.0, 57344.0).astype(np.float32)
    model = R.ScaleModel(N_SLOTS, H, margin, fmax)
    hist = torch.zeros(N_SLOTS, H, dtype=torch.float32, device=DEV)
    amax = _amax0(N_SLOTS)
    qscale = torch.ones(N_SLOTS, dtype=torch.float32, device=DEV)
    dscale = torch.ones(N_SLOTS, dtype=torch.float32, device=DEV)
    fmax_d = torch.from_numpy(fmax).to(DEV)
    worst_q = worst_d = 0
    forgot = clamped = False
    for step in range(72):
        vals = AMAX_SEQ[(step + np.arange(N_SLOTS)) % AMAX_SEQ.size]
        s0, s1 = RANGES[step % len(RANGES)]
        # slots outside the range keep their pending amax on both sides (max with the new value, as the
        # quantize passes would): only an update clears it
        words = np.maximum(model.amax, vals.view(np.uint32))
        model.amax[:] = words
        amax.copy_(torch.from_numpy(words.view(np.int32)))
        prev_max = model.hist.max(axis=1).copy()
        model.update(s0, s1)
        ext.fp8_scale_update(hist, amax, qscale, dscale, fmax_d, s0, s1, 2.0 ** -margin)
        forgot |= bool((model.hist.max(axis=1) < prev_max).any())
        clamped |= bool((model.qscale == R.FLT_MAX).any())
        h, a = hist.cpu().numpy(), amax.cpu().numpy().view(np.uint32)
        q, d = qscale.cpu().numpy(), dscale.cpu().numpy()
        assert np.array_equal(h.view(np.uint32), model.hist.view(np.uint32)), f"step {step}: history"
        assert np.array_equal(a, model.amax), f"step {step}: amax words"
        bad = ~(np.isfinite(q) & (q > 0) & np.isfinite(d) & (d > 0))
        assert not bad.any(), (f"step {step}: scales not finite and positive at slots {np.flatnonzero(bad)[:4]}: window max "
                               f"{model.hist.max(axis=1)[bad][:4]} qscale {q[bad][:4]} dscale {d[bad][:4]}")
        dq = R.ulp_distance(q, model.qscale)
        dd = R.ulp_distance(d, np.float32(1.0) / q)
        worst_q, worst_d = max(worst_q, int(dq.max())), max(worst_d, int(dd.max()))
        assert dq.max() <= 1, f"step {step}: qscale {int(dq.max())} ulp from the model"
        assert dd.max() <= 1, f"step {step}: dscale {int(dd.max())} ulp from 1 / qscale"
    assert forgot and clamped  # the window dropped a maximum; the overflowing quotient was reached
    print(f"FP8EDGE scale_update H{H} margin{margin}: qscale ulp {worst_q} dscale ulp {worst_d}")


@FMTS
@pytest.mark.parametrize("tiny", [1e-37, BF16_SUBNORMAL], ids=["1e-37", "bf16-subnormal"])
def test_tiny_amax_quantize_has_no_nan(fmt, tiny):
    """A tensor of zeros and one tiny amax (fmax / amax overflows float32): the current-scaling
    quantize must give finite positive scales and no NaN byte; zeros stay zeros."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    bits = np.zeros((8, 32), dtype=np.uint16)
    t = int(R.f32_to_bf16_bits(np.array([tiny], dtype=np.float32))[0])
    bits[1::2] = 0x8000
    bits[3, 7], bits[4, 9] = t, t | 0x8000
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
    y, ds = meta.quantize(_dev_bf16(bits), 0, current=True)
    got, q, d = y.cpu().numpy(), meta.qscale.item(), ds.item()
    print(f"FP8EDGE tiny amax {tiny:.3g} fmt{fmt}: qscale {q:.6g} dscale {d:.6g} NaN bytes {int(R.is_nan_code(got, fmt).sum())}")
    assert math.isfinite(q) and q > 0 and math.isfinite(d) and d > 0
    assert not R.is_nan_code(got, fmt).any()
    zero = (bits & 0x7FFF) == 0
    assert np.array_equal(got[zero], (bits[zero] >> 8).astype(np.uint8))
    assert q == float(R.FLT_MAX)
    if tiny >= 2.0 ** -126:  # a normal float32: its product is defined
        assert _mismatches(got, _lut(q, fmt)[bits], fmt) == 0
    assert (np.abs(R.decode_table(fmt)[got]) < R.FMAX[fmt]).all()


# ------------------------------------------------------------------------------------------------
# scales with a saturating share set by construction
def _scale_for(absy: np.ndarray, target: float, fmt: int) -> np.float32:
    """fmax over the order statistic of |y| that a share `target` of the elements exceeds; target 0:
    the largest float32 scale at which max|y| * scale stays <= fmax."""
    a = absy.ravel()
    fmax = np.float32(R.FMAX[fmt])
    if target == 0.0:
        m = a.max()
        qs = fmax / m
        while float(m) * float(qs) > float(fmax):
            qs = np.nextafter(qs, np.float32(0))
        return qs
    k = int(round(target * a.size))
    return fmax / np.partition(a, a.size - k)[a.size - k]


def _share(absy: np.ndarray, qs, fmt: int) -> float:
    return float((absy.astype(np.float64) * float(qs) > R.FMAX[fmt]).mean())


def _check_share(share: float, target: float):
    if target == 0.0:
        assert share == 0.0
    else:
        assert target / 2 <= share <= target * 2, f"saturating share {share:.4f} not within a factor 2 of {target}"


def _absf(bits: np.ndarray) -> np.ndarray:
    return np.abs(R.bf16_to_f32(bits))


# ------------------------------------------------------------------------------------------------
# (c) column sums with the fp8 copy: the input is already bf16, so the bytes are exact
@FMTS
@pytest.mark.parametrize("N", [768, 2304])
def test_colsum_copy_exact(N, fmt):
    ext = _ext()
    T = 130
    rng = np.random.default_rng(N + fmt)
    bits = R.f32_to_bf16_bits((rng.standard_normal((T, N)) * 0.3).astype(np.float32))
    dy = _dev_bf16(bits)
    db0 = torch.zeros(N, device=DEV)
    ext.colsum(dy, T, N, db0, None, None, 0, 0.0)
    vals = R.bf16_to_f32(bits).astype(np.float64)
    # f32 adds in any order: each of the T - 1 adds of a column rounds a partial sum <= sum|dy|
    tol = (T - 1) * 2.0 ** -24 * np.abs(vals).sum(axis=0)
    assert (np.abs(db0.cpu().numpy() - vals.sum(axis=0)) <= tol).all()
    for target in SETTINGS:
        qs = _scale_for(_absf(bits), target, fmt)
        share = _share(_absf(bits), qs, fmt)
        q = torch.full((T, N), SENTINEL, dtype=torch.uint8, device=DEV)
        am, db1 = _amax0(), torch.zeros(N, device=DEV)
        ext.colsum(dy, T, N, db1, None, None, 0, 0.0, q_out=q, q_scale=_f32(qs), q_amax=am, q_fmt=fmt)
        got = q.cpu().numpy()
        bad = _mismatches(got, _lut(qs, fmt)[bits], fmt)
        print(f"FP8EDGE colsum T{T} N{N} fmt{fmt} target {target}: share {share:.5f} mismatches {bad}")
        _check_share(share, target)
        assert bad == 0
        assert _word(am) == _exact_amax_word(bits)
        assert (np.abs(db1.cpu().numpy() - vals.sum(axis=0)) <= tol).all()
        assert (np.abs(db1.cpu().numpy() - db0.cpu().numpy()) <= 2 * tol).all()
    # one NaN element, at the scale with saturating and direct waves: its byte is NaN, the amax
    # non-finite, every other byte as before
    qs = _scale_for(_absf(bits), 0.005, fmt)
    b = bits.copy()
    b[77, 333] = 0x7FC0
    q = torch.full((T, N), SENTINEL, dtype=torch.uint8, device=DEV)
    am = _amax0()
    ext.colsum(_dev_bf16(b), T, N, torch.zeros(N, device=DEV), None, None, 0, 0.0, q_out=q, q_scale=_f32(qs), q_amax=am, q_fmt=fmt)
    got, ref = q.cpu().numpy(), _lut(qs, fmt)[bits]
    assert R.is_nan_code(got[77, 333], fmt)
    assert _word(am) >= INF_WORD
    got[77, 333] = ref[77, 333]
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------------
# (d) producers that round an fp32 value once to fp8 and once to bf16
def _bracket_check(name, fmt, run, identical_to_plain=True, copy_only=None):
    """run(None) -> the bf16 output without the copy; run(qs) -> (bf16 output, bytes, amax tensor).
    copy_only(qs) -> bytes of the kernel's copy-only mode, which must equal the storing mode's."""
    y0 = _bits(run(None))
    for target in SETTINGS:
        qs = _scale_for(_absf(y0), target, fmt)
        y, q, am = run(qs)
        yb, got = _bits(y), q.cpu().numpy()
        same = np.array_equal(yb, y0)
        absy = _absf(yb)
        assert np.isfinite(absy).all()
        share = _share(absy, qs, fmt)
        lo, hi = R.bracket(yb, qs, fmt)
        dist = R.bracket_distance(got, yb, qs, fmt)
        must_sat = lo == R.MAX_CODE[fmt]
        amax = np.array([_word(am)], dtype=np.uint32).view(np.float32)[0]
        amax_rel = abs(float(amax) - float(absy.max())) / float(absy.max())
        print(f"FP8EDGE {name} fmt{fmt} target {target}: share {share:.5f} must-saturate {must_sat.mean():.5f} "
              f"brackets wider than one code {(hi > lo).mean():.4f} worst distance {int(dist.max())} "
              f"outside {int((dist > 0).sum())} amax_rel {amax_rel:.2e} bf16 identical {same}")
        if identical_to_plain:
            assert same, "the bf16 output changed with the copy"
        if same:
            _check_share(share, target)
        elif target == 0.0:  # another kernel computed y0: a handful of elements may pass its maximum
            assert share <= 1e-4
        else:
            _check_share(share, target)
        assert not R.is_nan_code(got, fmt).any() and ((got & 0x7F) <= R.MAX_CODE[fmt]).all()
        assert int(dist.max()) == 0, f"{int((dist > 0).sum())} bytes outside their bracket, worst {int(dist.max())} codes"
        assert ((got[must_sat] & 0x7F) == R.MAX_CODE[fmt]).all()
        assert amax_rel <= 2.0 ** -8
        if copy_only is not None:
            assert np.array_equal(copy_only(qs).cpu().numpy(), got), "copy-only mode wrote other bytes"


def _ln_inputs(T, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(T, D, generator=g) * 2 + 0.5).to(torch.bfloat16).to(DEV)
    w = (torch.randn(D, generator=g) * 0.5 + 1.0).to(DEV)
    b = (torch.randn(D, generator=g) * 0.1).to(DEV)
    return x, w, b, g


@pytest.mark.parametrize("D", [768, 1280])
def test_layernorm_fwd_copy(D):
    ext = _ext()
    T = 70
    x, w, b, _ = _ln_inputs(T, D, D)

    def run(qs, skip_y=False):
        if qs is None:
            return ext.layernorm_fwd(x, w, b, 1e-6, T, D)[0]
        q = torch.full((T, D), SENTINEL, dtype=torch.uint8, device=DEV)
        am = _amax0()
        y = ext.layernorm_fwd_q8(x, w, b, 1e-6, T, D, q, _f32(qs), am, skip_y)[0]
        return y, q, am

    _bracket_check(f"layernorm_fwd T{T} D{D}", R.E4M3, run, copy_only=lambda qs: run(qs, True)[1])


@pytest.mark.parametrize("D", [768, 1280])
def test_layernorm_fwd_copy_nan_row(D):
    """One NaN input element: its row's bytes are NaN, the amax is non-finite, the other rows' bytes
    are unchanged, and a following scale update leaves history and scales as they were."""
    ext = _ext()
    T = 70
    x, w, b, _ = _ln_inputs(T, D, D)
    y0 = _bits(ext.layernorm_fwd(x, w, b, 1e-6, T, D)[0])
    qs = _scale_for(_absf(y0), 0.005, R.E4M3)
    outs = []
    for poison in (False, True):
        xi = x.clone()
        if poison:
            xi[7, 13] = float("nan")
        q = torch.full((T, D), SENTINEL, dtype=torch.uint8, device=DEV)
        am = _amax0()
        ext.layernorm_fwd_q8(xi, w, b, 1e-6, T, D, q, _f32(qs), am, False)
        outs.append((q.cpu().numpy(), am))
    (q0, _), (q1, am) = outs
    assert R.is_nan_code(q1[7], R.E4M3).all()
    assert _word(am) >= INF_WORD
    rest = np.arange(T) != 7
    assert np.array_equal(q1[rest], q0[rest])
    hist = torch.tensor([[1.5, 0.5]], device=DEV)
    qscale, dscale = _f32(7.0), _f32(1.0 / 7.0)
    ext.fp8_scale_update(hist, am, qscale, dscale, _f32(448.0), 0, 1, 1.0)
    assert hist.cpu().tolist() == [[1.5, 0.5]] and qscale.item() == 7.0 and dscale.item() == np.float32(1.0 / 7.0)
    assert _word(am) == 0


@FMTS
@pytest.mark.parametrize("linked", [False, True], ids=["plain", "linked"])
@pytest.mark.parametrize("D", [768, 1280])
def test_layernorm_bwd_copy(D, linked, fmt):
    ext = _ext()
    T = 70
    x, w, b, g = _ln_inputs(T, D, D + 1)
    _, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5, T, D)
    dy = torch.randn(T, D, generator=g).to(torch.bfloat16).to(DEV)
    dres = torch.randn(T, D, generator=g).to(torch.bfloat16).to(DEV)
    seed = torch.tensor([4242], dtype=torch.int64, device=DEV)

    def run(qs, nostore=False):
        dx, dz = torch.empty_like(x), (torch.empty_like(x) if linked else None)
        dw, db, ds = (torch.zeros(D, device=DEV) for _ in range(3))
        kw = dict(dsum=ds, dz=dz, seed=seed if linked else None, seed_offset=3 << 32, drop_p=0.1 if linked else 0.0)
        if qs is None:
            ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, dres, D, dx, D, dw, db, T, **kw)
            return dz if linked else dx
        q = torch.full((T, D), SENTINEL, dtype=torch.uint8, device=DEV)
        am = _amax0()
        ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, dres, D, dx, D, dw, db, T, q_out=q, q_scale=_f32(qs), q_amax=am,
                          q_fmt=fmt, dz_nostore=nostore, **kw)
        return (dz if linked else dx), q, am

    _bracket_check(f"layernorm_bwd {'linked' if linked else 'plain'} T{T} D{D}", fmt, run,
                   copy_only=(lambda qs: run(qs, True)[1]) if linked else None)


ATTN_SHAPES = pytest.mark.parametrize("B,N,H,dh", [(2, 257, 2, 80), (2, 197, 2, 64)])


def _qkv(B, N, H, dh, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B * N, 3 * H * dh, generator=g) * 2).to(torch.bfloat16).to(DEV), g


@ATTN_SHAPES
def test_attn_fwd_copy(B, N, H, dh):
    ext = _ext()
    D, sc = H * dh, 1.0 / math.sqrt(dh)
    qkv, _ = _qkv(B, N, H, dh, N)

    def run(qs, q_only=False):
        if qs is None:
            return ext.attn_fwd(qkv, B, N, H, sc)[0]
        q = torch.full((B * N, D), SENTINEL, dtype=torch.uint8, device=DEV)
        am = _amax0()
        o, _ = ext.attn_fwd(qkv, B, N, H, sc, None, 0, 0.0, q, _f32(qs), am, q_only)
        return o, q, am

    # dh 64 with N <= 256: the plain call takes the whole-head kernel, the copy the generic one, so the
    # two bf16 outputs are not the same computation
    _bracket_check(f"attn_fwd B{B} N{N} H{H} dh{dh}", R.E4M3, run, identical_to_plain=not (dh == 64 and N <= 256),
                   copy_only=lambda qs: run(qs, True)[1])


@FMTS
@ATTN_SHAPES
def test_attn_bwd_copy(B, N, H, dh, fmt):
    """dQKV's copy. At N 197 with dh 64 the backward without attention dropout is the pipelined kernel,
    which writes no copy (attn_bwd_q8_ok): that shape runs with attention dropout 0.1, as the model
    does when it takes a copy there."""
    ext = _ext()
    D, sc = H * dh, 1.0 / math.sqrt(dh)
    qkv, g = _qkv(B, N, H, dh, N + 1)
    p = 0.0 if ext.attn_bwd_q8_ok(B, N, H, D, False) else 0.1
    assert ext.attn_bwd_q8_ok(B, N, H, D, p > 0)
    seed = torch.tensor([4321], dtype=torch.int64, device=DEV) if p > 0 else None
    o, lse = ext.attn_fwd(qkv, B, N, H, sc, seed, 5 << 32, p)
    do = torch.randn(B * N, D, generator=g).to(torch.bfloat16).to(DEV)

    def run(qs, q_only=False):
        if qs is None:
            return ext.attn_bwd(do, qkv, o, lse, B, N, H, sc, None, None, seed, 5 << 32, p)
        q = torch.full((B * N, 3 * D), SENTINEL, dtype=torch.uint8, device=DEV)
        am = _amax0()
        dqkv = ext.attn_bwd(do, qkv, o, lse, B, N, H, sc, None, None, seed, 5 << 32, p, q_out=q, q_scale=_f32(qs), q_amax=am,
                            q_only=q_only, q_fmt=fmt)
        return dqkv, q, am

    _bracket_check(f"attn_bwd B{B} N{N} H{H} dh{dh} p{p}", fmt, run, copy_only=lambda qs: run(qs, True)[1])


@pytest.mark.parametrize("dgelu", [False, True], ids=["gelu-e4m3", "dgelu-e5m2"])
def test_gemm_fp8_producer_epilogue(dgelu):
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    M, N, K = 520, 768, 256
    fmt = R.E5M2 if dgelu else R.E4M3
    g = torch.Generator(device="cpu").manual_seed(77 + dgelu)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    xq, xs = F8.Fp8Meta(1, DEV, history=1, fmt=fmt).quantize(x, 0, current=True)  # dgrad: an e5m2 gradient operand
    wq, ws = F8.Fp8Meta(1, DEV, history=1, fmt=F8.E4M3).quantize(w, 0, current=True)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    if dgelu:
        aux.copy_((torch.rand(M, N, generator=g) * 1.1).to(torch.bfloat16))

    def run(qs, skip_out=False):
        quant = None
        if qs is not None:
            meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
            meta.calibrated[0] = True
            meta.qscale.fill_(float(qs))
            assert meta.qscale.item() == float(qs)
            quant = meta.producer(0)
        if dgelu:
            r = F8.linear_dgrad_fp8(xq, xs, wq, ws, dgelu_aux=aux, quant=quant, skip_out=skip_out)
        else:
            r = F8.linear_fwd_fp8(xq, xs, wq, ws, bias, gelu_aux=aux, quant=quant, skip_out=skip_out)
        if qs is None:
            return r
        y, (q, _) = r
        return y, q, meta.amax

    _bracket_check(f"gemm_fp8 {'dGELU' if dgelu else 'GELU'} M{M} N{N} K{K}", fmt, run, copy_only=lambda qs: run(qs, True)[1])
