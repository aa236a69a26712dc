"""The operand split of the conv kernels (conv_common.h: x = hi + lo, hi = rne16(x), lo = rne16(x - hi)) bit for bit against
numpy, fp16 and bf16 halves, in the forms the kernels inline (iss_diag_split16: split4_pk and the one-value form of the
epilogues).  This is the yardstick for any other instruction sequence that forms the halves (a single-rounding fp16 residual,
v_fma_mix{lo,hi}_f16, passed it: profiles/conv2_front_end_ab.md), so ties, fp16-subnormal and underflowing lo parts, the overflow
of hi to inf and the f32 neighbours of every fp16 value are all in the input.  A half that is NaN in the reference (NaN inputs; inf - inf for +-inf inputs) is compared
as "is NaN" only."""
import numpy as np
import pytest


def make_inputs():
    """~1.3 x 10^6 float32 values (the same array every time)."""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    f = h.astype(np.float32)                                         # every fp16 value (NaN patterns and +-inf included)
    fin = np.isfinite(f)
    up = np.nextafter(f[fin], np.float32(np.inf)).astype(np.float32)
    dn = np.nextafter(f[fin], np.float32(-np.inf)).astype(np.float32)
    pos = np.sort(f[fin & (f >= 0)])                                 # 0 ... 65504: midpoints of adjacent values = the ties of rne16
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64) * 2, pos[:-1].astype(np.float64) + pos[1:].astype(np.float64))      # exact in f32
    rng = np.random.default_rng(16)
    mag = np.exp2(rng.uniform(-30.0, 17.0, 1 << 20)).astype(np.float32)
    mag[1::2] *= -1
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5.9e-39, 65504.0, 65519.996, 65520.0, 1e5,
                        -65504.0, -65519.996, -65520.0, -1e5, np.inf, -np.inf, np.nan], dtype=np.float32)
    return np.concatenate([f, up, dn, mid, -mid, mag, special]).astype(np.float32)


def _rne_bf16(x):
    """bf16 pattern of float32 x, round to nearest even by bit arithmetic (NaN stays NaN: quiet bit set)."""
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), ((u >> 16) | 0x40).astype(np.uint16), r)


def reference(x, f16):
    """(hi, lo) uint16 patterns and the mask of halves that are NaN, per the definition."""
    with np.errstate(over='ignore', invalid='ignore'):
        if f16:
            hi = x.astype(np.float16)
            lo = (x - hi.astype(np.float32)).astype(np.float16)
            return hi.view(np.uint16), lo.view(np.uint16), np.isnan(hi), np.isnan(lo)
        hi = _rne_bf16(x)
        hf = (hi.astype(np.uint32) << 16).view(np.float32)
        r = (x - hf).astype(np.float32)
        lo = _rne_bf16(r)
        return hi, lo, np.isnan(hf), np.isnan(r)


def _is_nan16(bits, f16):
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0) if f16 else ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def _lo_classes(x, hi, lo):
    """fp16 lo parts that are subnormal, and lo parts that are zero although x != hi (the residual underflowed)."""
    mag = lo & 0x7FFF
    sub = (mag != 0) & (mag < 0x0400)
    with np.errstate(invalid='ignore', over='ignore'):
        under = (mag == 0) & np.isfinite(x) & (x != hi.view(np.float16).astype(np.float32))
    return sub, under


def test_reference_has_subnormal_and_underflowing_lo_parts():
    """CPU: the numpy reference itself produces both kinds of small lo part for this input set, and splits exactly where it can:
    hi + lo == x wherever lo is a normal fp16."""
    x = make_inputs()
    assert 1.2e6 < x.size < 1.5e6
    hi, lo, nan_h, nan_l = reference(x, True)
    sub, under = _lo_classes(x, hi, lo)
    print(f'{x.size} inputs: {int(sub.sum())} fp16-subnormal lo parts, {int(under.sum())} lo parts underflow to zero, '
          f'{int(nan_h.sum())} / {int(nan_l.sum())} NaN hi / lo')
    assert sub.sum() > 1000 and under.sum() > 1000
    assert nan_l.sum() >= nan_h.sum() + 2                            # +-inf: lo = inf - inf
    ok = np.isfinite(x) & (np.abs(x) < 65520) & ~sub & ~under & ((lo & 0x7FFF) != 0)
    with np.errstate(invalid='ignore'):
        back = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
    assert np.all(np.abs(back[ok] - x[ok].astype(np.float64)) <= np.abs(x[ok].astype(np.float64)) * 2.0 ** -21)
    hb, lb, _, _ = reference(x, False)
    fin = np.isfinite(x) & (np.abs(x) < 3e38)
    backb = (hb.astype(np.uint32) << 16).view(np.float32).astype(np.float64) + (lb.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert np.all(np.abs(backb[fin] - x[fin].astype(np.float64)) <= np.abs(x[fin].astype(np.float64)) * 2.0 ** -16 + 1e-40)


@pytest.fixture(scope='module')
def inputs():
    x = make_inputs()
    return x, {True: reference(x, True), False: reference(x, False)}


@pytest.mark.gpu
@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('half', ['f16', 'bf16'])
def test_split16_bits(ctx, inputs, half, form):
    x, refs = inputs
    f16 = half == 'f16'
    want_h, want_l, nan_h, nan_l = refs[f16]
    hi, lo = ctx.diag_split16(x, f16, form)
    bad_h = np.where(nan_h, ~_is_nan16(hi, f16), hi != want_h)
    bad_l = np.where(nan_l, ~_is_nan16(lo, f16), lo != want_l)
    print(f'{half} form {form}: {x.size} values, {int(bad_h.sum())} hi / {int(bad_l.sum())} lo parts differ')
    for name, bad, got, want in (('hi', bad_h, hi, want_h), ('lo', bad_l, lo, want_l)):
        if bad.any():
            i = np.flatnonzero(bad)[:8]
            print(name, [(float(x[k]), hex(int(x[k:k + 1].view(np.uint32)[0])), hex(int(got[k])), hex(int(want[k]))) for k in i])
    if f16:
        sub, under = _lo_classes(x, hi, lo)
        assert sub.sum() > 1000 and under.sum() > 1000               # the device's own lo parts: subnormal ones and flushed-by-rounding ones
    assert not bad_h.any() and not bad_l.any()
