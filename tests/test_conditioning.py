"""Host side of the conditioning tests (tests/conditioning.py): the inputs are what they claim to be, the float32 reference
alone stays inside the cap that gives tests/test_gpu_conditioning.py's relative bound its meaning, and the float32 emulation of
the two first-layer formulas -- the reasoning behind those tests -- can be re-run without a device."""
import numpy as np
import pytest

import conditioning as CD


@pytest.mark.parametrize('case', CD.CASES, ids=CD.case_id)
def test_window_ratio_is_nominal(case):
    """Median |mean| / std over the segmenter's own 200 windows, at 21 and at 24 bands: within 25 % of the case's nominal ratio."""
    m = CD.make_mspec(*case)
    assert m.dtype == np.float32 and m.shape == (CD.T, 24)
    rows = CD.rows_overlapping()
    assert len(rows) == 200
    for nmel in (21, 24):
        med = np.median(CD.window_ratios(m, nmel, rows))
        print(f'{CD.case_id(case)} nmel {nmel}: nominal {CD.ratio(case):.1f}, median window ratio {med:.1f}')
        assert abs(med - CD.ratio(case)) <= 0.25 * CD.ratio(case), (case, nmel, med)


def test_mixed_has_two_regimes_and_a_dead_region():
    m = CD.mixed()
    rows = CD.rows_overlapping()
    r = CD.window_ratios(m, 21, rows)
    dead = ~np.isfinite(r)
    assert np.array_equal(dead, (rows + 68 > 120) & (rows <= 122)) and 30 < dead.sum() < 40
    assert np.nanmax(r) > 48 and np.nanmin(r) < 3                        # ratio-64 windows and ordinary ones on one recording


@pytest.mark.parametrize('name', sorted(CD.NETS))
@pytest.mark.parametrize('case', CD.CASES, ids=CD.case_id)
def test_reference_stays_inside_the_cap(case, name):
    """e_ref = max |reference32 - truth| <= REF_CAP on both window lists: a case whose float32 reference were further from float64
    would make `PROB_TOL + REF_MARGIN * e_ref` meaningless, so this is a condition of the device test, not a tolerance."""
    o = CD.oracle(name, case)
    for lst in ('overlapping', 'scattered'):
        p64, f64, p32, f32 = o[lst]
        assert f64.all() and f32.all()
        e_ref = np.abs(p32 - p64).max()
        print(f'{CD.case_id(case)} (ratio {CD.ratio(case):.0f}) {name} {lst}: e_ref {e_ref:.2e}')
        assert e_ref <= CD.REF_CAP, (case, name, lst, e_ref)


# (mean, std) of the emulation table the device tests were motivated by, and the ladder's own rungs
_EMU = sorted(set([(-3.0, 1.7), (-18.0, 0.5), (5.0, 0.05), (-20.0, 0.1), (-20.0, 0.01)] + CD.CASES), key=CD.ratio)


def test_float32_emulation_shared_formula_loses_to_normalise_first():
    """relu(R * rstd + (bias - mean * rstd * S)) on raw rows against conv((x - mean) / std), both in float32 without FMA, layer 1 of
    the 21-band net on one window: from ratio 36 up the shared formula is the less accurate of the two.  Only the direction is
    asserted -- the figures are printed; what the device does is test_gpu_conditioning.py's business."""
    layers, _ = CD.net('standin21')
    for mean, std in _EMU:
        window = CD.make_mspec(mean, std)[100:168, :21]
        e_first, e_shared, scale = CD.emulate_first_layer(layers, window)
        print(f'mean {mean:g} std {std:g} (ratio {abs(mean) / std:.0f}): normalise-first {e_first:.1e}, shared formula {e_shared:.1e}, '
              f'activation scale {scale:.1f}')
        assert e_first < 1e-3 * scale and e_shared < 1e-2 * scale         # both formulas compute the layer at all
        if abs(mean) / std >= 36:
            assert e_shared > e_first, (mean, std, e_first, e_shared)
