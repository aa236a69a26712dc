"""The window-normalised first layer on quiet and stationary windows (tests/conditioning.py: |mean| / std from 2 to 2000, and two
regimes with a non-finite region on one recording), against float64, in all three arithmetic modes, on every form of the
shared first layer and on the per-window first layer it replaces.

Measured on an MI355X, max |p - truth| per run (case = mean_std of the rows; e_ref / e_ref_sc: the float32 reference's own
distance from float64 over the overlapping / the scattered list; shared, per-win: the overlapping list with and without the
shared first layer; scat, scat-pw: the scattered list likewise; in exact f32 conv1_same and conv1_pool have no shared form).
Every figure is inside its bound, the largest at 0.56 of it (ratio 2000, conv1_same, split bf16): the kernels are unchanged.
Up to ratio 64 the two paths agree; the shared path is up to 5 x worse at 100 - 200 and 2 - 4 x worse at 2000, where the float32
reference itself is 1.5e-4 .. 2.4e-4 from float64.

case          net           e_ref e_ref_sc | bf16x3: shared  per-win     scat  scat-pw | f16x3: shared  per-win     scat  scat-pw | f32: shared  per-win
m-3_s1.9      conv1_pool  1.4e-06  1.3e-06 |        1.8e-05  1.7e-05  1.2e-05  1.3e-05 |       1.6e-05  1.9e-05  6.9e-06  8.9e-06 |     2.3e-06  2.3e-06
m-3_s1.9      conv1_same  2.3e-06  1.6e-06 |        2.8e-05  3.4e-05  2.2e-05  3.4e-05 |       9.8e-06  9.0e-06  9.8e-06  9.0e-06 |     5.2e-06  5.2e-06
m-3_s1.9      standin21   2.0e-06  1.6e-06 |        2.9e-05  2.5e-05  1.9e-05  2.3e-05 |       5.9e-06  1.0e-05  4.4e-06  1.0e-05 |     3.1e-06  3.6e-06
m-3_s1.9      standin24   1.2e-06  9.6e-07 |        2.0e-05  2.1e-05  1.6e-05  1.4e-05 |       3.9e-06  6.9e-06  3.2e-06  5.6e-06 |     2.9e-06  2.5e-06
m-13.3_s0.72  conv1_pool  2.5e-06  1.8e-06 |        1.4e-05  1.6e-05  1.2e-05  1.3e-05 |       1.3e-05  1.7e-05  7.3e-06  7.8e-06 |     2.7e-06  2.7e-06
m-13.3_s0.72  conv1_same  2.5e-06  2.2e-06 |        3.7e-05  3.7e-05  2.0e-05  3.7e-05 |       9.6e-06  6.8e-06  1.0e-05  7.9e-06 |     3.7e-06  3.7e-06
m-13.3_s0.72  standin21   2.6e-06  2.8e-06 |        3.1e-05  3.2e-05  2.5e-05  2.6e-05 |       9.2e-06  1.2e-05  5.4e-06  1.0e-05 |     5.3e-06  3.3e-06
m-13.3_s0.72  standin24   3.6e-06  1.8e-06 |        1.9e-05  1.6e-05  1.6e-05  1.3e-05 |       4.4e-06  6.4e-06  3.4e-06  5.4e-06 |     3.3e-06  2.5e-06
m-12.6_s0.48  conv1_pool  4.4e-06  2.5e-06 |        1.8e-05  1.8e-05  8.3e-06  1.3e-05 |       2.1e-05  2.4e-05  1.1e-05  7.1e-06 |     3.8e-06  3.8e-06
m-12.6_s0.48  conv1_same  3.9e-06  2.9e-06 |        3.0e-05  3.9e-05  2.7e-05  2.7e-05 |       1.1e-05  7.6e-06  1.2e-05  9.1e-06 |     4.0e-06  4.0e-06
m-12.6_s0.48  standin21   5.9e-06  4.2e-06 |        3.2e-05  3.1e-05  2.2e-05  1.7e-05 |       1.4e-05  1.2e-05  7.0e-06  1.0e-05 |     7.7e-06  3.5e-06
m-12.6_s0.48  standin24   1.9e-06  1.9e-06 |        2.4e-05  2.2e-05  1.8e-05  1.9e-05 |       6.5e-06  6.5e-06  5.8e-06  7.0e-06 |     4.5e-06  2.7e-06
m-20_s0.5     conv1_pool  3.2e-06  1.4e-06 |        1.9e-05  1.8e-05  1.4e-05  1.1e-05 |       1.6e-05  1.3e-05  7.9e-06  6.9e-06 |     2.9e-06  2.9e-06
m-20_s0.5     conv1_same  3.8e-06  3.3e-06 |        3.3e-05  3.3e-05  2.3e-05  2.3e-05 |       9.5e-06  8.9e-06  8.1e-06  1.1e-05 |     5.0e-06  5.0e-06
m-20_s0.5     standin21   4.9e-06  4.7e-06 |        3.0e-05  3.3e-05  2.7e-05  1.7e-05 |       1.0e-05  9.3e-06  1.7e-05  9.6e-06 |     9.9e-06  3.9e-06
m-20_s0.5     standin24   7.4e-06  3.7e-06 |        2.1e-05  2.5e-05  2.1e-05  1.8e-05 |       8.0e-06  5.5e-06  7.5e-06  4.2e-06 |     6.6e-06  4.3e-06
m-20_s0.3125  conv1_pool  7.9e-06  4.2e-06 |        2.5e-05  1.6e-05  1.3e-05  1.3e-05 |       2.3e-05  1.8e-05  9.4e-06  9.3e-06 |     3.0e-06  3.0e-06
m-20_s0.3125  conv1_same  7.7e-06  5.7e-06 |        4.0e-05  2.9e-05  2.8e-05  2.9e-05 |       2.1e-05  1.3e-05  2.1e-05  1.3e-05 |     5.2e-06  5.2e-06
m-20_s0.3125  standin21   7.2e-06  1.4e-05 |        3.6e-05  2.7e-05  2.5e-05  2.7e-05 |       1.6e-05  1.1e-05  1.2e-05  1.1e-05 |     1.5e-05  7.0e-06
m-20_s0.3125  standin24   4.1e-06  4.6e-06 |        2.3e-05  1.5e-05  1.5e-05  1.5e-05 |       1.1e-05  6.6e-06  7.8e-06  5.5e-06 |     1.2e-05  5.0e-06
m5_s0.05      conv1_pool  6.6e-06  4.2e-06 |        1.9e-05  1.8e-05  1.3e-05  1.4e-05 |       1.9e-05  1.8e-05  1.2e-05  6.8e-06 |     5.6e-06  5.6e-06
m5_s0.05      conv1_same  7.0e-06  8.6e-06 |        3.1e-05  3.0e-05  2.9e-05  2.9e-05 |       1.8e-05  8.9e-06  1.4e-05  7.6e-06 |     9.3e-06  9.3e-06
m5_s0.05      standin21   1.3e-05  1.3e-05 |        4.3e-05  4.0e-05  3.6e-05  2.6e-05 |       3.2e-05  1.3e-05  2.2e-05  1.1e-05 |     3.2e-05  9.0e-06
m5_s0.05      standin24   8.2e-06  6.3e-06 |        3.3e-05  2.2e-05  1.6e-05  1.5e-05 |       2.3e-05  1.0e-05  1.6e-05  9.0e-06 |     2.1e-05  6.8e-06
m-20_s0.1     conv1_pool  1.1e-05  7.6e-06 |        3.1e-05  1.9e-05  2.4e-05  1.6e-05 |       3.0e-05  2.0e-05  2.6e-05  9.7e-06 |     7.7e-06  7.7e-06
m-20_s0.1     conv1_same  1.4e-05  1.5e-05 |        4.0e-05  4.1e-05  6.1e-05  2.8e-05 |       2.8e-05  1.4e-05  5.6e-05  8.3e-06 |     1.2e-05  1.2e-05
m-20_s0.1     standin21   3.0e-05  3.2e-05 |        4.5e-05  3.2e-05  6.0e-05  3.1e-05 |       3.9e-05  1.7e-05  5.2e-05  1.8e-05 |     4.0e-05  1.5e-05
m-20_s0.1     standin24   9.1e-06  1.1e-05 |        3.1e-05  2.2e-05  2.8e-05  2.1e-05 |       4.1e-05  1.3e-05  2.8e-05  8.5e-06 |     4.4e-05  9.2e-06
m-20_s0.01    conv1_pool  1.7e-04  9.3e-05 |        3.4e-04  1.0e-04  2.0e-04  8.7e-05 |       3.5e-04  1.0e-04  2.0e-04  8.9e-05 |     9.4e-05  9.4e-05
m-20_s0.01    conv1_same  1.5e-04  1.5e-04 |        3.9e-04  1.2e-04  2.8e-04  8.0e-05 |       3.9e-04  1.3e-04  2.6e-04  6.9e-05 |     1.3e-04  1.3e-04
m-20_s0.01    standin21   2.4e-04  2.1e-04 |        4.4e-04  1.8e-04  4.2e-04  1.4e-04 |       4.3e-04  1.8e-04  4.2e-04  1.4e-04 |     4.4e-04  1.9e-04
m-20_s0.01    standin24   1.6e-04  1.6e-04 |        3.2e-04  1.5e-04  2.7e-04  7.0e-05 |       3.2e-04  1.3e-04  2.7e-04  6.7e-05 |     3.3e-04  1.2e-04
mixed         conv1_pool  4.2e-06  4.2e-06 |        1.7e-05  1.6e-05  1.1e-05  1.3e-05 |       1.2e-05  1.1e-05  7.0e-06  8.5e-06 |     3.0e-06  3.0e-06
mixed         conv1_same  2.6e-06  1.6e-06 |        3.7e-05  3.2e-05  2.7e-05  1.9e-05 |       1.7e-05  6.3e-06  5.9e-06  5.2e-06 |     4.6e-06  4.6e-06
mixed         standin21   6.8e-06  6.8e-06 |        3.6e-05  2.7e-05  2.5e-05  2.7e-05 |       1.4e-05  1.1e-05  6.5e-06  6.9e-06 |     1.4e-05  7.0e-06
mixed         standin24   4.1e-06  4.1e-06 |        2.3e-05  1.5e-05  1.5e-05  1.5e-05 |       8.2e-06  6.9e-06  6.7e-06  4.7e-06 |     8.3e-06  3.0e-06
"""
import numpy as np
import pytest

from inaspeechsegmenter_amd import keras_model as KM, _native
import conditioning as CD

pytestmark = pytest.mark.gpu

_PRECS = (('bf16x3', _native.PREC_BF16X3), ('f16x3', _native.PREC_F16X3), ('f32', _native.PREC_F32))
# a first layer of its own, once per window: conv1_patch_x3_kernel, or the generic kernels in PATCH mode (MODE 2)
_PER_WINDOW = ('conv1_patch_x3_kernel<', 'conv_igemm_kernel<2>', 'conv_x3_kernel<2,')
# the conv that consumes the shared rows, per net (split-operand modes)
_CONSUMER = {k: v[1] for k, v in CD.NETS.items()}


def _run(ctx, rows, diag=0):
    """(probabilities, finite mask, conv instantiations launched) of net 5 on `rows`."""
    ctx.set_diag(diag)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        p, f = ctx.cnn_probs(5, rows)
        used = sorted(e['kernel'] for e in ctx.prof_instances())
    finally:
        ctx.prof_enable(False)
        ctx.set_diag(0)
    return p, f.astype(bool), used


@pytest.mark.parametrize('name', sorted(CD.NETS))
@pytest.mark.parametrize('case', CD.CASES + ['mixed'], ids=CD.case_id)
def test_first_layer_conditioning(ctx, name, case):
    """Per arithmetic mode four runs: the segmenter's overlapping list (shared first layer), the same list with the shared first
    layer switched off (per-window: normalise, then convolve), and 64 scattered windows (odd first rows, gaps) both ways -- on a
    400-row recording those overlap 10-fold, so they take the shared path too unless it is switched off.

    Every run: the finite mask of the float32 reference, non-finite windows exactly 0.5, and
        max |p - truth| <= 1e-4 + 4 e_ref      e_ref = max |reference32 - truth| over the same windows (never a device figure)
    and at the ratios real audio is known to reach (<= 64) and on `mixed`, max |p - truth| <= 1e-4 outright.  The shared path
    gets the bound of the per-window path: no allowance for being faster.  The conv instantiations say which first layer ran."""
    layers, shp = CD.net(name)
    mspec = CD.mspec_of(case)
    lists = {'overlapping': CD.rows_overlapping(), 'scattered': CD.rows_scattered()}
    assert len(lists['overlapping']) == 200 and len(lists['scattered']) == 64
    oracle = CD.oracle(name, case)
    e_ref = {}
    for lst, (p64, f64, p32, f32) in oracle.items():
        assert np.array_equal(f64, f32)
        e_ref[lst] = float(np.abs(p32 - p64).max())
        assert e_ref[lst] <= CD.REF_CAP, (lst, e_ref[lst])
    if case == 'mixed':
        assert 30 < (~oracle['overlapping'][3]).sum() < 40 and (~oracle['scattered'][3]).any()
    hard = case == 'mixed' or CD.ratio(case) <= 64
    ctx.set_mspec(mspec)
    ctx.cnn_load(5, KM.compile_layers(layers, shp))
    bad = []
    try:
        for pname, prec in _PRECS:
            ctx.set_precision(prec)
            err = {}
            for lst, rows in lists.items():
                p64, _, _, f32 = oracle[lst]
                for path, diag in (('shared', 0), ('per_window', 'no_shared_first')):
                    p, f, used = _run(ctx, rows, diag)
                    per_window = [k for k in used if k.startswith(_PER_WINDOW)]
                    if path == 'per_window':
                        assert per_window, (pname, lst, used)
                    elif pname != 'f32' or name.startswith('standin'):    # (exact f32 shares the valid 4x5 first layer only)
                        assert not per_window, (pname, lst, used)
                        if lst == 'overlapping':                          # ... and the form of the consumer the net was chosen for
                            want = _CONSUMER[name] if pname != 'f32' else 'conv_x3_ws_kernel<5,3,'
                            assert any(k.startswith(want) for k in used), (pname, used)
                            assert name != 'conv1_same' or any(k.endswith(',fs>') for k in used), (pname, used)
                    assert np.array_equal(f, f32), (pname, lst, path)
                    assert np.all(p[~f] == 0.5), (pname, lst, path)
                    e = err[lst, path] = float(np.abs(p - p64).max())
                    bound = CD.PROB_TOL + CD.REF_MARGIN * e_ref[lst]
                    if e > bound or (hard and e > CD.PROB_TOL):
                        bad.append((pname, lst, path, e, CD.PROB_TOL if hard else bound))
                    if pname == 'bf16x3' and path == 'shared' and name.startswith('standin'):
                        # first_layer_raw_kernel (one thread per output) forms the same fmaf chains as first_layer_rows_kernel
                        p_raw, f_raw, _ = _run(ctx, rows, 'no_flrows')
                        assert np.array_equal(p_raw, p) and np.array_equal(f_raw, f), (lst, np.abs(p_raw - p).max())
            print(f'{CD.case_id(case)} {name} {pname}: e_ref {e_ref["overlapping"]:.2e} e_shared {err["overlapping", "shared"]:.2e} '
                  f'e_per_window {err["overlapping", "per_window"]:.2e} | scattered: e_ref {e_ref["scattered"]:.2e} '
                  f'e_scattered {err["scattered", "shared"]:.2e} e_scattered_per_window {err["scattered", "per_window"]:.2e}')
    finally:
        ctx.set_precision(_native.PREC_BF16X3)
        ctx.set_diag(0)
    assert not bad, bad

