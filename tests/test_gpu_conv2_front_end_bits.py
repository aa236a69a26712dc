"""conv2's fused front end and address arithmetic (conv_wq.h) may be rearranged freely, its floating-point work may not: the
probabilities and finite flags of iss_cnn_probs are compared BIT FOR BIT with those recorded from the library of the commit
before the scratch reloads were taken out of that kernel (tests/golden/conv2_parent_bits.npz, written by
tests/golden/make_conv2_parent_bits.py, whose header names the commit).  Both stand-in nets (21 mel: tiles of 508 rows; 24 mel:
512), fp16 and bf16 halves, the cases of tests/conv2_bits_cases.py.  Where the recorded commit gave the same bits with conv2 on
conv_x3_ws_kernel (ISS_DIAG_NO_WQ), that identity is asserted here too."""
import os

import numpy as np
import pytest

import conv2_bits_cases as CB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def recorded(golden):
    z = np.load(os.path.join(golden, 'conv2_parent_bits.npz'))
    assert np.array_equal(z['mspec'].view(np.uint32), CB.make_mspec().view(np.uint32)), 'the generator of the inputs drifted: use the stored rows'
    return z


@pytest.mark.parametrize('mode', list(CB.MODES))
def test_conv2_bits_match_parent(recorded, mode):
    mspec = recorded['mspec']
    c = CB.context(mode)
    try:
        for net_id, (nmel, ncls, seed) in enumerate(CB.NETS):
            for name, feats, rows in CB.cases(mspec):
                k = CB.key(mode, net_id, name)
                want_p, want_f = recorded[k + '.p'], recorded[k + '.f']
                p, f, kern = CB.run(c, net_id, feats, rows)
                nbad = int((p.view(np.uint32) != want_p.view(np.uint32)).sum())
                print(f'{k}: {len(rows)} windows, {int((~f).sum())} not finite, {nbad} of {p.size} values differ in bits, '
                      f'max |d p| {float(np.abs(p - want_p).max()):.2e}; {[x for x in kern if x.startswith("conv_x3_w")]}')
                assert any(x.startswith(CB.CONV2) for x in kern) == bool(recorded[k + '.wq']), kern
                assert np.array_equal(f, want_f), k
                assert nbad == 0, k
                if bool(recorded[k + '.same_no_wq']):
                    p2, f2, kern2 = CB.run(c, net_id, feats, rows, no_wq=True)
                    assert not any(x.startswith(CB.CONV2) for x in kern2), kern2
                    assert np.array_equal(p2.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(f2, want_f), k
    finally:
        c.close()


def test_cases_reach_conv2(recorded):
    """Every case from 7 windows on ran conv2 on conv_x3_wq_kernel<5,3,...> when it was recorded (the selection gives the one-
    and two-window lists of the 70-row input to another kernel; they are kept: whatever runs them gives the recorded bits), and
    the non-finite cases have dead and live windows."""
    for mode in CB.MODES:
        for net_id in range(len(CB.NETS)):
            for name, feats, rows in CB.cases(recorded['mspec']):
                k = CB.key(mode, net_id, name)
                assert bool(recorded[k + '.wq']) or name.startswith('t70_'), k
                if name in ('t300_inf_row', 'scattered_333', 'runs_with_gaps'):
                    f = recorded[k + '.f']
                    assert f.any() and not f.all(), k
