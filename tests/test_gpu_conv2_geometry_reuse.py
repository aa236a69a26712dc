"""conv2's slice geometry is computed once per tile and reused by the blocks that build the tile's other chunks, and tile 0's is
handed from a group's last block to the next group's first (conv_wq.h).  The window lists of tests/conv2_reuse_cases.py give every
one of the launch's 256 workgroups at least three groups, so that hand-over runs everywhere, twice; probabilities and finite flags
of iss_cnn_probs are compared BIT FOR BIT with those recorded from the parent commit's library (tests/golden/conv2_reuse_bits.npz,
written by tests/golden/make_conv2_reuse_bits.py, whose header names the commit).  Where that commit gave the same bits with
conv2 on conv_x3_ws_kernel (ISS_DIAG_NO_WQ: bf16 halves), that identity is asserted too."""
import os

import numpy as np
import pytest

import conv2_reuse_cases as CR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def recorded(golden):
    return np.load(os.path.join(golden, 'conv2_reuse_bits.npz')), np.load(os.path.join(golden, 'conv2_parent_bits.npz'))['mspec']


@pytest.mark.parametrize('mode', list(CR.MODES))
def test_conv2_bits_match_parent_over_three_groups_per_workgroup(recorded, mode):
    z, mspec = recorded
    c = CR.context(mode)
    try:
        for net_id in range(len(CR.NETS)):
            for name, feats, rows in CR.cases(mspec, net_id):
                k = CR.key(mode, net_id, name)
                want_p, want_f = z[k + '.p'], z[k + '.f']
                p, f, kern = CR.run(c, net_id, feats, rows)
                nbad = int((p.view(np.uint32) != want_p.view(np.uint32)).sum())
                print(f'{k}: {len(rows)} windows, {int((~f).sum())} not finite, {CR.groups(net_id, int(f.sum()))} groups, {nbad} of {p.size} values '
                      f'differ in bits, max |d p| {float(np.abs(p - want_p).max()):.2e}; {[x for x in kern if x.startswith("conv_x3_w")]}')
                assert bool(z[k + '.wq']) and any(x.startswith(CR.CONV2) for x in kern), kern
                assert np.array_equal(f, want_f), k
                assert f.any() and not f.all(), k                    # the non-finite row: dead and live windows
                assert CR.groups(net_id, int(f.sum())) >= 3 * CR.WORKGROUPS, k
                assert nbad == 0, k
                if mode == 'bf16x3':
                    assert bool(z[k + '.same_no_wq']), k
                if bool(z[k + '.same_no_wq']):
                    p2, f2, kern2 = CR.run(c, net_id, feats, rows, no_wq=True)
                    assert not any(x.startswith(CR.CONV2) for x in kern2), kern2
                    assert np.array_equal(p2.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(f2, want_f), k
    finally:
        c.close()
