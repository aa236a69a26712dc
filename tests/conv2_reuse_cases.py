"""Inputs of tests/test_gpu_conv2_geometry_reuse.py and of the generator of its fixture (tests/golden/make_conv2_reuse_bits.py).

conv_x3_wq_kernel<5,3,...> keeps a tile's slice geometry (byte offsets, window / row-parity flags) in registers from the block
that builds the tile's first chunk to the blocks that build the others, and hands tile 0's over from a group's last block to the
next group's first.  A launch has at most 256 workgroups, and the lists of tests/conv2_bits_cases.py stop at 276 groups: hardly
any workgroup walks to a second group there.  These lists give EVERY workgroup at least three groups: live windows x conv2 rows
per window / rows per tile / 2 tiles per group >= 3 x 256 (checked in `groups`), per net, as one list of consecutive windows and
one of scattered windows with gaps, each over one non-finite row.  The rows are those stored in conv2_parent_bits.npz."""
import numpy as np

import conv2_bits_cases as CB

NETS, MODES, CONV2, run, context, key = CB.NETS, CB.MODES, CB.CONV2, CB.run, CB.context, CB.key
ROWS_TILE = ((62 * 17, 508), (62 * 20, 512))         # per net: conv2 GEMM rows per window, rows per tile (tests/conv2_bits_cases.py)
NWIN = (830, 710)                                    # windows per list, per net
WORKGROUPS = 256


def groups(net_id, nlive):
    rows, tmr = ROWS_TILE[net_id]
    tiles = -(-nlive * rows // tmr)
    return -(-tiles // 2)


def cases(mspec, net_id):
    """[(name, features, window rows)] for one net."""
    assert mspec.shape == (CB.T_LONG, 24)
    n = NWIN[net_id]
    out = []
    m = mspec.copy()
    m[400, :] = np.nan                               # the windows that start in rows 333..400 are dead
    out.append(('consecutive', m, np.arange(0, n, dtype=np.int32)))
    m2 = mspec.copy()
    m2[777, 5] = -np.inf
    rng = np.random.default_rng(100 + net_id)
    out.append(('scattered', m2, rng.integers(0, CB.T_LONG - 67, n).astype(np.int32)))
    return out
