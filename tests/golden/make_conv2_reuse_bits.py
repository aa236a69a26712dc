"""Generator of tests/golden/conv2_reuse_bits.npz (tests/test_gpu_conv2_geometry_reuse.py).

The recorded bits are those of commit 1c2b96a ("Take conv2's scratch spills out of its MFMA stream; check it at build"), the
parent of the change that keeps conv2's slice geometry per tile and forms the fp16 residual in one instruction
(profiles/conv2_front_end_ab.md): that commit's library was built separately and this script ran on it, on one MI355X,

    ISS_LIB=/path/to/that/libiss_hip.so python tests/golden/make_conv2_reuse_bits.py [out.npz]

Per (mode, net, case of tests/conv2_reuse_cases.py): `<key>.p` probabilities (float32 bits), `<key>.f` finite flags, `<key>.wq`
whether conv2 ran on conv_x3_wq_kernel<5,3,...>, and `<key>.same_no_wq`: whether ISS_DIAG_NO_WQ (conv2 on conv_x3_ws_kernel) gave
the same bits on that commit.  The input rows are the `mspec` of conv2_parent_bits.npz.  Run it again only to record another
commit ON PURPOSE, and say which one here.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import conv2_reuse_cases as CR                       # noqa: E402
from inaspeechsegmenter_amd import _native          # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'conv2_reuse_bits.npz')
    print('library:', _native.LIB_PATH)
    mspec = np.load(os.path.join(HERE, 'conv2_parent_bits.npz'))['mspec']
    rec = {}
    for mode in CR.MODES:
        c = CR.context(mode)
        try:
            for net_id in range(len(CR.NETS)):
                for name, feats, rows in CR.cases(mspec, net_id):
                    p, f, kern = CR.run(c, net_id, feats, rows)
                    p2, f2, kern2 = CR.run(c, net_id, feats, rows, no_wq=True)
                    p3, f3, _ = CR.run(c, net_id, feats, rows)
                    assert np.array_equal(p.view(np.uint32), p3.view(np.uint32)) and np.array_equal(f, f3), 'not repeatable'
                    wq = any(k.startswith(CR.CONV2) for k in kern)
                    assert not any(k.startswith(CR.CONV2) for k in kern2), kern2
                    same = bool(np.array_equal(p.view(np.uint32), p2.view(np.uint32)) and np.array_equal(f, f2))
                    k = CR.key(mode, net_id, name)
                    rec[k + '.p'], rec[k + '.f'], rec[k + '.wq'], rec[k + '.same_no_wq'] = p, f, np.bool_(wq), np.bool_(same)
                    print(f'{k}: {len(rows)} windows, {int((~f).sum())} not finite, {CR.groups(net_id, int(f.sum()))} groups, conv2 on wq: {wq}, '
                          f'no_wq same bits: {same}, max |d p| no_wq {float(np.abs(p - p2).max()):.2e}')
        finally:
            c.close()
    np.savez_compressed(out, **rec)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
