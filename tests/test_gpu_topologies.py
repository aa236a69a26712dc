"""GPU parity of the CNN engine over the topology sweep (tests/topologies.py): every plausible variant of the
un-vendored nets -- padded / small / large filters, 32..128 channels incl. 48 / 96 (channel-padded), BatchNorm before
or after the activation, big dense heads, pools in odd places -- must match the Keras-semantics oracle to 1e-4 on
probabilities, on the overlapping-window path (shared first layer where it applies) AND on scattered windows, and
through the asynchronous entry.  Plus the BASELINE config-size check: one hour of slots in several passes."""
import os

import numpy as np
import pytest

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, _native
from oracle import keras_cnn as ocnn
import topologies as TP

pytestmark = pytest.mark.gpu


def _mspec(rng, T):
    """log-mel-like rows with slow and fast structure (values around -3 +- 2), a silent gap and a constant stretch."""
    t = np.arange(T)[:, None]
    m = -3 + 1.5 * np.sin(t / 37.0 + np.arange(24)[None, :] / 5.0) + rng.normal(0, 1.2, (T, 24))
    return m.astype(np.float32)


def _oracle_probs(layers, mspec, nmel, rows):
    patches = np.stack([mspec[r:r + 68, :nmel] for r in rows])
    flat = patches.reshape(len(rows), -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        z = (flat - flat.mean(axis=1, keepdims=True)) / flat.std(axis=1, keepdims=True)
    fin = np.all(np.isfinite(z), axis=1)
    z = np.where(fin[:, None], z, 0).reshape(len(rows), 68, nmel, 1).astype(np.float32)
    p = ocnn.forward(layers, z)
    p[~fin] = 0.5
    return p, fin


@pytest.mark.parametrize('name', sorted(TP.SPECS))
def test_topology_parity(ctx, name):
    rng = np.random.default_rng(sum(map(ord, name)))
    T = 1500
    mspec = _mspec(rng, T)
    mspec[700:703, 5] = -np.inf
    ctx.set_mspec(mspec)
    for k, (net, (layers, shp)) in enumerate(sorted(TP.nets(name).items())):
        nmel = shp[1]
        ctx.cnn_load(5, KM.compile_layers(layers, shp))
        rows = S._window_rows(T)                                        # overlapping: the segmenter's own list
        probs, fin = ctx.cnn_probs(5, rows)
        ref, rfin = _oracle_probs(layers, mspec, nmel, rows)
        assert np.array_equal(fin, rfin), (name, net)
        err = np.abs(probs - ref).max()
        ctx.set_diag('no_wq')                                            # the one-wave-per-SIMD kernels (where the topology takes them)
        try:                                                             # accumulate what the kernels they replaced do: same bits
            p_old, f_old = ctx.cnn_probs(5, rows)
        finally:
            ctx.set_diag(0)
        assert np.array_equal(p_old, probs) and np.array_equal(f_old, fin), (name, net, np.abs(p_old - probs).max())
        # round-5 forms of the weight-stationary kernel: the ring form for second convs with more than 16 taps (7x7) and the
        # shared ZERO-PADDED first layer ('same' first conv: S table + per-window edge rows).  Where a topology takes one, it
        # must be the kernel that ran, and switching it off (gather kernel / per-window first layer) must give the same
        # probabilities up to the summation order
        want_new = {'conv2_7x7': 'ring>', 'conv1_same': 'fs>', 'vgg_same_3x3': 'fs>', 'conv1_same_conv2_same': 'fs>',
                    'conv1_same3x3_avg': 'fs>', 'conv2_7x7_same_avg': 'ring>', 'conv2_5x5': 'ring>', 'conv2_4x5_same': 'ring>', 'conv1_same_nopool': 'fs>', 'ch32_64': 'ncb1>', 'ch48_96': 'plain>', 'conv2_stride2': ',2>', 'conv1_same_conv2_stride2': ',2>', 'conv1_pool': ',2>'}.get(name)   # (',2>': conv_x3_kernel<3 | 4,..,2>)
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.cnn_probs(5, rows)
        insts = [i['kernel'] for i in ctx.prof_instances()]
        ctx.prof_enable(False)
        took = [k for k in insts if k.endswith(('ring>', 'fs>', 'ncb1>', 'plain>')) or k.startswith(('conv_x3_kernel<3,', 'conv_x3_kernel<4,'))]
        assert (want_new is None and not took) or (want_new and any(k.endswith(want_new) for k in took)), (name, net, insts)
        if took:
            ctx.set_diag('no_ring,no_fsame,no_ncb1,no_wsu3,no_gfused')
            try:
                p_off, f_off = ctx.cnn_probs(5, rows)
            finally:
                ctx.set_diag(0)
            d_off = np.abs(p_off - probs).max()
            print(f'{name}/{net}: {took[0]} vs the path it replaces: max |dp| {d_off:.2e}')
            assert np.array_equal(f_off, fin) and d_off < 5e-5, (name, net, d_off)
            # ... and in ~10 passes instead of one (per-pass first-layer rows, per-window edge rows and window scalars are
            # indexed relative to the pass): the same probabilities up to where the tile boundaries fall
            prev_limit = getattr(ctx, 'workspace_limit', None) or (24 << 30)
            ctx.set_workspace_limit(64 << 20)
            try:
                p_ch, f_ch = ctx.cnn_probs(5, rows)
            finally:
                ctx.set_workspace_limit(prev_limit)
            assert np.array_equal(f_ch, fin) and np.abs(p_ch - probs).max() < 5e-6, (name, net, np.abs(p_ch - probs).max())
        scat = np.sort(rng.integers(0, T - 68, 64)).astype(np.int32)     # scattered: per-window first layer
        p2, f2 = ctx.cnn_probs(5, scat)
        r2, rf2 = _oracle_probs(layers, mspec, nmel, scat)
        err2 = np.abs(p2 - r2).max()
        # the library's default arithmetic (round 6): fp16 operand halves where a kernel has them, exact f32 for small layers without,
        # bf16 halves elsewhere -- per layer, so every topology mixes them its own way; same finite mask, same tolerance
        ctx.set_precision(_native.PREC_F16X3)
        try:
            p16, f16 = ctx.cnn_probs(5, rows)
            p16s, f16s = ctx.cnn_probs(5, scat)
        finally:
            ctx.set_precision(_native.PREC_BF16X3)
        err16, err16s = np.abs(p16 - ref).max(), np.abs(p16s - r2).max()
        print(f'{name}/{net}: overlapping {err:.2e}, scattered {err2:.2e}; fp16 halves {err16:.2e} / {err16s:.2e}')
        assert err < 1e-4 and err2 < 1e-4 and np.array_equal(f2, rf2), (name, net, err, err2)
        assert err16 < 1e-4 and err16s < 1e-4 and np.array_equal(f16, rfin) and np.array_equal(f16s, rf2), (name, net, err16, err16s)
        # asynchronous entry: same bits, result arrays in page-locked memory
        pp = ctx.pinned_empty((len(rows), probs.shape[1]), np.float32)
        pf = ctx.pinned_empty((len(rows),), np.uint8)
        rows_tmp = rows.copy()
        tk, _, _ = ctx.cnn_probs_async(5, rows_tmp, pp, pf)
        rows_tmp[:] = 0                                                  # the list is consumed before the call returns
        tk2, p3, f3 = ctx.cnn_probs_async(5, scat)                       # a second request queued behind the first
        ctx.wait(tk)
        assert np.array_equal(pp, probs) and np.array_equal(pf.astype(bool), fin)
        ctx.wait(tk2)
        assert np.array_equal(p3, p2) and np.array_equal(f3.astype(bool), f2)
        ctx.pinned_free(pp)
        ctx.pinned_free(pf)


def test_one_hour_of_slots_config_size(ctx):
    """BASELINE.json configs[1] size: 359 998 frames -> 179 999 overlapping slots through both stand-in nets, in ~11
    passes of the default 6 GiB workspace and in 2 passes of a 48 GiB one (large first-layer row buffers and batch
    offsets); 768 sampled slots (pass boundaries and both ends included) against the oracle, and pass-size independence."""
    rng = np.random.default_rng(2024)
    T = 359998
    mspec = _mspec(rng, T)
    mspec[100000:100050, :] = -np.inf
    ctx.set_mspec(mspec)
    rows = S._window_rows(T)
    assert len(rows) == 179999
    for nmel, ncls, seed in ((21, 3, 1), (24, 2, 2)):
        layers, shp = KM.synthetic_ina_like(nmel, ncls, seed=seed)
        ctx.cnn_load(5, KM.compile_layers(layers, shp))
        ctx.set_workspace_limit(6 << 30)
        a, fa = ctx.cnn_probs(5, rows)
        ctx.set_workspace_limit(48 << 30)
        b, fb = ctx.cnn_probs(5, rows)
        ctx.set_workspace_limit(6 << 30)
        assert np.array_equal(fa, fb) and np.abs(a - b).max() < 2e-6      # tile boundaries move with the pass size
        idx = np.unique(np.concatenate((np.arange(0, 40), np.arange(len(rows) - 40, len(rows)),
                                        rng.integers(0, len(rows), 600), np.arange(49990, 50040))))
        ref, rfin = _oracle_probs(layers, mspec, nmel, rows[idx])
        assert np.array_equal(fa[idx], rfin) and (~rfin).sum() > 10
        err = np.abs(a[idx] - ref).max()
        lerr = np.abs(np.log(np.maximum(a[idx], 1e-30)) - np.log(np.maximum(ref, 1e-30)))[ref > 1e-6].max()
        print(f'1 h, nmel {nmel}: max |p_gpu - p_oracle| = {err:.2e}, max |d log p| = {lerr:.2e} over {len(idx)} sampled slots of {len(rows)}')
        # north star: frame logits within 1e-3 of the fp32 reference (log-probabilities are logits up to a common term).
        # The calibrated heads (|W| rms 0.27, tests/golden/make_standin_heads.py) amplify input differences ~2x more than
        # the seeded random ones this bound was first written for (1e-4 on probabilities); the input here is white noise
        assert err < 2e-4 and lerr < 1e-3


_PRECS = (('bf16x3', _native.PREC_BF16X3), ('f16x3', _native.PREC_F16X3), ('f32', _native.PREC_F32))


def _selection_cases(ctx):
    """(case, outputs) of every case tests/golden/kernel_selection.json pins: small runs that between them reach every conv launch
    site.  Consumed one at a time: the caller reads ctx.prof_instances() after each.  Leaves precision, diag and workspace limit
    changed (the caller restores them)."""
    import graph_nets as GN
    import test_gpu_cnn as TC
    from inaspeechsegmenter_amd import vbx as V
    from oracle import vbx as ovbx

    def run(case, fn, prec=_native.PREC_BF16X3, diag=0, limit=24 << 30):
        ctx.set_precision(prec)
        ctx.set_diag(diag)
        ctx.set_workspace_limit(limit)
        ctx.prof_reset()
        out = fn()
        return case, [np.asarray(o) for o in (out if isinstance(out, tuple) else (out,))]

    T = 1500
    for name in sorted(TP.SPECS):                                       # test_topology_parity's inputs
        rng = np.random.default_rng(sum(map(ord, name)))
        mspec = _mspec(rng, T)
        mspec[700:703, 5] = -np.inf
        ctx.set_mspec(mspec)
        rows = S._window_rows(T)
        for net, (layers, shp) in sorted(TP.nets(name).items()):
            ctx.cnn_load(5, KM.compile_layers(layers, shp))
            scat = np.sort(rng.integers(0, T - 68, 64)).astype(np.int32)
            for pname, p in _PRECS:
                yield run(f'topo/{name}/{net}/{pname}/overlapping', lambda: ctx.cnn_probs(5, rows), p)
                yield run(f'topo/{name}/{net}/{pname}/scattered', lambda: ctx.cnn_probs(5, scat), p)
            yield run(f'topo/{name}/{net}/bf16x3/overlapping_64MiB', lambda: ctx.cnn_probs(5, rows), limit=64 << 20)
            if name == 'standin':
                for bit in sorted(_native.DIAG_BITS):
                    if bit != 'no_skip_dead':
                        yield run(f'diag/{bit}/{net}', lambda: ctx.cnn_probs(5, rows), _native.PREC_F16X3, _native.DIAG_BITS[bit])
    for name in sorted(TC.TOPOLOGIES):                                  # test_layer_semantics' inputs at 21 mel
        rng = np.random.default_rng(sum(map(ord, name)) + 21)
        ctx.cnn_load(5, KM.compile_layers(TC.TOPOLOGIES[name](rng, 21), (68, 21, 1)))
        ctx.set_mspec(TC._mspec(rng, 400))
        rows = rng.integers(0, 400 - 68, 301).astype(np.int32)
        for pname, p in _PRECS:
            yield run(f'layers/{name}/{pname}', lambda: ctx.cnn_probs(5, rows), p)
    ex = V.VBxExtractor(ctx, ovbx.resnet101_random_params(0), batch_windows=8)      # test_gpu_vbx's seeded ResNet-101
    fea = np.random.default_rng(9).normal(0, 1, (144 + 24 * 3, 64)).astype(np.float32)
    for pname, p in _PRECS:                                             # (the suite's mode, the library's default, exact f32)
        for dname in ('', 'no_dual', 'no_chain') if p != _native.PREC_F32 else ('',):
            yield run(f'resnet101/{pname}/{dname or "all"}', lambda: ex.get_embeddings(fea, [0, 24, 48], 144), p, _native.diag_flags(dname))
    for name in sorted(GN.NETS):                                        # host-fed (iss_cnn_forward): no patch first layer
        for nmel, ncls in ((21, 3), (24, 2)):
            layers, shp = GN.NETS[name](nmel, ncls, 5)
            ctx.cnn_load(5, KM.compile_layers(layers, shp, patch_input=False))
            x = np.random.default_rng(nmel).normal(0, 1, (5,) + tuple(shp)).astype(np.float32)
            for pname, p in _PRECS:
                yield run(f'graph/{name}/{nmel}/{pname}', lambda: ctx.cnn_forward(5, x), p)


def _selection_run(ctx):
    """{case: {instantiation: launches}} over _selection_cases, the context's settings restored."""
    prev_limit = getattr(ctx, 'workspace_limit', None) or (24 << 30)
    table = {}
    ctx.prof_enable(True)
    try:
        for case, _ in _selection_cases(ctx):
            table[case] = {i['kernel']: int(i['launches']) for i in ctx.prof_instances()}
    finally:
        ctx.prof_enable(False)
        ctx.set_precision(_native.PREC_BF16X3)
        ctx.set_diag(0)
        ctx.set_workspace_limit(prev_limit)
    return table


def test_kernel_selection_is_pinned(ctx, golden):
    """Which kernel instantiation runs each conv row, and how often, over every topology of the sweep (both nets, three arithmetic
    modes, overlapping and scattered windows, several passes), each diagnostic switch on the stand-in, the layer-semantics nets,
    the seeded ResNet-101 and the host-fed graph models: equal to tests/golden/kernel_selection.json, which was recorded before
    kernel selection was split from the launch code.  A kernel change that renames or re-routes an instantiation on purpose
    re-records the file; a refactor of the selection must not."""
    import json
    with open(os.path.join(golden, 'kernel_selection.json')) as f:
        want = json.load(f)
    got = _selection_run(ctx)
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
