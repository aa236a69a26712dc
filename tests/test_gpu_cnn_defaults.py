"""The segmenter CNNs at the library's shipped defaults (ISS_PREC_F16X3, the precision guard on, passes sized to the 24 GiB
workspace and the 2^31-element cap), against the float64 oracle (oracle/keras_cnn.py, dtype=np.float64, log=True).  The shared
`ctx` fixture runs another configuration (split bf16, guard off, a smaller workspace): every test here builds fresh contexts and
closes them.  Errors are max |log p - log p64| over the finite windows' classes with p64 > 1e-30 (the softmax squashes errors in p).
Also: the mode a network runs is the mode the caller asked for (iss_set_precision re-arms the guard's decision; a caller's
iss_cnn_set_net_precision survives it), and a small layer demoted to exact f32 in fp16 mode is not handed the CHL layout."""
import time

import numpy as np
import pytest

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, _native
from oracle import keras_cnn as ocnn
import topologies

pytestmark = pytest.mark.gpu

# the fp16-operand instantiations of the segmenter nets' kernels (tests/test_gpu_cnn.py _F16_KERNELS)
F16_KERNELS = {'conv_x3_wq_kernel<5,3,true,true>', 'conv_x3_wq3h_kernel<0,true,true>', 'conv_x3_wq3h_kernel<1,true,true>',
               'conv_dhl_kernel<true,8>'}
CONV2_F16 = 'conv_x3_wq_kernel<5,3,true,true>'      # the first layer's consumer: one launch per pass
# max |d log p| against float64 per mode.  F32: an fmaf chain, float32 rounding only (the float32 oracle itself sits at 2e-5 on the
# stand-in, tests/test_oracle_cnn64.py); F16X3: the figure test_f16x3_mode holds against float32; BF16X3: the north star
BOUND = {'f32': 5e-5, 'f16x3': 1e-4, 'bf16x3': 1e-3}
# the hot net below: logits ~6 x the stand-in's, and its errors with them (f16x3 measured 1.9e-4)
BOUND_HOT = {k: 6 * v for k, v in BOUND.items()}
MODES = {'f16x3': _native.PREC_F16X3, 'f32': _native.PREC_F32, 'bf16x3': _native.PREC_BF16X3}


def _fresh():
    from inaspeechsegmenter_amd import tables
    c = _native.Context(0)
    c.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank())
    return c


def _oracle64(layers, mspec, nmel, rows):
    """float64 log p of the given windows (z-normalised in float64) and their finite mask."""
    patches = np.stack([mspec[r:r + 68, :nmel] for r in rows]).astype(np.float64)
    flat = patches.reshape(len(rows), -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        z = (flat - flat.mean(axis=1, keepdims=True)) / flat.std(axis=1, keepdims=True)
    fin = np.all(np.isfinite(z), axis=1)
    z = np.where(fin[:, None], z, 0).reshape(len(rows), 68, nmel, 1)
    return ocnn.forward(layers, z, dtype=np.float64, log=True), fin


def _dlogp(p, lp64, fin):
    ok = fin[:, None] & (lp64 > np.log(1e-30))
    with np.errstate(divide='ignore'):
        return float(np.abs(np.log(p.astype(np.float64)) - lp64)[ok].max())


def _argmax_agrees(p, lp64, fin):
    s = np.sort(lp64, axis=1)
    sure = fin & (s[:, -1] - s[:, -2] > 1e-3)
    return bool(np.array_equal(p.argmax(1)[sure], lp64.argmax(1)[sure])), int(sure.sum())


def _probs(c, net_id, rows):
    """(probs, finite, {kernel instance: launches}) of one iss_cnn_probs call."""
    c.prof_enable(True)
    c.prof_reset()
    try:
        p, f = c.cnn_probs(net_id, rows)
        return p, f, {e['kernel']: e['launches'] for e in c.prof_instances()}
    finally:
        c.prof_enable(False)


def _plan_chunk(comp, total, ws=24 << 30):
    """Host restatement of cnn.hip plan_chunk: windows per pass, and the largest buffer's floats per window."""
    be = [int(v) for v in comp.buf_elems]
    bc = min(ws // (sum(be) * 4), total, ((1 << 31) - 1) // max(be))
    if bc > 8:
        bc -= bc % 8
    return bc, max(be)


def test_one_hour_default_precision_production_passes():
    """One hour of the bench generator's audio (silence, noise, voiced sources, chords; -inf mel rows) through both stand-in nets
    over all 179 999 slots, one iss_cnn_probs call per net, on a context that keeps every library default: the guard probes and
    keeps fp16 halves, the fp16 kernels run, the passes are the cap-sized ones plan_chunk makes, and sampled windows (every pass's
    edges, both ends, a run across non-finite windows, 300 random) match float64 within the F16X3 bound; a 1 GiB workspace (many
    passes) gives the same probabilities to 2e-6 (tile boundaries move with the pass size)."""
    import bench
    c = _fresh()
    c2 = _fresh()
    try:
        pcm = bench.synth_recording(0, 3600 * 16000, 'cpu').numpy()
        c.set_signal(pcm)
        T = c.sidekit()
        mspec = c.get_mspec()
        rows = S._window_rows(T)
        assert len(rows) == 179999, (T, len(rows))
        c2.set_workspace_limit(1 << 30)
        c2.set_mspec(mspec)
        N = len(rows)
        for net_id, (nmel, ncls, seed) in enumerate(((21, 3, 1), (24, 2, 2))):
            layers, shp = KM.synthetic_ina_like(nmel, ncls, seed=seed)
            comp = KM.compile_layers(layers, shp)
            c.cnn_load(net_id, comp)
            assert c.cnn_precision_info(net_id)['state'] == 'pending'
            p, fin, first = _probs(c, net_id, rows)
            info = c.cnn_precision_info(net_id)
            p_again, fin_again, launches = _probs(c, net_id, rows)        # decided: no probe, the same arithmetic
            bc, emax = _plan_chunk(comp, N)
            passes = -(-N // bc)
            print(f'nmel {nmel}: guard {info}; {bc} windows per pass, {passes} passes, largest buffer {bc * emax} floats '
                  f'({emax} per window); launches {launches}')
            assert info['state'] in ('passed', 'escalated') and info['slots'] > 100 and info['mode'] == 'f16x3', info
            assert F16_KERNELS <= set(first) and F16_KERNELS <= set(launches), sorted(first)
            assert np.array_equal(p_again, p) and np.array_equal(fin_again, fin)
            assert launches[CONV2_F16] == passes, (launches, passes)
            assert bc * emax < 1 << 31 and (bc + 8) * emax >= 1 << 31            # cap-sized: the 2^31-element cap binds
            # sampled windows against float64
            rng = np.random.default_rng(2026 + net_id)
            idx = set(range(40)) | set(range(N - 40, N)) | set(rng.choice(N, 300, replace=False).tolist())
            for k in range(passes):
                s, e = k * bc, min(k * bc + bc, N) - 1
                idx |= {s - 1, s, s + 1, e - 1, e, e + 1}
            edge = np.flatnonzero(fin[:-1] & ~fin[1:])                          # a finite -> non-finite transition
            assert len(edge), 'no non-finite window in an hour of the generator'
            idx |= set(range(int(edge[0]) - 20, int(edge[0]) + 20))
            idx = np.array(sorted(i for i in idx if 0 <= i < N))
            t0 = time.time()
            lp64, rfin = _oracle64(layers, mspec, nmel, rows[idx])
            t_or = time.time() - t0
            err = _dlogp(p[idx], lp64, rfin)
            agree, nsure = _argmax_agrees(p[idx], lp64, rfin)
            print(f'nmel {nmel}: {len(idx)} windows ({(~rfin).sum()} non-finite) vs float64: max |d log p| {err:.2e}; '
                  f'arg-max on {nsure}; float64 oracle {t_or:.1f} s CPU')
            assert np.array_equal(fin[idx], rfin) and (~rfin).sum() > 0
            assert err < BOUND['f16x3'] and agree
            # pass-size independence
            c2.cnn_load(net_id, comp)
            p2, fin2 = c2.cnn_probs(net_id, rows)
            bc2, _ = _plan_chunk(comp, N, 1 << 30)
            print(f'nmel {nmel}: 1 GiB workspace: {-(-N // bc2)} passes, max |d p| {np.abs(p2 - p).max():.2e}')
            assert -(-N // bc2) > 50 and c2.cnn_precision_info(net_id)['mode'] == 'f16x3'
            assert np.array_equal(fin2, fin) and np.abs(p2 - p).max() < 2e-6
    finally:
        c.close()
        c2.close()


def _hot(layers):
    """The stand-in with its last two layers x 2.5 (test_precision_guard_escalates_a_net_with_inflated_activation_range): split bf16
    is too coarse for it, fp16 halves are not."""
    hot = [dict(L) for L in layers]
    for i in (-2, -1):
        hot[i]['W'] = (hot[i]['W'] * 2.5).astype(np.float32)
        hot[i]['b'] = (hot[i]['b'] * 2.5).astype(np.float32)
    return hot


def test_mode_in_use_is_the_mode_asked_for():
    """One context at the library defaults; the stand-in (id 3) switched F16X3 -> F32 -> BF16X3 -> F16X3, the hot net (id 4) first
    run in BF16X3 (the guard escalates it to fp16 halves) then switched to F32 and back to F16X3, and a stand-in whose first call
    ran in F32 (id 5) switched to F16X3.  After every switch: the reported mode is the one asked for (or the guard's documented
    escalation), a split mode was probed again, the kernels fit the mode, the probabilities are bit-identical to a fresh context
    that started in that mode, and the error against float64 is within the mode's bound.  A caller's per-network override survives
    iss_set_precision and is never probed."""
    import bench
    pcm = bench.synth_recording(0, 60 * 16000, 'cpu').numpy()
    layers, shp = KM.synthetic_ina_like(21, 3, seed=1)
    hot = _hot(layers)
    comp, comp_hot = KM.compile_layers(layers, shp), KM.compile_layers(hot, shp)
    c = _fresh()
    refs = {}
    try:
        c.set_signal(pcm)
        T = c.sidekit()
        mspec = c.get_mspec()
        rows = S._window_rows(T)
        # fresh contexts that start in each mode (the guard at its default): what each switch must reproduce bit for bit
        want = {}
        for mode in ('f16x3', 'f32', 'bf16x3'):
            r = refs[mode] = _fresh()
            if mode != 'f16x3':
                r.set_precision(MODES[mode])
            r.set_mspec(mspec)
            r.cnn_load(3, comp)
            r.cnn_load(4, comp_hot)
            want[mode, 3] = r.cnn_probs(3, rows)[0]
            want[mode, 4] = r.cnn_probs(4, rows)[0]
            print(f'fresh {mode}: stand-in {r.cnn_precision_info(3)}, hot {r.cnn_precision_info(4)}')
        rng = np.random.default_rng(7)
        idx = np.unique(np.concatenate((np.arange(0, 20), rng.choice(len(rows), 240, replace=False))))
        lp64 = {3: _oracle64(layers, mspec, 21, rows[idx]), 4: _oracle64(hot, mspec, 21, rows[idx])}
        figures = []

        def check(net_id, asked, mode, probed=True):
            p, fin, used = _probs(c, net_id, rows)
            info = c.cnn_precision_info(net_id)
            lp, rfin = lp64[4 if net_id == 4 else 3]
            err = _dlogp(p[idx], lp, rfin)
            figures.append((net_id, asked, info['mode'], err))
            print(f'net {net_id}, asked {asked}: {info}; max |d log p| vs float64 {err:.2e}; kernels {sorted(used)}')
            assert info['mode'] == mode, (net_id, asked, info)
            if probed:
                assert info['state'] != 'fixed' and info['slots'] > 0, info
            if mode == 'f32':
                assert sum(k.endswith('f32>') for k in used) == 3 and not (F16_KERNELS & set(used)), sorted(used)
            elif mode == 'bf16x3':
                assert not (F16_KERNELS & set(used)), sorted(used)
            else:
                assert F16_KERNELS <= set(used), sorted(used)
            assert np.array_equal(fin[idx], rfin)
            assert np.array_equal(p, want[asked, 4 if net_id == 4 else 3]), (net_id, asked, np.abs(p - want[asked, 4 if net_id == 4 else 3]).max())
            assert err < (BOUND_HOT if net_id == 4 else BOUND)[mode], (net_id, asked, err)
            return p

        c.cnn_load(3, comp)
        check(3, 'f16x3', 'f16x3')                                       # the library default
        c.set_precision(_native.PREC_F32)
        check(3, 'f32', 'f32', probed=False)
        c.cnn_load(5, comp)                                              # a first call in exact f32: 'fixed'
        p5 = c.cnn_probs(5, rows)[0]
        assert c.cnn_precision_info(5)['state'] == 'fixed' and np.array_equal(p5, want['f32', 3])
        c.set_precision(_native.PREC_BF16X3)
        check(3, 'bf16x3', 'bf16x3')
        c.cnn_load(4, comp_hot)
        check(4, 'bf16x3', 'f16x3')                                      # escalated: fp16 halves pass where bf16 ones do not
        assert c.cnn_precision_info(4)['state'] == 'escalated'
        c.set_precision(_native.PREC_F32)
        check(4, 'f32', 'f32', probed=False)                             # not the guard's f16x3 any more
        check(3, 'f32', 'f32', probed=False)
        c.set_precision(_native.PREC_F16X3)
        check(4, 'f16x3', 'f16x3')                                       # probed again in the mode asked for
        check(3, 'f16x3', 'f16x3')
        # id 5 was 'fixed' by its exact-f32 first call: probed now, like any other network
        p5, f5, used5 = _probs(c, 5, rows)
        info5 = c.cnn_precision_info(5)
        print('first call in f32, then f16x3:', info5)
        assert info5['mode'] == 'f16x3' and info5['state'] == 'passed' and info5['slots'] > 0, info5
        assert F16_KERNELS <= set(used5) and np.array_equal(p5, want['f16x3', 3])
        # the caller's own choice survives a mode change and is never probed
        c.cnn_set_net_precision(3, _native.PREC_BF16X3)
        c.set_precision(_native.PREC_F32)
        pf = c.cnn_probs(3, rows)[0]
        info = c.cnn_precision_info(3)
        assert info['mode'] == 'bf16x3' and info['state'] == 'fixed' and np.array_equal(pf, want['bf16x3', 3]), info
        c.set_precision(_native.PREC_F16X3)
        assert c.cnn_precision_info(3)['state'] == 'fixed' and c.cnn_precision_info(3)['mode'] == 'bf16x3'
        c.cnn_set_net_precision(3, -1)
        assert c.cnn_precision_info(3)['state'] == 'pending' and c.cnn_precision_info(3)['mode'] == 'f16x3'
        print('float64 figures (net, asked, mode, max |d log p|):', [(n, a, m, f'{e:.2e}') for n, a, m, e in figures])
    finally:
        c.close()
        for r in refs.values():
            r.close()


# a pooled-relu conv (3 x 3, 14 x 9 -> 12 x 7, 2 x 2 max-pool -> 6 x 3) in front of a 3 x 3 128 -> 128 bias + relu conv on that tiny
# map (-> 4 x 1, 1.2 MFLOP: under 2e6 and under 0.5 % of the net's ~324 MFLOP): in fp16 mode that conv is demoted to exact f32
SMALL_TAIL = [('conv', 4, 5, 64), ('bn_relu',), ('conv', 5, 3, 128), ('bn_relu',), ('maxpool', 2, 2),    # 61 x 18 -> 30 x 9
              ('conv', 3, 1, 128), ('relu',), ('maxpool', 2, 1),                                       # 28 x 9 -> 14 x 9
              ('conv', 3, 3, 128), ('relu',), ('maxpool', 2, 2),                                       # 12 x 7 -> 6 x 3
              ('conv', 3, 3, 128), ('relu',),                                                          # 4 x 1
              ('flatten',), ('dense', 64)]


def test_small_demoted_layer_is_not_handed_the_chl_layout():
    """A pooled-relu producer in front of a 3 x 3, stride-1, 128 -> 128 bias + relu conv small enough to be demoted to exact f32 in
    fp16 mode (conv_igemm_kernel).  The producer may hand its output over in the CHL layout only to a conv_x3_wq3h_kernel launch
    (want_hl_out), and the producer asks the consumer's own selection (select_conv), demotion included, so a demoted consumer is never handed CHL
    (it used to be possible in principle: "internal: row N reads a CHL tensor on a kernel that expects f32").  On this map the
    hand-over is not taken in either mode: a tile of the one-wave-per-SIMD kernel (192 - 256 output pixels) over 4 x 1 outputs
    reads a 4.5 x larger footprint than its 512-pixel capacity (and the weight-stationary kernel's 2 x) -- the same footprint
    test blocks every layer small enough to be demoted.  Both modes run, at the defaults, within their float64 bounds."""
    import bench
    nmel = 24
    layers, shp = topologies.build(SMALL_TAIL, nmel, 2, seed=11)
    comp = KM.compile_layers(layers, shp)
    fl = ocnn.flops_per_sample(layers, shp)
    assert 2 * 9 * 128 * 128 * 4 < min(2e6, 0.005 * fl), fl
    pcm = bench.synth_recording(2, 30 * 16000, 'cpu').numpy()
    c, b = _fresh(), _fresh()
    try:
        c.set_signal(pcm)
        T = c.sidekit()
        mspec = c.get_mspec()
        rows = S._window_rows(T)
        rng = np.random.default_rng(3)
        idx = np.unique(np.concatenate((np.arange(0, 10), rng.choice(len(rows), 200, replace=False))))
        lp, rfin = _oracle64(layers, mspec, nmel, rows[idx])
        b.set_precision(_native.PREC_BF16X3)
        b.set_precision_guard(0)                                         # (split bf16 whatever its probe would say: the hand-over)
        b.set_mspec(mspec)
        b.cnn_load(0, comp)
        pb, fb, ub = _probs(b, 0, rows)
        c.cnn_load(0, comp)                                              # library defaults: fp16 halves
        ph, fh, uh = _probs(c, 0, rows)
        ih, ib = c.cnn_precision_info(0), b.cnn_precision_info(0)
        eh, eb = _dlogp(ph[idx], lp, rfin), _dlogp(pb[idx], lp, rfin)
        print(f'net flops {fl / 1e6:.0f} M; bf16x3 {ib} {eb:.2e}: {sorted(ub)}\nf16x3 {ih} {eh:.2e}: {sorted(uh)}')
        assert ih['mode'] == 'f16x3' and ib['mode'] == 'bf16x3', (ih, ib)
        assert not [k for k in uh if k.startswith('conv_x3_wq3h_kernel<0,')], sorted(uh)
        assert any(k.startswith('conv_igemm_kernel') for k in uh), sorted(uh)    # the demoted layers: exact f32
        assert np.array_equal(fh[idx], rfin) and np.array_equal(fb[idx], rfin)
        assert eh < BOUND['f16x3'] and eb < BOUND[ib['mode']]
    finally:
        c.close()
        b.close()
