"""Dead windows (include/iss.h, iss_cnn_probs): a window that holds a non-finite log-mel value is left out of the CNN passes and
gets its 0.5 / finite = 0 row directly.  Against the compute-then-mask path (ISS_DIAG_NO_SKIP_DEAD) on the same context: `finite`
identical, dead rows exactly 0.5, live rows within 2e-6 with the same arg-max (tile boundaries move with the list, as they do
with the pass size: tests/test_gpu_cnn_defaults.py allows the same figure), bit-identical when no window is dead; against the
float64 oracle the per-mode BOUND of tests/test_gpu_cnn_defaults.py.  On fresh contexts at the shipped defaults (fp16 halves, the
guard on) and on the shared `ctx` (split bf16, guard off)."""
import numpy as np
import pytest

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, _native
from test_gpu_cnn_defaults import BOUND, _fresh, _oracle64, _dlogp, _argmax_agrees

pytestmark = pytest.mark.gpu

NETS = ((21, 3, 1), (24, 2, 2))                      # (mel columns, classes, seed) of the two stand-ins


def _nets():
    out = []
    for nmel, ncls, seed in NETS:
        layers, shp = KM.synthetic_ina_like(nmel, ncls, seed=seed)
        out.append((nmel, layers, KM.compile_layers(layers, shp)))
    return out


def _dead_host(mspec, nmel, rows):
    """The windows the library can prove dead: a non-finite value in the first nmel columns of their 68 rows."""
    bad = np.concatenate([[0], np.cumsum(~np.isfinite(mspec[:, :nmel]).all(axis=1))])
    rows = np.asarray(rows)
    return bad[rows + 68] != bad[rows]


def _both(c, net_id, rows):
    """(p, finite) with dead windows left out, and compute-then-mask, on one context."""
    diag = getattr(c, 'diag', 0)
    p, f = c.cnn_probs(net_id, rows)
    c.set_diag(diag | _native.DIAG_BITS['no_skip_dead'])
    try:
        pm, fm = c.cnn_probs(net_id, rows)
    finally:
        c.set_diag(diag)
    return p, f, pm, fm


def _check(c, net_id, nmel, layers, mspec, rows, oracle_idx=None):
    rows = np.asarray(rows, dtype=np.int32)
    dead = _dead_host(mspec, nmel, rows)
    before = c.cnn_dead_stats()
    p, f, pm, fm = _both(c, net_id, rows)
    after = c.cnn_dead_stats()
    mode = c.cnn_precision_info(net_id)['mode']                       # the arithmetic in use (a fresh context's guard has decided by now)
    dmax = float(np.abs(p - pm)[~dead].max()) if (~dead).any() else 0.0
    print(f'nmel {nmel} {mode}: {len(rows)} windows, {int(dead.sum())} dead, {int((~f).sum())} not finite; '
          f'max |d p| live vs compute-then-mask {dmax:.2e}')
    # (the guard's probes are not counted: one call with the step, one under the switch)
    assert after['windows'] - before['windows'] == 2 * len(rows) and after['dead'] - before['dead'] == int(dead.sum())
    assert np.array_equal(f, fm)
    assert not f[dead].any() and np.all(p[dead] == 0.5) and np.all(p[~f] == 0.5)
    if not dead.any():
        assert np.array_equal(p, pm)
    else:
        assert dmax < 2e-6
        assert np.array_equal(p[f].argmax(1), pm[f].argmax(1))
    idx = np.arange(len(rows)) if oracle_idx is None else np.asarray(oracle_idx)
    lp64, rfin = _oracle64(layers, mspec, nmel, rows[idx])
    assert np.array_equal(f[idx], rfin)
    if rfin.any():
        err = _dlogp(p[idx], lp64, rfin)
        agree, nsure = _argmax_agrees(p[idx], lp64, rfin)
        print(f'nmel {nmel} {mode}: {len(idx)} windows vs float64: max |d log p| {err:.2e}, arg-max on {nsure}')
        assert err < BOUND[mode] and agree
    return p, f, dead


def _cells_mspec(c, rec, T=700):
    """Log-mel rows of the bench generator's audio (the features BOUND was measured on; its own non-finite rows taken out so that
    the layout below is known) with isolated inf / nan / -inf cells in column 22 (dead for the 24-wide net only), one -inf row
    (dead for both), and a stretch of constant rows (std = 0: finite values that do not normalise).  (Random-normal rows in
    place of the generator's were tried first: fp16 halves sit at 1.4e-4 against float64 there, with and without this step alike.)"""
    import bench
    c.set_signal(bench.synth_recording(rec, 40 * 16000, 'cpu').numpy())
    c.sidekit()
    m = c.get_mspec()
    m = m[np.isfinite(m).all(axis=1)][:T].copy()
    assert len(m) == T
    m[100, 22] = np.inf
    m[101, 22] = np.nan
    m[260, 22] = -np.inf
    m[400, :] = -np.inf
    m[520:600, :] = 1.25
    return m


def _irregular(T, rng):
    """Repeats, gaps, descending runs: not the segmenter's own list."""
    a = np.arange(0, T - 68, 2)
    return np.concatenate([a[:40], a[:40], a[::-5], rng.integers(0, T - 67, 100), a[200:260], [T - 68, 0, T - 68]]).astype(np.int32)


def _run_cases(c, ids):
    nets = _nets()
    for k, (nmel, layers, comp) in enumerate(nets):
        c.cnn_load(ids[k], comp)
    rng = np.random.default_rng(11)
    # isolated cells, a constant stretch
    m = _cells_mspec(c, 3)
    T = len(m)
    c.set_mspec(m)
    for k, (nmel, layers, comp) in enumerate(nets):
        rows = S._window_rows(T)
        p, f, dead = _check(c, ids[k], nmel, layers, m, rows)
        col22 = (rows <= 100) & (rows + 68 > 100) & ~((rows <= 400) & (rows + 68 > 400))
        assert col22.any() and np.all(dead[col22] == (nmel == 24))          # column 22: dead for the 24-wide net only
        const = (rows >= 520) & (rows + 68 <= 600)
        assert const.any() and not dead[const].any() and not f[const].any()  # std = 0: not dead, not finite (the device decides)
        _check(c, ids[k], nmel, layers, m, _irregular(T, rng))
        # entirely dead, and entirely live
        alld = np.arange(340, 400, 1, dtype=np.int32)
        p, f, dead = _check(c, ids[k], nmel, layers, m, alld)
        assert dead.all() and np.all(p == 0.5) and not f.any()
        live = np.arange(410, 450, 2, dtype=np.int32)
        p, f, dead = _check(c, ids[k], nmel, layers, m, live)
        assert not dead.any() and f.all()
    # a feature change between two calls: the flags follow it (iss_set_mspec and the front end both)
    m2 = _cells_mspec(c, 4)
    m2[400, :] = m2[399, :]
    m2[30, 3] = np.nan
    c.set_mspec(m2)
    for k, (nmel, layers, comp) in enumerate(nets):
        p, f, dead = _check(c, ids[k], nmel, layers, m2, S._window_rows(T))
        assert dead[0] and not dead[(S._window_rows(T) > 340) & (S._window_rows(T) < 400)].any()
    import bench
    pcm = bench.synth_recording(1, 120 * 16000, 'cpu').numpy()
    c.set_signal(pcm)
    T = c.sidekit()
    m3 = c.get_mspec()
    rows = S._window_rows(T)
    for k, (nmel, layers, comp) in enumerate(nets):
        idx = np.unique(np.concatenate([np.arange(0, len(rows), 13), np.arange(60)]))
        p, f, dead = _check(c, ids[k], nmel, layers, m3, rows, oracle_idx=idx)
        assert dead.any() and (~dead).any(), 'the generator gave no digital silence in two minutes'
    return nets, m3, rows


def test_dead_windows_fresh_context_shipped_defaults():
    """fp16 halves, the guard on (it probes the live list: a list that starts dead still gives it windows to compare)."""
    c = _fresh()
    try:
        nets, m3, rows = _run_cases(c, (0, 1))
        for k in (0, 1):
            info = c.cnn_precision_info(k)
            print(f'net {k}: {info}')
            assert info['state'] in ('passed', 'escalated') and info['slots'] > 0, info
    finally:
        c.close()


def test_guard_probes_live_windows_only():
    """A fresh context whose first call is mostly dead: the all-dead call leaves the guard pending, the next one decides from live
    windows (every probed window is finite, so `slots` is the full probe)."""
    c = _fresh()
    try:
        nmel, layers, comp = _nets()[0]
        c.cnn_load(0, comp)
        rng = np.random.default_rng(3)
        m = rng.normal(-3.0, 1.5, (2000, 24)).astype(np.float32)
        m[0:1200:60, :] = -np.inf                                      # every window that starts below ~1130 is dead
        c.set_mspec(m)
        p, f = c.cnn_probs(0, np.arange(0, 1000, 2, dtype=np.int32))
        assert np.all(p == 0.5) and not f.any() and c.cnn_precision_info(0)['state'] == 'pending'
        rows = np.arange(0, 2000 - 68, 1, dtype=np.int32)
        dead = _dead_host(m, nmel, rows)
        assert dead[:1100].all() and (~dead).sum() >= 256
        p, f = c.cnn_probs(0, rows)
        info = c.cnn_precision_info(0)
        print(f'guard after a call with {int(dead.sum())} of {len(rows)} windows dead: {info}')
        assert info['state'] in ('passed', 'escalated') and info['slots'] == 256, info
        assert np.array_equal(f, ~dead)
    finally:
        c.close()


def test_dead_windows_shared_context(ctx):
    """Split bf16, guard off, the smaller workspace of the shared context; then conv2's credited flops and the two async tickets."""
    nets, m3, rows = _run_cases(ctx, (6, 7))
    for k in range(2):                                               # the BOUND applied was the one of the mode the context was given
        assert ctx.cnn_precision_info(6 + k)['mode'] == {_native.PREC_F16X3: 'f16x3', _native.PREC_F32: 'f32'}.get(ctx.precision, 'bf16x3')
    diag = getattr(ctx, 'diag', 0)
    # flops follow the rows a launch really has: conv2 (the first layer's consumer, conv_x3_wq_kernel<5,3,..>) live / all
    for k, (nmel, layers, comp) in enumerate(nets):
        dead = _dead_host(m3, nmel, rows)

        def conv2_flops():
            ctx.prof_enable(True)
            ctx.prof_reset()
            try:
                ctx.cnn_probs(6 + k, rows)
                inst = [e for e in ctx.prof_instances() if e['kernel'].startswith('conv_x3_wq_kernel<5,3')]
            finally:
                ctx.prof_enable(False)
            assert len(inst) == 1, inst
            return inst[0]['flops']
        fl = conv2_flops()
        ctx.set_diag(diag | _native.DIAG_BITS['no_skip_dead'])
        try:
            fl_all = conv2_flops()
        finally:
            ctx.set_diag(diag)
        print(f'nmel {nmel}: conv2 flops {fl:.6e} live, {fl_all:.6e} all; live share {(~dead).mean():.4f}')
        assert fl_all > 0 and abs(fl / fl_all - (~dead).sum() / len(rows)) < 1e-9
    # both tickets of the dense path in flight together == two synchronous calls
    want = [ctx.cnn_probs(6 + k, rows) for k in range(2)]
    t0, p0, f0 = ctx.cnn_probs_async(6, rows)
    t1, p1, f1 = ctx.cnn_probs_async(7, rows)
    ctx.wait(t0)
    ctx.wait(t1)
    ctx.wait(-1)
    assert np.array_equal(p0, want[0][0]) and np.array_equal(f0.astype(bool), want[0][1])
    assert np.array_equal(p1, want[1][0]) and np.array_equal(f1.astype(bool), want[1][1])
