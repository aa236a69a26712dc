"""The x-vector ResNet at every last-window width the product runs (10..144 frames, vbx.plan_windows) against the float64 oracle,
on a context with the library's defaults (ISS_PREC_F16X3, 24 GiB workspace, guard on) and features from the device front end.

One arena (iss_vbx_features_batch_pcm16) holds 135 files of w + 24 frames (one last window of width w each, w = 10..144) and two
multi-minute files in shuffled order, then a 20-frame file (no window), so every last window is followed by another file's frames.
For every width three windows -- the arena's first row, that width's last window, the window ending on the arena's last row --
are checked through the device-window entry (iss_vbx_embed) in both split and exact-f32 arithmetic and through the host entry
(iss_cnn_forward); nine windows in one call must equal the same windows one per call, and a program on shared parameters must
equal a full load, bit for bit; the batch path (VBxExtractor.embed_batch) must equal __call__ file by file.

Acceptance rule for one x-vector (test_vbx_widths.check_xvector): finite -> within 1e-4 of the oracle's max |x|; NaN -> only
where the float64 pooled statistics are ill-conditioned (at widths 10..16, where stage 4 is two frames wide, every window is).
"""
import numpy as np
import pytest

import bench
from inaspeechsegmenter_amd import _native, vbx as V, keras_model as KM
from test_gpu_vbx import _fresh_context, _f16_instance
from test_vbx_widths import WIDTHS, check_xvector, ill_conditioned, oracle64
from oracle import vbx as ovbx
from conftest import synth_pcm

pytestmark = pytest.mark.gpu
NET_W, NET_HOST, NET_SHARED = 0, 1, 3                  # (VBxExtractor uses 2 and 4..7)
NET_SRC = 5                                             # the full-width window program, as VBxExtractor loads it: the shared programs' source
SHORT = 20                                              # frames of the file with no window


def _pcm_of_frames(T):
    return 160 * (T - 1) + 80                           # V.frame_count(160 (T - 1) + 80) == T


class Bed:
    """The arena, its host copy, the per-width windows and their float64 oracle."""

    def __init__(self):
        self.c = _fresh_context()
        self.params = KM.synthetic_resnet101(0)
        rng = np.random.default_rng(144)
        src = bench.synth_recording_numpy(3, 16000 * 600)                # speech-like source of the short files
        pcms, names = [], []
        for w in WIDTHS:
            n = _pcm_of_frames(w + 24)
            o = int(rng.integers(0, len(src) - n))
            pcms.append(src[o:o + n])
            names.append(f'tail{w:03}')
        pcms += [synth_pcm(11, 16000 * 150 + 37), bench.synth_recording_numpy(1, 16000 * 130 + 1234)]
        names += ['long150', 'long130']
        order = list(rng.permutation(len(pcms)))
        self.pcms = [pcms[i] for i in order] + [src[:_pcm_of_frames(SHORT)]]
        self.names = [names[i] for i in order] + ['short']
        self.fe = V.FeatureExtractor(self.c)
        self.fe._ensure_dither(max(len(p) for p in self.pcms))
        self.foff, self.arena = self.c.vbx_features_batch_pcm16(self.pcms)
        self.T = int(self.foff[-1])
        assert list(np.diff(self.foff)) == [V.frame_count(len(p)) for p in self.pcms] and np.diff(self.foff)[-1] == SHORT
        self.file_of = {nm: f for f, nm in enumerate(self.names)}
        self.windows = {w: [0, int(self.foff[self.file_of[f'tail{w:03}']]) + 24, self.T - w] for w in WIDTHS}
        self.ref, self.pooled, self.nan32 = {}, {}, {}
        for w in WIDTHS:
            x = self.x(w, self.windows[w])
            self.ref[w], self.pooled[w] = oracle64(self.params, x)
            # the reference's own float32 arithmetic, where the rule allows a NaN (information: printed, not asserted)
            ill = ill_conditioned(self.pooled[w])
            self.nan32[w] = int(np.isnan(ovbx.resnet101_forward(self.params, x[ill])).any(axis=1).sum()) if ill.any() else 0
        src144 = KM.compile_resnet101(self.params, V.FEAT_DIM, V.WINLEN, window_input=True)
        self.blob = src144.blob
        self.c.cnn_load(NET_SRC, src144)

    def x(self, w, starts):
        return np.stack([self.arena[s:s + w].T for s in starts])

    def resident(self):
        """Make the arena the resident features again (a per-file front-end call replaces them)."""
        foff, _ = self.c.vbx_features_batch_pcm16(self.pcms, to_host=False)
        assert np.array_equal(foff, self.foff)

    def program(self, w, window=True):
        comp = KM.compile_resnet101(self.params, V.FEAT_DIM, w, window_input=window)
        assert np.array_equal(comp.blob, self.blob)
        comp.blob = self.blob                                          # one copy of the 63 MB of parameters on the host
        return comp


@pytest.fixture(scope='module')
def bed():
    b = Bed()
    yield b
    b.c.close()


def _check_widths(bed, name, run):
    """run(w) -> (3, 256) x-vectors of bed.windows[w]; every window against the acceptance rule."""
    bad, worst, nans = [], (0.0, None), {}
    for w in WIDTHS:
        got = run(w)
        nans[w] = 0
        for i, s in enumerate(bed.windows[w]):
            ok, err = check_xvector(got[i], bed.ref[w][i], bed.pooled[w][i])
            nans[w] += int(np.isnan(err))
            if not ok:
                bad.append((w, s, err))
            elif err > worst[0]:
                worst = (err, (w, s))
    shown = [w for w in WIDTHS if nans[w] or bed.nan32[w]]
    print(f'\n{name}: worst per-window error {worst[0]:.2e} of the window\'s max |x| (width, start {worst[1]}); '
          f'NaN windows (device / torch-f32 of 3) ' + ', '.join(f'{w}: {nans[w]}/{bed.nan32[w]}' for w in shown))
    assert not bad, f'{name}: windows outside the rule (width, start, error): {bad}'


def test_device_window_entry_every_width(bed):
    """A: iss_vbx_embed on a full load of every width's program, the library's default arithmetic (bf16 halves for this net)."""
    c = bed.c
    bed.resident()
    sets = {}

    def run(w):
        c.cnn_load(NET_W, bed.program(w))
        c.prof_enable(True)
        c.prof_reset()
        try:
            out = c.vbx_embed(NET_W, bed.windows[w])
            sets[w] = frozenset(e['kernel'] for e in c.prof_instances())
        finally:
            c.prof_enable(False)
        assert c.cnn_precision_info(NET_W)['mode'] == 'bf16x3', w
        assert not [k for k in sets[w] if _f16_instance(k)], (w, sorted(sets[w]))
        return out

    _check_widths(bed, 'iss_vbx_embed, bf16x3', run)
    ranges = []
    for w in WIDTHS:
        if ranges and sets[ranges[-1][1]] == sets[w] and ranges[-1][1] == w - 1:
            ranges[-1][1] = w
        else:
            ranges.append([w, w])
    distinct = sorted(set(sets.values()), key=lambda s: min(w for w in WIDTHS if sets[w] == s))
    print(f'{len(distinct)} kernel sets over widths 10..144:')
    for k, s in enumerate(distinct):
        print(f'  set {k} ({len(s)} instances): widths ' + ', '.join(f'{a}-{b}' if a != b else f'{a}' for a, b in ranges
                                                                   if sets[a] == s))
        if k:
            print('    vs set 0: +', sorted(s - distinct[0]), ' -', sorted(distinct[0] - s))
    assert len(distinct) > 1


def test_host_entry_every_width(bed):
    """B: iss_cnn_forward (window_input=False: the host stacks the windows) at every width."""
    c = bed.c

    def run(w):
        c.cnn_load(NET_HOST, bed.program(w, window=False))
        return c.cnn_forward(NET_HOST, bed.x(w, bed.windows[w])[..., None].astype(np.float32))

    _check_widths(bed, 'iss_cnn_forward, bf16x3', run)


def test_exact_f32_every_width(bed):
    """C: iss_vbx_embed in the exact-f32 arithmetic (ISS_PREC_F32) at every width."""
    c = bed.c
    bed.resident()

    def run(w):
        c.cnn_load(NET_W, bed.program(w))
        out = c.vbx_embed(NET_W, bed.windows[w])
        assert c.cnn_precision_info(NET_W)['mode'] == 'f32', w
        return out

    c.set_precision(_native.PREC_F32)
    try:
        _check_widths(bed, 'iss_vbx_embed, f32', run)
    finally:
        c.set_precision(_native.PREC_F16X3)


def _instances(c, run):
    c.prof_enable(True)
    c.prof_reset()
    try:
        return run(), frozenset(e['kernel'] for e in c.prof_instances())
    finally:
        c.prof_enable(False)


def test_pass_composition_every_width(bed):
    """D: nine windows of one width over nine files in one call (the last row tile partial) == each window alone, bit for bit
    (NaN where NaN), through the same kernel instances; the program on the full-width program's parameters (iss_cnn_load_shared,
    what embed_batch runs) == a full load of the same width.  (A footprint kernel once fitted a 1-window call's single tile at
    every width and not the 9-window call's: __call__'s lone last window and embed_batch's grouped ones ran different kernels.)"""
    c = bed.c
    bed.resident()
    rng = np.random.default_rng(9)
    bad = []
    for w in WIDTHS:
        files = rng.choice(len(bed.names) - 1, 9, replace=False)
        starts = [min(int(bed.foff[f]) + int(rng.integers(0, 24)), bed.T - w) for f in files]
        comp = bed.program(w)
        c.cnn_load(NET_W, comp)
        together, k9 = _instances(c, lambda: c.vbx_embed(NET_W, starts))
        alone, k1 = _instances(c, lambda: np.concatenate([c.vbx_embed(NET_W, [s]) for s in starts]))
        comp.blob = None
        c.cnn_load_shared(NET_SHARED, NET_SRC, comp)
        shared = c.vbx_embed(NET_SHARED, starts)
        if not np.array_equal(together, alone, equal_nan=True) or k1 != k9:
            diff = [i for i in range(9) if not np.array_equal(together[i], alone[i], equal_nan=True)]
            bad.append((w, 'alone', diff, sorted(k1 - k9), sorted(k9 - k1)))
        if not np.array_equal(shared, together, equal_nan=True):
            bad.append((w, 'shared'))
    for b in bad:
        print(b)
    assert not bad, f'widths {[b[0] for b in bad]}'


def test_batch_path_every_width(bed):
    """E: VBxExtractor.embed_batch on the arena == __call__ on every file's own resident features (keys, times, the windows
    dropped for NaN, x-vector bits); every last window and a sample of full windows within the rule against the oracle."""
    c = bed.c
    bed.resident()
    ex = V.VBxExtractor(c, bed.params)
    counts = list(np.diff(bed.foff))
    durs = [len(p) / V.SR for p in bed.pcms]
    plan = V.plan_windows(counts, durs, bed.names)
    _, files, full, tails = plan
    assert sorted(tails) == list(WIDTHS)
    got = ex.embed_batch(plan)
    assert len(got) == len(bed.names) and got[-1] == [] and files[-1] == []

    for f, (pcm, name, dur) in enumerate(zip(bed.pcms, bed.names, durs)):
        want = ex(name, bed.fe(pcm, to_host=False), dur)
        assert [k for k, _, _ in got[f]] == [k for k, _, _ in want], name
        assert [t for _, t, _ in got[f]] == [t for _, t, _ in want], name
        assert all(np.array_equal(a[2], b[2]) for a, b in zip(got[f], want)), name

    # the oracle: every last window (dropped = NaN), the first and last full window of every file and 1 % of the others
    rng = np.random.default_rng(3)
    checks, bad = [], []
    for f, wins in enumerate(files):
        emb = {k: x for k, _, x in got[f]}
        nfull = sum(1 for *_, slot in wins if not isinstance(slot, tuple))
        for i, (key, _, slot) in enumerate(wins):
            if isinstance(slot, tuple):
                checks.append((key, int(tails[slot[0]][slot[1]]), slot[0], emb.get(key)))
            elif i in (0, nfull - 1) or rng.random() < 0.01:
                checks.append((key, int(full[slot]), V.WINLEN, emb.get(key)))
    for w in sorted({w for _, _, w, _ in checks}):
        group = [(k, s, x) for k, s, ww, x in checks if ww == w]
        ref, pooled = oracle64(bed.params, bed.x(w, [s for _, s, _ in group]))
        for (key, s, x), r, p in zip(group, ref, pooled):
            x10 = np.full(V.EMBED_DIM, np.nan, np.float32) if x is None else x      # x-vectors come out x 10 (:246)
            ok, err = check_xvector(x10, 10 * r, p)
            if not ok:
                bad.append((key, w, err))
    dropped = {w: sum(1 for _, _, ww, x in checks if ww == w and x is None) for w in range(10, 17)}
    print(f'\nembed_batch: {len(checks)} windows checked against the oracle; last windows dropped for NaN at widths 10..16: {dropped}')
    assert not bad, bad


def test_window_start_bounds(bed):
    """F: a window must lie inside the resident frames: starts -1 and T - w + 1 are refused, T - w is taken."""
    c = bed.c
    bed.resident()
    w = 65
    c.cnn_load(NET_W, bed.program(w))
    for s in (-1, bed.T - w + 1):
        with pytest.raises(_native.NativeError, match='outside'):
            c.vbx_embed(NET_W, [0, s])
    assert c.vbx_embed(NET_W, [bed.T - w]).shape == (1, V.EMBED_DIM)
