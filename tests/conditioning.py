"""Ill-conditioned log-mel windows for the window-normalised first layer (tests/test_conditioning.py on the host,
tests/test_gpu_conditioning.py on the device).  Host code only: numpy and the oracle.

The segmenter nets read z = (x - mean_b) / std_b of each 68-row window b.  The per-window first layer forms z and then convolves
(the reference's order, segmenter.py:82-88); the shared first layer convolves the RAW rows once per log-mel row and the consumer
applies relu(R * rstd + (bias - mean * rstd * S)) -- a difference of two numbers each about |mean| / std times the result, so the
float32 rounding of R is amplified by that ratio.  Every other parity test draws rows with |mean| / std ~ 2; the only real
features of the suite (musanmix_mspec) reach 18.  CASES walks the ratio from 2 to 2000: quiet (dither: 11) and spectrally flat
(brown noise: 26) audio sits in the middle of the ladder.
"""
import functools

import numpy as np

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S
from oracle import keras_cnn as ocnn
import topologies as TP

T = 400
# (mean, std) of the whole array; |mean| / std = 2 (control), 18 (musanmix's worst window), 26 (brown noise), 40, 64, 100, 200, 2000
CASES = [(-3.0, 1.9), (-13.3, 0.72), (-12.6, 0.48), (-20.0, 0.5), (-20.0, 0.3125), (5.0, 0.05), (-20.0, 0.1), (-20.0, 0.01)]
# the bound that holds at ratios real audio is known to reach (<= 64) and on `mixed`: the suite's tolerance on probabilities
PROB_TOL = 1e-4
# ... and the condition under which the relative bound PROB_TOL + REF_MARGIN * e_ref means anything: the float32 reference itself
# within REF_CAP of float64 (measured: 3.1e-4 at ratio 2000 on conv1_same, <= 1.2e-5 at ratios <= 64)
REF_CAP = 5e-4
# An implementation that normalises in float32 differs from the reference in how mean and std are rounded: each within 1 ulp of the
# reference's, worth about 2 x the reference's own error; doubled for the other summation order of the first convolution
REF_MARGIN = 4.0


def ratio(case):
    return abs(case[0]) / case[1]


def case_id(case):
    return case if isinstance(case, str) else f'm{case[0]:g}_s{case[1]:g}'


def _pattern(T, seed):
    """The rows the topology tests draw (slow sine across time and bands + white noise), zero mean and unit variance over the array."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    b = 1.5 * np.sin(t / 37.0 + np.arange(24)[None, :] / 5.0) + rng.normal(0, 1.2, (T, 24))
    return (b - b.mean()) / b.std()


def make_mspec(mean, std, T=T, seed=2026):
    """float32 (T, 24) log-mel-like rows mean + std * b, b = _pattern (float64) before the cast."""
    return (mean + std * _pattern(T, seed)).astype(np.float32)


def mixed():
    """Two regimes on one recording: rows 0..199 quiet (-20, 0.3125; ratio 64), rows 200..399 ordinary (-3, 1.9), three -inf values
    in between.  Neighbouring windows on the same shared rows carry very different affine maps, one region is non-finite."""
    m = make_mspec(-3.0, 1.9)
    m[:200] = make_mspec(-20.0, 0.3125)[:200]
    m[120:123, 5] = -np.inf
    return m


def mspec_of(case):
    return mixed() if isinstance(case, str) else make_mspec(*case)


def window_ratios(mspec, nmel, rows):
    """|mean| / std of every window in float64 (nan for a non-finite window)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        flat = np.stack([mspec[r:r + 68, :nmel] for r in rows]).reshape(len(rows), -1).astype(np.float64)
        return np.abs(flat.mean(axis=1)) / flat.std(axis=1)


def _per_unique(rows, fn):
    """fn(unique rows) -> per-row arrays expanded to `rows` (the segmenter's list repeats its first and last window 17 / 16 times)."""
    u, inv = np.unique(np.asarray(rows), return_inverse=True)
    return tuple(a[inv] for a in fn(u))


def truth(layers, mspec, nmel, rows):
    """float64 all the way from the float32 rows: window mean and population std, the normalisation and the network.
    -> (probabilities float64 with non-finite windows at 0.5, finite mask)."""
    def run(u):
        flat = np.stack([mspec[r:r + 68, :nmel] for r in u]).reshape(len(u), -1).astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            z = (flat - flat.mean(axis=1, keepdims=True)) / flat.std(axis=1, keepdims=True)
        fin = np.all(np.isfinite(z), axis=1)
        z = np.where(fin[:, None], z, 0).reshape(len(u), 68, nmel, 1)
        p = ocnn.forward(layers, z, dtype=np.float64)
        p[~fin] = 0.5
        return p, fin
    return _per_unique(rows, run)


def reference32(layers, mspec, nmel, rows):
    """The Keras float32 semantics every other parity test compares with: float32 mean / std of the window (segmenter.py:82),
    float32 normalisation, float32 network.  -> (probabilities float32 with non-finite windows at 0.5, finite mask)."""
    def run(u):
        flat = np.stack([mspec[r:r + 68, :nmel] for r in u]).reshape(len(u), -1)
        with np.errstate(invalid='ignore', divide='ignore'):
            z = (flat - flat.mean(axis=1, keepdims=True)) / flat.std(axis=1, keepdims=True)
        fin = np.all(np.isfinite(z), axis=1)
        z = np.where(fin[:, None], z, 0).reshape(len(u), 68, nmel, 1).astype(np.float32)
        p = ocnn.forward(layers, z)
        p[~fin] = 0.5
        return p, fin
    return _per_unique(rows, run)


# The four forms of the shared first layer: name -> (build the net, the conv instantiation that consumes the shared rows in the
# split-operand modes, as iss_prof_get_instance spells it).  'vad' is the first net of a topology (21 mel, 3 classes).
NETS = {
    'standin21': (lambda: KM.synthetic_ina_like(21, 3, seed=3), 'conv_x3_wq_kernel<5,3,'),         # valid 4x5: first_layer_rows_kernel<4,5,17>
    'standin24': (lambda: KM.synthetic_ina_like(24, 2, seed=3), 'conv_x3_wq_kernel<5,3,'),         # valid 4x5: first_layer_rows_kernel<4,5,20>
    'conv1_same': (lambda: TP.nets('conv1_same')['vad'], 'conv_x3_ws_kernel<5,3,'),                # first_layer_same_kernel + first_layer_edge_kernel (.., fs>)
    'conv1_pool': (lambda: TP.nets('conv1_pool')['vad'], 'conv_x3_kernel<3,'),                     # first_layer_rows_kernel + pool_rows_kernel (MODE 3 gather)
}


@functools.lru_cache(maxsize=None)
def net(name):
    """(layers, input shape) of NETS[name]; drawn once."""
    return NETS[name][0]()


def rows_overlapping():
    """The segmenter's own window list of a T-row recording: every second row, the first and last window replicated."""
    return S._window_rows(T)


def rows_scattered():
    """64 sorted scattered windows, odd first rows included: too little overlap for the shared first layer (per-window path)."""
    return np.sort(np.random.default_rng(64).integers(0, T - 68, 64)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle(name, case):
    """truth and reference32 of net `name` on `case` ((mean, std) or 'mixed') over the overlapping and the scattered list, computed
    once per process and handed out read-only: {'overlapping' | 'scattered': (truth, truth mask, reference32, reference32 mask)}."""
    layers, shp = net(name)
    mspec = mspec_of(case)
    ov, sc = rows_overlapping(), rows_scattered()
    both = np.concatenate([ov, sc])
    out = truth(layers, mspec, shp[1], both) + reference32(layers, mspec, shp[1], both)
    for a in out:
        a.setflags(write=False)
    return {'overlapping': tuple(a[:len(ov)] for a in out), 'scattered': tuple(a[len(ov):] for a in out)}


# ------------------------------------------------------------------------------------------
# float32 emulation of the two first-layer formulas (no device, no FMA): layer 1 of a net with its BatchNorm folded in, one window

def folded_first_layer(layers):
    """(w [K][C], bias [C]) float32 of conv -> BatchNorm as one convolution (k = ky * kw + kx, the kernels' order)."""
    conv, bn = layers[0], layers[1]
    assert conv['type'] == 'conv2d' and bn['type'] == 'batchnorm' and conv['W'].shape[2] == 1
    sc = bn['gamma'].astype(np.float64) / np.sqrt(bn['var'].astype(np.float64) + bn['eps'])
    kh, kw, _, c = conv['W'].shape
    w = conv['W'].astype(np.float64).reshape(kh * kw, c) * sc
    b = (conv['b'].astype(np.float64) - bn['mean']) * sc + bn['beta']
    return w.astype(np.float32), b.astype(np.float32), (kh, kw)


def _taps(x, kh, kw):
    """(H - kh + 1, W - kw + 1, kh * kw) view of the valid patches of x."""
    H, W = x.shape
    return np.stack([x[ky:ky + H - kh + 1, kx:kx + W - kw + 1] for ky in range(kh) for kx in range(kw)], axis=-1)


def _chain32(a, w):
    """sum_k a[..., k] * w[k][c] in float32, every product and every sum rounded, in k order."""
    acc = np.zeros(a.shape[:-1] + (w.shape[1],), np.float32)
    for k in range(w.shape[0]):
        acc = acc + a[..., k, None] * w[k][None, None, :]
    return acc


def emulate_first_layer(layers, window):
    """Layer-1 pre-activations of one float32 (68, nmel) window -> (max error of normalise-first f32, of the shared formula f32,
    activation scale): both against float64."""
    w, b, (kh, kw) = folded_first_layer(layers)
    x64 = window.astype(np.float64)
    want = _taps((x64 - x64.mean()) / x64.std(), kh, kw) @ w.astype(np.float64) + b
    mean, sd = np.float32(x64.mean()), np.float32(x64.std())           # patch_stats_kernel: float64 sums, rounded once
    first = _chain32(_taps((window - mean) / sd, kh, kw), w) + b
    rstd = np.float32(1.0) / sd
    S_ = w.astype(np.float64).sum(axis=0).astype(np.float32)            # ConvArgs::f_wsum
    shared = _chain32(_taps(window, kh, kw), w) * rstd + (b - mean * rstd * S_)
    assert first.dtype == shared.dtype == np.float32
    return np.abs(first - want).max(), np.abs(shared - want).max(), np.abs(want).max()
