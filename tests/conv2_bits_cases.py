"""Inputs of tests/test_gpu_conv2_front_end_bits.py and of the generator of its fixture (tests/golden/make_conv2_parent_bits.py):
the smallest window lists that reach every piece of conv2's fused front end (conv_wq.h: slice fetch, window scalars, conversion,
the epilogue that rides along) -- one and two windows, an odd frame count, a non-finite row, a partial last tile, and lists whose
tiles span two unrelated windows and whose trailing slices lie beyond `need`."""
import numpy as np

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, _native

NETS = ((21, 3, 1), (24, 2, 2))                      # (mel columns, classes, seed) of the two stand-ins: conv2 tiles of 508 / 512 rows
MODES = {'f16x3': _native.PREC_F16X3, 'bf16x3': _native.PREC_BF16X3}
CONV2 = 'conv_x3_wq_kernel<5,3,'
T_LONG = 1200


def make_mspec():
    """1 200 log-mel-like rows (what the fixture stores as `mspec`; seeded, but numpy does not promise the stream for ever)."""
    rng = np.random.default_rng(20261020)
    base = rng.normal(-3.0, 1.5, (T_LONG, 24))
    drift = np.cumsum(rng.normal(0, 0.05, (T_LONG, 1)), axis=0)
    return (base + drift).astype(np.float32)


def cases(mspec):
    """[(name, features, window rows)]; every `features` is a slice or a copy of the stored rows."""
    assert mspec.shape == (T_LONG, 24)
    out = []
    m70 = mspec[100:170].copy()
    out.append(('t70_one', m70, np.array([0], dtype=np.int32)))
    out.append(('t70_two', m70, np.array([0, 2], dtype=np.int32)))
    out.append(('t70_slots', m70, S._window_rows(70).astype(np.int32)))       # the segmenter's own list: 35 slots on two windows
    m141 = mspec[200:341].copy()
    out.append(('t141', m141, S._window_rows(141).astype(np.int32)))
    m300 = mspec[400:700].copy()
    m300[150, :] = -np.inf                           # one non-finite log-mel row: the windows over it are dead
    out.append(('t300_inf_row', m300, S._window_rows(300).astype(np.int32)))
    # 7 windows of 62 x 17 (62 x 20) conv2 rows = 14.5 tiles of 508 (16.95 of 512): a partial last tile, an odd tile count
    out.append(('partial_tile', m300, np.arange(160, 174, 2, dtype=np.int32)))
    m1200 = mspec.copy()
    m1200[600, :] = np.nan
    rng = np.random.default_rng(5)
    out.append(('scattered_333', m1200, rng.integers(0, T_LONG - 67, 333).astype(np.int32)))
    runs = np.concatenate([np.arange(0, 40, 2), np.arange(301, 331, 2), np.arange(520, 680, 2), np.arange(1100, 1133, 1),
                           np.arange(900, 880, -2), [T_LONG - 68, 0]]).astype(np.int32)
    out.append(('runs_with_gaps', m1200, runs))
    return out


def nets():
    out = []
    for nmel, ncls, seed in NETS:
        layers, shp = KM.synthetic_ina_like(nmel, ncls, seed=seed)
        out.append((nmel, KM.compile_layers(layers, shp)))
    return out


def context(mode):
    """A fresh context in one arithmetic mode, the guard off (no probe, no switch), both stand-ins loaded as nets 0 and 1."""
    from inaspeechsegmenter_amd import tables
    c = _native.Context(0)
    c.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank())
    c.set_precision_guard(0)
    c.set_precision(MODES[mode])
    for k, (nmel, comp) in enumerate(nets()):
        c.cnn_load(k, comp)
    return c


def run(c, net_id, feats, rows, no_wq=False):
    """(probs, finite, kernel instantiations launched) of one iss_cnn_probs call."""
    diag = getattr(c, 'diag', 0)
    c.set_mspec(feats)
    if no_wq:
        c.set_diag(diag | _native.DIAG_BITS['no_wq'])
    c.prof_enable(True)
    c.prof_reset()
    try:
        p, f = c.cnn_probs(net_id, rows)
        return p, np.asarray(f, dtype=bool), sorted(e['kernel'] for e in c.prof_instances())
    finally:
        c.prof_enable(False)
        if no_wq:
            c.set_diag(diag)


def key(mode, net_id, name):
    return f'{mode}.net{net_id}.{name}'
