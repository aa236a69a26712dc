"""The float64 Keras CNN oracle (oracle/keras_cnn.py, dtype=np.float64) that the device's arithmetic modes are measured against
(tests/test_gpu_cnn_defaults.py): its two independent implementations agree to float64 rounding, and the float32 one sits within
float32 rounding of it, on tiny nets with the stand-ins' layer kinds and the Keras edges (a 'same'-padded conv, a 'same' avgpool
whose mean excludes the padding, ELU)."""
import numpy as np
import pytest

from inaspeechsegmenter_amd import keras_model as KM
from oracle import keras_cnn as ocnn


def _conv(rng, kh, kw, cin, cout, padding='valid', act='linear'):
    return dict(type='conv2d', W=rng.normal(0, np.sqrt(2.0 / (kh * kw * cin)), (kh, kw, cin, cout)).astype(np.float32),
                b=rng.normal(0, 0.1, cout).astype(np.float32), strides=(1, 1), padding=padding, activation=act)


def _bn(rng, c):
    return dict(type='batchnorm', gamma=rng.uniform(0.5, 1.5, c).astype(np.float32), beta=rng.normal(0, 0.2, c).astype(np.float32),
                mean=rng.normal(0, 0.2, c).astype(np.float32), var=rng.uniform(0.5, 1.5, c).astype(np.float32), eps=1e-3)


def _dense(rng, i, o, act):
    return dict(type='dense', W=rng.normal(0, np.sqrt(2.0 / i), (i, o)).astype(np.float32),
                b=rng.normal(0, 0.1, o).astype(np.float32), activation=act)


def _chain(rng):
    """The stand-ins' kinds: conv-BN-relu twice, a 2 x 2 max-pool, flatten, dense-relu, dropout, dense-softmax.  (16, 9, 1)."""
    relu = dict(type='activation', fn='relu')
    return [_conv(rng, 4, 5, 1, 8), _bn(rng, 8), relu, _conv(rng, 5, 3, 8, 8), _bn(rng, 8), relu,
            dict(type='maxpool', pool=(2, 2), strides=(2, 2), padding='valid'),             # (9, 3) -> (4, 1)
            dict(type='flatten'), _dense(rng, 32, 16, 'relu'), dict(type='dropout'), _dense(rng, 16, 3, 'softmax')], (16, 9, 1)


def _edges(rng):
    """'same' conv with an ELU, a 'same' avgpool over an odd width (padded cells outside the mean), an ELU layer.  (12, 7, 1)."""
    return [_conv(rng, 3, 3, 1, 6, padding='same', act='elu'),
            dict(type='avgpool', pool=(2, 2), strides=(2, 2), padding='same'),              # (12, 7) -> (6, 4)
            dict(type='activation', fn='elu'), _conv(rng, 3, 3, 6, 8, act='relu'),        # -> (4, 2)
            dict(type='flatten'), _dense(rng, 64, 2, 'softmax')], (12, 7, 1)


def _standin(rng):
    return KM.synthetic_ina_like(21, 3, seed=1)


NETS = {'chain': (_chain, 5), 'edges': (_edges, 5), 'standin': (_standin, 2)}


@pytest.mark.parametrize('name', sorted(NETS))
def test_float64_oracle_agrees_with_its_naive_twin(name):
    make, n = NETS[name]
    rng = np.random.default_rng(4)
    layers, shp = make(rng)
    x = rng.normal(0, 1.5, (n,) + shp).astype(np.float32)
    p64 = ocnn.forward(layers, x, dtype=np.float64)
    naive64 = ocnn.forward_naive(layers, x, dtype=np.float64)
    assert p64.dtype == np.float64 and naive64.dtype == np.float64
    rel = np.abs(p64 - naive64) / np.abs(naive64)
    print(f'{name}: float64 forward vs naive {rel.max():.1e} relative')
    assert rel.max() < 1e-12, rel.max()
    # log=True: the log-softmax of the same network, not log() of a rounded p
    lp64 = ocnn.forward(layers, x, dtype=np.float64, log=True)
    assert np.abs(lp64 - np.log(p64)).max() < 1e-12
    # float32: the default arithmetic, within float32 rounding of float64 (and not float64 itself)
    p32 = ocnn.forward(layers, x)
    assert p32.dtype == np.float32 and np.array_equal(p32, ocnn.forward(layers, x, dtype=np.float32))
    lp32 = ocnn.forward(layers, x, log=True)
    assert lp32.dtype == np.float32
    d = np.abs(lp32.astype(np.float64) - lp64).max()
    print(f'{name}: float32 vs float64 max |d log p| {d:.1e}, max |d p| {np.abs(p32 - p64).max():.1e}')
    assert 0 < d < 5e-5 and np.abs(p32 - p64).max() < 1e-5
    naive32 = ocnn.forward_naive(layers, x)
    assert naive32.dtype == np.float32 and np.abs(naive32 - p64).max() < 1e-5


def test_log_output_needs_a_softmax_head():
    rng = np.random.default_rng(5)
    layers, shp = _chain(rng)
    layers[-1] = dict(layers[-1], activation='linear')
    with pytest.raises(ValueError):
        ocnn.forward(layers, np.zeros((1,) + shp, np.float32), log=True)
