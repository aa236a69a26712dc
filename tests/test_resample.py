"""CPU: the resampler's filter design and float64 reference (inaspeechsegmenter_amd/resample.py) against scipy, the
ffmpeg-free source reader, the Segmenter / CLI argument checks of resample=True."""
import importlib.util
import os

import numpy as np
import pytest

from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd import segmenter as S
from inaspeechsegmenter_amd import pipeline
from conftest import GOLDEN
from wavgen import FORMATS, encode, as_read, write_wav, make_signal

RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000, 44056, 4000, 384000)


def test_filter_table_equals_firwin():
    ss = pytest.importorskip('scipy.signal')
    for sr in RATES:
        up, down, h = R.plan(sr)
        mr = max(up, down)
        ref = ss.firwin(2 * 10 * mr + 1, 1.0 / mr, window=('kaiser', 5.0)) * up
        assert h.shape == ref.shape and np.max(np.abs(h - ref)) <= 1e-15, sr
    assert R.plan(44100)[:2] == (160, 441) and R.plan(44100)[2].size == 8821
    assert R.plan(44056)[:2] == (2000, 5507) and R.plan(44056)[2].size == 110141
    assert R.plan(44100)[2] is R.plan(44100)[2]                 # cached per rate


def test_reference_equals_resample_poly():
    ss = pytest.importorskip('scipy.signal')
    rng = np.random.default_rng(5)
    for sr in RATES + (16000,):
        up, down, h = R.plan(sr)
        hl = (h.size - 1) // 2
        for n in sorted({1, 5, max(hl - 1, 1), 1000, 48037}):
            m = rng.uniform(-1, 1, n)
            got = R.resample_float(m, sr)
            want = ss.resample_poly(m, up, down)
            assert got.shape == want.shape == (R.out_len(n, sr),), (sr, n)
            assert np.max(np.abs(got - want)) <= 1e-12, (sr, n)


def test_reference_steps():
    x = encode(make_signal(3000, 2, 1), 'i16')
    m = (x[:, 0] / 32768.0 + x[:, 1] / 32768.0) / 2
    assert np.array_equal(R.downmix(x), m)
    assert np.array_equal(R.resample_ref(x, 16000), np.rint(m * 32768).astype(np.int16))   # 16 kHz: downmix + quantise only
    y = np.array([-2.0, -1.0, -0.5 / 32768, 0.5 / 32768, 1.5 / 32768, 32767.5 / 32768, 1.0, 3.0])
    assert R.quantise(y).tolist() == [-32768, -32768, 0, 0, 2, 32767, 32767, 32767]      # half to even, then saturate


def test_invalid_rates_raise():
    for bad in (3999, 384001, 0, -16000, 44100.0, '44100', True, None):
        with pytest.raises(ValueError, match=str(bad).replace('.', r'\.') if bad is not None else 'None'):
            R.plan(bad)
    for ok in (4000, 384000, np.int64(22050)):
        R.plan(ok)


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('ch', (1, 2, 6))
def test_decode_source_formats(tmp_path, fmt, ch):
    st = encode(make_signal(1001, ch, 7), fmt)
    p = write_wav(tmp_path / f'x_{fmt}_{ch}.wav', st, 44100, fmt)
    x, sr = iss_io.decode_source(p)
    want = as_read(st, fmt)
    assert sr == 44100 and x.dtype == want.dtype and x.shape == want.shape
    assert np.array_equal(x, want)
    if fmt == 'i24':
        assert np.array_equal(iss_io._to_float(x, np.float64), st / 2.0 ** 23)


def test_load_source(tmp_path):
    mus = os.path.join(GOLDEN, 'musanmix.wav')
    a = S._load_source(mus, None, None, None, resample=True)
    assert a.dtype == np.int16 and np.array_equal(a, iss_io.decode_pcm(mus, ffmpeg=None))
    lam = os.path.join(GOLDEN, 'lamartine.wav')                 # 16 kHz mono float: the float32 path, unchanged
    assert np.array_equal(S._load_source(lam, None, None, None, resample=True), iss_io.decode_pcm(lam, ffmpeg=None))
    st = encode(make_signal(48000, 2, 3), 'i16')
    p48 = write_wav(tmp_path / 's48.wav', st, 48000, 'i16')
    r = S._load_source(p48, None, None, None, resample=True)
    assert isinstance(r, S.RawSource) and r.sr == 48000 and r.size == 16000 and np.array_equal(r.x, st)
    assert pipeline._held(r) == max(16000, st.nbytes // 2) and pipeline._held(a) == a.size
    p16s = write_wav(tmp_path / 's16st.wav', st, 16000, 'i16')   # 16 kHz stereo: downmixed on the device
    assert isinstance(S._load_source(p16s, None, None, None, resample=True), S.RawSource)
    with pytest.raises(AssertionError):                         # the default is unchanged
        S._load_source(p48, None, None, None)
    with pytest.raises(NotImplementedError):
        S._load_source(p48, 1.0, None, None, resample=True)
    p3k = write_wav(tmp_path / 's3k.wav', st, 3000, 'i16')
    with pytest.raises(ValueError, match='3000'):
        S._load_source(p3k, None, None, None, resample=True)


def test_segmenter_resample_needs_no_ffmpeg():
    with pytest.raises(ValueError, match='ffmpeg'):
        S.Segmenter(ffmpeg='ffmpeg', resample=True)


def _cli(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name', ('ina_speech_segmenter_amd', 'ina_voice_femininity_amd'))
def test_cli_resample_flag(name, tmp_path):
    cli = _cli(name)
    out = ['-o', str(tmp_path)] if name == 'ina_speech_segmenter_amd' else ['-o', str(tmp_path / 'o.tsv')]
    a = cli.build_parser().parse_args(['-i', 'x.wav'] + out + ['-b', 'None', '--resample'])
    assert a.resample is True and a.ffmpeg_binary == 'None'
    assert cli.build_parser().parse_args(['-i', 'x.wav'] + out).resample is False
    with pytest.raises(SystemExit) as e:                        # refused before anything is read or a device is opened
        cli.main(['-i', 'x.wav'] + out + ['-b', 'ffmpeg', '--resample'])
    assert e.value.code == 2
