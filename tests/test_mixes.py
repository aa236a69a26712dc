"""CPU: weighted channel mixes of a file.  The specification normaliser and the command line's grammar; resample.mixdown against a
scalar loop; the two identities of a mix on the reference itself (a one-term mix is the channel, the all-channel mean is the
downmix) and the float64 caveat that keeps numpy's mean out of it; windows of mix_ref; io.decode_mixes / decode_mix_excerpts on
WAV, FLAC, IMA and Microsoft ADPCM files; the .mix<k> naming.  Every comparison is exact."""
import importlib.util
import os

import numpy as np
import pytest

import flacgen
import msadpcmgen
import sndgen
import wavgen
from test_channels import flac_int
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd import sources
from inaspeechsegmenter_amd.resample import Mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the specification
def test_every_spelling():
    spec = [1, [0, 1], (2, 0, 2), {0: 1, 1: -1}, [(0, 0.5), (0, 0.25)], Mix(((1, 2), (0, 3.5)), 3), np.int64(2)]
    assert R.normalise_mixes(spec, 3) == [
        Mix(((1, 1.0),), 1.0),                                       # an int: that channel alone
        Mix(((0, 1.0), (1, 1.0)), 2.0),                              # ints: their mean, in the order given
        Mix(((2, 1.0), (0, 1.0), (2, 1.0)), 3.0),                    # (repeats count)
        Mix(((0, 1.0), (1, -1.0)), 1.0),                             # a mapping: the weighted sum
        Mix(((0, 0.5), (0, 0.25)), 1.0),                             # pairs: the weighted sum
        Mix(((1, 2.0), (0, 3.5)), 3.0),                              # the general form
        Mix(((2, 1.0),), 1.0)]
    out = R.normalise_mixes(spec, 3)
    assert all(type(c) is int and type(w) is float for m in out for c, w in m.terms) and all(type(m.divisor) is float for m in out)
    assert R.normalise_mixes(out, 3) == out                          # normalised mixes pass unchanged
    assert R.normalise_mixes([7]) == [Mix(((7, 1.0),), 1.0)]         # without a channel count only the sign is checked


@pytest.mark.parametrize('spec,why', [
    ([0, 2], r'mix 1 \(2\): channel 2 is outside the file\'s 2 channels \(0 \.\. 1\)'),
    ([[0, -1]], r'mix 0 .*channel -1 is outside'),
    ([{0: float('nan')}], r'mix 0 .*weight nan of channel 0 is not finite'),
    ([0, {1: float('inf')}], r'mix 1 .*weight inf of channel 1 is not finite'),
    ([Mix(((0, 1.0),), 0.0)], r'mix 0 .*divisor 0\.0 must be finite and not zero'),
    ([Mix(((0, 1.0),), float('inf'))], r'mix 0 .*divisor inf must be finite and not zero'),
    ([Mix(((0, 1.0),), float('nan'))], r'mix 0 .*divisor nan must be finite and not zero'),
    ([0, []], r'mix 1 \(\[\]\): empty mix'),
    ([{}], r'mix 0 .*empty mix'),
    ([Mix((), 1.0)], r'mix 0 .*empty mix'),
    ([], r'empty mix specification'),
    ([True], r'mix 0 \(True\)'),
    (['0+1'], r"mix 0 \('0\+1'\)"),
    ([[(0, 1.0, 2.0)]], r'mix 0 .*is not a \(channel, weight\) pair'),
    ([[(0.5, 1.0)]], r'mix 0 .*is not a \(channel, weight\) pair'),
    ('0,1', r'a mix specification is a sequence of mixes'),
    (None, r'a mix specification is a sequence of mixes'),
    ({0: 1}, r'a mix specification is a sequence of mixes'),
    (Mix(((0, 1.0),), 1.0), r'a mix specification is a sequence of mixes'),
])
def test_every_refusal_names_the_mix_and_the_reason(spec, why):
    with pytest.raises(ValueError, match=r'^call\.wav: ' + why):
        R.normalise_mixes(spec, 2, 'call.wav')


def test_cli_grammar():
    assert R.parse_mixes('0+1,2+3,0.7*4+0.7*5+1*2') == [
        Mix(((0, 1.0), (1, 1.0)), 2.0), Mix(((2, 1.0), (3, 1.0)), 2.0), Mix(((4, 0.7), (5, 0.7), (2, 1.0)), 1.0)]
    assert R.parse_mixes('3') == [Mix(((3, 1.0),), 1.0)]                             # one bare channel: that channel
    assert R.parse_mixes(' 1 + 0 + 1 ') == [Mix(((1, 1.0), (0, 1.0), (1, 1.0)), 3.0)]    # bare channels: their mean, repeats counted
    assert R.parse_mixes('0+-1*1') == [Mix(((0, 1.0), (1, -1.0)), 1.0)]              # a weighted term: bare channels weigh 1, no division
    assert R.parse_mixes('1e-1*0') == [Mix(((0, 0.1),), 1.0)]
    for bad in ('', '0,,1', '0+', 'a', '0.5', '1*0.5', '0*1*2', '-1', 'nan*0', '0;1'):
        with pytest.raises(ValueError, match='--mixes'):
            R.parse_mixes(bad)


def _cli():
    spec = importlib.util.spec_from_file_location('ina_cli_mixes', os.path.join(ROOT, 'scripts', 'ina_speech_segmenter_amd.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag_reaches_batch_process(tmp_path, monkeypatch):
    import inaspeechsegmenter_amd
    seen = {}

    class FakeSegmenter:
        def __init__(self, **kw):
            seen['init'] = kw

        def batch_process(self, inputs, outputs, **kw):
            seen['batch'] = kw

    monkeypatch.setattr(inaspeechsegmenter_amd, 'Segmenter', FakeSegmenter)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    src = wavgen.write_wav(tmp_path / 'a.wav', wavgen.encode(wavgen.make_signal(800, 2, 9), 'i16'), 16000, 'i16')
    assert _cli().main(['-i', src, '-o', str(tmp_path), '-b', 'None', '--mixes', '0+1,2*0+1']) == 0
    assert seen['batch'].get('mixes') == [Mix(((0, 1.0), (1, 1.0)), 2.0), Mix(((0, 2.0), (1, 1.0)), 1.0)]
    assert 'channels' not in seen['batch'] and seen['init']['ffmpeg'] is None
    assert _cli().main(['-i', src, '-o', str(tmp_path), '-b', 'None']) == 0
    assert 'mixes' not in seen['batch']
    for bad in (['--mixes', '0+1'], ['-b', 'None', '--mixes', '0+1', '--channels', 'split'], ['-b', 'None', '--mixes', '0+x']):
        with pytest.raises(SystemExit):
            _cli().main(['-i', src, '-o', str(tmp_path)] + bad)


def test_segmenter_refuses_ffmpeg_and_both_modes():
    from inaspeechsegmenter_amd import Segmenter
    seg = Segmenter.__new__(Segmenter)
    seg.ffmpeg, seg.resample = 'ffmpeg', False
    for call in (lambda: seg.load_pcm_mixes('a.wav', [0]), lambda: seg.segment_mixes('a.wav', [0]),
                 lambda: seg.load_pcm_mix_excerpts('a.wav', [(0, 1)], [0]), lambda: seg.segment_mix_excerpts('a.wav', [(0, 1)], [0]),
                 lambda: seg.batch_process(['a.wav'], ['a.csv'], mixes=[0])):
        with pytest.raises(ValueError, match='ffmpeg'):
            call()
    seg.ffmpeg = None
    with pytest.raises(ValueError, match='exclude each other'):
        seg.batch_process(['a.wav'], ['a.csv'], mixes=[0], channels='split')
    with pytest.raises(ValueError, match='mix 0'):
        seg.batch_process(['a.wav'], ['a.csv'], mixes=[[]])


def test_output_naming():
    assert iss_io.mix_name('a.csv', 0) == 'a.mix0.csv'
    assert iss_io.mix_name('/out/dir.v2/call.07.TextGrid', 1) == '/out/dir.v2/call.07.mix1.TextGrid'
    assert iss_io.mix_name('noext', 11) == 'noext.mix11'


# ------------------------------------------------------------------------------------------------ the reference
FMTS = ('u8', 'i16', 'i24', 'i32', 'f32', 'f64')
MIX3 = Mix(((2, 0.7071067811865476), (0, -1.0 / 3.0), (2, 1.0), (1, 3.0)), 1.7)


def _stored(n, ch, fmt, seed):
    return wavgen.as_read(wavgen.encode(wavgen.make_signal(n, ch, seed), fmt), fmt)


@pytest.mark.parametrize('fmt', FMTS)
def test_mixdown_against_a_scalar_loop(fmt):
    """Python floats are float64 and `*`, `+`, `/` round each on its own: the definition, one frame at a time."""
    x = _stored(300, 3, fmt, 41)
    xf = iss_io._to_float(x, np.float64)
    got = R.mixdown(x, MIX3)
    assert got.dtype == np.float64 and got.shape == (300,)
    for j in range(300):
        acc = MIX3.terms[0][1] * float(xf[j, MIX3.terms[0][0]])
        for c, w in MIX3.terms[1:]:
            acc = acc + w * float(xf[j, c])
        assert got[j] == acc / MIX3.divisor, j
    mono = x[:, 1].copy()                                               # a one-channel file: (n,) reads as (n, 1)
    np.testing.assert_array_equal(R.mixdown(mono, Mix(((0, -0.3),), 1.0)), -0.3 * xf[:, 1])
    with pytest.raises(ValueError, match='channel 1 is outside'):
        R.mixdown(mono, 1)


@pytest.mark.parametrize('fmt,sr', [('i16', 44100), ('f32', 48000), ('u8', 8000), ('i16', 16000)])
def test_one_term_mix_is_the_channel(fmt, sr):
    x = _stored(2500, 3, fmt, 42)
    for c in range(3):
        np.testing.assert_array_equal(R.mixdown(x, c), iss_io._to_float(x[:, c], np.float64))
        np.testing.assert_array_equal(R.mix_ref(x, sr, c), R.resample_ref(x[:, c], sr))


@pytest.mark.parametrize('fmt,ch', [(f, c) for f in ('i16', 'u8', 'i32') for c in (2, 3, 9)] + [('f32', 3)])
def test_all_channel_mean_is_the_downmix(fmt, ch):
    """Integer formats: every partial sum is exact, so numpy's order cannot matter; float formats: fewer than 8 channels."""
    x = _stored(2500, ch, fmt, 43)
    np.testing.assert_array_equal(R.mixdown(x, list(range(ch))), R.downmix(x))
    np.testing.assert_array_equal(R.mix_ref(x, 22050, list(range(ch))), R.resample_ref(x, 22050))


def test_numpy_mean_is_not_the_in_order_sum_at_8_float64_channels():
    """Why mixdown states the loop: numpy's mean(axis=1) adds float64 rows of 8 channels pairwise, the device in order."""
    x = np.random.default_rng(44).uniform(-1, 1, (20000, 8))
    in_order = R.mixdown(x, list(range(8)))
    acc = x[:, 0].copy()
    for c in range(1, 8):
        acc = acc + x[:, c]
    np.testing.assert_array_equal(in_order, acc / 8.0)                  # (1.0 * x is x)
    assert np.count_nonzero(in_order != x.mean(axis=1)) > 1000
    x7 = x[:, :7]
    np.testing.assert_array_equal(R.mixdown(x7, list(range(7))), x7.mean(axis=1))


def test_a_mix_saturates():
    x = np.array([[30000, 30000], [-30000, -30000], [100, -50]], dtype='<i2')
    np.testing.assert_array_equal(R.mix_ref(x, 16000, {0: 1, 1: 1}), [32767, -32768, 50])
    np.testing.assert_array_equal(R.mix_ref(x, 16000, [0, 1]), [30000, -30000, 25])


def test_mix_ref_windows_are_slices_of_the_whole():
    sr, n = 44100, 9000
    x = _stored(n, 3, 'i16', 45)
    whole = R.mix_ref(x, sr, MIX3)
    nout = R.out_len(n, sr)
    assert whole.size == nout
    for a, count in ((0, 700), (nout - 650, 650), (1000, 1100), (17, 1)):
        j_lo, j_hi = R.input_span(sr, n, a, count)
        got = R.mix_ref(x[j_lo:j_hi + 1], sr, MIX3, a, count, j_lo, n)
        np.testing.assert_array_equal(got, whole[a:a + count], err_msg=f'window [{a}, +{count})')


# ------------------------------------------------------------------------------------------------ files
SPEC = [1, [0, 1], {0: 0.7071067811865476, 1: -1.0 / 3.0}, Mix(((1, 1.0), (1, 1.0), (0, 1.0)), 3.0)]


def _files(d):
    out = {}
    out['wav'] = wavgen.write_wav(d / 'w.wav', wavgen.encode(wavgen.make_signal(9000, 2, 46), 'i16'), 44100, 'i16')
    out['wav_f32'] = wavgen.write_wav(d / 'wf.wav', wavgen.encode(wavgen.make_signal(9000, 2, 47), 'f32'), 48000, 'f32')
    out['flac'] = flacgen.write(d / 'f.flac', flac_int(9000, 2, 16, 48), 44100, 16, blocksize=1152, channel_mode='left_side',
                                subframe={'type': 'fixed', 'order': 2})
    out['ima'] = sndgen.write(d / 'i.wav', 'wav', 'ima', False, wavgen.make_signal(9000, 2, 49), 8000, block_align=256)[0]
    out['ms'] = msadpcmgen.write(d / 'm.wav', wavgen.make_signal(9000, 2, 50, peak=0.5), 8000, 256)[0]
    out['mono'] = wavgen.write_wav(d / 'mono.wav', wavgen.encode(wavgen.make_signal(9000, 1, 51), 'i16'), 16000, 'i16')
    return out


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return _files(tmp_path_factory.mktemp('mixes'))


@pytest.mark.parametrize('name', ['wav', 'wav_f32', 'flac', 'ima', 'ms'])
def test_decode_mixes_is_mix_ref_of_the_host_decode(files, name):
    from inaspeechsegmenter_amd import flac, sndfmt
    path = files[name]
    x, sr = iss_io.decode_source(path)
    assert x.ndim == 2 and x.shape[1] == 2
    got = iss_io.decode_mixes(path, SPEC)
    want = R.normalise_mixes(SPEC, 2)
    assert len(got) == 4
    for g, m in zip(got, want):
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, R.mix_ref(x, sr, m))
    np.testing.assert_array_equal(got[0], iss_io.decode_channels(path, [1])[0])          # the one-term identity, through the readers
    assert not np.array_equal(got[1], got[2])
    mixes, sig = iss_io.mix_source(path, SPEC, resample=True)
    cls = {'wav': sources.RawSource, 'wav_f32': sources.RawSource, 'flac': flac.FlacSource, 'ima': sndfmt.AdpcmSource,
           'ms': sndfmt.MsAdpcmSource}[name]
    assert mixes == want and type(sig) is cls and sig.sel == want and sig.parts == 4 and sig.size == got[0].size
    assert sig.reselect([mixes[2], 0]).sel == [want[2], 0] and sig.parts == 4


@pytest.mark.parametrize('name', ['wav', 'wav_f32', 'flac', 'ima', 'ms'])
def test_decode_mix_excerpts_are_slices_of_decode_mixes(files, name):
    path = files[name]
    whole = iss_io.decode_mixes(path, SPEC)
    n16 = whole[0].size
    ranges = [(0.0, 0.05), (0.06, None), (0.031, 0.09)]
    got = iss_io.decode_mix_excerpts(path, ranges, SPEC)
    mixes, sigs = iss_io.mix_excerpts(path, ranges, SPEC, resample=True)
    assert len(got) == 3 and len(sigs) == 3
    for r, (start, stop) in enumerate(ranges):
        a, b = iss_io.excerpt_bounds(path, n16, start, stop)
        assert len(got[r]) == 4 and sigs[r].sel == mixes and sigs[r].parts == 4 and sigs[r].size == b - a
        for k in range(4):
            np.testing.assert_array_equal(got[r][k], whole[k][a:b], err_msg=f'{name} range {r} mix {k}')
    x, sr = iss_io.decode_source(path)
    assert sigs[2].payload.nbytes < x.nbytes                           # only what the range needs


def test_a_one_channel_file_takes_mixes_of_channel_0(files):
    x, sr = iss_io.decode_source(files['mono'])
    got = iss_io.decode_mixes(files['mono'], [0, {0: -0.5}])
    np.testing.assert_array_equal(got[0], x)                            # 16 kHz PCM16 through the identity filter
    np.testing.assert_array_equal(got[1], R.mix_ref(x, sr, {0: -0.5}))
    assert iss_io.mix_source(files['mono'], [0])[1].parts == 1


@pytest.mark.parametrize('reader', ['decode_mixes', 'mix_source'])
def test_file_refusals_name_the_file_and_the_mix(files, reader):
    read = getattr(iss_io, reader)
    with pytest.raises(ValueError, match=r'w\.wav: mix 1 \(\[0, 2\]\): channel 2 is outside the file\'s 2 channels'):
        read(files['wav'], [0, [0, 2]])
    with pytest.raises(ValueError, match=r'mono\.wav: mix 0 .*channel 1 is outside the file\'s 1 channel '):
        read(files['mono'], [1])
    with pytest.raises(ValueError, match=r'nowhere\.wav: empty mix specification'):
        read('nowhere.wav', [])                                         # refused before the file is opened
    with pytest.raises(ValueError, match=r'http://host/a\.wav'):
        read('http://host/a.wav', [0])
    with pytest.raises(AssertionError, match=r'can only take files sampled at 16000 Hz'):
        read(files['wav'], [0], resample=False)
    with pytest.raises(ValueError, match=r'w\.wav: mix 0 .*channel 5'):
        iss_io.mix_excerpts(files['wav'], [(0, 0.05)], [5], resample=True)
