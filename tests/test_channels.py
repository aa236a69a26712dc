"""Host side of "every channel of a file on its own": io.decode_channels (the host-only twin of Segmenter.load_pcm_channels) against
resample.resample_ref of each stored column and, once, against scipy; selections; refusals; output naming; the CLI flag.
No device: the kernels are tested in test_gpu_channels.py."""
import importlib.util
import os

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd import sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flac_int(n, ch, bps, seed):
    """Integer samples (n, ch) within `bps` bits, every channel different."""
    x = np.stack([np.round(wavgen.make_signal(n, 1, seed + 7 * c, peak=0.5) * (1 << (bps - 1))) for c in range(ch)], axis=1)
    return np.clip(x, -(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int64)


def _files(d):
    """name -> path of one small multi-channel file per format family."""
    out = {}
    for fmt, sr, ch in (('i16', 44100, 2), ('f32', 48000, 3), ('i16', 16000, 2)):
        out[f'wav_{fmt}_{sr}'] = wavgen.write_wav(d / f'w_{fmt}_{sr}.wav', wavgen.encode(wavgen.make_signal(3000, ch, 1), fmt), sr, fmt)
    out['ulaw'] = sndgen.write(d / 'u.wav', 'wav', 'ulaw', False, wavgen.make_signal(2500, 2, 2), 8000)[0]
    out['aiff_be'] = sndgen.write(d / 'a.aiff', 'aiff', 'i16', True, wavgen.make_signal(2500, 2, 3), 22050)[0]
    for mode in ('independent', 'left_side', 'mid_side'):
        for bps in (16, 24):
            out[f'flac_{mode}_{bps}'] = flacgen.write(d / f'f_{mode}_{bps}.flac', flac_int(2600, 2, bps, 4), 44100 if bps == 24 else 16000,
                                                      bps, blocksize=1152, channel_mode=mode, subframe={'type': 'fixed', 'order': 2})
    out['ima'] = sndgen.write(d / 'i.wav', 'wav', 'ima', False, wavgen.make_signal(2700, 2, 5), 8000, block_align=256)[0]
    return out


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return _files(tmp_path_factory.mktemp('channels'))


NAMES = ['wav_i16_44100', 'wav_f32_48000', 'wav_i16_16000', 'ulaw', 'aiff_be', 'flac_independent_16', 'flac_left_side_16',
         'flac_mid_side_16', 'flac_independent_24', 'flac_left_side_24', 'flac_mid_side_24', 'ima']


@pytest.mark.parametrize('name', NAMES)
def test_decode_channels_is_resample_ref_of_each_column(files, name):
    path = files[name]
    x, sr = iss_io.decode_source(path)
    assert x.ndim == 2 and x.shape[1] >= 2
    got = iss_io.decode_channels(path)
    assert len(got) == x.shape[1]
    for c, g in enumerate(got):
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, R.resample_ref(x[:, c], sr), err_msg=f'{name} channel {c}')
    assert not np.array_equal(got[0], got[1])                        # (the generators give every channel its own signal)
    if sr == 16000 and x.dtype == np.int16:                          # the identity: the stored columns themselves
        np.testing.assert_array_equal(got[1], x[:, 1])


def test_decode_channels_against_scipy(files):
    """44.1 kHz stereo PCM16: each channel is scipy's polyphase resampling of that column, quantised like ffmpeg's pcm_s16le.
    resample_float is pinned to scipy within 1e-12 by the resampler's own tests (3.3e-8 after the scaling by 32768), so the two
    may differ, by one step, only where y * 32768 falls within 1e-6 of a half."""
    scipy_signal = pytest.importorskip('scipy.signal')
    path = files['wav_i16_44100']
    x, sr = iss_io.decode_source(path)
    up, down, h = R.plan(sr)
    for c, g in enumerate(iss_io.decode_channels(path)):
        y = scipy_signal.resample_poly(x[:, c] / 32768.0, up, down) * 32768.0
        want = np.clip(np.rint(y), -32768, 32767)
        assert y.shape == g.shape
        near_tie = np.abs(y - np.floor(y) - 0.5) < 1e-6
        assert np.all((g == want) | (near_tie & (np.abs(g - want) <= 1)))
        assert near_tie.sum() < 5


def test_selection_order_and_repeats(files):
    path = files['wav_f32_48000']
    allch = iss_io.decode_channels(path)
    got = iss_io.decode_channels(path, [1, 0, 1])
    assert len(got) == 3
    for g, c in zip(got, (1, 0, 1)):
        np.testing.assert_array_equal(g, allch[c])
    np.testing.assert_array_equal(iss_io.decode_channels(path, (2,))[0], allch[2])
    sel, sig = iss_io.split_source(path, [2, 0], resample=True)
    assert sel == [2, 0] and isinstance(sig, sources.RawSource) and sig.sel == [2, 0] and sig.parts == 2
    assert sig.stride == -(-sig.size // 160) * 160 and sig.reselect([1]).parts == 1 and sig.parts == 2


def test_mono_file_returns_decode_pcm(tmp_path):
    for fmt in ('i16', 'f32'):                                        # the float path included
        path = wavgen.write_wav(tmp_path / f'm_{fmt}.wav', wavgen.encode(wavgen.make_signal(2000, 1, 6), fmt), 16000, fmt)
        got = iss_io.decode_channels(path)
        want = iss_io.decode_pcm(path, ffmpeg=None)
        assert len(got) == 1 and got[0].dtype == want.dtype
        np.testing.assert_array_equal(got[0], want)
        sel, sig = iss_io.split_source(path)
        assert sel == [0] and isinstance(sig, np.ndarray)


def test_source_classes_carry_the_selection(files):
    from inaspeechsegmenter_amd import flac, sndfmt
    for name, cls in (('flac_left_side_16', flac.FlacSource), ('ima', sndfmt.AdpcmSource), ('ulaw', sources.RawSource)):
        sel, sig = iss_io.split_source(files[name], None, resample=True)
        assert isinstance(sig, cls) and sig.sel == [0, 1] == sel and sig.parts == 2, name
        assert sig.size == R.out_len(iss_io.decode_source(files[name])[0].shape[0], iss_io.decode_source(files[name])[1])
    plain = flac.FlacStream(open(files['flac_left_side_16'], 'rb').read(), 'x').source(True)
    assert plain.parts == 1 and plain.sel is None


@pytest.mark.parametrize('reader', ['decode_channels', 'split_source'])
def test_refusals_name_the_file(files, reader):
    read = getattr(iss_io, reader)
    path = files['wav_i16_16000']
    with pytest.raises(ValueError, match=r'w_i16_16000\.wav: channel 2 is outside'):
        read(path, [0, 2])
    with pytest.raises(ValueError, match=r'w_i16_16000\.wav: channel -1 is outside'):
        read(path, [-1])
    with pytest.raises(ValueError, match=r'w_i16_16000\.wav: empty channel selection'):
        read(path, [])
    with pytest.raises(ValueError, match=r'http://host/a\.wav'):
        read('http://host/a.wav')
    mono = wavgen.write_wav(os.path.join(os.path.dirname(path), 'mono.wav'), wavgen.encode(wavgen.make_signal(900, 1, 8), 'i16'), 16000, 'i16')
    with pytest.raises(ValueError, match=r'mono\.wav: channel 1 is outside'):
        read(mono, [1])


@pytest.mark.parametrize('reader', ['decode_channels', 'split_source'])
def test_rate_rule_without_resample(files, reader):
    """Without `resample` a rate other than 16 kHz is refused with the whole-file read's text; two channels at 16 kHz are not."""
    read = getattr(iss_io, reader)
    with pytest.raises(AssertionError, match=r'can only take files sampled at 16000 Hz\. The file .*w_i16_44100\.wav is sampled at 44100 Hz'):
        read(files['wav_i16_44100'], None, resample=False)
    read(files['wav_i16_16000'], None, resample=False)


def test_segmenter_refuses_ffmpeg():
    """The three entry points name the argument when ffmpeg is set (checked before anything touches a device)."""
    from inaspeechsegmenter_amd import Segmenter
    seg = Segmenter.__new__(Segmenter)
    seg.ffmpeg, seg.resample = 'ffmpeg', False
    for call in (lambda: seg.load_pcm_channels('a.wav'), lambda: seg.segment_channels('a.wav'),
                 lambda: seg.batch_process(['a.wav'], ['a.csv'], channels='split')):
        with pytest.raises(ValueError, match='ffmpeg'):
            call()
    seg.ffmpeg = None
    with pytest.raises(ValueError, match="channels='both'"):
        seg.batch_process(['a.wav'], ['a.csv'], channels='both')


def test_output_naming():
    assert iss_io.channel_name('a.csv', 0) == 'a.ch0.csv'
    assert iss_io.channel_name('/out/dir.v2/call.07.TextGrid', 1) == '/out/dir.v2/call.07.ch1.TextGrid'
    assert iss_io.channel_name('noext', 11) == 'noext.ch11'


def _cli():
    spec = importlib.util.spec_from_file_location('ina_cli', os.path.join(ROOT, 'scripts', 'ina_speech_segmenter_amd.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('flag,want', [([], None), (['--channels', 'mix'], None), (['--channels', 'split'], 'split')])
def test_cli_flag_reaches_batch_process(tmp_path, monkeypatch, flag, want):
    import inaspeechsegmenter_amd
    seen = {}

    class FakeSegmenter:
        def __init__(self, **kw):
            seen['init'] = kw

        def batch_process(self, inputs, outputs, **kw):
            seen['batch'] = (inputs, outputs, kw)

    monkeypatch.setattr(inaspeechsegmenter_amd, 'Segmenter', FakeSegmenter)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    src = wavgen.write_wav(tmp_path / 'a.wav', wavgen.encode(wavgen.make_signal(800, 2, 9), 'i16'), 16000, 'i16')
    assert _cli().main(['-i', src, '-o', str(tmp_path), '-b', 'None'] + flag) == 0
    inputs, outputs, kw = seen['batch']
    assert inputs == [src] and outputs == [str(tmp_path / 'a.csv')] and kw.get('channels') == want
    assert seen['init']['ffmpeg'] is None


def test_cli_split_needs_no_ffmpeg(tmp_path):
    with pytest.raises(SystemExit):
        _cli().main(['-i', 'a.wav', '-o', str(tmp_path), '--channels', 'split'])
