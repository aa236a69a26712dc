"""GPU: the channel survey.  Segmenter.survey_channels (survey_kernel and its second stage) against io.survey_channels, the
host-only twin: every measured field equal to the bit (the int64 view of every float64 is compared, no tolerance anywhere).
The shapes are the smallest at which the kernel can go wrong: frames on every edge of the chunk geometry the library exports
(one lane row, one chunk, one more, several chunks and a tail), one channel, a group that is not a power of two, the 16
channels that fill the LDS rows and the 17 that need a second group and carry no pairs; one file per stored format the readers
take; the three decoders' staging buffers; ranges on the device; a ragged launch over files of different classes; and a
small job after a large one on the same workspace."""
import math
import os

import numpy as np
import pytest

import flacgen
import msadpcmgen
import sndgen
import wavgen
from conftest import GOLDEN, read_wav_int16, synth_pcm
from inaspeechsegmenter_amd import _native, Segmenter
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.survey import ChannelSurvey

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


@pytest.fixture(scope='module')
def C(seg):
    chunk, lanes, pair_channels = seg.ctx.survey_geometry()
    assert (chunk, lanes, pair_channels) == (R.SURVEY_CHUNK, R.SURVEY_LANES, R.SURVEY_PAIR_CHANNELS)
    return chunk


def same(got, want):
    """Two surveys equal to the bit, field by field (so that a failure names the field)."""
    assert isinstance(got, ChannelSurvey), got
    assert (got.sr, got.first, got.n, got.channels) == (want.sr, want.first, want.n, want.channels)
    for name in ('peak', 'zeros', 'fullscale', 'nonfinite', 's1', 's2'):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64)), (name, a, b)
    assert (got.s12 is None) == (want.s12 is None)
    if want.s12 is not None:
        assert np.array_equal(got.s12.view(np.int64), want.s12.view(np.int64)), ('s12', got.s12, want.s12)
    assert got == want


def _signal(n, ch, seed):
    x = wavgen.make_signal(max(n, 2), ch, seed)[:n].reshape(n, ch) * 0.7
    x[::5, 0] = 0.0                                             # digital zeros, and (below) samples at full scale
    x[1::9, ch - 1] = 1.0
    return x


def _flac_pcm(n, ch, seed, bps=16):
    """Integer samples the test encoder takes (a smooth signal): a run of zeros and a run at full scale in it."""
    x = np.rint(wavgen.make_signal(n, ch, seed).reshape(n, ch) * 0.7 * ((1 << (bps - 1)) - 1)).astype(np.int64)
    x[200:210, 0] = 0
    x[100:103, ch - 1] = (1 << (bps - 1)) - 1
    return x


# ------------------------------------------------------------------------------------------------ chunk edges x channel counts
FRAMES = ('1', '255', '256', '257', 'C-1', 'C', 'C+1', '3C+17')


@pytest.mark.parametrize('frames', FRAMES)
@pytest.mark.parametrize('ch', [1, 2, 3, 8, 16, 17])
def test_bit_equal_at_chunk_edges(seg, C, tmp_path, frames, ch):
    n = eval(frames.replace('3C', '3*C'), {'C': C})
    stored = wavgen.encode(_signal(n, ch, 7 * ch + n % 97), 'i16')
    path = wavgen.write_wav(tmp_path / 'a.wav', stored, 48000, 'i16')
    got, want = seg.survey_channels(path), iss_io.survey_channels(path)
    same(got, want)
    assert want.n == n and want.zeros[0] >= 1 and want.fullscale[ch - 1] >= (1 if n > 1 else 0)
    assert (want.s12 is None) == (ch == 17)


# ------------------------------------------------------------------------------------------------ one file per stored format
RAW = [('wav', k, False) for k in wavgen.FORMATS] + [('wav', 'ulaw', False), ('wav', 'alaw', False), ('aiff', 'i8', True),
      ('aiff', 'i16', True), ('aiff', 'i32', True), ('aiff', 'i24', True), ('aifc', 'f32', True), ('aifc', 'f64', True), ('caf', 'i16', False)]


@pytest.mark.parametrize('container,kind,big', RAW, ids=[f'{c}-{k}-{"be" if b else "le"}' for c, k, b in RAW])
def test_bit_equal_every_stored_format(seg, C, tmp_path, container, kind, big):
    x = _signal(C + 1, 2, 11)
    if kind in ('f32', 'f64'):
        x[40, 0], x[41, 1], x[42, 1] = np.nan, np.inf, -np.inf
    if container == 'wav' and kind in wavgen.FORMATS:
        path = wavgen.write_wav(tmp_path / 'a.wav', wavgen.encode(x, kind), 22050, kind)
    else:
        path, _, _ = sndgen.write(tmp_path / f'a.{container}', container, kind, big, x, 22050)
    before = seg.ctx.survey_stats()
    got, want = seg.survey_channels(path), iss_io.survey_channels(path)
    after = seg.ctx.survey_stats()
    same(got, want)
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)
    assert want.fullscale[1] >= 1 and (want.zeros[0] >= 1 or kind == 'alaw')      # (A-law has no code for zero)
    if kind in ('f32', 'f64'):
        assert list(want.nonfinite) == [1, 2]


def test_swapped_and_g711_bytes_reach_the_kernel_unexpanded(seg, tmp_path):
    """The device sources of these files carry the stored bytes with the format codes of the readers, not a host expansion."""
    x = _signal(500, 2, 12)
    seen = set()
    for container, kind, big in RAW:
        if container == 'wav' and kind in wavgen.FORMATS:
            continue
        path, _, _ = sndgen.write(tmp_path / f'b-{kind}.{container}', container, kind, big, x, 22050)
        (src, _), = iss_io.survey_sources(path)[1]
        seen.add(src.fmt)
    assert {_native.RS_ULAW, _native.RS_ALAW, _native.RS_I8, 1 | _native.RS_SWAP, 2 | _native.RS_SWAP, 3 | _native.RS_SWAP,
            4 | _native.RS_SWAP} <= seen


# ------------------------------------------------------------------------------------------------ the decoders' staging buffers
@pytest.mark.parametrize('bps,mode', [(16, 'left_side'), (24, 'independent')])
def test_bit_equal_flac(seg, C, tmp_path, bps, mode):
    x = _flac_pcm(3 * C + 17, 2, bps, bps)
    path = flacgen.write(tmp_path / 'a.flac', x, 16000, bps, blocksize=1152, channel_mode=mode)
    before = seg.ctx.flac_stats(), seg.ctx.survey_stats()
    got, want = seg.survey_channels(path), iss_io.survey_channels(path)
    same(got, want)
    assert seg.ctx.flac_stats()[0] - before[0][0] == 1 and seg.ctx.survey_stats()[0] - before[1][0] == 1
    assert want.fullscale[1] >= 1 and want.n == 3 * C + 17


def test_bit_equal_ima_two_channels(seg, C, tmp_path):
    path, _, _ = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, _signal(2 * C + 100, 2, 13), 8000)
    same(seg.survey_channels(path), iss_io.survey_channels(path))


def test_bit_equal_msadpcm_mono_with_a_cut_last_block(seg, C, tmp_path):
    n = 5 * msadpcmgen.samples_per_block(256, 1) + 77
    path, twin = msadpcmgen.write(tmp_path / 'a.wav', _signal(n, 1, 14)[:, 0], 8000, 256)
    got, want = seg.survey_channels(path), iss_io.survey_channels(path)
    same(got, want)
    assert want.n == n == len(twin) and want.s12 is not None and len(want.s12) == 0 and want.downmix_loss_db == 0.0


# ------------------------------------------------------------------------------------------------ ranges on the device
@pytest.fixture(scope='module')
def ranged(tmp_path_factory, C):
    d = tmp_path_factory.mktemp('ranged')
    n, sr = 3 * C + 17, 8000
    pcm = _flac_pcm(n, 2, 15).astype('<i2')
    x = pcm / 32768.0
    return n, sr, {'wav': wavgen.write_wav(d / 'a.wav', pcm, sr, 'i16'),
                   'aiff': sndgen.write(d / 'a.aiff', 'aiff', 'i16', True, x, sr)[0],
                   'flac': flacgen.write(d / 'a.flac', pcm.astype(np.int64), sr, 16, blocksize=576, channel_mode='left_side'),
                   'ima': sndgen.write(d / 'b.wav', 'wav', 'ima', False, x, sr)[0],
                   'ms': msadpcmgen.write(d / 'c.wav', x, sr, 256)[0]}


@pytest.mark.parametrize('what', ['wav', 'aiff', 'flac', 'ima', 'ms'])
def test_ranges_on_the_device(seg, C, ranged, what):
    n, sr, paths = ranged
    a = C + C // 2 + 3                                          # starts in the middle of a chunk of the file
    ranges = [(a / sr, (a + 2 * C + 5) / sr if a + 2 * C + 5 < n else None), ((2 * C + 9) / sr, 99.0), ((C - 1) / sr, C / sr)]
    got, want = seg.survey_channels(paths[what], ranges), iss_io.survey_channels(paths[what], ranges)
    assert [(w.first, w.n) for w in want] == [(a, n - a), (2 * C + 9, n - 2 * C - 9), (C - 1, 1)]
    for g, w in zip(got, want):
        same(g, w)
    with pytest.raises(ValueError, match='holds no frame'):
        seg.survey_channels(paths[what], [(n / sr + 0.5, None)])


def test_wav_ranges_read_byte_ranges_only(seg, C, ranged, monkeypatch):
    n, sr, paths = ranged
    reads = []
    real = iss_io._read_range
    monkeypatch.setattr(iss_io, '_read_range', lambda path, off, size: (reads.append(size), real(path, off, size))[1])
    seg.survey_channels(paths['wav'], [((C - 1) / sr, C / sr)])
    assert max(reads) <= 64 and sum(reads) < 200                # the chunk headers and one frame


def test_window_inside_the_staged_frames(seg, C):
    """The planner's own offset: a job whose bytes hold frames [100, 100 + 2C + 50) of a file, surveyed over [C, 2C + 7)."""
    x = wavgen.encode(_signal(3 * C, 3, 16), 'i16')
    held = np.ascontiguousarray(x[100:100 + 2 * C + 50])
    full = R.SURVEY_FULL['i16']
    got, = seg.ctx.survey(held.reshape(-1).view(np.uint8), [(0, len(held), 3, 1, full)], [(100, 100 + len(held), 3 * C, C, C + 7)])
    same(ChannelSurvey(got, 8000), ChannelSurvey(R.survey_ref(x, full, C, 2 * C + 7), 8000))
    for bad in [(100, 100 + len(held), 3 * C, 99, 5), (100, 100 + len(held), 3 * C, C, 2 * C), (0, len(held) + 1, 3 * C, 0, 1)]:
        with pytest.raises(_native.NativeError, match='iss_survey: job 0'):
            seg.ctx.survey(held.reshape(-1).view(np.uint8), [(0, len(held), 3, 1, full)], [bad])
    with pytest.raises(_native.NativeError, match='outside the'):
        seg.ctx.survey(held.reshape(-1).view(np.uint8), [(2, len(held), 3, 1, full)])


# ------------------------------------------------------------------------------------------------ ragged launch
def test_survey_files_one_launch_per_class(seg, C, tmp_path):
    files = [wavgen.write_wav(tmp_path / 'w8.wav', wavgen.encode(_signal(5 * C + 3, 8, 20), 'i16'), 48000, 'i16'),
             wavgen.write_wav(tmp_path / 'f1.wav', wavgen.encode(_signal(300, 1, 21), 'f32'), 16000, 'f32'),
             sndgen.write(tmp_path / 'be.aiff', 'aiff', 'i16', True, _signal(C + 1, 2, 22), 44100)[0],
             flacgen.write(tmp_path / 'a.flac', _flac_pcm(2 * C + 9, 2, 23), 16000, 16, blocksize=1152),
             sndgen.write(tmp_path / 'ima.wav', 'wav', 'ima', False, _signal(C - 1, 2, 24), 8000)[0],
             wavgen.write_wav(tmp_path / 'u3.wav', wavgen.encode(_signal(257, 3, 25), 'u8'), 11025, 'u8')]
    bad = flacgen.encode(_flac_pcm(3000, 2, 26), 16000, 16, blocksize=1152)
    bad = bad[:-5] + bytes([bad[-5] ^ 0x5A]) + bad[-4:]         # inside the last frame: its CRC-16 no longer matches
    with open(tmp_path / 'bad.flac', 'wb') as f:
        f.write(bad)
    files.insert(4, str(tmp_path / 'bad.flac'))
    files.append(str(tmp_path / 'missing.wav'))
    before = seg.ctx.survey_stats(), seg.ctx.flac_stats(), seg.ctx.adpcm_stats()
    got = seg.survey_files(files)
    after = seg.ctx.survey_stats(), seg.ctx.flac_stats(), seg.ctx.adpcm_stats()
    assert after[0][0] - before[0][0] == 3 and after[0][1] - before[0][1] == 7      # stored bytes, FLAC, IMA: one launch each
    assert after[1][0] - before[1][0] == 1 and after[2][0] - before[2][0] == 1
    assert len(got) == len(files)
    for k, path in enumerate(files):
        if k in (4, 7):
            assert isinstance(got[k], str) and got[k].startswith('error: ') and os.path.basename(path) in got[k]
        else:
            same(got[k], seg.survey_channels(path))
            same(got[k], iss_io.survey_channels(path))
    assert 'CRC-16' in got[4]
    with pytest.raises(ValueError, match='CRC-16'):
        seg.survey_channels(files[4])
    split = seg.survey_files(files, batch_files=2)               # other passes, the same entries
    assert [type(s) for s in split] == [type(s) for s in got]
    for s, g in zip(split, got):
        if isinstance(g, ChannelSurvey):
            same(s, g)


def test_small_job_after_a_large_one(seg, C, tmp_path):
    long8 = wavgen.write_wav(tmp_path / 'l.wav', wavgen.encode(_signal(20 * C + 5, 8, 30), 'i16'), 48000, 'i16')
    short = wavgen.write_wav(tmp_path / 's.wav', wavgen.encode(_signal(300, 1, 31), 'i16'), 48000, 'i16')
    first = seg.survey_channels(long8)
    second = seg.survey_channels(short)
    third = seg.survey_channels(long8)
    same(third, first)
    same(second, iss_io.survey_channels(short))
    same(first, iss_io.survey_channels(long8))


def test_with_ffmpeg_the_calls_raise():
    s = Segmenter.__new__(Segmenter)
    s.ffmpeg = 'ffmpeg'
    with pytest.raises(ValueError, match='without ffmpeg'):
        s.survey_channels('a.wav')
    with pytest.raises(ValueError, match='without ffmpeg'):
        s.survey_files(['a.wav'])


# ------------------------------------------------------------------------------------------------ end to end
def test_out_of_phase_stereo_end_to_end(seg, tmp_path):
    """A stereo file with one side polarity-inverted: the default downmix cancels it and the plain call finds no energy; the
    survey names the pair, and channel 0 alone is segmented as the mono recording is."""
    left = np.maximum(read_wav_int16(os.path.join(GOLDEN, 'musanmix.wav')), -32767)
    path = wavgen.write_wav(tmp_path / 'oop.wav', np.stack([left, -left], axis=1).astype('<i2'), 16000, 'i16')
    survey = seg.survey_channels(path)
    same(survey, iss_io.survey_channels(path))
    assert survey.inverted() == [(0, 1)] and survey.corr(0, 1) == -1.0 and survey.downmix_loss_db == -math.inf
    assert survey.active() == [0, 1]
    plain = seg(path)
    speech = {'speech', 'male', 'female'}
    assert {lab for lab, _, _ in plain} == {'noEnergy'}
    alone, = seg.segment_channels(path, [0])
    assert speech & {lab for lab, _, _ in alone}
    assert alone == seg.segment_signal(left)


def test_active_channels_end_to_end(seg, tmp_path):
    n = 48000
    rng = np.random.default_rng(33)
    cols = [synth_pcm(1, n), np.zeros(n, dtype=np.int16), synth_pcm(2, n), rng.integers(-4, 5, size=n).astype(np.int16)]
    path = wavgen.write_wav(tmp_path / 'four.wav', np.stack(cols, axis=1).astype('<i2'), 16000, 'i16')
    survey = seg.survey_channels(path)
    same(survey, iss_io.survey_channels(path))
    assert survey.active() == [0, 2]
    assert seg.segment_channels(path, survey.active()) == seg.segment_channels(path, [0, 2])
