"""Time ranges of a file without ffmpeg (CPU): io.decode_excerpts -- the host builds of the decoders on the frames, blocks and
bytes of each excerpt alone -- against slices of the whole-file read, the windowed resample_ref and its input span, the
refusals, the bytes an excerpt reads from disk, and malformed frames / blocks inside and outside an excerpt.

Everything is bit-exact: an excerpt is twin[a:b], a = floor(start_sec * 16000 + 0.5), b = n16 or min(n16, floor(stop_sec *
16000 + 0.5)).  Ranges are given as sample / 16000, which that rounding maps back to the sample."""
import os

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from conftest import synth_pcm
from inaspeechsegmenter_amd import sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.segmenter import Segmenter

VAR_BLOCKS = [192, 4096, 17, 1, 4608, 100] * 3 + [2000]
IMA_SPB = 505                                                    # samples per 256-byte mono block


def sec(k):
    return k / 16000.0


def unit_ranges(bounds, n):
    """The ranges the issue lists, for a file of n samples (16 kHz mono) whose frames / blocks start at `bounds`: whole file,
    inside one unit, mid-unit to mid-unit across units, exactly on boundaries, the last partial unit, a stop past the end, two
    overlapping ranges and a repeated one -> [(start_sec, stop_sec | None)] and the (a, b) they mean."""
    bounds = sorted(set(bounds) | {n})
    big = next(i for i in range(len(bounds) - 1) if bounds[i + 1] - bounds[i] >= 500)
    lo = next(i for i in range(1, len(bounds)) if bounds[i] >= 450)              # a boundary with room before and after
    hi = next(i for i in range(lo + 1, len(bounds)) if bounds[i] - bounds[lo] >= 400 and i - lo >= 1)
    far = min(len(bounds) - 2, hi + 2)
    ab = [(0, n),
          (bounds[big] + 50, bounds[big] + 450),                                   # inside one unit
          (bounds[lo] - 7, bounds[far] + 5),                                       # starts and ends mid-unit
          (bounds[lo], bounds[hi]),                                                # exactly on boundaries
          (max(bounds[-2] - 13, n - 450) if n - bounds[-2] >= 400 else n - 450, n),   # the last (partial) unit
          (n - 1000, n),                                                           # stop_sec past the end: clamped
          (bounds[lo] - 300, bounds[hi] + 100), (bounds[lo] + 100, bounds[hi] + 300),  # overlapping
          (bounds[lo] - 7, bounds[far] + 5)]                                       # repeated
    ranges = [(sec(a), sec(b)) for a, b in ab]
    ranges[0] = (0, None)
    ranges[4] = (ranges[4][0], None)
    ranges[5] = (ranges[5][0], sec(n) + 5.0)
    return ranges, ab


def _flac_signal(n, bps, seed):
    x = synth_pcm(seed, n).astype(np.int64)
    return x if bps == 16 else x >> 8


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """name -> (path, frame / block starts).  All 16 kHz mono."""
    d = tmp_path_factory.mktemp('excerpts')
    out = {}
    n = 1152 * 10 + 500
    x = wavgen.make_signal(n, 1, 3)
    out['pcm16'] = (wavgen.write_wav(d / 'pcm16.wav', wavgen.encode(x, 'i16'), 16000, 'i16'), range(0, n, 1152))
    for kind in ('ulaw', 'alaw'):
        out[kind] = (sndgen.write(d / f'{kind}.wav', 'wav', kind, False, x, 16000)[0], range(0, n, 1152))
    out['aiff'] = (sndgen.write(d / 'be.aiff', 'aiff', 'i16', True, x, 16000)[0], range(0, n, 1152))
    nima = IMA_SPB * 20 + 123
    out['ima'] = (sndgen.write(d / 'ima.wav', 'wav', 'ima', False, wavgen.make_signal(nima, 1, 4), 16000, block_align=256)[0],
                  range(0, nima, IMA_SPB))
    spec = {'type': 'fixed', 'order': 2}
    out['flac16'] = (flacgen.write(d / 'f16.flac', _flac_signal(n, 16, 5), 16000, 16, blocksize=1152, subframe=spec), range(0, n, 1152))
    out['flac8'] = (flacgen.write(d / 'f8.flac', _flac_signal(n, 8, 6), 16000, 8, blocksize=1152, subframe=spec), range(0, n, 1152))
    out['flacvar'] = (flacgen.write(d / 'fvar.flac', _flac_signal(sum(VAR_BLOCKS), 16, 7), 16000, 16, blocksize=VAR_BLOCKS,
                                    variable=True), np.concatenate(([0], np.cumsum(VAR_BLOCKS)[:-1])))
    return out


@pytest.mark.parametrize('name', ['pcm16', 'ulaw', 'alaw', 'aiff', 'ima', 'flac16', 'flac8', 'flacvar'])
def test_decode_excerpts_equal_twin_slices(files, name):
    path, bounds = files[name]
    twin = iss_io.decode_pcm(path, ffmpeg=None)
    assert twin.dtype == np.int16
    ranges, ab = unit_ranges([int(b) for b in bounds], twin.size)
    got = iss_io.decode_excerpts(path, ranges)
    assert len(got) == len(ab)
    for g, (a, b), r in zip(got, ab, ranges):
        assert b - a >= 400, (a, b)
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, twin[a:b], err_msg=f'{name} {r} = [{a}, {b})')


def test_float_path_excerpts(tmp_path):
    """Float-path files (here a 32-bit float WAV and a 24-bit FLAC, 16 kHz mono) satisfy the same definition."""
    x = wavgen.make_signal(5000, 1, 8)
    f = wavgen.write_wav(tmp_path / 'f32.wav', wavgen.encode(x, 'f32'), 16000, 'f32')
    g = flacgen.write(tmp_path / 'f24.flac', synth_pcm(9, 5000).astype(np.int64) << 8, 16000, 24, blocksize=1152,
                      subframe={'type': 'fixed', 'order': 2})
    for path in (f, g):
        twin = iss_io.decode_pcm(path, ffmpeg=None)
        assert twin.dtype == np.float32
        got = iss_io.decode_excerpts(path, [(sec(700), sec(3000)), (sec(4000), None)])
        np.testing.assert_array_equal(got[0], twin[700:3000])
        np.testing.assert_array_equal(got[1], twin[4000:])


@pytest.mark.parametrize('what', ['wav44k2', 'ima8k', 'flac44k2', 'ulaw8k'])
def test_decode_excerpts_resampled_sources(tmp_path, what):
    """Sources at another rate or channel count: the excerpt is the slice of resample_ref of the whole file, computed from the
    input span of the window alone (the host twin of the staged-and-resampled device path)."""
    if what == 'wav44k2':
        path = wavgen.write_wav(tmp_path / 'a.wav', wavgen.encode(wavgen.make_signal(30000, 2, 1), 'i16'), 44100, 'i16')
    elif what == 'ima8k':
        path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, wavgen.make_signal(9000, 1, 2), 8000, block_align=256)[0]
    elif what == 'ulaw8k':
        path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ulaw', False, wavgen.make_signal(9000, 1, 2), 8000)[0]
    else:
        x = np.stack([synth_pcm(3, 30000), np.roll(synth_pcm(3, 30000), 29)], axis=1).astype(np.int64)
        path = flacgen.write(tmp_path / 'a.flac', x, 44100, 16, blocksize=1152, channel_mode='mid_side',
                             subframe={'type': 'fixed', 'order': 2})
    twin = R.resample_ref(*iss_io.decode_source(path))
    n16 = twin.size
    ab = [(0, 500), (3, 1003), (1234, 3734), (n16 - 777, n16), (0, n16)]
    got = iss_io.decode_excerpts(path, [(sec(a), sec(b)) for a, b in ab], resample=True)
    for g, (a, b) in zip(got, ab):
        np.testing.assert_array_equal(g, twin[a:b], err_msg=f'{what} [{a}, {b})')


# ------------------------------------------------------------------------------------------------ resample_ref windows
RATES = [(44100, 2), (8000, 1), (48000, 1)]


def _windows(n16):
    return [(0, 700), (3, 1500), (n16 - 900, 900), (1235, 2501)]          # (out_begin, out_count); the last: mid-file, not k * 1024


@pytest.mark.parametrize('sr,ch', RATES)
def test_resample_ref_window_is_the_slice(sr, ch):
    x = wavgen.encode(wavgen.make_signal(3 * sr // 4, ch, sr % 97), 'i16')
    full = R.resample_ref(x, sr)
    assert full.size == R.out_len(x.shape[0], sr)
    for ob, oc in _windows(full.size):
        np.testing.assert_array_equal(R.resample_ref(x, sr, ob, oc), full[ob:ob + oc])
        np.testing.assert_array_equal(R.resample_ref(x, sr, out_begin=ob, out_count=oc), full[ob:ob + oc])
    np.testing.assert_array_equal(R.resample_ref(x, sr, 0, None), full)


@pytest.mark.parametrize('sr,ch', RATES)
def test_input_span_suffices(sr, ch):
    """From only the frames [j_lo, j_hi] of a window (every other frame counts as zero) the result is the slice."""
    x = wavgen.encode(wavgen.make_signal(3 * sr // 4, ch, sr % 97), 'i16')
    n = x.shape[0]
    full = R.resample_ref(x, sr)
    for ob, oc in _windows(full.size):
        j_lo, j_hi = R.input_span(sr, n, ob, oc)
        assert 0 <= j_lo <= j_hi <= n - 1
        np.testing.assert_array_equal(R.resample_ref(x[j_lo:j_hi + 1], sr, ob, oc, j_lo, n), full[ob:ob + oc])


@pytest.mark.parametrize('sr,ch', [(44100, 2), (8000, 1)])
def test_input_span_is_tight(sr, ch):
    """One frame fewer at either end of a mid-file window changes the result, so the test above can fail.
    The samples are at full scale so that the outermost taps show in the PCM16 output.  (j_lo is the ceil form of the span's
    low end: the floor form names one more frame whenever the division is not exact, whose tap lies outside the table.  48 kHz
    is left out: with up = 1 the outermost taps of every output are the windowed sinc's zero crossings, |h| ~ 1e-19, so a
    missing end frame cannot show in any output, float64 included.)"""
    rng = np.random.default_rng(sr)
    x = rng.choice(np.array([-32768, 32767], dtype=np.int16), size=(3 * sr // 4, ch))
    x = x[:, 0] if ch == 1 else np.repeat(x[:, :1], ch, axis=1)                 # (equal channels: the mean stays at full scale)
    n = x.shape[0]
    ob, oc = 1235, 2501
    want = R.resample_ref(x, sr)[ob:ob + oc]
    j_lo, j_hi = R.input_span(sr, n, ob, oc)
    assert j_lo > 0 and j_hi < n - 1
    np.testing.assert_array_equal(R.resample_ref(x[j_lo:j_hi + 1], sr, ob, oc, j_lo, n), want)
    assert not np.array_equal(R.resample_ref(x[j_lo + 1:j_hi + 1], sr, ob, oc, j_lo + 1, n), want)
    assert not np.array_equal(R.resample_ref(x[j_lo:j_hi], sr, ob, oc, j_lo, n), want)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(files, tmp_path):
    path = files['pcm16'][0]
    n = iss_io.decode_pcm(path, ffmpeg=None).size
    for bad in (-0.5, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match=r'pcm16\.wav.*start_sec'):
            iss_io.decode_excerpts(path, [(bad, None)])
    for start, stop in ((0.5, 0.5), (0.5, 0.25), (0.0, 0.0)):
        with pytest.raises(ValueError, match=r'pcm16\.wav.*stop_sec.*not after start_sec'):
            iss_io.decode_excerpts(path, [(start, stop)])
    for start in (sec(n), sec(n) + 3.0):
        with pytest.raises(ValueError, match=r'pcm16\.wav.*past the end of the file.*%.3f s' % sec(n)):
            iss_io.decode_excerpts(path, [(start, None)])
    with pytest.raises(ValueError, match=r'media .*pcm16\.wav: 399 samples, less than one 25 ms analysis window'):
        iss_io.decode_excerpts(path, [(sec(100), sec(499))])
    with pytest.raises(ValueError, match=r'media .*pcm16\.wav: 10 samples, less than one 25 ms analysis window'):
        iss_io.decode_excerpts(path, [(sec(n - 10), None)])
    assert iss_io.decode_excerpts(path, [(sec(100), sec(500))])[0].size == 400
    # a good range in front of a bad one: nothing comes back
    with pytest.raises(ValueError):
        iss_io.decode_excerpts(path, [(0, None), (0.5, 0.25)])
    # the refusals of a range are made before the file is opened
    with pytest.raises(ValueError, match='start_sec'):
        iss_io.decode_excerpts(str(tmp_path / 'no_such_file.wav'), [(-1.0, None)])


def test_not_16k_mono_is_refused_as_today(tmp_path):
    f = wavgen.write_wav(tmp_path / 'a.wav', wavgen.encode(wavgen.make_signal(30000, 2, 1), 'i16'), 44100, 'i16')
    with pytest.raises(AssertionError, match='44100 Hz'):                        # the rate first, as decode_pcm
        iss_io.decode_excerpts(f, [(0, None)])
    with pytest.raises(AssertionError, match='44100 Hz'):
        iss_io.decode_pcm(f, ffmpeg=None)
    g = wavgen.write_wav(tmp_path / 'b.wav', wavgen.encode(wavgen.make_signal(30000, 2, 1), 'i16'), 16000, 'i16')
    with pytest.raises(ValueError, match='2 channels'):
        iss_io.decode_excerpts(g, [(0, None)])


def test_entry_points_that_keep_refusing(files):
    path = files['pcm16'][0]
    with pytest.raises(NotImplementedError):
        iss_io.decode_pcm(path, start_sec=1.0, ffmpeg=None)
    seg = Segmenter.__new__(Segmenter)                                           # (a double: no device, no networks)
    seg.ffmpeg, seg.resample = 'ffmpeg', False
    for method in (seg.segment_excerpts, seg.load_pcm_excerpts):
        with pytest.raises(ValueError, match=r'start_sec / stop_sec.*__call__'):
            method(path, [(0, None)])


# ------------------------------------------------------------------------------------------------ bytes read
@pytest.fixture()
def counted(monkeypatch):
    calls = []
    real = iss_io._read_range

    def counting(path, offset, size):
        buf = real(path, offset, size)
        calls.append((offset, size))
        return buf
    monkeypatch.setattr(iss_io, '_read_range', counting)
    return calls


def _ten_minutes(tmp_path, what):
    """A 10-minute file, written from one second of signal repeated (IMA blocks are independent: encoded once)."""
    if what == 'pcm16k':
        sec1 = wavgen.encode(wavgen.make_signal(16000, 1, 1), 'i16')
        return wavgen.write_wav(tmp_path / 'long.wav', np.tile(sec1, 600), 16000, 'i16'), False
    if what == 'pcm48k2':
        sec1 = wavgen.encode(wavgen.make_signal(48000, 2, 2), 'i16')
        return wavgen.write_wav(tmp_path / 'long.wav', np.tile(sec1, (600, 1)), 48000, 'i16'), True
    blocks = sndgen.ima_encode(wavgen.encode(wavgen.make_signal(IMA_SPB * 32, 1, 3), 'i16'), 256)
    data = bytes(blocks) * 594                                                    # 32 * 594 blocks of 505 samples: 10 min
    return sndgen.write_riff(tmp_path / 'long.wav', sndgen.wav_fmt('ima', 16000, 1, 256), data, fact=IMA_SPB * 32 * 594), False


@pytest.mark.parametrize('what', ['pcm16k', 'pcm48k2', 'ima16k'])
def test_an_excerpt_reads_only_its_bytes(tmp_path, counted, what):
    """A 2 s excerpt in the middle of a 10-minute file: header plus span, capped at 0.5 % of the file (the issue: under 1 %)."""
    path, resample = _ten_minutes(tmp_path, what)
    size = os.path.getsize(path)
    got = iss_io.decode_excerpts(path, [(300.0, 302.0)], resample=resample)[0]
    assert got.size == 32000
    asked = sum(s for _, s in counted)
    assert asked < 0.005 * size, (asked, size)
    assert all(o + s <= size for o, s in counted)
    del counted[:]
    # ... and they are the right bytes (the whole-file read is the reference; it does not go through the counter)
    if resample:
        want = R.resample_ref(*iss_io.decode_source(path))[300 * 16000:302 * 16000]
    else:
        want = iss_io.decode_pcm(path, ffmpeg=None)[300 * 16000:302 * 16000]
    assert not counted
    np.testing.assert_array_equal(got, want)


def test_data_chunk_behind_a_large_chunk(tmp_path, counted):
    x = wavgen.make_signal(20000, 1, 5)
    path = sndgen.write_riff(tmp_path / 'junk.wav', sndgen.wav_fmt('i16', 16000, 1), wavgen.encode(x, 'i16').tobytes(),
                             before=[(b'JUNK', bytes(1 << 20))], after=[(b'LIST', b'INFOabcd')])
    got = iss_io.decode_excerpts(path, [(sec(5000), sec(9000)), (sec(19000), None)])
    twin = iss_io.decode_pcm(path, ffmpeg=None)
    assert twin.size == 20000
    np.testing.assert_array_equal(got[0], twin[5000:9000])
    np.testing.assert_array_equal(got[1], twin[19000:])
    assert sum(s for _, s in counted) < 2 * (4000 + 1000) + 200              # the JUNK megabyte is skipped, not read


def test_aiff_ssnd_offset(tmp_path):
    """A layout whose samples are found only from the whole file's chunks stays correct (read whole, cut from its bytes)."""
    x = wavgen.make_signal(6000, 1, 6)
    data, _, twin, n = sndgen.encode(x, 'i16', big=True)
    path = sndgen.write_aiff(tmp_path / 'o.aiff', 'i16', True, data, 16000, 1, n, ssnd_offset=10, before=[(b'ANNO', b'x' * 33)])
    np.testing.assert_array_equal(iss_io.decode_pcm(path, ffmpeg=None), twin)
    got = iss_io.decode_excerpts(path, [(sec(1000), sec(2500))])[0]
    np.testing.assert_array_equal(got, twin[1000:2500])


# ------------------------------------------------------------------------------------------------ malformed input
def test_flac_bad_frame_inside_and_outside(tmp_path):
    x = _flac_signal(1152 * 8, 16, 11)
    data, offs = flacgen.encode(x, 16000, 16, blocksize=1152, subframe={'type': 'fixed', 'order': 2}, return_offsets=True)
    clean = tmp_path / 'clean.flac'
    clean.write_bytes(data)
    twin = iss_io.decode_pcm(str(clean), ffmpeg=None)
    bad = bytearray(data)
    bad[offs[6] - 4] ^= 0x10                                                      # inside frame 5, in front of its CRC-16
    path = tmp_path / 'bad.flac'
    path.write_bytes(bytes(bad))
    inside = (sec(1152 * 4 + 100), sec(1152 * 5 + 600))                           # frames 4 and 5
    with pytest.raises(ValueError, match=r'bad\.flac: frame at byte %d: ' % offs[5]):
        iss_io.decode_excerpts(str(path), [inside])
    with pytest.raises(ValueError, match=r'bad\.flac: frame at byte %d: ' % offs[5]):
        iss_io.decode_pcm(str(path), ffmpeg=None)
    a, b = 1152 * 2 + 100, 1152 * 5                                               # frames 2 to 4; ends where frame 5 starts
    got = iss_io.decode_excerpts(str(path), [(sec(a), sec(b)), (sec(1152 * 6), None)])
    np.testing.assert_array_equal(got[0], twin[a:b])
    np.testing.assert_array_equal(got[1], twin[1152 * 6:])


def test_ima_bad_block_inside_and_outside(tmp_path):
    x = wavgen.make_signal(IMA_SPB * 12, 1, 12)
    clean, _, twin = sndgen.write(tmp_path / 'clean.wav', 'wav', 'ima', False, x, 16000, block_align=256)
    base = sndfmt.parse(open(clean, 'rb').read(), clean).base
    bad = bytearray(open(clean, 'rb').read())
    bad[base + 7 * 256 + 2] = 89                                                  # block 7: step index above 88
    path = tmp_path / 'bad.wav'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.wav: block at byte %d: step index above 88' % (base + 7 * 256)):
        iss_io.decode_excerpts(str(path), [(sec(IMA_SPB * 6 + 10), sec(IMA_SPB * 7 + 450))])
    a, b = IMA_SPB * 4 + 10, IMA_SPB * 7                                          # blocks 4 to 6
    got = iss_io.decode_excerpts(str(path), [(sec(a), sec(b)), (sec(IMA_SPB * 8), None)])
    np.testing.assert_array_equal(got[0], twin[a:b])
    np.testing.assert_array_equal(got[1], twin[IMA_SPB * 8:])
