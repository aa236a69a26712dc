"""GPU: time ranges of a file cut on the device.  Segmenter.load_pcm_excerpts must return exactly the slices of
Segmenter.load_pcm (the windowed resample, FLAC and IMA ADPCM kernels against their whole-file launches), segment_excerpts exactly
what segment_signal gives on those slices, all ranges of a call in one pass, malformed frames / blocks reported by their
offset in the file when they are among the decoded ones, and the unwindowed calls unchanged afterwards.  Every comparison is exact.
The shapes are the smallest at which each window can go wrong: a = 0, a inside the filter's reach of the file start, both ends
off the tile / frame / block grid, the last output, one sample, offsets past 2^31."""
import os
import warnings

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from conftest import GOLDEN, synth_pcm
from test_excerpts import IMA_SPB, VAR_BLOCKS, sec, unit_ranges
from inaspeechsegmenter_amd import _native, Segmenter, sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _check_slices(seg, path, ab, ranges=None):
    """load_pcm_excerpts of the sample ranges `ab` against the slices of load_pcm -> the whole-file samples."""
    twin = seg.load_pcm(path)
    ranges = [(sec(a), sec(b)) for a, b in ab] if ranges is None else ranges
    got = seg.load_pcm_excerpts(path, ranges)
    assert len(got) == len(ab)
    for g, (a, b) in zip(got, ab):
        assert 0 <= a < b <= twin.size and g.dtype == twin.dtype
        np.testing.assert_array_equal(g, twin[a:b], err_msg=f'{os.path.basename(path)} [{a}, {b})')
    return twin


def _window_direct(ctx, x, sr, fmt, out_begin, out_count, frames_total=None, in_begin=None):
    """The native wrapper with one window: stage the input span of `x` (the file's frames, or -- with in_begin -- its frames
    from there on) and resample outputs [out_begin, +out_count) into a signal of their own."""
    total = x.shape[0] if frames_total is None else frames_total
    j_lo, j_hi = R.input_span(sr, total, out_begin, out_count)
    part = np.ascontiguousarray(x[j_lo:j_hi + 1] if in_begin is None else x[j_lo - in_begin:j_hi + 1 - in_begin])
    assert part.shape[0] == j_hi - j_lo + 1
    fid, _, _ = ctx.resample_filter(sr)
    job = (0, part.shape[0], 1 if part.ndim == 1 else part.shape[1], fmt, fid, 0, 0, out_count)
    ctx.resample(part.reshape(-1).view(np.uint8), [job], n_signal=out_count, windows=[(j_lo, j_hi + 1, total, out_begin, out_count)])
    return ctx.get_signal_pcm16(0, out_count)


def _resample_windows(n16):
    return [(0, 700), (3, 1003), (1234, 3734), (n16 - 900, n16)]


# ------------------------------------------------------------------------------------------------ resample kernel
def test_resample_plain_instantiation(seg, tmp_path):
    x = wavgen.encode(wavgen.make_signal(44100, 2, 1), 'i16')
    path = wavgen.write_wav(tmp_path / 'a.wav', x, 44100, 'i16')
    twin = _check_slices(seg, path, _resample_windows(16000))
    assert twin.size == 16000
    np.testing.assert_array_equal(twin, R.resample_ref(x, 44100))
    for i in (0, 5000, 15999):                                                   # a window of one sample
        np.testing.assert_array_equal(_window_direct(seg.ctx, x, 44100, _native.RS_FORMAT[x.dtype], i, 1), twin[i:i + 1])


@pytest.mark.parametrize('what', ['ulaw8k', 'aiff48k_be32'])
def test_resample_ext_instantiation(seg, tmp_path, what):
    if what == 'ulaw8k':
        path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ulaw', False, wavgen.make_signal(8000, 1, 2), 8000)[0]
    else:                                                                        # 24-bit values in 32-bit big-endian words
        x = np.round(wavgen.make_signal(48000, 1, 3) * 2 ** 23) / 2 ** 23
        path = sndgen.write(tmp_path / 'a.aiff', 'aiff', 'i32', True, x, 48000)[0]
    twin = _check_slices(seg, path, _resample_windows(16000))
    assert twin.size == 16000
    snd = sndfmt.parse(open(path, 'rb').read(), path)
    raw, fmt = snd.raw()
    assert fmt > 4                                                               # a format of the EXT instantiation
    for i in (0, 5000, 15999):
        np.testing.assert_array_equal(_window_direct(seg.ctx, raw, snd.sr, fmt, i, 1), twin[i:i + 1])


def test_resample_table_read_through_cache(seg, tmp_path):
    """44 056 Hz: 110 141 taps, more than LDS holds next to the span."""
    x = wavgen.encode(wavgen.make_signal(30000, 1, 4), 'i16')
    path = wavgen.write_wav(tmp_path / 'a.wav', x, 44056, 'i16')
    assert R.plan(44056)[2].size == 110141
    _check_slices(seg, path, [(3000, 4500)])


def test_resample_offsets_past_2_31(seg):
    """A window 7 000 000 outputs into a 44.1 kHz file declared 30 000 000 frames long, staged for the span only:
    out_begin * down = 3.09e9."""
    total, a, count = 30_000_000, 7_000_000, 3000
    j_lo, j_hi = R.input_span(44100, total, a, count)
    assert a * 441 > 2 ** 31 and j_lo * 2 > 2 ** 24
    x = wavgen.encode(wavgen.make_signal(j_hi - j_lo + 1, 1, 5), 'i16')
    got = _window_direct(seg.ctx, x, 44100, _native.RS_FORMAT[x.dtype], a, count, frames_total=total, in_begin=j_lo)
    np.testing.assert_array_equal(got, R.resample_ref(x, 44100, a, count, j_lo, total))


def test_planner_refuses_a_window_that_reaches_unstaged_frames(seg):
    x = wavgen.encode(wavgen.make_signal(20000, 1, 6), 'i16')
    fid, _, _ = seg.ctx.resample_filter(44100)
    j_lo, j_hi = R.input_span(44100, 20000, 1234, 2500)
    for lo, hi in ((j_lo + 1, j_hi + 1), (j_lo, j_hi)):                          # one frame short at either end
        part = np.ascontiguousarray(x[lo:hi])
        with pytest.raises(_native.NativeError, match='reach'):
            seg.ctx.resample(part.view(np.uint8), [(0, part.size, 1, 1, fid, 0, 0, 2500)], n_signal=2500,
                             windows=[(lo, hi, 20000, 1234, 2500)])


# ------------------------------------------------------------------------------------------------ FLAC
def _flac_int(n, ch, bps, seed):
    base = synth_pcm(seed, n).astype(np.int64)
    x = np.stack([np.roll(base, 29 * c) - 40 * c for c in range(ch)], axis=1)
    x = (x << 8) + np.random.default_rng(seed).integers(-128, 128, x.shape) if bps == 24 else x
    x = np.clip(x, -(1 << (bps - 1)), (1 << (bps - 1)) - 1)
    return x[:, 0] if ch == 1 else x


@pytest.mark.parametrize('what', ['bs1152', 'lpc32', 'variable'])
def test_flac_to_signal(seg, tmp_path, what):
    if what == 'bs1152':
        n, kw, bounds = 1152 * 10 + 500, {'blocksize': 1152}, range(0, 1152 * 10 + 500, 1152)
    elif what == 'lpc32':
        n, kw, bounds = 20231, {'subframe': {'type': 'lpc', 'order': 32, 'precision': 15}}, range(0, 20231, 4096)
    else:
        n, kw = sum(VAR_BLOCKS), {'blocksize': VAR_BLOCKS, 'variable': True}
        bounds = np.concatenate(([0], np.cumsum(VAR_BLOCKS)[:-1]))
    path = flacgen.write(tmp_path / 'a.flac', _flac_int(n, 1, 16, 7), 16000, 16, **kw)
    ranges, ab = unit_ranges([int(b) for b in bounds], n)
    twin = _check_slices(seg, path, ab, ranges)
    np.testing.assert_array_equal(twin, iss_io.decode_pcm(path, ffmpeg=None))


@pytest.mark.parametrize('sr,bps,mode', [(44100, 16, 'mid_side'), (48000, 24, 'side_right')])
def test_flac_to_stage_and_resample(seg, tmp_path, sr, bps, mode):
    n = sr // 2
    path = flacgen.write(tmp_path / 'a.flac', _flac_int(n, 2, bps, 8), sr, bps, blocksize=1152, channel_mode=mode,
                         subframe={'type': 'fixed', 'order': 2})
    n16 = R.out_len(n, sr)
    twin = _check_slices(seg, path, [(3, 1003), (1234, 3734), (n16 - 900, n16)])
    np.testing.assert_array_equal(twin, R.resample_ref(*iss_io.decode_source(path)))


# ------------------------------------------------------------------------------------------------ IMA ADPCM
@pytest.mark.parametrize('sr,ch,align', [(16000, 1, 256), (8000, 1, 256), (16000, 2, 512)])
def test_ima(seg, tmp_path, sr, ch, align):
    spb = sndgen.ima_samples_per_block(align, ch)
    n = spb * 12 + 123                                                           # the last block is cut by the `fact` count
    path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, wavgen.make_signal(n, ch, 9), sr, block_align=align)[0]
    n16 = R.out_len(n, sr)
    k = n16 // n if sr != 16000 else 1                                           # outputs per stored sample (8 kHz: 2)
    ab = [(k * (spb * 3 + 20), k * (spb * 3 + 20) + 420),                         # mid-block
          (k * (spb * 5) - 250, k * (spb * 5) + 250),                            # across a block boundary
          (n16 - 410, n16),                                                      # the last, partial block
          (0, n16)]
    twin = _check_slices(seg, path, ab)
    want = iss_io.decode_source(path)
    np.testing.assert_array_equal(twin, want[0] if (sr, ch) == (16000, 1) else R.resample_ref(*want))


# ------------------------------------------------------------------------------------------------ segmentation
RANGES = [(0, 4.0), (2.5, 9.0), (6.0, None), (2.5, 9.0)]


@pytest.fixture(scope='module')
def musan(tmp_path_factory):
    """12 s of musanmix.wav as 16 kHz mono FLAC and as 48 kHz stereo WAV (both channels the same)."""
    import scipy.signal
    d = tmp_path_factory.mktemp('musan')
    pcm = iss_io.decode_pcm(os.path.join(GOLDEN, 'musanmix.wav'), ffmpeg=None)[16000 * 10:16000 * 22]
    f = flacgen.write(d / 'm.flac', pcm.astype(np.int64), 16000, 16, subframe={'type': 'fixed', 'order': 2})
    up = scipy.signal.resample_poly(pcm.astype(np.float64) / 32768.0, 3, 1)
    w = wavgen.write_wav(d / 'm48.wav', wavgen.encode(np.stack([up, up], axis=1) * 0.9, 'i16'), 48000, 'i16')
    return {'flac': f, 'wav48': w}


@pytest.mark.parametrize('what', ['flac', 'wav48'])
def test_segment_excerpts_equal_segment_signal(seg, musan, what):
    path = musan[what]
    twin = seg.load_pcm(path)
    assert twin.size == 16000 * 12
    ctx = seg.ctx
    before = ctx.resample_stats(), ctx.flac_stats()
    got = seg.segment_excerpts(path, RANGES)
    after = ctx.resample_stats(), ctx.flac_stats()
    # one pass: one launch per kernel class for the four excerpts
    if what == 'flac':
        assert after[1][0] - before[1][0] == 1 and after[0] == before[0]
    else:
        assert (after[0][0] - before[0][0], after[0][1] - before[0][1]) == (1, 4) and after[1] == before[1]
    assert len(got) == len(RANGES)
    for g, (start, stop) in zip(got, RANGES):
        a, b = iss_io.excerpt_bounds(path, twin.size, start, stop)
        assert g == seg.segment_signal(twin[a:b], start_sec=start), (what, start, stop)
        assert g[0][1] == start
    assert got[1] == got[3]


def test_flac_frames_of_a_pass_are_the_covering_ones(seg, musan):
    """flac_stats counts the frames decoded: for the four excerpts, those that cover them (4096 samples each) and no others."""
    before = seg.ctx.flac_stats()
    seg.load_pcm_excerpts(musan['flac'], RANGES)
    after = seg.ctx.flac_stats()
    n = 16000 * 12
    want = sum((min(n, b) - 1) // 4096 - a // 4096 + 1 for a, b in ((0, 64000), (40000, 144000), (96000, n), (40000, 144000)))
    assert after[0] - before[0] == 1 and after[1] - before[1] == want


def test_short_excerpt_takes_the_short_media_path(seg, musan):
    twin = seg.load_pcm(musan['flac'])
    with pytest.warns(UserWarning, match='duration is short'):
        got = seg.segment_excerpts(musan['flac'], [(3.0, 3.5)])[0]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert got == seg.segment_signal(twin[48000:56000], start_sec=3.0)


def test_ima_excerpts_share_one_pass(seg, tmp_path):
    n = 16000 * 3
    path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, wavgen.make_signal(n, 2, 10), 16000, block_align=512)[0]
    twin = seg.load_pcm(path)
    ranges = [(0, 1.0), (0.5, 2.0), (1.5, None), (0.5, 2.0)]
    ctx = seg.ctx
    before = ctx.adpcm_stats(), ctx.resample_stats()
    got = seg.segment_excerpts(path, ranges)
    after = ctx.adpcm_stats(), ctx.resample_stats()
    assert after[0][0] - before[0][0] == 1
    assert (after[1][0] - before[1][0], after[1][1] - before[1][1]) == (1, 4)
    for g, (start, stop) in zip(got, ranges):
        a, b = iss_io.excerpt_bounds(path, twin.size, start, stop)
        assert g == seg.segment_signal(twin[a:b], start_sec=start)


def test_limits_split_a_request_into_passes(seg, musan):
    before = seg.ctx.flac_stats()
    got = seg.segment_excerpts(musan['flac'], RANGES, batch_files=3)
    assert seg.ctx.flac_stats()[0] - before[0] == 2
    assert got == seg.segment_excerpts(musan['flac'], RANGES)


# ------------------------------------------------------------------------------------------------ errors on the device path
def test_flac_bad_frame_inside_and_outside(seg, tmp_path):
    data, offs = flacgen.encode(_flac_int(1152 * 8, 1, 16, 11), 16000, 16, blocksize=1152, subframe={'type': 'fixed', 'order': 2},
                                return_offsets=True)
    clean = tmp_path / 'clean.flac'
    clean.write_bytes(data)
    twin = seg.load_pcm(str(clean))
    bad = bytearray(data)
    bad[offs[6] - 4] ^= 0x10                                                      # inside frame 5, in front of its CRC-16
    path = tmp_path / 'bad.flac'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.flac: frame at byte %d: ' % offs[5]):
        seg.load_pcm_excerpts(str(path), [(sec(1152 * 4 + 100), sec(1152 * 5 + 600))])
    a, b = 1152 * 2 + 100, 1152 * 5
    got = seg.load_pcm_excerpts(str(path), [(sec(a), sec(b)), (sec(1152 * 6), None)])
    np.testing.assert_array_equal(got[0], twin[a:b])
    np.testing.assert_array_equal(got[1], twin[1152 * 6:])


def test_ima_bad_block_inside_and_outside(seg, tmp_path):
    clean, _, _ = sndgen.write(tmp_path / 'clean.wav', 'wav', 'ima', False, wavgen.make_signal(IMA_SPB * 12, 1, 12), 16000,
                               block_align=256)
    twin = seg.load_pcm(clean)
    base = sndfmt.parse(open(clean, 'rb').read(), clean).base
    bad = bytearray(open(clean, 'rb').read())
    bad[base + 7 * 256 + 2] = 89
    path = tmp_path / 'bad.wav'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.wav: block at byte %d: step index above 88' % (base + 7 * 256)):
        seg.load_pcm_excerpts(str(path), [(sec(IMA_SPB * 6 + 10), sec(IMA_SPB * 7 + 450))])
    a, b = IMA_SPB * 4 + 10, IMA_SPB * 7
    got = seg.load_pcm_excerpts(str(path), [(sec(a), sec(b)), (sec(IMA_SPB * 8), None)])
    np.testing.assert_array_equal(got[0], twin[a:b])
    np.testing.assert_array_equal(got[1], twin[IMA_SPB * 8:])


# ------------------------------------------------------------------------------------------------ unwindowed calls untouched
def test_unwindowed_calls_after_windowed_ones(seg, tmp_path):
    """The job tables and staging buffers a windowed call leaves behind do not reach the next whole-file call."""
    f = flacgen.write(tmp_path / 'a.flac', _flac_int(22050, 2, 16, 13), 44100, 16, blocksize=1152, channel_mode='mid_side',
                      subframe={'type': 'fixed', 'order': 2})
    i = sndgen.write(tmp_path / 'i.wav', 'wav', 'ima', False, wavgen.make_signal(IMA_SPB * 9 + 50, 1, 14), 8000, block_align=256)[0]
    w = wavgen.write_wav(tmp_path / 'w.wav', wavgen.encode(wavgen.make_signal(22050, 2, 15), 'i16'), 44100, 'i16')
    for path in (f, i, w):
        want = R.resample_ref(*iss_io.decode_source(path))
        got = seg.load_pcm_excerpts(path, [(sec(1500), sec(4000)), (sec(100), sec(7000))])
        np.testing.assert_array_equal(got[0], want[1500:4000])
        np.testing.assert_array_equal(got[1], want[100:7000])
        np.testing.assert_array_equal(seg.load_pcm(path), want)
