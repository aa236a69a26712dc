"""GPU: time ranges of single channels, cut and split on the device.  The WIN + SPLIT instantiations of resample_kernel through
ctx.resample(..., windows=..., splits=...) against the windowed resample.resample_ref of each stored column, staged for the
window's input span only; the planner's refusals; FLAC and IMA ADPCM through Segmenter.load_pcm_channel_excerpts against slices
of load_pcm_channels; segment_channel_excerpts against segment_signal on those slices; and the plain, windows-only and
splits-only calls afterwards.  Every comparison is exact.
The shapes are the smallest at which the joint instantiation can go wrong: a = 0, a inside the filter's reach of the file
start, a window over more than two tiles that starts off the tile grid with in_begin > 0, the last output, one sample,
selections that are not the identity, more channels than one group holds, the identity filter, a filter table too large for
LDS, offsets past 2^31."""
import warnings

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from conftest import synth_pcm
from test_channels import flac_int
from test_excerpts import sec
from inaspeechsegmenter_amd import _native, Segmenter, pipeline, sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _hop(n):
    return -(-n // 160) * 160


def _staged(x, sr, a, count, total=None, in_begin=0):
    """-> (the frames of `x` -- the file's frames from in_begin on -- that carry a tap of outputs [a, a + count), the window row)."""
    total = x.shape[0] if total is None else total
    j_lo, j_hi = R.input_span(sr, total, a, count)
    part = np.ascontiguousarray(x[j_lo - in_begin:j_hi + 1 - in_begin])
    assert part.shape[0] == j_hi - j_lo + 1
    return part, (j_lo, j_hi + 1, total, a, count)


def _joint_direct(ctx, raw, sr, fmt, sel, a, count, stored=None, total=None, in_begin=0):
    """One windowed split job on its own, staged for the window's span only: -> the whole signal (len(sel) strides), checked
    against the windowed resample_ref of every selected column of `stored` (what the host reads for `raw`), with the samples
    between a channel's end and the next stride still zero."""
    part, win = _staged(raw, sr, a, count, total, in_begin)
    ref, _ = _staged(raw if stored is None else stored, sr, a, count, total, in_begin)
    fid, _, _ = ctx.resample_filter(sr)
    stride = _hop(count)
    job = (0, part.shape[0], part.shape[1], fmt, fid, 0, 0, count)
    before = ctx.resample_stats()
    ctx.resample(part.reshape(-1).view(np.uint8), [job], n_signal=len(sel) * stride, windows=[win], splits=[(stride, sel)])
    sig = ctx.get_signal_pcm16(0, len(sel) * stride)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)            # a windowed split job counts as one job
    for k, c in enumerate(sel):
        want = R.resample_ref(ref[:, c], sr, a, count, win[0], win[2])
        np.testing.assert_array_equal(sig[k * stride:k * stride + count], want, err_msg=f'[{a}, +{count}) selected {k} = channel {c}')
        assert not sig[k * stride + count:(k + 1) * stride].any()
    return sig


def _windows(n16):
    return [(0, 700), (3, 1000), (1234, 2500), (n16 - 900, 900)]      # (out_begin, out_count)


# ------------------------------------------------------------------------------------------------ kernel
def test_joint_plain_instantiation(seg):
    """44.1 kHz stereo i16, 13 230 frames -> 4 800 outputs per channel, tile 1 024: (1234, 3734) spans more than two tiles,
    starts off the tile grid and has in_begin > 0."""
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(13230, 2, 41), 'i16')
    fmt = _native.RS_FORMAT[x.dtype]
    assert R.out_len(13230, 44100) == 4800 and ctx.resample_split_geometry(44100, 2) == (1024, 2)
    assert R.input_span(44100, 13230, 1234, 2500)[0] > 0
    full = [R.resample_ref(x[:, c], 44100) for c in range(2)]
    for sel in ([0, 1], [1, 0]):
        for a, count in _windows(4800) + [(0, 1), (2400, 1), (4799, 1)]:
            sig = _joint_direct(ctx, x, 44100, fmt, sel, a, count)
            for k, c in enumerate(sel):                                          # ... which is the whole-file result's slice
                np.testing.assert_array_equal(sig[k * _hop(count):k * _hop(count) + count], full[c][a:a + count])


@pytest.mark.parametrize('sr,fmt,ch,n', [(48000, 'f32', 3, 15000), (16000, 'i16', 2, 4000)])
def test_joint_further_shapes(seg, sr, fmt, ch, n):
    x = wavgen.encode(wavgen.make_signal(n, ch, 42), fmt)
    n16 = R.out_len(n, sr)
    for sel in (list(range(ch)), [ch - 1, 0]):
        for a, count in _windows(n16):
            sig = _joint_direct(seg.ctx, x, sr, _native.RS_FORMAT[x.dtype], sel, a, count)
            if sr == 16000:                                                      # the identity filter: the stored values
                np.testing.assert_array_equal(sig[:count], x[a:a + count, sel[0]])


def test_joint_ext_instantiation(seg, tmp_path):
    path = sndgen.write(tmp_path / 'u.wav', 'wav', 'ulaw', False, wavgen.make_signal(3000, 2, 43), 8000)[0]
    snd = sndfmt.parse(open(path, 'rb').read(), path)
    raw, fmt = snd.raw()
    assert fmt == _native.RS_ULAW
    for a, count in _windows(6000):
        _joint_direct(seg.ctx, raw, 8000, fmt, [1, 1, 0], a, count, snd.stored())


def test_joint_table_read_through_cache(seg):
    """44 056 Hz: 110 141 taps, more than LDS holds next to the spans."""
    assert R.plan(44056)[2].size == 110141
    x = wavgen.encode(wavgen.make_signal(30000, 2, 44), 'i16')
    _joint_direct(seg.ctx, x, 44056, _native.RS_FORMAT[x.dtype], [0, 1], 3000, 1500)


def test_joint_more_channels_than_a_group(seg):
    ctx = seg.ctx
    tile, group = ctx.resample_split_geometry(22050, 11)
    assert group < 11 and -(-11 // group) > 1                                   # 11 channels need more than one group
    assert 2500 > 2 * tile
    x = wavgen.encode(wavgen.make_signal(6000, 11, 45), 'i16')
    fmt = _native.RS_FORMAT[x.dtype]
    for sel in ([10, 0, 7, 7, 3], list(range(11)), list(range(10, -1, -1))):
        _joint_direct(ctx, x, 22050, fmt, sel, 1234, 2500)


def test_joint_offsets_past_2_31(seg):
    """A window 7 000 000 outputs into a 44.1 kHz stereo file declared 30 000 000 frames long, staged for the span only:
    out_begin * down = 3.09e9."""
    total, a, count = 30_000_000, 7_000_000, 3000
    j_lo, j_hi = R.input_span(44100, total, a, count)
    assert a * 441 > 2 ** 31 and j_lo * 4 > 2 ** 24
    x = wavgen.encode(wavgen.make_signal(j_hi - j_lo + 1, 2, 46), 'i16')
    _joint_direct(seg.ctx, x, 44100, _native.RS_FORMAT[x.dtype], [1, 0], a, count, total=total, in_begin=j_lo)


def test_one_launch_mixed(seg):
    """Two windows of file A with a selection, one window of file B downmixed, one window of A downmixed: one launch, four
    jobs; afterwards the plain, windows-only and splits-only entry points on the same inputs."""
    ctx = seg.ctx
    A = wavgen.encode(wavgen.make_signal(13230, 2, 47), 'i16')
    B = wavgen.encode(wavgen.make_signal(15000, 3, 48), 'f32')
    fa, fb = ctx.resample_filter(44100)[0], ctx.resample_filter(48000)[0]
    cases = [(A, 44100, fa, (1234, 2500), [0, 1]), (A, 44100, fa, (3, 1000), [1, 0]), (B, 48000, fb, (700, 2100), None),
             (A, 44100, fa, (3900, 900), None)]
    jobs, wins, splits, parts, dsts, pos, bpos = [], [], [], [], [], 0, 0
    for x, sr, fid, (a, count), sel in cases:
        part, win = _staged(x, sr, a, count)
        jobs.append((bpos, part.shape[0], part.shape[1], _native.RS_FORMAT[x.dtype], fid, 0, pos, count))
        wins.append(win)
        splits.append(None if sel is None else (_hop(count), sel))
        parts.append(part.reshape(-1).view(np.uint8))
        pad = -part.nbytes % 16
        if pad:
            parts.append(np.zeros(pad, np.uint8))
        bpos += part.nbytes + pad
        dsts.append(pos)
        pos += _hop(count) * (1 if sel is None else len(sel))
    staged = np.concatenate(parts)
    before = ctx.resample_stats()
    ctx.resample(staged, jobs, n_signal=pos, windows=wins, splits=splits)
    sig = ctx.get_signal_pcm16(0, pos)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 4)
    written = np.zeros(pos, bool)
    for (x, sr, fid, (a, count), sel), dst in zip(cases, dsts):
        for k, c in enumerate([None] if sel is None else sel):
            want = R.resample_ref(x if c is None else x[:, c], sr)[a:a + count]
            o = dst + k * _hop(count)
            np.testing.assert_array_equal(sig[o:o + count], want, err_msg=f'{sr} [{a}, +{count}) channel {c}')
            written[o:o + count] = True
    assert not sig[~written].any()
    # the three other entry points afterwards
    fullA = R.resample_ref(A, 44100)
    ctx.resample(A.reshape(-1).view(np.uint8), [ctx.resample_job(A, 44100, 0, 0)], n_signal=4800)
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 4800), fullA)
    part, win = _staged(A, 44100, 1234, 2500)
    ctx.resample(part.reshape(-1).view(np.uint8), [(0, part.shape[0], 2, 1, fa, 0, 0, 2500)], n_signal=2500, windows=[win])
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 2500), fullA[1234:3734])
    ctx.resample(A.reshape(-1).view(np.uint8), [ctx.resample_job(A, 44100, 0, 0)], n_signal=2 * 4800, splits=[(4800, [1, 0])])
    got = ctx.get_signal_pcm16(0, 2 * 4800)
    np.testing.assert_array_equal(got[:4800], R.resample_ref(A[:, 1], 44100))
    np.testing.assert_array_equal(got[4800:], R.resample_ref(A[:, 0], 44100))


# ------------------------------------------------------------------------------------------------ planner refusals
def test_planner_refusals(seg, tmp_path):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(13230, 2, 49), 'i16')
    fid, _, _ = ctx.resample_filter(44100)
    a, count = 1234, 2500
    part, win = _staged(x, 44100, a, count)
    src = part.reshape(-1).view(np.uint8)
    job = (0, part.shape[0], 2, 1, fid, 0, 0, count)
    stride = _hop(count)
    before = ctx.resample_stats(), ctx.adpcm_stats()
    with pytest.raises(_native.NativeError, match=r'job 0: dst_stride %d below the %d outputs' % (count - 1, count)):
        ctx.resample(src, [job], n_signal=2 * stride, windows=[win], splits=[(count - 1, [0, 1])])
    with pytest.raises(_native.NativeError, match=r'job 0: output .* of selected channel 1 outside'):
        ctx.resample(src, [job], n_signal=stride + count - 1, windows=[win], splits=[(stride, [0, 1])])
    with pytest.raises(_native.NativeError, match=r'job 0: selected channel 2 of 2'):
        ctx.resample(src, [job], n_signal=2 * stride, windows=[win], splits=[(stride, [0, 2])])
    j_lo, j_hi1 = win[0], win[1]
    for lo, hi in ((j_lo + 1, j_hi1), (j_lo, j_hi1 - 1)):                        # one frame short at either end
        short = np.ascontiguousarray(x[lo:hi])
        with pytest.raises(_native.NativeError, match='reach'):
            ctx.resample(short.reshape(-1).view(np.uint8), [(0, short.shape[0], 2, 1, fid, 0, 0, count)], n_signal=2 * stride,
                         windows=[(lo, hi, 13230, a, count)], splits=[(stride, [0, 1])])
    two = np.concatenate([src, np.zeros(-src.size % 16, np.uint8), src])
    job2 = (src.size + -src.size % 16, part.shape[0], 2, 1, fid, 0, stride + 100, count)      # on top of job 0's second channel
    with pytest.raises(_native.NativeError, match='overlap'):
        ctx.resample(two, [job, job2], n_signal=4 * stride, windows=[win, win], splits=[(stride, [0, 1]), (stride, [1])])
    path = sndgen.write(tmp_path / 'm.wav', 'wav', 'ima', False, wavgen.make_signal(3000, 1, 50), 16000, block_align=256)[0]
    s = sndfmt.AdpcmExcerpt(sndfmt.parse(open(path, 'rb').read(), path), 'pcm', 600, 1800)
    row, w, _ = s.job(ctx, 0, 0, 0)
    assert row[6] == _native.ADPCM_TO_SIGNAL
    with pytest.raises(_native.NativeError, match=r'job 0: a channel selection needs a TO_STAGE job with a filter'):
        ctx.adpcm_decode(s.payload, [row], s.units, n_signal=s.size, windows=[w], splits=[(_hop(s.size), [0])])
    assert (ctx.resample_stats(), ctx.adpcm_stats()) == before                  # nothing launched


# ------------------------------------------------------------------------------------------------ files
def _stats(ctx):
    return ctx.flac_stats()[0], ctx.adpcm_stats()[0], ctx.resample_stats()[0]


def _check_file(seg, path, ab, sel, want_launches):
    """load_pcm_channel_excerpts of the sample ranges `ab` against slices of load_pcm_channels, all in one launch per kernel."""
    whole = seg.load_pcm_channels(path)
    before = _stats(seg.ctx)
    got = seg.load_pcm_channel_excerpts(path, [(sec(a), sec(b)) for a, b in ab], sel)
    after = _stats(seg.ctx)
    assert tuple(y - x for x, y in zip(before, after)) == want_launches
    want_sel = list(range(len(whole))) if sel is None else sel
    assert len(got) == len(ab)
    for g, (a, b) in zip(got, ab):
        assert len(g) == len(want_sel)
        for k, c in enumerate(want_sel):
            assert g[k].dtype == np.int16
            np.testing.assert_array_equal(g[k], whole[c][a:b], err_msg=f'[{a}, {b}) channel {c}')
    return whole


@pytest.mark.parametrize('sr,mode', [(16000, 'left_side'), (44100, 'mid_side')])
def test_flac_channel_excerpts(seg, tmp_path, sr, mode):
    n = 1152 * 10 + 500
    path = flacgen.write(tmp_path / 'a.flac', flac_int(n, 2, 16, 51), sr, 16, blocksize=1152, channel_mode=mode,
                         subframe={'type': 'fixed', 'order': 2})
    n16 = R.out_len(n, sr)
    ab = [(3, 1003), (1234, 3734), (n16 - 777, n16), (1000, 3000)]              # off the frame grid, overlapping, the last output
    whole = _check_file(seg, path, ab, [1, 0], (1, 0, 1))
    x, _ = iss_io.decode_source(path)
    np.testing.assert_array_equal(whole[1], R.resample_ref(x[:, 1], sr))


def test_ima_channel_excerpts(seg, tmp_path):
    spb = sndgen.ima_samples_per_block(512, 2)
    n = spb * 12 + 123
    path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, wavgen.make_signal(n, 2, 52), 8000, block_align=512)[0]
    n16 = 2 * n
    ab = [(2 * (spb * 3 + 20), 2 * (spb * 3 + 20) + 420), (2 * spb * 5 - 250, 2 * spb * 5 + 250), (n16 - 410, n16), (0, n16)]
    _check_file(seg, path, ab, None, (0, 1, 1))


def test_flac_bad_frame_inside_and_outside(seg, tmp_path):
    x = flac_int(1152 * 8, 2, 16, 53)
    data, offs = flacgen.encode(x, 16000, 16, blocksize=1152, channel_mode='left_side', subframe={'type': 'fixed', 'order': 2},
                                return_offsets=True)
    bad = bytearray(data)
    bad[offs[6] - 4] ^= 0x10                                                      # inside frame 5, in front of its CRC-16
    path = tmp_path / 'bad.flac'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.flac: frame at byte %d: ' % offs[5]):
        seg.load_pcm_channel_excerpts(str(path), [(sec(1152 * 4 + 100), sec(1152 * 5 + 600))])
    with pytest.raises(ValueError, match=r'bad\.flac: frame at byte %d: ' % offs[5]):
        seg.segment_channel_excerpts(str(path), [(0, sec(1152 * 3)), (sec(1152 * 4 + 100), sec(1152 * 5 + 600))])
    a, b = 1152 * 2 + 100, 1152 * 5                                               # frames 2 to 4; ends where frame 5 starts
    got = seg.load_pcm_channel_excerpts(str(path), [(sec(a), sec(b)), (sec(1152 * 6), None)])
    for c in range(2):
        np.testing.assert_array_equal(got[0][c], x[a:b, c])
        np.testing.assert_array_equal(got[1][c], x[1152 * 6:, c])


def test_ima_bad_block_inside_and_outside(seg, tmp_path):
    spb = sndgen.ima_samples_per_block(512, 2)
    clean = sndgen.write(tmp_path / 'clean.wav', 'wav', 'ima', False, wavgen.make_signal(spb * 12, 2, 54), 16000, block_align=512)[0]
    whole = seg.load_pcm_channels(clean)
    base = sndfmt.parse(open(clean, 'rb').read(), clean).base
    bad = bytearray(open(clean, 'rb').read())
    bad[base + 7 * 512 + 2] = 89                                                  # block 7: step index above 88
    path = tmp_path / 'bad.wav'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.wav: block at byte %d: step index above 88' % (base + 7 * 512)):
        seg.load_pcm_channel_excerpts(str(path), [(sec(spb * 6 + 10), sec(spb * 7 + 450))])
    a, b = spb * 4 + 10, spb * 7                                                  # blocks 4 to 6 (16 kHz: the identity reaches no further)
    got = seg.load_pcm_channel_excerpts(str(path), [(sec(a), sec(b)), (sec(spb * 8), None)], [1])
    np.testing.assert_array_equal(got[0][0], whole[1][a:b])
    np.testing.assert_array_equal(got[1][0], whole[1][spb * 8:])


def test_plain_wav_is_read_by_byte_ranges(seg, tmp_path, monkeypatch):
    x = wavgen.encode(wavgen.make_signal(44100, 2, 55), 'i16')
    path = wavgen.write_wav(tmp_path / 'a.wav', x, 44100, 'i16')
    whole = seg.load_pcm_channels(path)

    def refuse(p):
        raise AssertionError('the whole file was read')
    monkeypatch.setattr(iss_io, '_read_file', refuse)
    got = seg.load_pcm_channel_excerpts(path, [(sec(1234), sec(3734)), (sec(15000), None)])
    for c in range(2):
        np.testing.assert_array_equal(got[0][c], whole[c][1234:3734])
        np.testing.assert_array_equal(got[1][c], whole[c][15000:])


def test_one_channel_file_is_load_pcm_excerpts(seg, tmp_path):
    ranges = [(sec(500), sec(2500)), (sec(2000), None)]
    for fmt in ('i16', 'f32'):                                                   # the float path included
        path = wavgen.write_wav(tmp_path / f'm_{fmt}.wav', wavgen.encode(wavgen.make_signal(3000, 1, 56), fmt), 16000, fmt)
        got = seg.load_pcm_channel_excerpts(path, ranges, [0, 0])
        want = seg.load_pcm_excerpts(path, ranges)
        for g, w in zip(got, want):
            assert len(g) == 2 and g[0].dtype == w.dtype
            np.testing.assert_array_equal(g[0], w)
            np.testing.assert_array_equal(g[1], w)


# ------------------------------------------------------------------------------------------------ segmentation
RANGES = [(0, 4.0), (1.5, 5.0), (2.0, None)]                     # (each holds sound and silence of both channels)


@pytest.fixture(scope='module')
def pair48(tmp_path_factory):
    """6 s at 48 kHz, two channels that the energy detector alone tells apart: each silent where the other sounds."""
    import scipy.signal
    n = 16000 * 6
    a, b = synth_pcm(1, n), synth_pcm(2, n)
    a[:n // 2] = 0
    b[n // 2:] = 0
    up = np.stack([scipy.signal.resample_poly(c / 32768.0, 3, 1) for c in (a, b)], axis=1)
    return wavgen.write_wav(tmp_path_factory.mktemp('pair48') / 'p48.wav', wavgen.encode(up * 0.9, 'i16'), 48000, 'i16')


def _want(seg, path, ranges, sel):
    pcm = [seg.load_pcm_channels(path, [c])[0] for c in range(2)]
    out = []
    for start, stop in ranges:
        a, b = iss_io.excerpt_bounds(path, pcm[0].size, start, stop)
        out.append([seg.segment_signal(pcm[c][a:b], start_sec=start) for c in sel])
    return out


def test_segment_channel_excerpts_equal_segment_signal(seg, pair48):
    want = _want(seg, pair48, RANGES, [0, 1])
    worker = pipeline._workers(seg, 1)[0]
    before = seg.ctx.resample_stats(), worker.stats['batches']
    got = seg.segment_channel_excerpts(pair48, RANGES)
    after = seg.ctx.resample_stats(), worker.stats['batches']
    # six (range, channel) pairs: one resample launch of three jobs, one feature pass
    assert (after[0][0] - before[0][0], after[0][1] - before[0][1], after[1] - before[1]) == (1, 3, 1)
    assert got == want
    for r, (start, _) in enumerate(RANGES):
        assert got[r][0][0][1] == start and got[r][0] != got[r][1]              # (a downmix would give one list twice)
    assert seg.segment_channel_excerpts(pair48, RANGES, [1, 0, 1]) == [[w[1], w[0], w[1]] for w in want]
    before = worker.stats['batches']
    assert seg.segment_channel_excerpts(pair48, RANGES, batch_files=2) == want  # two pairs per pass
    assert worker.stats['batches'] - before == 3


def test_short_range_takes_the_short_media_path(seg, pair48):
    ranges = [(2.75, 3.25), (1.5, 5.0)]
    with pytest.warns(UserWarning, match='duration is short'):
        got = seg.segment_channel_excerpts(pair48, ranges)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert got == _want(seg, pair48, ranges, [0, 1])
