"""GPU: every channel of a file on its own, split on the device.  The SPLIT instantiations of resample_kernel through
ctx.resample(..., splits=...) against resample.resample_ref of each stored column; the planner's refusals; FLAC and IMA ADPCM
through Segmenter.load_pcm_channels; segment_channels against per-channel segment_signal; batch_process(channels='split') against
the mono twins; and the unsplit calls afterwards.  Every comparison is exact.
The shapes are the smallest at which the split can go wrong: more than one tile per channel (a tile boundary and the last output
inside every case), more channels than one group holds, selections that are not the identity, the 16 kHz identity filter, a
filter table too large for LDS."""
import os
import warnings

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from conftest import synth_pcm
from test_channels import flac_int
from inaspeechsegmenter_amd import _native, Segmenter, sndfmt
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


def _split_direct(ctx, raw, sr, fmt, sel, stored=None):
    """One split job on its own: -> the whole signal (len(sel) strides), checked against resample_ref of every selected column
    of `stored` (what the host reads for `raw`), with the samples between a channel's end and the next stride still zero."""
    stored = raw if stored is None else stored
    job = ctx.resample_job(raw, sr, 0, 0, fmt)
    nout, stride = job[-1], _hop(job[-1])
    before = ctx.resample_stats()
    ctx.resample(raw.reshape(-1).view(np.uint8), [job], n_signal=len(sel) * stride, splits=[(stride, sel)])
    sig = ctx.get_signal_pcm16(0, len(sel) * stride)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)            # a split job counts as one job
    tile, _ = ctx.resample_split_geometry(sr, len(sel))
    assert nout > tile                                                          # more than one tile per channel
    for k, c in enumerate(sel):
        np.testing.assert_array_equal(sig[k * stride:k * stride + nout], R.resample_ref(stored[:, c], sr), err_msg=f'selected {k} = channel {c}')
        assert not sig[k * stride + nout:(k + 1) * stride].any()
    return sig


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('sr,fmt,ch,n', [(44100, 'i16', 2, 6000), (48000, 'f32', 3, 5000), (16000, 'i16', 2, 2000)])
def test_split_plain_instantiation(seg, sr, fmt, ch, n):
    x = wavgen.encode(wavgen.make_signal(n, ch, 21), fmt)
    sig = _split_direct(seg.ctx, x, sr, _native.RS_FORMAT[x.dtype], list(range(ch)))
    if sr == 16000:                                                             # the identity filter: the stored columns themselves
        np.testing.assert_array_equal(sig[:n], x[:, 0])
        np.testing.assert_array_equal(sig[_hop(n):_hop(n) + n], x[:, 1])
    _split_direct(seg.ctx, x, sr, _native.RS_FORMAT[x.dtype], [ch - 1, 0])       # not the identity


def test_split_ext_instantiation(seg, tmp_path):
    path = sndgen.write(tmp_path / 'u.wav', 'wav', 'ulaw', False, wavgen.make_signal(3000, 2, 22), 8000)[0]
    snd = sndfmt.parse(open(path, 'rb').read(), path)
    raw, fmt = snd.raw()
    assert fmt == _native.RS_ULAW
    _split_direct(seg.ctx, raw, 8000, fmt, [0, 1], snd.stored())
    _split_direct(seg.ctx, raw, 8000, fmt, [1, 1, 0], snd.stored())


def test_split_table_read_through_cache(seg):
    """44 056 Hz: 110 141 taps, more than LDS holds next to the spans."""
    assert R.plan(44056)[2].size == 110141
    x = wavgen.encode(wavgen.make_signal(30000, 2, 23), 'i16')
    _split_direct(seg.ctx, x, 44056, _native.RS_FORMAT[x.dtype], [0, 1])


def test_split_more_channels_than_a_group(seg):
    """22 050 Hz, 11 channels: a tile's span is 11.5 KB of float64, so 64 KiB hold 5 channels side by side."""
    ctx = seg.ctx
    tile, group = ctx.resample_split_geometry(22050, 11)
    assert group < 11 and -(-11 // group) > 1                                   # 11 channels need more than one group
    assert ctx.resample_split_geometry(22050, 2) == (tile, 2)                    # a stereo file stays in one group
    x = wavgen.encode(wavgen.make_signal(3000, 11, 24), 'i16')
    fmt = _native.RS_FORMAT[x.dtype]
    _split_direct(ctx, x, 22050, fmt, [10, 0, 7, 7, 3])
    _split_direct(ctx, x, 22050, fmt, list(range(11)))                          # the identity over three groups
    _split_direct(ctx, x, 22050, fmt, list(range(10, -1, -1)))                  # a selection over three groups


def test_split_and_downmix_in_one_call(seg):
    ctx = seg.ctx
    a = wavgen.encode(wavgen.make_signal(6000, 2, 25), 'i16')
    b = wavgen.encode(wavgen.make_signal(5000, 3, 26), 'f32')
    ja = ctx.resample_job(a, 44100, 0, 0)
    sa = _hop(ja[-1])
    jb = ctx.resample_job(b, 48000, a.nbytes, 2 * sa)
    staged = np.concatenate([a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)])
    nsig = 2 * sa + _hop(jb[-1])
    before = ctx.resample_stats()
    ctx.resample(staged, [ja, jb], n_signal=nsig, splits=[(sa, [0, 1]), None])
    sig = ctx.get_signal_pcm16(0, nsig)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 2)
    for k in range(2):
        np.testing.assert_array_equal(sig[k * sa:k * sa + ja[-1]], R.resample_ref(a[:, k], 44100))
    np.testing.assert_array_equal(sig[2 * sa:2 * sa + jb[-1]], R.resample_ref(b, 48000))
    assert not sig[2 * sa + jb[-1]:].any() and not sig[ja[-1]:sa].any()
    ctx.resample(b.reshape(-1).view(np.uint8), [ctx.resample_job(b, 48000, 0, 0)], n_signal=jb[-1])      # the plain entry point
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, jb[-1]), sig[2 * sa:2 * sa + jb[-1]])


# ------------------------------------------------------------------------------------------------ planner refusals
def test_planner_refusals(seg, tmp_path):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(3000, 2, 27), 'i16')
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, 44100, 0, 0)
    nout, stride = job[-1], _hop(job[-1])
    before = ctx.resample_stats(), ctx.adpcm_stats()
    with pytest.raises(_native.NativeError, match=r'job 0: dst_stride %d below' % (nout - 1)):
        ctx.resample(src, [job], n_signal=2 * stride, splits=[(nout - 1, [0, 1])])
    with pytest.raises(_native.NativeError, match=r'job 0: selected channel 2 of 2'):
        ctx.resample(src, [job], n_signal=2 * stride, splits=[(stride, [0, 2])])
    rows = np.array([(stride, 1, 2)], dtype=_native.SPLIT)
    with pytest.raises(_native.NativeError, match=r'job 0: selection rows \[1, \+2\) outside the 2'):
        ctx.resample(src, [job], n_signal=2 * stride, splits=(rows, np.array([0, 1], dtype=np.int32)))
    with pytest.raises(_native.NativeError, match=r'job 0: output .* of selected channel 1 outside'):
        ctx.resample(src, [job], n_signal=2 * stride - 200, splits=[(stride, [0, 1])])
    two = np.concatenate([src, src])
    job2 = ctx.resample_job(x, 44100, src.size, stride)                          # on top of job 0's second channel
    with pytest.raises(_native.NativeError, match='overlap'):
        ctx.resample(two, [job, job2], n_signal=4 * stride, splits=[(stride, [0, 1]), (stride, [1])])
    path = sndgen.write(tmp_path / 'm.wav', 'wav', 'ima', False, wavgen.make_signal(3000, 1, 28), 16000, block_align=256)[0]
    s = sndfmt.AdpcmSource(sndfmt.parse(open(path, 'rb').read(), path), 'pcm')
    with pytest.raises(_native.NativeError, match=r'job 0: a channel selection needs a TO_STAGE job with a filter'):
        ctx.adpcm_decode(s.payload, [s.job(ctx, 0, 0, 0).row], s.units, n_signal=s.size, splits=[(_hop(s.size), [0])])
    assert (ctx.resample_stats(), ctx.adpcm_stats()) == before                  # nothing launched


# ------------------------------------------------------------------------------------------------ FLAC and IMA ADPCM
def _stats(ctx):
    return ctx.flac_stats()[0], ctx.adpcm_stats()[0], ctx.resample_stats()[0]


@pytest.mark.parametrize('sr,bps,mode', [(16000, 16, 'left_side'), (44100, 24, 'mid_side')])
def test_flac_channels(seg, tmp_path, sr, bps, mode):
    path = flacgen.write(tmp_path / 'a.flac', flac_int(12000, 2, bps, 29), sr, bps, blocksize=1152, channel_mode=mode,
                         subframe={'type': 'fixed', 'order': 2})
    x, _ = iss_io.decode_source(path)
    before = _stats(seg.ctx)
    got = seg.load_pcm_channels(path)
    after = _stats(seg.ctx)
    assert tuple(b - a for a, b in zip(before, after)) == (1, 0, 1)
    assert len(got) == 2
    for c in range(2):
        np.testing.assert_array_equal(got[c], R.resample_ref(x[:, c], sr))
    np.testing.assert_array_equal(seg.load_pcm_channels(path, [1])[0], got[1])


def test_ima_channels(seg, tmp_path):
    path = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, wavgen.make_signal(5000, 2, 30), 8000, block_align=256)[0]
    x, _ = iss_io.decode_source(path)
    before = _stats(seg.ctx)
    got = seg.load_pcm_channels(path, [1, 0])
    after = _stats(seg.ctx)
    assert tuple(b - a for a, b in zip(before, after)) == (0, 1, 1)
    for g, c in zip(got, (1, 0)):
        np.testing.assert_array_equal(g, R.resample_ref(x[:, c], 8000))


def test_mono_file_is_load_pcm(seg, tmp_path):
    for fmt in ('i16', 'f32'):
        path = wavgen.write_wav(tmp_path / f'm_{fmt}.wav', wavgen.encode(wavgen.make_signal(3000, 1, 31), fmt), 16000, fmt)
        got = seg.load_pcm_channels(path)
        want = seg.load_pcm(path)
        assert len(got) == 1 and got[0].dtype == want.dtype
        np.testing.assert_array_equal(got[0], want)


# ------------------------------------------------------------------------------------------------ segmentation
def _pair(n):
    """Two channels that the energy detector alone tells apart: each silent where the other sounds."""
    a, b = synth_pcm(1, n), synth_pcm(2, n)
    a[:n // 2] = 0
    b[n // 2:] = 0
    return np.stack([a, b], axis=1)


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    import scipy.signal
    d = tmp_path_factory.mktemp('pairs')
    x = _pair(48000)
    up = np.stack([scipy.signal.resample_poly(x[:, c] / 32768.0, 441, 160) for c in range(2)], axis=1)
    return {'16k': wavgen.write_wav(d / 'p16.wav', x.astype('<i2'), 16000, 'i16'),
            '44k': wavgen.write_wav(d / 'p44.wav', wavgen.encode(up, 'i16'), 44100, 'i16'),
            'short': wavgen.write_wav(d / 'short.wav', _pair(8000).astype('<i2'), 16000, 'i16')}


@pytest.mark.parametrize('what', ['16k', '44k'])
def test_segment_channels_equal_segment_signal(seg, pairs, what):
    path = pairs[what]
    pcm = seg.load_pcm_channels(path)
    before = seg.ctx.resample_stats()
    got = seg.segment_channels(path)
    after = seg.ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)              # both channels: one launch, one job
    assert len(got) == 2
    for k in range(2):
        assert got[k] == seg.segment_signal(pcm[k]), (what, k)
        assert got[k] == seg.segment_signal(seg.load_pcm_channels(path, [k])[0])
    assert got[0] != got[1]                                                     # (a downmix would give one list twice)
    assert got[0][0][0] == 'noEnergy' and got[1][-1][0] == 'noEnergy'
    assert seg.segment_channels(path, [1, 0, 1]) == [got[1], got[0], got[1]]
    assert seg.segment_channels(path, batch_files=1) == got                    # one channel per pass


def test_short_channels_take_the_short_media_path(seg, pairs):
    with pytest.warns(UserWarning, match='duration is short'):
        got = seg.segment_channels(pairs['short'])
    pcm = seg.load_pcm_channels(pairs['short'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert got == [seg.segment_signal(p) for p in pcm]


# ------------------------------------------------------------------------------------------------ batch_process
def test_batch_process_split(seg, tmp_path):
    n = 16000
    files = {
        'mono': wavgen.write_wav(tmp_path / 'mono.wav', synth_pcm(3, n).astype('<i2'), 16000, 'i16'),
        'wav48': wavgen.write_wav(tmp_path / 'wav48.wav', wavgen.encode(wavgen.make_signal(3 * n, 2, 32, peak=0.3), 'i16'), 48000, 'i16'),
        'flac': flacgen.write(tmp_path / 'flac.flac', _pair(n).astype(np.int64), 16000, 16, blocksize=1152, channel_mode='left_side',
                              subframe={'type': 'fixed', 'order': 2}),
        'ima': sndgen.write(tmp_path / 'ima.wav', 'wav', 'ima', False, _pair(n)[::2] / 32768.0, 8000, block_align=256)[0],
    }
    data, offs = flacgen.encode(_pair(n).astype(np.int64), 16000, 16, blocksize=1152, channel_mode='left_side',
                                subframe={'type': 'fixed', 'order': 2}, return_offsets=True)
    bad = bytearray(data)
    bad[offs[6] - 4] ^= 0x10                                                    # inside frame 5, in front of its CRC-16
    (tmp_path / 'bad.flac').write_bytes(bytes(bad))
    names = ['mono', 'wav48', 'flac', 'ima', 'bad']
    inputs = [files.get(k, str(tmp_path / 'bad.flac')) for k in names]
    outputs = [str(tmp_path / 'out' / f'{k}.csv') for k in names]
    ctx = seg.ctx
    before = _stats(ctx)
    _, nb, _, lmsg = seg.batch_process(inputs, outputs, channels='split', workers=1, batch_files=16)
    after = _stats(ctx)
    # one pass: one launch per decoder, and one resample launch per source class (stored samples, FLAC's and IMA's staging)
    assert tuple(b - a for a, b in zip(before, after)) == (1, 1, 3)
    want_dst = [iss_io.channel_name(outputs[0], 0)] + [iss_io.channel_name(o, k) for o in outputs[1:4] for k in (0, 1)] + [outputs[4]]
    assert [m[0] for m in lmsg] == want_dst and nb == 7
    assert [m[1] for m in lmsg] == [0] * 7 + [2]
    assert 'frame at byte %d' % offs[5] in lmsg[-1][2] and 'bad.flac' in lmsg[-1][2]
    assert not os.path.exists(outputs[4]) and not os.path.exists(iss_io.channel_name(outputs[4], 0))
    # every CSV against batch_process on the mono twin of that channel
    twins, touts, souts = [], [], []
    for k, o in zip(names[:4], outputs[:4]):
        for c, pcm in enumerate(seg.load_pcm_channels(files[k])):
            twins.append(wavgen.write_wav(tmp_path / f'twin_{k}_{c}.wav', pcm.astype('<i2'), 16000, 'i16'))
            touts.append(str(tmp_path / 'twin_out' / f'{k}_{c}.csv'))
            souts.append(iss_io.channel_name(o, c))
    assert len(twins) == 7
    assert seg.batch_process(twins, touts, workers=1)[1] == 7
    for s, t in zip(souts, touts):
        assert open(s, 'rb').read() == open(t, 'rb').read(), s
    assert open(souts[3], 'rb').read() != open(souts[4], 'rb').read()            # the two channels of the FLAC pair differ
    # skipifexist goes by .ch0
    os.remove(iss_io.channel_name(outputs[1], 1))
    os.remove(iss_io.channel_name(outputs[2], 0))
    _, nb, _, lmsg = seg.batch_process(inputs[:3], outputs[:3], channels='split', workers=1, skipifexist=True)
    assert [(m[0], m[1]) for m in lmsg] == [(iss_io.channel_name(outputs[0], 0), 1), (iss_io.channel_name(outputs[1], 0), 1),
                                            (iss_io.channel_name(outputs[2], 0), 0), (iss_io.channel_name(outputs[2], 1), 0)]
    # unsplit calls afterwards, on the same Segmenter
    for k in ('wav48', 'flac', 'ima'):
        np.testing.assert_array_equal(seg.load_pcm(files[k]), R.resample_ref(*iss_io.decode_source(files[k])))
