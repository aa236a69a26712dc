"""GPU: the Microsoft ADPCM instantiations of adpcm_decode_kernel against the host build of the same block decoder, every
sample, through all four entry points; a pass holding IMA and Microsoft files at once; and Segmenter, the command line and
VoiceFemininityScoring on a Microsoft ADPCM file against its PCM16 WAV twin.  Every comparison is exact: the decode is integer
arithmetic and the resampler is bit-identical to resample.resample_ref."""
import filecmp
import os
import sys

import numpy as np
import pytest

import bench
import msadpcmgen as M
import sndgen
import wavgen
from conftest import synth_pcm
from inaspeechsegmenter_amd import _native, Segmenter, seg2csv, sndfmt, vfs
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R

pytestmark = pytest.mark.gpu

MATRIX = [(1, 256), (2, 512), (3, 210), (5, 80), (64, 512)]      # 500, 500, 128, 20 and 4 samples per block


def sec(k):
    return k / 16000.0


@pytest.fixture(scope='module')
def mctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def segs():
    a = Segmenter(ffmpeg=None, models='synthetic')
    b = Segmenter(ffmpeg=None, models='synthetic', resample=True)
    yield a, b
    a.close(); b.close()


def _pcm(x):
    return np.clip(np.round(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype(np.int16)


def _sound(x, sr, align, name='<test>', frames=None):
    """float samples -> (sndfmt.Sound over the Microsoft ADPCM blocks, its samples by the host build of the decoder)."""
    pcm = _pcm(x)
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    d = np.frombuffer(M.encode(pcm, align), dtype=np.uint8)
    s = sndfmt.Sound(name, sr, ch, 'ms', False, d, 0, frames=len(pcm) if frames is None else frames, block_align=align,
                     spb=M.samples_per_block(align, ch))
    return s, s.stored()


def _staged(ctx, s):
    st = ctx.msadpcm_decode(s.data, [(0, 0, s.nblocks, s.n, s.ch, s.block_align, _native.ADPCM_TO_STAGE, -1, 0, 0)], s.nblocks, n_signal=0)
    got = ctx.msadpcm_get_stage(0, s.n, s.ch)
    assert not st.any(), st
    return got


def _speech(seed, n, ch=1):
    base = synth_pcm(seed, n).astype(np.float64) / 32768.0
    if ch == 1:
        return base
    return np.stack([np.roll(base, 31 * c) * (1.0 - 0.1 * c) for c in range(ch)], axis=1)


def _pair(d, stem, x, sr, align, container='wav'):
    """(Microsoft ADPCM file, its PCM16 WAV twin in twins/) with the same stem."""
    os.makedirs(d / 'twins', exist_ok=True)
    p, twin = M.write(d / f'{stem}.{container}', x, sr, align, container)
    return p, wavgen.write_wav(d / 'twins' / f'{stem}.wav', twin, sr, 'i16')


# ------------------------------------------------------------------------------------------------ kernel against the host build
@pytest.mark.parametrize('ch,align', MATRIX)
def test_kernel_equals_host(mctx, ch, align):
    spb = M.samples_per_block(align, ch)
    n = spb * 7 + spb // 2 + 1 if ch < 64 else spb * 40 + 1
    x = wavgen.make_signal(n, ch, 60 + ch)
    s, host = _sound(x, 16000, align)
    assert s.n == n and host.shape == ((n,) if ch == 1 else (n, ch))
    if ch <= 3:                                                   # (the host build itself against the Python decoder: test_msadpcm.py)
        np.testing.assert_array_equal(host, M.decode(s.data.tobytes(), ch, align, n))
    np.testing.assert_array_equal(_staged(mctx, s), host)         # TO_STAGE, read back
    if ch == 1:                                                   # TO_SIGNAL: mono at 16 kHz
        src = sndfmt.source(s)
        assert type(src) is sndfmt.MsAdpcmSource and src.kind == 'pcm'
        before = mctx.msadpcm_stats(), mctx.adpcm_stats(), mctx.resample_stats()
        st = sndfmt.decode_on(mctx, src)
        got = mctx.get_signal_pcm16(0, n)
        assert not st.any()
        assert mctx.msadpcm_stats() == (before[0][0] + 1, before[0][1] + s.nblocks) and mctx.adpcm_stats() == before[1]
        assert mctx.resample_stats() == before[2]
        np.testing.assert_array_equal(got, host)
    # TO_STAGE with a filter, in the same call
    s8, host8 = _sound(x, 8000, align)
    src = sndfmt.source(s8, resample=True)
    assert type(src) is sndfmt.MsAdpcmSource and src.kind == 'resample'
    st = sndfmt.decode_on(mctx, src)
    got = mctx.get_signal_pcm16(0, src.size)
    assert not st.any()
    np.testing.assert_array_equal(got, R.resample_ref(host8, 8000))


def test_kernel_stereo_11025(mctx):
    s, host = _sound(wavgen.make_signal(4321, 2, 71), 11025, 512)
    src = sndfmt.source(s, resample=True)
    st = sndfmt.decode_on(mctx, src)
    got = mctx.get_signal_pcm16(0, src.size)
    assert not st.any()
    np.testing.assert_array_equal(got, R.resample_ref(host, 11025))


def test_largest_block(mctx):
    """Mono, 32768-byte blocks: 65 524 samples a block, 131 048 bytes of dynamic LDS (above the 64 KiB a kernel gets by default)."""
    spb = M.samples_per_block(32768, 1)
    assert spb == 65524
    s, host = _sound(wavgen.make_signal(spb * 2 - 100, 1, 72), 16000, 32768)
    assert s.nblocks == 2
    np.testing.assert_array_equal(_staged(mctx, s), host)
    st = sndfmt.decode_on(mctx, sndfmt.source(s))
    got = mctx.get_signal_pcm16(0, s.n)
    assert not st.any()
    np.testing.assert_array_equal(got, host)


def test_ragged_batch_one_launch(mctx):
    specs = [(16000, 1, 256, 500 * 3 + 1), (8000, 2, 512, 500 * 2 + 2), (16000, 3, 210, 128 * 9 + 3), (11025, 5, 80, 20 * 33),
             (8000, 64, 512, 4 * 25 + 1), (16000, 1, 70, 128 * 4 + 127)]
    sounds, kinds, wants = [], [], []
    for k, (sr, ch, align, n) in enumerate(specs):
        s, host = _sound(wavgen.make_signal(n, ch, 80 + k), sr, align, name=f'r{k}.wav')
        kind = 'stage' if k == 2 else 'pcm' if (sr, ch) == (16000, 1) else 'resample'
        sounds.append(s); kinds.append(kind)
        wants.append(R.resample_ref(host, sr) if kind == 'resample' else host)
    src, jobs, offs = [], [], []
    pos = bbeg = dpos = 0
    for s, kind in zip(sounds, kinds):
        offs.append(dpos)
        if kind == 'stage':
            jobs.append((pos, bbeg, s.nblocks, s.n, s.ch, s.block_align, _native.ADPCM_TO_STAGE, -1, 0, 0))
        else:
            a = sndfmt.MsAdpcmSource(s, kind)
            jobs.append(a.job(mctx, pos, bbeg, dpos).row)
            dpos += a.size
        pad = -s.data.size % 16
        src += [s.data, np.zeros(pad, np.uint8)]
        pos += s.data.size + pad
        bbeg += s.nblocks
        dpos += 160
    sig = np.full(dpos, 12345, dtype=np.int16)
    mctx.set_signal(sig)
    before = mctx.msadpcm_stats(), mctx.resample_stats()[0], mctx.adpcm_stats()
    st = mctx.msadpcm_decode(np.concatenate(src), jobs, bbeg)
    got = mctx.get_signal_pcm16(0, sig.size)
    assert mctx.msadpcm_stats() == (before[0][0] + 1, before[0][1] + bbeg)
    assert mctx.resample_stats()[0] == before[1] + 1 and mctx.adpcm_stats() == before[2]
    assert not st.any()
    covered = np.zeros(sig.size, bool)
    for j, (s, kind, w, o) in enumerate(zip(sounds, kinds, wants, offs)):
        if kind == 'stage':
            np.testing.assert_array_equal(mctx.msadpcm_get_stage(j, s.n, s.ch), w)
        else:
            np.testing.assert_array_equal(got[o:o + w.size], w, err_msg=f'job {j}')
            covered[o:o + w.size] = True
    assert np.all(got[~covered] == 12345)


# ------------------------------------------------------------------------------------------------ windows and splits
def test_windowed_split_and_windowed_split_entry_points(segs, tmp_path):
    plain, rs = segs
    ctx = rs.ctx
    # windows, mono at 16 kHz (TO_SIGNAL): excerpts starting on sample 0, 1 and 2 of a block, one ending on a block's first sample
    spb = 500
    n = spb * 8 + 250
    p, twin = M.write(tmp_path / 'm.wav', wavgen.make_signal(n, 1, 90), 16000, 256)
    np.testing.assert_array_equal(rs.load_pcm(p), twin)
    ab = [(spb * 2, spb * 2 + 700), (spb * 2 + 1, spb * 3 + 450), (spb * 2 + 2, spb * 4), (spb - 450, spb * 3 + 1), (0, n)]
    before = ctx.msadpcm_stats(), ctx.adpcm_stats()
    got = rs.load_pcm_excerpts(p, [(sec(a), sec(b)) for a, b in ab])
    assert ctx.msadpcm_stats() == (before[0][0] + 1, before[0][1] + 2 + 2 + 2 + 4 + 9) and ctx.adpcm_stats() == before[1]
    for g, (a, b) in zip(got, ab):
        np.testing.assert_array_equal(g, twin[a:b])
    # stereo at 8 kHz: split (a repeated channel index), windows (downmix), windows and split
    n = spb * 9 + 77
    p, twin = M.write(tmp_path / 's.wav', wavgen.make_signal(n, 2, 91), 8000, 512)
    whole = R.resample_ref(twin, 8000)
    cols = [R.resample_ref(twin[:, c], 8000) for c in (0, 1)]
    np.testing.assert_array_equal(rs.load_pcm(p), whole)
    sel = [1, 0, 1]
    before = ctx.msadpcm_stats()[0]
    for g, c in zip(rs.load_pcm_channels(p, sel), sel):
        np.testing.assert_array_equal(g, cols[c])
    ab = [(2 * a, 2 * b) for a, b in ab[:4]] + [(0, 2 * n)]
    ranges = [(sec(a), sec(b)) for a, b in ab]
    for g, (a, b) in zip(rs.load_pcm_excerpts(p, ranges), ab):
        np.testing.assert_array_equal(g, whole[a:b])
    for g, (a, b) in zip(rs.load_pcm_channel_excerpts(p, ranges, sel), ab):
        assert len(g) == 3
        for gk, c in zip(g, sel):
            np.testing.assert_array_equal(gk, cols[c][a:b])
    assert ctx.msadpcm_stats()[0] == before + 3                   # one launch per call


# ------------------------------------------------------------------------------------------------ both coders in one pass
def test_mixed_pass_keeps_the_coders_apart(segs, tmp_path):
    """One batch_process pass over 2 IMA and 2 Microsoft files, one of each malformed: each bad file is a code-2 entry naming
    its own block, each good file gives its twin's CSV.  With one status array or one staging buffer for both coders the second
    launch of the pass would overwrite what the first left before the pass reads it."""
    plain, rs = segs
    d = tmp_path
    os.makedirs(d / 'twins')
    x = _speech(11, 8000 * 9)
    ima, tfmt, twin = sndgen.write(d / 'ima_good.wav', 'wav', 'ima', False, x, 8000, block_align=256)
    ima_twin = sndgen.wav_twin(d / 'twins' / 'ima_good.wav', twin, 8000, tfmt)
    ms, ms_twin = _pair(d, 'ms_good', _speech(12, 8000 * 8, 2), 8000, 512)
    blocks = bytearray(sndgen.ima_encode(wavgen.encode(_speech(13, 8000 * 7), 'i16'), 256))
    blocks[5 * 256 + 2] = 89                                      # IMA block 5: step index 89
    ima_bad = sndgen.write_riff(d / 'ima_bad.wav', sndgen.wav_fmt('ima', 8000, 1, 256), bytes(blocks), fact=8000 * 7)
    blocks = bytearray(M.encode(_pcm(_speech(14, 8000 * 6)), 256))
    blocks[9 * 256] = 7                                           # Microsoft block 9: predictor 7
    ms_bad = M.write_riff(d / 'ms_bad.wav', M.fmt(8000, 1, 256), bytes(blocks), fact=8000 * 6)
    files = [ima, ms_bad, ms, ima_bad]
    outs = [str(d / 'out' / (os.path.basename(f) + '.csv')) for f in files]
    before = rs.ctx.adpcm_stats()[0], rs.ctx.msadpcm_stats()[0]
    _, nb, _, lmsg = rs.batch_process(files, outs, batch_files=8, batch_seconds=600)
    assert (rs.ctx.adpcm_stats()[0], rs.ctx.msadpcm_stats()[0]) == (before[0] + 1, before[1] + 1)       # one pass, one launch each
    assert [m[1] for m in lmsg] == [0, 2, 0, 2] and nb == 2, lmsg
    assert f'ima_bad.wav: block at byte {M.data_offset(ima_bad) + 5 * 256}: step index above 88' in lmsg[3][2], lmsg[3]
    assert f'ms_bad.wav: block at byte {M.data_offset(ms_bad) + 9 * 256}: predictor index above 6' in lmsg[1][2], lmsg[1]
    for f, o, t in ((ima, outs[0], ima_twin), (ms, outs[2], ms_twin)):
        seg2csv(rs(t), str(d / 'twin.csv'))
        assert filecmp.cmp(o, str(d / 'twin.csv'), shallow=False), f


# ------------------------------------------------------------------------------------------------ Segmenter, command line, voice femininity
def test_segmenter_reads_like_wav_twin(segs, tmp_path):
    plain, rs = segs
    p, w = _pair(tmp_path, 'm16', _speech(21, 16000 * 9), 16000, 256)
    for seg in (plain, rs):
        assert seg(p) == seg(w)
        np.testing.assert_array_equal(seg.load_pcm(p), seg.load_pcm(w))
    for k, container in enumerate(('rf64', 'w64')):
        q, _ = M.write(tmp_path / f'm16.{container}', _speech(21, 16000 * 9), 16000, 256, container)
        assert plain(q) == plain(w)
    p8, w8 = _pair(tmp_path, 's8', _speech(22, 8000 * 9, 2), 8000, 512)
    assert rs(p8) == rs(w8)
    np.testing.assert_array_equal(rs.load_pcm(p8), rs.load_pcm(w8))
    ranges = [(0, 4.0), (2.5, 8.0), (5.0, None)]
    assert rs.segment_channels(p8) == rs.segment_channels(w8)
    assert rs.segment_channels(p8, [1]) == rs.segment_channels(w8, [1])
    assert rs.segment_excerpts(p8, ranges) == rs.segment_excerpts(w8, ranges)
    assert plain.segment_excerpts(p, ranges) == plain.segment_excerpts(w, ranges)
    assert rs.segment_channel_excerpts(p8, ranges, [1, 0]) == rs.segment_channel_excerpts(w8, ranges, [1, 0])
    for fn in (plain, plain.load_pcm):                            # without resample: the twin's refusal, the file's name in it
        with pytest.raises((AssertionError, ValueError)) as e1:
            fn(p8)
        with pytest.raises((AssertionError, ValueError)) as e2:
            fn(w8)
        assert type(e1.value) is type(e2.value) and str(e1.value).replace(p8, '') == str(e2.value).replace(w8, '')
    outs = [str(tmp_path / 'split' / 'a.csv'), str(tmp_path / 'split' / 'b.csv')]
    _, nb, _, lmsg = rs.batch_process([p8, w8], outs, channels='split')
    assert len(lmsg) == 4 and all(m[1] == 0 for m in lmsg), lmsg
    for k in range(2):
        assert filecmp.cmp(iss_io.channel_name(outs[0], k), iss_io.channel_name(outs[1], k), shallow=False)


def test_cli_reads_like_wav_twin(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    import ina_speech_segmenter_amd as cli
    d = tmp_path / 'in'
    os.makedirs(d)
    pairs = [_pair(d, 'c0', _speech(31, 8000 * 8), 8000, 256), _pair(d, 'c1', _speech(32, 16000 * 8), 16000, 256)]
    for name, inputs in (('files', [p for p, _ in pairs]), ('twins', [w for _, w in pairs])):
        os.makedirs(tmp_path / name)
        assert cli.main(['-i'] + inputs + ['-o', str(tmp_path / name), '-b', 'None', '--resample', '--models', 'synthetic']) == 0
    for k in range(len(pairs)):
        assert filecmp.cmp(str(tmp_path / 'files' / f'c{k}.csv'), str(tmp_path / 'twins' / f'c{k}.csv'), shallow=False), k


def test_voice_femininity_like_wav_twin(tmp_path):
    v = vfs.VoiceFemininityScoring(ffmpeg=None, models='synthetic', resample=True)
    try:
        x = bench.synth_recording_numpy(3, 8000 * 15).astype(np.float64) / 32768.0
        p, w = _pair(tmp_path, 'v', np.stack([x, np.roll(x, 17) * 0.8], axis=1), 8000, 512)
        want = v(w)
        assert v(p) == want and want[2] > 0, want
        assert v.score_channels(p) == v.score_channels(w)
        assert v.batch_process([p]) == [want]
    finally:
        v.vad.close()


# ------------------------------------------------------------------------------------------------ the IMA instantiations
def test_ima_entry_points_give_what_they_gave(mctx):
    for k, (sr, ch, align) in enumerate(((16000, 1, 256), (8000, 2, 512), (16000, 3, 516))):
        n = 3000 + 7 * k
        data, _, twin, frames = sndgen.encode(wavgen.make_signal(n, ch, 95 + k), 'ima', False, align)
        d = np.frombuffer(data, np.uint8)
        spb = sndgen.ima_samples_per_block(align, ch)
        host, st = _native.adpcm_decode_host(d, len(d) // align, ch, align, n)
        assert not st.any()
        np.testing.assert_array_equal(host, twin)
        s = sndfmt.Sound(f'i{k}.wav', sr, ch, 'ima', False, d, 0, frames=frames, block_align=align, spb=spb)
        before = mctx.msadpcm_stats()
        st = mctx.adpcm_decode(s.data, [(0, 0, s.nblocks, s.n, s.ch, align, _native.ADPCM_TO_STAGE, -1, 0, 0)], s.nblocks, n_signal=0)
        got = mctx.adpcm_get_stage(0, s.n, s.ch)
        assert not st.any() and mctx.msadpcm_stats() == before
        np.testing.assert_array_equal(got, host)
        src = sndfmt.source(s, resample=True)
        assert type(src) is sndfmt.AdpcmSource
        st = sndfmt.decode_on(mctx, src)
        got = mctx.get_signal_pcm16(0, src.size)
        assert not st.any()
        np.testing.assert_array_equal(got, host if src.kind == 'pcm' else R.resample_ref(host, sr))
