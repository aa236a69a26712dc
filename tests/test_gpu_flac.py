"""GPU: FLAC decoded by flac_decode_kernel (iss_flac_decode) must be bit-identical to the host build of the decoder and to the
encoded samples, for every output (signal, staging buffer + resampler, staging buffer read back), and every entry point must
give a FLAC what it gives the file's WAV twin."""
import filecmp
import os

import numpy as np
import pytest

import bench
import flacgen
from conftest import GOLDEN, synth_pcm
from inaspeechsegmenter_amd import _native, Segmenter, seg2csv, seg2textgrid, flac, pipeline, vfs
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fctx():
    c = _native.Context(0)
    yield c
    c.close()


def _signal(n, ch, bps, seed):
    base = synth_pcm(seed, n).astype(np.int64)
    x = np.stack([np.roll(base, 29 * c) - 40 * c for c in range(ch)], axis=1)
    x = (x << 8) + np.random.default_rng(seed).integers(-128, 128, x.shape) if bps == 24 else x >> (16 - bps)
    x = np.clip(x, -(1 << (bps - 1)), (1 << (bps - 1)) - 1)
    return x[:, 0] if ch == 1 else x


def _stored(x, bps):
    x = np.asarray(x, dtype=np.int64)
    return (x << 8).astype(np.int32) if bps == 24 else (x << (16 - bps)).astype(np.int16)


MATRIX = [
    (16000, 1, 16, {}), (16000, 1, 8, {}), (16000, 1, 24, {}),
    (16000, 1, 16, {'subframe': {'type': 'lpc', 'order': 32, 'precision': 15}}),
    (16000, 1, 24, {'subframe': {'type': 'lpc', 'order': 12, 'precision': 15}}),
    (16000, 1, 16, {'subframe': {'type': 'fixed', 'order': 4, 'porder': 6, 'rice2': True}}),
    (16000, 1, 16, {'subframe': {'type': 'fixed', 'order': 1, 'escape': True, 'porder': 3}}),
    (16000, 1, 16, {'subframe': {'type': 'verbatim'}, 'blocksize': 1152}),
    (16000, 1, 16, {'blocksize': [192, 4096, 17, 1, 4608, 100] * 3 + [2000], 'variable': True}),
    (44100, 2, 16, {'channel_mode': 'left_side'}), (48000, 2, 24, {'channel_mode': 'side_right'}),
    (22050, 2, 8, {'channel_mode': 'mid_side'}), (44100, 2, 24, {'channel_mode': 'mid_side'}),
    (32000, 8, 16, {'blocksize': 576}), (16000, 3, 24, {}),
]


def _stream(sr, ch, bps, kw, seed):
    n = sum(kw['blocksize']) if isinstance(kw.get('blocksize'), list) else 20000 + 77 * seed
    x = _signal(n, ch, bps, seed)
    if kw.get('subframe', {}).get('type') == 'fixed' and kw['subframe'].get('porder') == 6:
        x = (x >> 2) << 2                                        # wasted bits
    return x, flac.FlacStream(flacgen.encode(x, sr, bps, **kw), f'm{seed}.flac')


@pytest.mark.parametrize('k', range(len(MATRIX)))
def test_device_matches_host_and_source(fctx, k):
    sr, ch, bps, kw = MATRIX[k]
    x, s = _stream(sr, ch, bps, kw, k)
    want = _stored(x, bps)
    np.testing.assert_array_equal(s.decode_host(), want)
    # (c) staged and read back
    st = fctx.flac_decode(s.audio, s.frames, [(0, 0, len(s.frames), s.n, ch, bps, _native.FLAC_TO_STAGE, -1, 0, 0)], n_signal=0)
    got = fctx.flac_get_stage(0, s.n, ch, bps)
    assert not st.any(), st
    np.testing.assert_array_equal(got, want)
    # (a) straight into a signal of its own
    if ch == 1 and bps <= 16 and sr == 16000:
        st = fctx.flac_decode(s.audio, s.frames, [(0, 0, len(s.frames), s.n, 1, bps, _native.FLAC_TO_SIGNAL, -1, 0, 0)],
                              n_signal=s.n)
        np.testing.assert_array_equal(fctx.get_signal_pcm16(0, s.n), want)
        assert not st.any()
    # (b) staged and resampled in the same call: the WAV twin's resampler result
    if sr != 16000 or ch > 1:
        src = flac.source(s, resample=True)
        st = flac.decode_on(fctx, src)
        got = fctx.get_signal_pcm16(0, src.size)
        assert not st.any()
        np.testing.assert_array_equal(got, R.resample_ref(want, sr))


def _pack(fctx, streams, kinds, pad_before=0):
    """Compressed bytes of every stream end to end (16-byte aligned, after pad_before zero bytes), jobs into a packed uploaded
    signal (gaps of 160 samples filled with a marker) -> (src, frames, jobs, signal, dst offsets)."""
    src, frames, jobs, offs = [np.zeros(pad_before, np.uint8)], [], [], []
    pos, fbeg, dpos = pad_before, 0, 0
    for s, kind in zip(streams, kinds):
        fs = flac.FlacSource(s, kind)
        offs.append(dpos)
        jobs.append(fs.job(fctx, pos, fbeg, dpos).row)
        frames.append(s.frames)
        src.append(s.audio)
        pad = -s.audio.size % 16
        src.append(np.zeros(pad, np.uint8))
        pos += s.audio.size + pad
        fbeg += len(s.frames)
        dpos += (fs.size if kind != 'float' else 0) + 160
    sig = np.full(dpos, 12345, dtype=np.int16)
    return np.concatenate(src), np.concatenate(frames), jobs, sig, offs


def test_ragged_batch_one_launch(fctx):
    streams, kinds, wants = [], [], []
    for k in range(44):
        sr, ch, bps = [(16000, 1, 16), (16000, 1, 8), (44100, 2, 16), (16000, 1, 24), (48000, 1, 24)][k % 5]
        n = 3000 + 1111 * k
        x = _signal(n, ch, bps, 100 + k)
        s = flac.FlacStream(flacgen.encode(x, sr, bps, blocksize=[4096, 1024, 4608][k % 3]), f'r{k}.flac')
        kind = 'float' if (sr, ch, bps) == (16000, 1, 24) else ('pcm' if sr == 16000 and ch == 1 else 'resample')
        streams.append(s); kinds.append(kind)
        wants.append(_stored(x, bps) if kind != 'resample' else R.resample_ref(_stored(x, bps), sr))
    src, frames, jobs, sig, offs = _pack(fctx, streams, kinds)
    fctx.set_signal(sig)
    l0, f0 = fctx.flac_stats()
    r0 = fctx.resample_stats()[0]
    st = fctx.flac_decode(src, frames, jobs)
    got = fctx.get_signal_pcm16(0, sig.size)
    assert fctx.flac_stats() == (l0 + 1, f0 + len(frames))
    assert fctx.resample_stats()[0] == r0 + 1
    assert not st.any()
    covered = np.zeros(sig.size, bool)
    j = 0
    for s, kind, w, o in zip(streams, kinds, wants, offs):
        if kind == 'float':
            np.testing.assert_array_equal(fctx.flac_get_stage(j, s.n, s.ch, s.bps), w)
        else:
            np.testing.assert_array_equal(got[o:o + w.size], w)
            covered[o:o + w.size] = True
        j += 1
    assert np.all(got[~covered] == 12345)


def test_file_past_2_28_bytes(fctx):
    x = _signal(50000, 1, 16, 7)
    s = flac.FlacStream(flacgen.encode(x, 16000, 16), 'far.flac')
    pad = (1 << 28) + 48
    src, frames, jobs, sig, offs = _pack(fctx, [s], ['pcm'], pad_before=pad)
    assert jobs[0][0] == pad and (pad + int(s.frames['offset'][-1])) * 8 > 2 ** 31
    fctx.set_signal(sig)
    st = fctx.flac_decode(src, frames, jobs)
    got = fctx.get_signal_pcm16(0, s.n)
    assert not st.any()
    np.testing.assert_array_equal(got, x.astype(np.int16))


def test_flipped_byte_reported_for_its_file_only(fctx):
    streams, wants = [], []
    for k in range(6):
        x = _signal(30000, 1, 16, 300 + k)
        data, fo = flacgen.encode(x, 16000, 16, return_offsets=True)
        if k == 3:
            data = bytearray(data)
            data[fo[2] + 200] ^= 0x21
        streams.append(flac.FlacStream(bytes(data), f'b{k}.flac'))
        wants.append(x.astype(np.int16))
    src, frames, jobs, sig, offs = _pack(fctx, streams, ['pcm'] * 6)
    fctx.set_signal(sig)
    st = fctx.flac_decode(src, frames, jobs)
    got = fctx.get_signal_pcm16(0, sig.size)                        # (synchronises: the status is valid from here)
    st = st.copy()
    fb = 0
    for k, s in enumerate(streams):
        part = st[fb:fb + len(s.frames)]
        fb += len(s.frames)
        if k == 3:
            assert np.flatnonzero(part).tolist() == [2], part
            with pytest.raises(ValueError, match=rf'b3.flac: frame at byte {s.base + int(s.frames["offset"][2])}: '):
                s.check(part)
        else:
            assert not part.any()
            np.testing.assert_array_equal(got[offs[k]:offs[k] + s.n], wants[k])


# ---------------------------------------------------------------- Segmenter / batch_process / voice femininity
@pytest.fixture(scope='module')
def segs():
    a = Segmenter(ffmpeg=None, models='synthetic')
    b = Segmenter(ffmpeg=None, models='synthetic', resample=True)
    yield a, b
    a.close(); b.close()


def _same_outputs(seg, a, b, tmp_path):
    ra, rb = seg(a), seg(b)
    assert ra == rb
    for fn, ext in ((seg2csv, 'csv'), (seg2textgrid, 'TextGrid')):
        fn(ra, str(tmp_path / f'a.{ext}')); fn(rb, str(tmp_path / f'b.{ext}'))
        assert filecmp.cmp(str(tmp_path / f'a.{ext}'), str(tmp_path / f'b.{ext}'), shallow=False)


def test_segmenter_reads_flac_like_wav(segs, tmp_path):
    plain, rs = segs
    for name in ('musanmix.wav', 'silence2sec.wav'):
        w = os.path.join(GOLDEN, name)
        pcm = iss_io.decode_pcm(w, ffmpeg=None)
        f = flacgen.write(tmp_path / (name + '.flac'), pcm, 16000, 16)
        _same_outputs(plain, f, w, tmp_path)
        np.testing.assert_array_equal(plain.load_pcm(f), pcm)
    short = synth_pcm(5, 8000)                                          # 49 frames: the mspec padding path
    f = flacgen.write(tmp_path / 'short.flac', short, 16000, 16)
    w = flacgen.wav_twin(tmp_path / 'short.wav', short, 16000, 16)
    _same_outputs(plain, f, w, tmp_path)
    x24 = _signal(16000 * 12, 1, 24, 3)                                # 24-bit: the float path
    _same_outputs(plain, flacgen.write(tmp_path / 'm24.flac', x24, 16000, 24), flacgen.wav_twin(tmp_path / 'm24.wav', x24, 16000, 24),
                  tmp_path)
    st = np.stack([x24[:44100 * 8], (x24[:44100 * 8] * 3) // 5], axis=1)      # 44.1 kHz stereo 24-bit, resampled
    f = flacgen.write(tmp_path / 's.flac', st, 44100, 24, channel_mode='mid_side')
    w = flacgen.wav_twin(tmp_path / 's.wav', st, 44100, 24)
    _same_outputs(rs, f, w, tmp_path)
    np.testing.assert_array_equal(rs.load_pcm(f), rs.load_pcm(w))
    with pytest.raises(AssertionError):
        plain(f)


def _flac_and_twins(d):
    flacs, wavs = [], []
    specs = [(16000, 1, 16, 20.0), (16000, 1, 8, 13.3), (16000, 1, 24, 9.1), (44100, 2, 16, 11.0), (48000, 1, 24, 6.0),
             (16000, 1, 16, 16.0), (22050, 2, 24, 8.0), (16000, 1, 16, 0.4)]
    for k, (sr, ch, bps, secs) in enumerate(specs):
        x = _signal(int(sr * secs), ch, bps, 60 + k)
        kw = {'channel_mode': 'mid_side'} if ch == 2 else {}
        flacs.append(flacgen.write(d / f'f{k}.flac', x, sr, bps, **kw))
        wavs.append(flacgen.wav_twin(d / f'f{k}.wav', x, sr, bps))
    x = _signal(16000 * 10, 1, 16, 99)
    data, fo = flacgen.encode(x, 16000, 16, return_offsets=True)
    bad = bytearray(data); bad[fo[5] + 300] ^= 0x08                    # found by the device (CRC-16)
    (d / 'crc.flac').write_bytes(bytes(bad))
    bad = bytearray(data); bad[fo[4] + 5] ^= 0x01                      # found by the index (CRC-8)
    (d / 'hdr.flac').write_bytes(bytes(bad))
    extra = [str(d / 'crc.flac'), str(d / 'hdr.flac'), str(d / 'missing.flac')]
    return flacs[:3] + extra[:1] + flacs[3:6] + extra[1:] + flacs[6:], wavs


def test_batch_process_flac_like_wav(segs, tmp_path, monkeypatch):
    plain, rs = segs
    files, wavs = _flac_and_twins(tmp_path)
    outs = [str(tmp_path / 'out' / (os.path.basename(f) + '.csv')) for f in files]
    per_batch = []
    run = pipeline._Worker.run

    def counted(self, batch):
        l0 = self.ctx.flac_stats()[0]
        out = run(self, batch)
        per_batch.append((sum(isinstance(x, flac.FlacSource) for x in batch.sigs), self.ctx.flac_stats()[0] - l0))
        return out
    monkeypatch.setattr(pipeline._Worker, 'run', counted)
    _, nb, _, lmsg = rs.batch_process(files, outs, batch_files=4, batch_seconds=60)
    errs = [i for i, m in enumerate(lmsg) if m[1] != 0]
    assert errs == [3, 7, 8] and nb == 8, lmsg                         # crc (device), hdr (index), missing
    assert 'crc.flac: frame at byte' in lmsg[3][2], lmsg[3]                      # found by the device: its reason
    assert lmsg[7][2] == "error: <class 'ValueError'>", lmsg[7]                 # a decode-thread error, as for any file
    assert sum(n for n, _ in per_batch) == 7, per_batch                 # 9 FLACs decoded; the 24-bit 16 kHz and the 0.4 s file go alone
    for n, launches in per_batch:
        assert launches == (1 if n else 0), per_batch                   # one decode launch per pass
    k = 0
    for f, o, m in zip(files, outs, lmsg):
        if m[1] == 0:
            w = f[:-5] + '.wav'
            seg2csv(rs(w), str(tmp_path / 'twin.csv'))
            assert filecmp.cmp(o, str(tmp_path / 'twin.csv'), shallow=False), f
            k += 1
    assert k == 8
    plain.dense_batches = True
    try:
        _, nb, _, lmsg3 = plain.batch_process(files[:3] + files[4:7], [o + '.d.csv' for o in outs[:6]], batch_files=3)
    finally:
        plain.dense_batches = False
    assert [m[1] for m in lmsg3] == [0, 0, 0, 2, 2, 0], lmsg3         # 44.1 / 48 kHz: the WAV path's AssertionError
    for f, o, m in zip(files[:3] + files[4:7], [o + '.d.csv' for o in outs[:6]], lmsg3):
        if m[1] == 0:
            seg2csv(plain(f[:-5] + '.wav'), str(tmp_path / 'twin.csv'))
            assert filecmp.cmp(o, str(tmp_path / 'twin.csv'), shallow=False), f
    seg2textgrid(plain(files[0]), str(tmp_path / 'a.TextGrid')); seg2textgrid(plain(wavs[0]), str(tmp_path / 'b.TextGrid'))
    assert filecmp.cmp(str(tmp_path / 'a.TextGrid'), str(tmp_path / 'b.TextGrid'), shallow=False)


def test_voice_femininity_flac_like_wav(tmp_path):
    v = vfs.VoiceFemininityScoring(ffmpeg=None, models='synthetic')
    try:
        flacs, wavs = [], []
        for k, (bps, secs) in enumerate(((16, 25.0), (8, 12.0), (24, 20.0))):
            x = bench.synth_recording_numpy(k, int(16000 * secs)).astype(np.int64)
            x = (x << 8) if bps == 24 else x >> (16 - bps)
            flacs.append(flacgen.write(tmp_path / f'v{k}.flac', x, 16000, bps))
            wavs.append(flacgen.wav_twin(tmp_path / f'v{k}.wav', x, 16000, bps))
        want = [v(p) for p in wavs]
        assert [v(p) for p in flacs] == want
        assert v.batch_process(flacs) == want
        assert any(w[2] > 0 for w in want), want
    finally:
        v.vad.close()
