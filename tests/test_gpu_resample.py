"""GPU: WAV sources at other rates / channel counts without ffmpeg (iss_resample_pcm16, Segmenter(resample=True)).
The device's PCM16 must be bit-identical to resample.resample_ref (float64, same summation order)."""
import filecmp
import os

import numpy as np
import pytest

from inaspeechsegmenter_amd import _native, Segmenter, seg2csv, pipeline, vfs
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
import bench
from conftest import GOLDEN, synth_pcm
from wavgen import FORMATS, encode, as_read, write_wav, make_signal

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000, 44056)


@pytest.fixture(scope='module')
def rctx():
    c = _native.Context(0)
    yield c
    c.close()


def _device(ctx, x, sr):
    n = ctx.resample_signal(x, sr)
    return ctx.get_signal_pcm16(0, n)


def _check(ctx, x, sr, what):
    got, want = _device(ctx, x, sr), R.resample_ref(x, sr)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:10], got[bad[:10]], want[bad[:10]])


@pytest.mark.parametrize('sr', RATES)
def test_bit_identical_every_format_and_channel_count(rctx, sr):
    up, down, h = R.plan(sr)
    hl = (h.size - 1) // 2
    lengths = (1, 5, max(1, hl // up - 3), 4801, 20011)          # shorter than the filter's half length, ragged outputs
    for fmt in FORMATS:
        for ch in (1, 2, 6):
            for k, n in enumerate(lengths):
                st = encode(make_signal(n, ch, 1000 * ch + k), fmt)
                if fmt in ('f32', 'f64'):
                    st = st * 1.25                              # float sources beyond full scale: saturation
                _check(rctx, as_read(st, fmt), sr, (sr, fmt, ch, n))
    assert any(R.out_len(n, sr) % 160 for n in lengths)


@pytest.mark.parametrize('fmt', FORMATS)
def test_16k_multichannel_is_downmix_and_quantise(rctx, fmt):
    for ch in (2, 6):
        x = as_read(encode(make_signal(7777, ch, ch), fmt), fmt)
        _check(rctx, x, 16000, (fmt, ch))


def test_long_file_64bit_index(rctx):
    n = 44100 * 360                                              # 6 min: i * down passes 2^31
    x = encode(make_signal(n, 1, 99), 'i16')
    got = _device(rctx, x, 44100)
    nout = R.out_len(n, 44100)
    assert got.size == nout and (nout - 1) * 441 > 2 ** 31
    want = R.resample_ref(x, 44100)
    for a in (0, nout // 2 - 50000, nout - 100000):
        assert np.array_equal(got[a:a + 100000], want[a:a + 100000]), a


def _pack(sources):
    """Today's packing of the pipeline (every file on a multiple of 160 samples, zero gaps), the resampled files' ranges
    left zero -> (buffer, offsets, end)."""
    offs, pos = [], 0
    for s in sources:
        n = s.size if isinstance(s, np.ndarray) else R.out_len(s[0].shape[0], s[1])
        offs.append((pos, n))
        pos += -(-n // 160) * 160
    buf = np.zeros(pos, np.int16)
    for s, (o, n) in zip(sources, offs):
        if isinstance(s, np.ndarray):
            buf[o:o + n] = s
    return buf, offs


def test_one_launch_for_a_mixed_batch(rctx):
    srcs = [encode(make_signal(16000 * 3 + 7, 1, 1), 'i16'),
            (as_read(encode(make_signal(44100 * 2 + 3, 2, 2), 'i24'), 'i24'), 44100),
            (encode(make_signal(48000 * 3 + 1, 6, 3), 'f32'), 48000),
            synth_pcm(4, 16000 * 2 + 100),
            (encode(make_signal(8000 * 2 + 11, 1, 5), 'u8'), 8000),
            (encode(make_signal(22050 * 1 + 5, 2, 6), 'f64'), 22050),
            (encode(make_signal(16000 * 2 + 9, 2, 7), 'i32'), 16000),
            (encode(make_signal(44056 * 2 + 1, 1, 8), 'i16'), 44056),
            synth_pcm(9, 16000 + 33)]
    buf, offs = _pack(srcs)
    raw, jobs, rpos = [], [], 0
    for s, (o, n) in zip(srcs, offs):
        if isinstance(s, tuple):
            b = np.ascontiguousarray(s[0]).reshape(-1).view(np.uint8)
            raw.append(b)
            raw.append(np.zeros(-(-b.size // 16) * 16 - b.size, np.uint8))
            jobs.append(rctx.resample_job(s[0], s[1], rpos, o))
            rpos += -(-b.size // 16) * 16
    l0, j0 = rctx.resample_stats()
    rctx.set_signal(buf)
    rctx.resample(np.concatenate(raw), jobs)
    got = rctx.get_signal_pcm16(0, buf.size)
    assert len(jobs) == 6 and rctx.resample_stats() == (l0 + 1, j0 + 6)
    keep = np.ones(buf.size, bool)
    for s, (o, n) in zip(srcs, offs):
        if isinstance(s, tuple):
            assert np.array_equal(got[o:o + n], _device(rctx, *s)), s[1]
            keep[o:o + n] = False
    assert got[keep].tobytes() == buf[keep].tobytes()            # 16 kHz files and zero gaps exactly as uploaded


def test_bad_jobs_are_refused(rctx):
    x = encode(make_signal(4410, 2, 1), 'i16')
    job = list(rctx.resample_job(x, 44100, 0, 0))
    src = x.reshape(-1).view(np.uint8)
    for k, v in ((3, 7), (4, 99), (7, 10), (0, 2), (0, 4), (6, 10 ** 9)):
        bad = list(job)
        bad[k] = v
        with pytest.raises(_native.NativeError):
            rctx.resample(src, [tuple(bad)], n_signal=job[7])
    with pytest.raises(_native.NativeError):                     # overlapping outputs
        rctx.resample(src, [tuple(job), tuple(job)], n_signal=2 * job[7])


# ---------------------------------------------------------------- Segmenter / batch_process / voice femininity
@pytest.fixture(scope='module')
def segs():
    a = Segmenter(ffmpeg=None, models='synthetic', resample=True)
    b = Segmenter(ffmpeg=None, models='synthetic')
    yield a, b
    a.close(); b.close()


def _musan_48k_stereo(path):
    """musanmix.wav upsampled to 48 kHz (linear interpolation), left = the signal, right = 0.6 x it + a little noise."""
    pcm = iss_io.decode_pcm(os.path.join(GOLDEN, 'musanmix.wav'), ffmpeg=None).astype(np.float64)
    t = np.arange(pcm.size * 3) / 3.0
    up = np.interp(t, np.arange(pcm.size), pcm)
    rng = np.random.default_rng(48)
    st = np.stack([up, 0.6 * up + rng.normal(0, 30, up.size)], axis=1)
    st = np.clip(np.round(st), -32768, 32767).astype('<i2')
    return write_wav(path, st, 48000, 'i16'), st


def test_segmenter_48k_stereo(segs, tmp_path):
    rs, plain = segs
    p, st = _musan_48k_stereo(tmp_path / 'musan48.wav')
    got = rs(p)
    want = plain.segment_signal(R.resample_ref(st, 48000))
    assert got == want
    seg2csv(got, str(tmp_path / 'a.csv')); seg2csv(want, str(tmp_path / 'b.csv'))
    assert filecmp.cmp(str(tmp_path / 'a.csv'), str(tmp_path / 'b.csv'), shallow=False)
    mus = os.path.join(GOLDEN, 'musanmix.wav')
    assert rs(mus) == plain(mus)                                  # 16 kHz mono: today's result
    with pytest.raises(AssertionError):
        plain(p)


def _mixed_files(d):
    files = []
    specs = [(48000, 2, 'i16', 20.0), (44100, 1, 'i24', 13.3), (16000, 1, 'i16', 9.1), (22050, 6, 'f32', 11.0),
             (8000, 2, 'u8', 15.2), (96000, 1, 'i32', 7.4), (16000, 2, 'f64', 12.5), (44056, 2, 'i16', 8.0),
             (32000, 1, 'f64', 0.4), (16000, 1, 'i16', 16.0)]
    for k, (sr, ch, fmt, secs) in enumerate(specs):
        n = int(sr * secs)
        base = synth_pcm(40 + k, int(16000 * secs) + 1) / 32768.0
        x = np.interp(np.arange(n) * 16000.0 / sr, np.arange(base.size), base)
        if ch > 1:
            x = np.stack([x * (1 - 0.1 * c) for c in range(ch)], axis=1)
        files.append(write_wav(d / f'f{k}_{sr}_{ch}_{fmt}.wav', encode(x, fmt), sr, fmt))
    short = write_wav(d / 'short_48k.wav', encode(make_signal(600, 2, 1), 'i16'), 48000, 'i16')   # 200 samples at 16 kHz
    corrupt = str(d / 'corrupt.wav')
    with open(corrupt, 'wb') as f:
        f.write(b'RIFF\x10\x00\x00\x00WAVEjunkjunkjunk')
    return files[:4] + [corrupt] + files[4:8] + [short] + files[8:]


def test_batch_process_mixed_files(segs, tmp_path, monkeypatch):
    rs, _ = segs
    files = _mixed_files(tmp_path)
    assert len(files) == 12
    per_batch = []
    run = pipeline._Worker.run

    def counted(self, batch):
        l0 = self.ctx.resample_stats()[0]
        out = run(self, batch)
        per_batch.append((sum(not isinstance(s, np.ndarray) for s in batch.sigs),
                          self.ctx.resample_stats()[0] - l0))
        return out
    monkeypatch.setattr(pipeline._Worker, 'run', counted)
    outs = [str(tmp_path / 'out' / (os.path.basename(f) + '.csv')) for f in files]
    _, nb, _, lmsg = rs.batch_process(files, outs, batch_files=3, batch_seconds=60)
    errs = [i for i, m in enumerate(lmsg) if m[1] != 0]
    assert errs == [4, 9] and nb == 10, lmsg
    assert len(per_batch) >= 3 and sum(n for n, _ in per_batch) >= 6
    for nraw, launches in per_batch:
        assert launches == (1 if nraw else 0), per_batch
    for f, o, m in zip(files, outs, lmsg):
        if m[1] == 0:
            seg2csv(rs(f), str(tmp_path / 'single.csv'))
            assert filecmp.cmp(o, str(tmp_path / 'single.csv'), shallow=False), f


def test_voice_femininity_resample(tmp_path):
    v = vfs.VoiceFemininityScoring(ffmpeg=None, models='synthetic', resample=True)
    try:
        srcs, refs = [], []
        for k, (sr, ch, secs) in enumerate(((48000, 2, 25.0), (44100, 2, 12.0), (48000, 1, 40.0))):
            base = bench.synth_recording_numpy(k, int(16000 * secs)) / 32768.0     # voiced stretches: x-vectors to score
            n = int(sr * secs)
            x = np.interp(np.arange(n) * 16000.0 / sr, np.arange(base.size), base)
            st = encode(np.stack([x, 0.8 * x], axis=1) if ch == 2 else x, 'i16')
            srcs.append(write_wav(tmp_path / f'v{k}.wav', st, sr, 'i16'))
            refs.append(write_wav(tmp_path / f'v{k}_16k.wav', R.resample_ref(st, sr), 16000, 'i16'))
        want = [v(p) for p in refs]
        assert [v(p) for p in srcs] == want
        assert v.batch_process(srcs) == want
        assert any(w[2] > 0 for w in want), want
    finally:
        v.vad.close()
