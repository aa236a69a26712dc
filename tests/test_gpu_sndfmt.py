"""GPU: the stored formats the resample kernel reads since sndfmt.py (signed bytes, G.711, big-endian samples) and
adpcm_decode_kernel must be bit-identical to the WAV twin's path (resample.resample_ref of the twin's samples, the host build
of the IMA decoder, the audioop-generated golden vectors), and every entry point must give a G.711 / IMA ADPCM / AIFF / AU /
CAF / Wave64 / RF64 file what it gives the file's WAV twin.  Every comparison is exact."""
import filecmp
import os
import sys

import numpy as np
import pytest

import bench
import flacgen
import sndgen
import wavgen
from conftest import GOLDEN, synth_pcm
from inaspeechsegmenter_amd import _native, Segmenter, seg2csv, seg2textgrid, flac, pipeline, sndfmt, vfs
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.segmenter import RawSource

pytestmark = pytest.mark.gpu

VEC = np.load(os.path.join(GOLDEN, 'sndfmt_vectors.npz'))
RATES = (8000, 11025, 16000, 44100, 48000)


@pytest.fixture(scope='module')
def sctx():
    c = _native.Context(0)
    yield c
    c.close()


def _sound(x, kind, big, sr, block_align=256, name='<test>'):
    """float samples -> (sndfmt.Sound over the stored bytes, the twin's array as io reads it)."""
    ch = 1 if x.ndim == 1 else x.shape[1]
    if kind == 'ima':
        block_align = -(-block_align // (4 * ch)) * 4 * ch
    data, tfmt, twin, n = sndgen.encode(x, kind, big, block_align)
    d = np.frombuffer(data, dtype=np.uint8)
    if kind == 'ima':
        s = sndfmt.Sound(name, sr, ch, kind, False, d, 0, frames=n, block_align=block_align, spb=sndgen.ima_samples_per_block(block_align, ch))
    else:
        s = sndfmt.Sound(name, sr, ch, kind, big, d, 0)
    return s, wavgen.as_read(twin, tfmt)


# ------------------------------------------------------------------------------------------------ resample kernel
FORMATS = [('i8', True), ('ulaw', False), ('alaw', False), ('i16', True), ('i24', True), ('i32', True), ('f32', True), ('f64', True)]


@pytest.mark.parametrize('kind,big', FORMATS, ids=[k for k, _ in FORMATS])
def test_resample_kernel_reads_stored_format(sctx, kind, big):
    for ch in range(1, 7):
        for sr in RATES:
            x = wavgen.make_signal(2600 + 37 * ch, ch, 11 * ch + sr % 89)
            s, twin = _sound(x, kind, big, sr)
            raw, fmt = s.raw()
            if kind in ('i16', 'i32', 'f32', 'f64'):
                assert fmt & _native.RS_SWAP and raw.dtype.kind == 'u'      # the bytes go as stored: swapped on the device
            if kind in ('ulaw', 'alaw', 'i8'):
                assert raw.dtype == np.uint8 and fmt in (_native.RS_ULAW, _native.RS_ALAW, _native.RS_I8)
            n = sctx.resample_signal(raw, sr, fmt)
            np.testing.assert_array_equal(sctx.get_signal_pcm16(0, n), R.resample_ref(twin, sr), err_msg=f'{kind} {ch} ch {sr} Hz')


def test_resample_kernel_refuses_swapped_bytes(sctx):
    x = np.zeros(100, np.uint8)
    for fmt in (_native.RS_ULAW | _native.RS_SWAP, _native.RS_I8 | _native.RS_SWAP, 0 | _native.RS_SWAP, 5, 7, 11, 0x200 | 1):
        with pytest.raises(_native.NativeError, match='bad format'):
            sctx.resample_signal(x, 8000, fmt)


def test_all_g711_codes_through_the_kernel(sctx):
    codes = np.tile(np.arange(256, dtype=np.uint8), 3)
    for law, fmt in (('ulaw', _native.RS_ULAW), ('alaw', _native.RS_ALAW)):
        n = sctx.resample_signal(np.stack([codes, codes], axis=1), 16000, fmt)      # two equal channels, identity filter
        np.testing.assert_array_equal(sctx.get_signal_pcm16(0, n), np.tile(VEC[law], 3))


# ------------------------------------------------------------------------------------------------ ADPCM kernel
def _decode_staged(ctx, s):
    st = ctx.adpcm_decode(s.data, [(0, 0, s.nblocks, s.n, s.ch, s.block_align, _native.ADPCM_TO_STAGE, -1, 0, 0)], s.nblocks, n_signal=0)
    got = ctx.adpcm_get_stage(0, s.n, s.ch)
    assert not st.any(), st
    return got


def test_adpcm_kernel_equals_golden(sctx):
    nib, pred, index, out = VEC['ima_nibbles'], VEC['ima_pred'], VEC['ima_index'], VEC['ima_out']
    align = 4 + nib.shape[1] // 2
    blocks = np.frombuffer(b''.join(sndgen.ima_block(nib[k], pred[k], index[k]) for k in range(len(nib))), np.uint8)
    want = np.concatenate((pred[:, None], out), axis=1).reshape(-1)
    s = sndfmt.Sound('golden', 16000, 1, 'ima', False, blocks, 0, block_align=align, spb=nib.shape[1] + 1)
    assert s.n == want.size
    np.testing.assert_array_equal(_decode_staged(sctx, s), want)
    st = sndfmt.decode_on(sctx, sndfmt.AdpcmSource(s, 'pcm'))
    np.testing.assert_array_equal(sctx.get_signal_pcm16(0, s.n), want)
    assert not st.any()


@pytest.mark.parametrize('block_align', [256, 512, 1024, 2048])
def test_adpcm_kernel_matches_host_every_output(sctx, block_align):
    for ch in (1, 2, 3, 5, 6):
        for sr in (8000, 16000, 44100):
            x = wavgen.make_signal(7000 + 501 * ch, ch, block_align + ch + sr % 7)
            s, twin = _sound(x, 'ima', False, sr, block_align)
            host = s.stored()
            np.testing.assert_array_equal(host, twin)
            np.testing.assert_array_equal(_decode_staged(sctx, s), twin)           # (c) staged and read back
            src = sndfmt.source(s, resample=True)
            assert isinstance(src, sndfmt.AdpcmSource) and src.kind == ('pcm' if (sr, ch) == (16000, 1) else 'resample')
            l0, r0 = sctx.adpcm_stats()[0], sctx.resample_stats()[0]
            st = sndfmt.decode_on(sctx, src)
            got = sctx.get_signal_pcm16(0, src.size)
            assert not st.any()
            assert sctx.adpcm_stats()[0] == l0 + 1 and sctx.resample_stats()[0] == r0 + (src.kind == 'resample')
            # (a) straight into the signal / (b) staged and resampled in the same call: the WAV twin's result
            np.testing.assert_array_equal(got, twin if src.kind == 'pcm' else R.resample_ref(twin, sr))


def test_adpcm_kernel_largest_blocks(sctx):
    """Blocks whose samples need more LDS than the 64 KiB a kernel gets by default: just under it next to the kernel's static
    LDS (16380 bytes mono: 65 506 bytes), and the largest block taken (32768 bytes: 131 058 bytes)."""
    for block_align, ch, sr in ((16380, 1, 16000), (32768, 1, 8000), (32768, 2, 44100), (32760, 3, 16000)):
        x = wavgen.make_signal(140000, ch, block_align + ch)
        s, twin = _sound(x, 'ima', False, sr, block_align)
        np.testing.assert_array_equal(_decode_staged(sctx, s), twin)
        src = sndfmt.source(s, resample=True)
        st = sndfmt.decode_on(sctx, src)
        got = sctx.get_signal_pcm16(0, src.size)
        assert not st.any()
        np.testing.assert_array_equal(got, twin if src.kind == 'pcm' else R.resample_ref(twin, sr))


def _pack(ctx, sounds, kinds, pad_before=0):
    """Blocks of every file end to end (16-byte aligned, after pad_before zero bytes), jobs into a packed uploaded signal
    (gaps of 160 samples filled with a marker; kind 'stage': decoded to the staging buffer only, no room in the signal)
    -> (src, jobs, nblocks, signal, dst offsets)."""
    src, jobs, offs = [np.zeros(pad_before, np.uint8)], [], []
    pos, bbeg, dpos = pad_before, 0, 0
    for s, kind in zip(sounds, kinds):
        offs.append(dpos)
        if kind == 'stage':                                             # staged only (no Source asks for it): nothing in the signal
            jobs.append((pos, bbeg, s.nblocks, s.n, s.ch, s.block_align, _native.ADPCM_TO_STAGE, -1, 0, 0))
        else:
            a = sndfmt.AdpcmSource(s, kind)
            jobs.append(a.job(ctx, pos, bbeg, dpos).row)
            dpos += a.size
        pad = -s.data.size % 16
        src += [s.data, np.zeros(pad, np.uint8)]
        pos += s.data.size + pad
        bbeg += s.nblocks
        dpos += 160
    return np.concatenate(src), jobs, bbeg, np.full(dpos, 12345, dtype=np.int16), offs


def test_adpcm_ragged_batch_one_launch(sctx):
    sounds, kinds, wants = [], [], []
    for k in range(37):
        sr, ch, align = [(16000, 1, 256), (8000, 1, 256), (8000, 2, 512), (44100, 2, 2048), (16000, 1, 1024), (11025, 3, 516)][k % 6]
        x = wavgen.make_signal(1500 + 977 * k, ch, 200 + k)
        s, twin = _sound(x, 'ima', False, sr, align, name=f'r{k}.wav')
        kind = 'stage' if k % 12 == 11 else 'pcm' if (sr, ch) == (16000, 1) else 'resample'
        sounds.append(s); kinds.append(kind)
        wants.append(R.resample_ref(twin, sr) if kind == 'resample' else twin)
    src, jobs, nblocks, sig, offs = _pack(sctx, sounds, kinds)
    sctx.set_signal(sig)
    l0, b0 = sctx.adpcm_stats()
    r0 = sctx.resample_stats()[0]
    st = sctx.adpcm_decode(src, jobs, nblocks)
    got = sctx.get_signal_pcm16(0, sig.size)
    assert sctx.adpcm_stats() == (l0 + 1, b0 + nblocks)
    assert sctx.resample_stats()[0] == r0 + 1
    assert not st.any()
    covered = np.zeros(sig.size, bool)
    for j, (s, kind, w, o) in enumerate(zip(sounds, kinds, wants, offs)):
        if kind == 'stage':
            np.testing.assert_array_equal(sctx.adpcm_get_stage(j, s.n, s.ch), w)
        else:
            np.testing.assert_array_equal(got[o:o + w.size], w)
            covered[o:o + w.size] = True
    assert np.all(got[~covered] == 12345)


def test_adpcm_file_past_2_28_bytes(sctx):
    s, twin = _sound(wavgen.make_signal(50000, 1, 7), 'ima', False, 16000, 1024)
    pad = (1 << 28) + 48
    src, jobs, nblocks, sig, offs = _pack(sctx, [s], ['pcm'], pad_before=pad)
    assert jobs[0][0] == pad and (pad + s.data.size) * 8 > 2 ** 31
    sctx.set_signal(sig)
    st = sctx.adpcm_decode(src, jobs, nblocks)
    got = sctx.get_signal_pcm16(0, s.n)
    assert not st.any()
    np.testing.assert_array_equal(got, twin)


def _corrupt(s, block, channel=0):
    d = s.data.copy()
    d[block * s.block_align + 4 * channel + 2] = 89 + block
    return sndfmt.Sound(s.name, s.sr, s.ch, 'ima', False, d, s.base, frames=s.n, block_align=s.block_align, spb=s.spb)


def test_bad_step_index_reported_for_its_file_only(sctx):
    sounds, wants = [], []
    for k in range(6):
        s, twin = _sound(wavgen.make_signal(30000, 1 + k % 2, 300 + k), 'ima', False, 16000 if k % 2 == 0 else 8000, 512, name=f'b{k}.wav')
        if k == 3:
            s = _corrupt(s, 2, channel=1)
        sounds.append(s)
        wants.append(twin if k % 2 == 0 else R.resample_ref(twin, 8000))
    kinds = ['pcm' if k % 2 == 0 else 'resample' for k in range(6)]
    src, jobs, nblocks, sig, offs = _pack(sctx, sounds, kinds)
    sctx.set_signal(sig)
    st = sctx.adpcm_decode(src, jobs, nblocks)
    got = sctx.get_signal_pcm16(0, sig.size)                        # (synchronises: the status is valid from here)
    st = st.copy()
    bb = 0
    for k, s in enumerate(sounds):
        part = st[bb:bb + s.nblocks]
        bb += s.nblocks
        if k == 3:
            assert np.flatnonzero(part).tolist() == [2], part
            with pytest.raises(ValueError, match=rf'b3\.wav: block at byte {2 * 512}: step index above 88'):
                s.check(part)
            with pytest.raises(ValueError, match=rf'b3\.wav: block at byte {2 * 512}: step index above 88'):
                s.stored()                                          # the host build says the same
        else:
            assert not part.any()
            np.testing.assert_array_equal(got[offs[k]:offs[k] + wants[k].size], wants[k])


# ------------------------------------------------------------------------------------------------ Segmenter / batch_process / voice femininity
@pytest.fixture(scope='module')
def segs():
    a = Segmenter(ffmpeg=None, models='synthetic')
    b = Segmenter(ffmpeg=None, models='synthetic', resample=True)
    yield a, b
    a.close(); b.close()


def _speech(seed, n, ch=1):
    base = synth_pcm(seed, n).astype(np.float64) / 32768.0
    if ch == 1:
        return base
    return np.stack([np.roll(base, 31 * c) * (1.0 - 0.1 * c) for c in range(ch)], axis=1)


def _pair(d, stem, container, kind, big, x, sr, **kw):
    """(file, WAV twin) with the same stem, the twin in the directory twins/."""
    os.makedirs(d / 'twins', exist_ok=True)
    ext = {'wav': 'wav', 'wavx': 'wav', 'rf64': 'rf64', 'bw64': 'wav', 'w64': 'w64', 'au': 'au', 'dns': 'snd', 'caf': 'caf'}.get(container, 'aif')
    p, tfmt, twin = sndgen.write(d / f'{stem}.{ext}', container, kind, big, x, sr, **kw)
    return p, sndgen.wav_twin(d / 'twins' / f'{stem}.wav', twin, sr, tfmt)


def _same_outputs(seg, a, b, tmp_path):
    ra, rb = seg(a), seg(b)
    assert ra == rb
    for fn, ext in ((seg2csv, 'csv'), (seg2textgrid, 'TextGrid')):
        fn(ra, str(tmp_path / f'a.{ext}')); fn(rb, str(tmp_path / f'b.{ext}'))
        assert filecmp.cmp(str(tmp_path / f'a.{ext}'), str(tmp_path / f'b.{ext}'), shallow=False)
    pa, pb = seg.load_pcm(a), seg.load_pcm(b)
    assert pa.dtype == pb.dtype
    np.testing.assert_array_equal(pa, pb)


SINGLE = [('wav', 'ulaw', False), ('wavx', 'alaw', False), ('wav', 'ima', False), ('aiff', 'i16', True), ('aiff', 'i8', True),
          ('aifc', 'f32', True), ('au', 'ulaw', True), ('au', 'i24', True), ('caf', 'i32', True), ('caf', 'f64', False), ('w64', 'ima', False),
          ('rf64', 'i16', False), ('aifc', 'u8', False), ('dns', 'i16', False)]


def test_segmenter_reads_like_wav_twin(segs, tmp_path):
    plain, rs = segs
    for k, (container, kind, big) in enumerate(SINGLE):
        p, w = _pair(tmp_path, f'm{k}', container, kind, big, _speech(k, 16000 * 9), 16000)     # 16 kHz mono: both Segmenters
        _same_outputs(plain, p, w, tmp_path)
        _same_outputs(rs, p, w, tmp_path)
        sr, ch = [(8000, 1), (8000, 2), (44100, 2), (16000, 3), (11025, 1)][k % 5]
        p, w = _pair(tmp_path, f's{k}', container, kind, big, _speech(50 + k, sr * 7, ch), sr)
        _same_outputs(rs, p, w, tmp_path)
        for fn in (plain, plain.load_pcm):                             # without resample: the twin's refusal, the file's name in it
            with pytest.raises((AssertionError, ValueError)) as e1:
                fn(p)
            with pytest.raises((AssertionError, ValueError)) as e2:
                fn(w)
            assert type(e1.value) is type(e2.value) and str(e1.value).replace(p, '') == str(e2.value).replace(w, '')
    p, w = _pair(tmp_path, 'short', 'wav', 'ima', False, _speech(5, 8000), 16000)              # 49 frames: the mspec padding path
    _same_outputs(plain, p, w, tmp_path)
    p, w = _pair(tmp_path, 'tiny', 'au', 'ulaw', True, _speech(5, 150), 8000)                  # under one analysis window
    for f in (p, w):
        with pytest.raises(ValueError, match='less than one 25 ms analysis window'):
            rs(f)


def _batch_files(d):
    specs = [('wav', 'ulaw', False, 8000, 1, 20.0), ('wav', 'ima', False, 8000, 1, 13.3), ('aiff', 'i16', True, 44100, 2, 9.1),
             ('wav', 'ima', False, 16000, 1, 11.0), ('au', 'alaw', True, 8000, 2, 6.0), ('caf', 'f32', True, 48000, 1, 7.0),
             ('wav', 'ima', False, 11025, 2, 8.0), ('aiff', 'i16', True, 16000, 1, 12.0), ('w64', 'ulaw', False, 16000, 1, 9.0),
             ('wav', 'ima', False, 8000, 1, 0.4), ('aifc', 'i8', True, 16000, 1, 6.0), ('au', 'i24', True, 22050, 1, 6.0)]
    files, wavs = [], []
    for k, (container, kind, big, sr, ch, secs) in enumerate(specs):
        p, w = _pair(d, f'f{k}', container, kind, big, _speech(60 + k, int(sr * secs), ch), sr)
        files.append(p); wavs.append(w)
    x = _speech(98, 16000 * 10)
    flacs = [flacgen.write(d / 'f90.flac', synth_pcm(98, 160000), 16000, 16), flacgen.write(d / 'f91.flac', synth_pcm(97, 80000), 8000, 16)]
    fw = [flacgen.wav_twin(d / 'twins' / 'f90.wav', synth_pcm(98, 160000), 16000, 16), flacgen.wav_twin(d / 'twins' / 'f91.wav', synth_pcm(97, 80000), 8000, 16)]
    pcm = [wavgen.write_wav(d / 'f92.wav', wavgen.encode(x, 'i16'), 16000, 'i16'), wavgen.write_wav(d / 'f93.wav', wavgen.encode(_speech(96, 48000 * 5, 2), 'i16'), 48000, 'i16')]
    s, _ = _sound(_speech(95, 80000), 'ima', False, 8000, name='bad')
    bad = _corrupt(s, 7)
    sndgen.write_riff(d / 'badidx.wav', sndgen.wav_fmt('ima', 8000, 1, 256), bad.data.tobytes(), fact=80000)
    (d / 'malformed.aif').write_bytes(open(files[2], 'rb').read()[:30])
    extra = [str(d / 'badidx.wav'), str(d / 'malformed.aif'), str(d / 'missing.au')]
    order = files[:4] + extra[:1] + flacs + files[4:8] + extra[1:] + pcm + files[8:]
    twins = dict(zip(files + flacs + pcm, wavs + fw + pcm))
    return order, twins


def test_batch_process_like_wav_twins(segs, tmp_path, monkeypatch):
    plain, rs = segs
    files, twins = _batch_files(tmp_path)
    per_batch = []
    run = pipeline._Worker.run

    def counted(self, batch):
        before = (self.ctx.adpcm_stats()[0], self.ctx.flac_stats()[0], self.ctx.resample_stats()[0])
        out = run(self, batch)
        after = (self.ctx.adpcm_stats()[0], self.ctx.flac_stats()[0], self.ctx.resample_stats()[0])
        kinds = (sum(isinstance(x, sndfmt.AdpcmSource) for x in batch.sigs), sum(isinstance(x, flac.FlacSource) for x in batch.sigs),
                 sum(isinstance(x, RawSource) for x in batch.sigs))
        per_batch.append((kinds, tuple(b - a for a, b in zip(before, after))))
        return out
    monkeypatch.setattr(pipeline._Worker, 'run', counted)
    for fmt, fexp in (('csv', seg2csv), ('textgrid', seg2textgrid)):
        outs = [str(tmp_path / f'out_{fmt}' / (os.path.basename(f) + '.' + fmt)) for f in files]
        del per_batch[:]
        _, nb, _, lmsg = rs.batch_process(files, outs, batch_files=6, batch_seconds=80, output_format=fmt)
        errs = {os.path.basename(files[i]): m[2] for i, m in enumerate(lmsg) if m[1] != 0}
        assert sorted(errs) == ['badidx.wav', 'malformed.aif', 'missing.au'] and nb == len(files) - 3, lmsg
        assert 'badidx.wav: block at byte' in errs['badidx.wav'] and 'step index above 88' in errs['badidx.wav']      # found by the device
        assert errs['malformed.aif'] == "error: <class 'ValueError'>"               # a decode-thread error, as for any file
        assert sum(k[0] for k, _ in per_batch) == 4 and sum(k[1] for k, _ in per_batch) == 2, per_batch   # (the 0.4 s ADPCM file goes alone)
        for (na, nf, nr), (la, lf, lr) in per_batch:
            assert la == (1 if na else 0) and lf == (1 if nf else 0), per_batch    # one decode launch per codec and pass
            assert lr <= (1 if nr else 0) + (1 if nf else 0) + (1 if na else 0), per_batch   # at most one resample launch per source kind
        for f, o, m in zip(files, outs, lmsg):
            if m[1] == 0:
                fexp(rs(twins[f]), str(tmp_path / 'twin.out'))
                assert filecmp.cmp(o, str(tmp_path / 'twin.out'), shallow=False), f
    # without resample: the 16 kHz mono files are segmented, the others are the WAV path's per-file errors
    outs = [str(tmp_path / 'out_plain' / (os.path.basename(f) + '.csv')) for f in files]
    plain.dense_batches = True
    try:
        _, nb, _, lmsg = plain.batch_process(files, outs, batch_files=5)
    finally:
        plain.dense_batches = False
    for f, o, m in zip(files, outs, lmsg):
        if f not in twins:
            assert m[1] == 2
            continue
        try:
            want = plain(twins[f])
        except (AssertionError, ValueError):
            assert m[1] == 2, (f, m)
            continue
        assert m[1] == 0, (f, m)
        seg2csv(want, str(tmp_path / 'twin.out'))
        assert filecmp.cmp(o, str(tmp_path / 'twin.out'), shallow=False), f
    assert nb == 6, lmsg


def test_cli_reads_like_wav_twins(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    import ina_speech_segmenter_amd as cli
    d = tmp_path / 'in'
    os.makedirs(d)
    pairs = [_pair(d, f'c{k}', c, kind, big, _speech(20 + k, sr * 8, ch), sr)
             for k, (c, kind, big, sr, ch) in enumerate((('wav', 'ulaw', False, 8000, 1), ('wav', 'ima', False, 8000, 2),
                                                         ('aiff', 'i16', True, 44100, 2), ('au', 'alaw', True, 16000, 1),
                                                         ('caf', 'i24', True, 16000, 1)))]
    for name, inputs in (('files', [p for p, _ in pairs]), ('twins', [w for _, w in pairs])):
        os.makedirs(tmp_path / name)
        assert cli.main(['-i'] + inputs + ['-o', str(tmp_path / name), '-b', 'None', '--resample', '--models', 'synthetic']) == 0
    for k in range(len(pairs)):
        assert filecmp.cmp(str(tmp_path / 'files' / f'c{k}.csv'), str(tmp_path / 'twins' / f'c{k}.csv'), shallow=False), k


def test_voice_femininity_like_wav_twins(tmp_path):
    for resample in (False, True):
        v = vfs.VoiceFemininityScoring(ffmpeg=None, models='synthetic', resample=resample)
        try:
            specs = [('wav', 'ulaw', False, 16000, 1, 25.0), ('wav', 'ima', False, 16000, 1, 12.0), ('aiff', 'i24', True, 16000, 1, 20.0)]
            if resample:
                specs += [('au', 'ulaw', True, 8000, 1, 20.0), ('wav', 'ima', False, 8000, 2, 15.0), ('caf', 'i16', True, 44100, 2, 12.0)]
            files, wavs = [], []
            for k, (c, kind, big, sr, ch, secs) in enumerate(specs):
                x = bench.synth_recording_numpy(k, int(sr * secs)).astype(np.float64) / 32768.0
                x = x if ch == 1 else np.stack([x, np.roll(x, 17) * 0.8], axis=1)
                p, w = _pair(tmp_path, f'v{int(resample)}{k}', c, kind, big, x, sr)
                files.append(p); wavs.append(w)
            want = [v(p) for p in wavs]
            assert [v(p) for p in files] == want
            assert v.batch_process(files) == want
            assert any(w[2] > 0 for w in want), want
        finally:
            v.vad.close()
