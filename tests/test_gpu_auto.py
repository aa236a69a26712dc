"""GPU: the survey-guided downmix (channels='auto').  Everything is an equality: load_pcm_auto against load_pcm_mixes / load_pcm
and against io.decode_auto, the host-only twin, to the bit; its survey against both survey_channels; segment_auto against
segment_mixes / the default call; the CSVs of a mixed pass against those of each file alone, byte for byte.  The counters say
that a file is uploaded once, decoded once, surveyed in one launch and resampled in one.  The staged entry point's refusals are
host-side checks: nothing here reaches a kernel with a bad row.  Files are 2 s of gated noise (autocases.py)."""
import filecmp
import os

import numpy as np
import pytest

import autocases
from inaspeechsegmenter_amd import _native, Segmenter, pipeline
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.export_funcs import seg2csv
from inaspeechsegmenter_amd.resample import Mix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _equalities(seg, f, want_mix='some'):
    """The equalities of a file whose survey asks for a mix -> (pcm, survey, mix, segments)."""
    pcm, survey, mix = seg.load_pcm_auto(f)
    assert survey == seg.survey_channels(f) and survey == iss_io.survey_channels(f)
    assert mix == survey.safe_mix() and isinstance(mix, Mix)
    if want_mix != 'some':
        assert mix == want_mix
    assert pcm.dtype == np.int16
    np.testing.assert_array_equal(pcm, seg.load_pcm_mixes(f, [mix])[0])
    host, hsurvey, hmix = iss_io.decode_auto(f)
    np.testing.assert_array_equal(pcm, host)
    assert hsurvey == survey and hmix == mix
    segments, s2, m2 = seg.segment_auto(f)
    assert s2 == survey and m2 == mix
    assert segments == seg.segment_mixes(f, [mix])[0] == seg.segment_signal(pcm)
    return pcm, survey, mix, segments


# ------------------------------------------------------------------------------------------------ 1, 2: the two stereo files
def test_inverted_stereo_is_saved(seg, tmp_path):
    """R = -L: the default call hears nothing from end to end; 'auto' hears channel 0.  Fails without the feature."""
    f = autocases.write(tmp_path / 'a.wav', 'inverted', 48000)
    pcm, survey, mix, segments = _equalities(seg, f, Mix(((0, 1.0), (1, -1.0)), 2.0))
    np.testing.assert_array_equal(pcm, seg.load_pcm_channels(f, [0])[0])
    assert not np.any(seg.load_pcm(f))
    plain = seg(f)
    assert len(plain) == 1 and plain[0][0] == 'noEnergy', plain
    assert segments != plain and any(lab != 'noEnergy' for lab, _, _ in segments), segments


def test_healthy_stereo_is_read_as_ever(seg, tmp_path):
    f = autocases.write(tmp_path / 'a.wav', 'healthy', 48000)
    pcm, survey, mix = seg.load_pcm_auto(f)
    assert mix is None and survey == seg.survey_channels(f) and survey == iss_io.survey_channels(f)
    np.testing.assert_array_equal(pcm, seg.load_pcm(f))
    np.testing.assert_array_equal(pcm, iss_io.decode_auto(f)[0])
    segments, s2, m2 = seg.segment_auto(f)
    assert m2 is None and s2 == survey and segments == seg(f)


def test_mono_takes_the_default_path(seg, tmp_path):
    launches = seg.ctx.survey_stats()[0]
    for sr in (16000, 8000):
        f = autocases.write(tmp_path / f'm{sr}.wav', 'mono', sr)
        pcm, survey, mix = seg.load_pcm_auto(f)
        assert survey is None and mix is None
        np.testing.assert_array_equal(pcm, seg.load_pcm(f))
        assert seg.segment_auto(f) == (seg(f), None, None)
    for kind, sr in (('flac', 16000), ('flac', 8000), ('ima', 16000), ('ima', 8000), ('ms', 8000)):      # the coders' one-channel files
        f = autocases.write(tmp_path / f'm{sr}.{kind}', 'mono', sr, kind)
        pcm, survey, mix = seg.load_pcm_auto(f)
        assert survey is None and mix is None
        np.testing.assert_array_equal(pcm, seg.load_pcm(f))
        assert seg.segment_auto(f) == (seg(f), None, None)
    assert seg.ctx.survey_stats()[0] == launches


# ------------------------------------------------------------------------------------------------ 3: every source class
CLASSES = [('i16', 44100), ('f32', 48000), ('flac', 16000), ('ima', 8000), ('ms', 8000)]


@pytest.mark.parametrize('kind,sr', CLASSES, ids=[f'{k}-{sr}' for k, sr in CLASSES])
@pytest.mark.parametrize('case', ['deadinv', 'dead4'])
def test_every_source_class(seg, tmp_path, case, kind, sr):
    f = autocases.write(tmp_path / 'a.bin', case, sr, kind)
    want = Mix(((1, 1.0), (2, -1.0)), 2.0) if case == 'deadinv' else Mix(((0, 1.0), (2, 1.0)), 2.0)
    pcm, survey, mix, segments = _equalities(seg, f, want)
    assert not np.array_equal(pcm, seg.load_pcm(f))               # (the plain downmix is another signal)


def test_inverted_left_side_flac(seg, tmp_path):
    """The damaged FLAC of an archive: 16 kHz, left/side coded, the side channel twice the left one."""
    f = autocases.write(tmp_path / 'a.flac', 'inverted', 16000, 'flac')
    from inaspeechsegmenter_amd import flac
    assert set(flac.FlacStream(open(f, 'rb').read(), f).frames['channel_mode']) == {8}
    pcm, survey, mix, segments = _equalities(seg, f, Mix(((0, 1.0), (1, -1.0)), 2.0))
    np.testing.assert_array_equal(pcm, autocases.stored('inverted', 16000)[:, 0])
    assert not np.any(seg.load_pcm(f)) and seg(f) != segments


# ------------------------------------------------------------------------------------------------ 4: geometry
def _three(n, sr, seed):
    """[L, 0, -R] of n frames, noise from the first frame on (the gate opens at 0)."""
    return autocases.stored('deadinv', sr, seed, n)[:, [1, 0, 2]]


@pytest.mark.parametrize('frames', ['C-1', 'C', 'C+1', '2T-1', '2T', '2T+1'])
def test_chunk_and_tile_edges(seg, tmp_path, frames):
    chunk = seg.ctx.survey_geometry()[0]
    tile = seg.ctx.resample_split_geometry(16000, 1)[0]           # one mix row, the identity filter: outputs = frames
    n = eval(frames.replace('2T', '2*T'), {'C': chunk, 'T': tile})
    f = autocases.wavgen.write_wav(tmp_path / 'a.wav', _three(n, 16000, n), 16000, 'i16')
    pcm, survey, mix = seg.load_pcm_auto(f)
    assert survey.n == n == pcm.size and mix == Mix(((0, 1.0), (2, -1.0)), 2.0)
    assert survey == iss_io.survey_channels(f)
    np.testing.assert_array_equal(pcm, seg.load_pcm_mixes(f, [mix])[0])
    np.testing.assert_array_equal(pcm, iss_io.decode_auto(f)[0])


def test_tile_edges_through_a_filter(seg, tmp_path):
    tile = seg.ctx.resample_split_geometry(48000, 1)[0]
    for n in (3 * tile - 3, 3 * tile, 3 * tile + 1):              # tile - 1, tile, tile + 1 outputs
        f = autocases.wavgen.write_wav(tmp_path / f'a{n}.wav', _three(n, 48000, n), 48000, 'i16')
        pcm, survey, mix = seg.load_pcm_auto(f)
        assert pcm.size == R.out_len(n, 48000) and mix is not None
        np.testing.assert_array_equal(pcm, iss_io.decode_auto(f)[0])


def test_seventeen_channels(seg, tmp_path):
    f = autocases.write(tmp_path / 'a.wav', 'wide17', 48000)
    pcm, survey, mix, _ = _equalities(seg, f)
    assert survey.s12 is None and mix == Mix(tuple((c, 1.0) for c in range(17) if c not in (3, 11)), 15.0)


# ------------------------------------------------------------------------------------------------ 5: one of everything
def _counters(ctx):
    return {'upload': ctx.upload_stats(), 'survey': ctx.survey_stats()[0], 'resample': ctx.resample_stats()[0],
            'flac': ctx.flac_stats()[0], 'adpcm': ctx.adpcm_stats()[0], 'msadpcm': ctx.msadpcm_stats()[0]}


def _grown(ctx, before):
    now = _counters(ctx)
    return {k: (now[k][0] - before[k][0], now[k][1] - before[k][1]) if k == 'upload' else now[k] - before[k] for k in now}


@pytest.mark.parametrize('kind,sr,coder', [('i16', 48000, None), ('flac', 16000, 'flac'), ('ima', 8000, 'adpcm'), ('ms', 8000, 'msadpcm')])
def test_one_upload_one_launch_of_each(seg, tmp_path, kind, sr, coder):
    f = autocases.write(tmp_path / 'a.bin', 'deadinv', sr, kind)
    nbytes = iss_io.auto_source(f, True).payload.size
    before = _counters(seg.ctx)
    pcm, survey, mix = seg.load_pcm_auto(f)
    got = _grown(seg.ctx, before)
    want = {'upload': (1, nbytes), 'survey': 1, 'resample': 1, 'flac': 0, 'adpcm': 0, 'msadpcm': 0}
    if coder:
        want[coder] = 1
    assert got == want
    before = _counters(seg.ctx)                                   # the route it replaces: the counter counts
    s2 = seg.survey_channels(f)
    np.testing.assert_array_equal(seg.load_pcm_mixes(f, [s2.safe_mix()])[0], pcm)
    old = _grown(seg.ctx, before)
    pad = -(-nbytes // 16) * 16                                   # (a survey pass stages its payloads on 16-byte boundaries)
    assert old['upload'] == (2, nbytes + pad) and old['survey'] == 1 and old['resample'] == 1      # twice the bytes
    if coder:
        assert old[coder] == 2


# ------------------------------------------------------------------------------------------------ 6: one mixed pass
def test_one_mixed_pass(seg, tmp_path, monkeypatch):
    d = tmp_path
    data, fo = autocases.flacgen.encode(autocases.stored('healthy', 16000).astype(np.int64), 16000, 16, blocksize=1152,
                                        channel_mode='left_side', subframe={'type': 'verbatim'}, return_offsets=True)
    bad = bytearray(data); bad[fo[5] + 300] ^= 0x08              # found by the device (CRC-16)
    (d / 'crc.flac').write_bytes(bytes(bad))
    files = [autocases.write(d / 'healthy.wav', 'healthy', 48000), autocases.write(d / 'inverted.wav', 'inverted', 48000),
             autocases.write(d / 'dead.flac', 'dead4', 16000, 'flac'), autocases.write(d / 'ima.wav', 'deadinv', 8000, 'ima'),
             autocases.write(d / 'mono.wav', 'mono', 16000), str(d / 'crc.flac'),
             autocases.write(d / 'mono.flac', 'mono', 16000, 'flac')]      # one-channel files of the coders, in the coders' one call
    blocks = bytearray(autocases.sndgen.ima_encode(autocases.stored('mono', 8000), 256))
    blocks[5 * 256 + 2] = 89                                      # block 5: step index 89
    files.append(autocases.sndgen.write_riff(d / 'mono_bad_ima.wav', autocases.sndgen.wav_fmt('ima', 8000, 1, 256), bytes(blocks),
                                             fact=16000))
    good = [0, 1, 2, 3, 4, 6]
    outs = [str(d / 'out' / (os.path.basename(f) + '.csv')) for f in files]
    passes = []
    run = pipeline._Worker.run

    def counted(self, batch):
        before = _counters(self.ctx)
        out = run(self, batch)
        passes.append(([type(s).__name__ for s in batch.sigs], _grown(self.ctx, before),
                       {type(s): sum(-(-t.payload.size // 16) * 16 for t in batch.sigs if type(t) is type(s))
                        for s in batch.sigs if isinstance(s, pipeline.sources.Source)}))
        return out
    monkeypatch.setattr(pipeline._Worker, 'run', counted)
    decisions = []
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='auto', decisions=decisions)
    assert [m[1] for m in lmsg] == [0, 0, 0, 0, 0, 2, 0, 2] and nb == 6, lmsg
    assert [m[0] for m in lmsg] == outs
    assert 'crc.flac: frame at byte' in lmsg[5][2], lmsg[5]       # each malformed file under its own name and offset, though a
    assert 'mono_bad_ima.wav: block at byte' in lmsg[7][2] and 'step index' in lmsg[7][2], lmsg[7]      # clean file shares its call
    assert len(passes) == 1, passes                               # all eight files in one pass ...
    names, grown, staged = passes[0]
    assert sorted(names) == ['AdpcmAuto', 'AdpcmAuto', 'FlacAuto', 'FlacAuto', 'FlacAuto', 'RawAuto', 'RawAuto', 'ndarray']
    assert grown == {'upload': (3, sum(staged.values())), 'survey': 3, 'resample': 3, 'flac': 1, 'adpcm': 1, 'msadpcm': 0}      # ... one launch per class
    assert sorted(d[0] for d in decisions) == sorted(files[k] for k in good)
    by = {d[0]: d for d in decisions}
    for f, o in ((files[k], outs[k]) for k in good):
        segments, survey, mix = seg.segment_auto(f)
        seg2csv(segments, str(d / 'alone.csv'))
        assert filecmp.cmp(o, str(d / 'alone.csv'), shallow=False), f
        assert by[f][2] == mix and (by[f][1] == survey if survey is not None else by[f][1] is None)
    assert [by[files[k]][2] is None for k in good] == [True, False, False, False, True, True]
    assert by[files[6]][1] is None                                # (a one-channel file of a coder: no survey, no decision)
    plain = [o + '.plain.csv' for o in outs]
    monkeypatch.setattr(pipeline._Worker, 'run', run)
    _, _, _, lmsg0 = seg.batch_process(files, plain)
    assert [m[1] for m in lmsg0] == [0, 0, 0, 0, 0, 2, 0, 2]
    for k in (0, 4, 6):                                           # the healthy and the mono files: the default call's bytes
        assert filecmp.cmp(outs[k], plain[k], shallow=False), files[k]
    assert not filecmp.cmp(outs[1], plain[1], shallow=False)      # the inverted file is not


# ------------------------------------------------------------------------------------------------ 7: the staged entry point's guards
def _refused(ctx, code, *words):
    def check(call):
        before = ctx.get_signal_pcm16(0, 4000)
        counters = _counters(ctx)
        with pytest.raises(_native.NativeError) as exc:
            call()
        text = str(exc.value)
        assert f'({code})' in text and all(w in text for w in words), text
        np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 4000), before)
        assert _counters(ctx) == counters                         # nothing uploaded, nothing launched
    return check


def test_staged_guards_raw():
    ctx = _native.Context(0)
    try:
        resident = (np.arange(4000) % 251 - 125).astype(np.int16)
        ctx.set_signal(resident)
        fid = ctx.resample_filter(48000)[0]
        x, y = autocases.stored('deadinv', 48000, n=3000), autocases.stored('healthy', 48000, n=3300)
        row = lambda a, frames=None: (0, a.shape[0] if frames is None else frames, a.shape[1], 1, fid, 0, 100, 1000)      # noqa: E731
        estate, einval = _refused(ctx, -4, 'iss_resample_staged_mix', 'survey'), _refused(ctx, -1, 'iss_resample_staged_mix')
        _refused(ctx, -4, 'iss_staged_payload', 'survey')(lambda: ctx.staged_payload(None))
        estate(lambda: ctx.resample_staged(None, 1, [row(x)]))                      # before any survey
        ctx.survey(x.reshape(-1).view(np.uint8), [(0, 3000, 3, 1, 32767 / 32768)])
        first = ctx.staged_payload(None)
        ctx.survey(y.reshape(-1).view(np.uint8), [(0, 3300, 2, 1, 32767 / 32768)])  # an intervening upload of that origin
        estate(lambda: ctx.resample_staged(None, first, [row(x)]))
        second = ctx.staged_payload(None)
        assert second > first
        einval(lambda: ctx.resample_staged(None, second, [row(y, 3301)]))           # more frames than were uploaded
        einval(lambda: ctx.resample_staged(None, second, [row(x)]))                 # another file's channels
        einval(lambda: ctx.resample_staged(None, second, [(0, 3300, 2, 1, fid, 0, 100, 1100)],      # what the _mix contract refuses
                                           mixes=[(1100, [Mix(((2, 1.0),), 1.0)])]))
        mix = Mix(((0, 1.0), (1, -1.0)), 2.0)
        ctx.resample_staged(None, second, [(0, 3300, 2, 1, fid, 0, 100, 1100)], mixes=[(1100, [mix])])      # and the call it accepts
        got = ctx.get_signal_pcm16(0, 4000)
        np.testing.assert_array_equal(got[100:1200], R.mix_ref(y, 48000, mix))
        np.testing.assert_array_equal(got[:100], resident[:100])
        np.testing.assert_array_equal(got[1200:], resident[1200:])
        ctx.scribble(0x7FC00000)                                                    # the bytes are gone, and so is the payload
        estate(lambda: ctx.resample_staged(None, second, [(0, 3300, 2, 1, fid, 0, 100, 1100)], mixes=[(1100, [mix])]))
    finally:
        ctx.close()


def test_staged_guards_flac(tmp_path):
    from inaspeechsegmenter_amd import flac
    ctx = _native.Context(0)
    try:
        resident = (np.arange(4000) % 251 - 125).astype(np.int16)
        ctx.set_signal(resident)
        fid = ctx.resample_filter(16000)[0]
        s = flac.FlacStream(open(autocases.write(tmp_path / 'a.flac', 'deadinv', 16000, 'flac', n=3000), 'rb').read(), 'a.flac')
        src = flac.FlacAuto(s)
        estate, einval = _refused(ctx, -4, 'iss_resample_staged_mix', 'flac'), _refused(ctx, -1, 'iss_resample_staged_mix')
        estate(lambda: ctx.resample_staged('flac', 1, [(0, 3000, 3, 1, fid, 0, 0, 3000)]))          # before any decode
        decode = lambda: ctx.flac_decode(s.audio, s.frames, [src.row(ctx, 0, 0, 0)])              # noqa: E731
        status = decode()
        first = ctx.staged_payload('flac')
        ctx.synchronize()
        assert not np.any(status)
        decode()                                                                                  # a later decode call of the codec
        estate(lambda: ctx.resample_staged('flac', first, [(0, 3000, 3, 1, fid, 0, 0, 3000)]))
        second = ctx.staged_payload('flac')
        einval(lambda: ctx.resample_staged('flac', second, [(0, 3001, 3, 1, fid, 0, 0, 3001)]))     # more frames than were staged
        einval(lambda: ctx.resample_staged('flac', second, [(1, 3000, 3, 1, fid, 0, 0, 3000)]))     # no such staged job
        einval(lambda: ctx.resample_staged('flac', second, [(0, 1500, 3, 2, fid, 0, 0, 1500)]))     # the same bytes, another format
        mix = Mix(((1, 1.0), (2, -1.0)), 2.0)
        ctx.resample_staged('flac', second, [(0, 3000, 3, 1, fid, 0, 500, 3000)], mixes=[(3000, [mix])])
        got = ctx.get_signal_pcm16(0, 4000)
        np.testing.assert_array_equal(got[500:3500], R.mix_ref(s.stored(), 16000, mix))
        np.testing.assert_array_equal(got[:500], resident[:500])
    finally:
        ctx.close()
