"""GPU: voice femininity per channel and per time range, scored where the decode pass left the parts.  The batch front end on
parts of the resident signal (iss_vbx_features_resident) against the single-file entry, bit for bit, with its refusals;
iss_vbx_features_batch_pcm16 unchanged; score_channels / score_excerpts / score_channel_excerpts against their definition
(score_signal on the samples load_pcm_* returns), tuple for tuple and x-vector for x-vector; passes, errors, the split TSV of
batch_process and the command line."""
import importlib.util
import os
import warnings

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from conftest import GOLDEN, ROOT, read_wav_int16
from test_excerpts import sec
from test_gpu_vfs_batch import BATCH_LENGTHS
from inaspeechsegmenter_amd import _native, sndfmt, vbx as V, vfs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ front end
PARTS = [200, 201, 359, 360, 361, 400, 16037, 48000]      # one frame; either side of a hop; 16037: no multiple of anything; last: ends on the grid


def _hop(n):
    return -(-n // 160) * 160


@pytest.fixture(scope='module')
def laid_out():
    """The parts as a pass lays them out: each start on a multiple of 160, the gap behind each filled with +-32767; the last
    part (a multiple of 160 long) ends at the last sample of the buffer.  -> (signal, begins, the parts' samples)"""
    rng = np.random.default_rng(31)
    pcms = [np.clip(np.round(rng.normal(0, 0.1, n) * 32768), -32768, 32767).astype(np.int16) for n in PARTS]
    begins = np.concatenate(([0], np.cumsum([_hop(n) for n in PARTS])))[:-1]
    sig = np.where(np.arange(begins[-1] + PARTS[-1]) % 2, 32767, -32767).astype(np.int16)
    for b, p in zip(begins, pcms):
        sig[b:b + p.size] = p
    assert sig.size == begins[-1] + PARTS[-1]
    return sig, [int(b) for b in begins], pcms


@pytest.fixture(scope='module')
def singles(ctx, laid_out):
    """vbx_features_pcm16 on each part alone: computed once, shared, left unchanged."""
    V.FeatureExtractor(ctx)._ensure_dither(max(PARTS))
    return [ctx.vbx_features_pcm16(p) for p in laid_out[2]]


def _check(ctx, begins, singles, order):
    foff, arena = ctx.vbx_features_resident([begins[p] for p in order], [PARTS[p] for p in order], to_host=True)
    assert foff[0] == 0 and list(np.diff(foff)) == [V.frame_count(PARTS[p]) for p in order]
    assert arena.shape == (foff[-1], 64)
    for k, p in enumerate(order):
        got = arena[foff[k]:foff[k + 1]]
        assert np.array_equal(got, singles[p]), (p, PARTS[p], np.abs(got - singles[p]).max())


def test_resident_front_end_equals_single_file_entry(ctx, laid_out, singles):
    sig, begins, _ = laid_out
    V.FeatureExtractor(ctx)._ensure_dither(max(PARTS))
    order = list(range(len(PARTS)))
    ctx.set_signal(sig)                                           # the last part ends at the signal's last sample
    before = ctx.vbx_resident_stats()
    _check(ctx, begins, singles, order)
    assert tuple(b - a for a, b in zip(before, ctx.vbx_resident_stats())) == (1, len(PARTS))
    _check(ctx, begins, singles, order[::-1])                     # descending offsets
    foff, none = ctx.vbx_features_resident(begins, PARTS)         # resident: what iss_vbx_embed gathers from
    assert none is None and foff[-1] == sum(V.frame_count(n) for n in PARTS)
    # ... and with a tail of +-32767 behind the last part
    ctx.set_signal(np.concatenate([sig, np.where(np.arange(160) % 2, 32767, -32767).astype(np.int16)]))
    _check(ctx, begins, singles, order)
    _check(ctx, begins, singles, order[::-1])


def test_resident_front_end_refusals(ctx, laid_out, singles):
    sig, begins, _ = laid_out
    fe = V.FeatureExtractor(ctx)
    fe._ensure_dither(max(PARTS))
    order = list(range(len(PARTS)))
    ctx.set_signal(sig)
    _check(ctx, begins, singles, order)

    def refused(match, b, n):
        before = ctx.vbx_resident_stats()
        with pytest.raises(_native.NativeError, match=match):
            ctx.vbx_features_resident(b, n)
        assert ctx.vbx_resident_stats() == before                 # nothing launched
        _check(ctx, begins, singles, order)                       # ... and nothing changed

    refused('part 1 has 199 samples', [0, 160], [200, 199])
    refused('part 1 .* is outside the signal', [0, sig.size - 300], [200, 301])
    refused('parts 1 and 0 overlap', [begins[6] + 200, begins[6]], [400, 201])     # by one sample
    refused('parts . and . overlap', [0, 0], [200, 200])
    refused('bad argument', [], [])
    ctx.set_signal(np.zeros(sig.size, np.float32))
    with pytest.raises(_native.NativeError, match='no resident PCM16 signal'):
        ctx.vbx_features_resident(begins, PARTS)
    ctx.set_signal(sig)
    _check(ctx, begins, singles, order)
    ctx.vbx_set_dither(V.dither_stream(PARTS[-1] - 1))            # one value short of the longest part
    with pytest.raises(_native.NativeError, match='dither stream holds 47999 values, the longest part needs 48000'):
        ctx.vbx_features_resident(begins, PARTS)
    _check(ctx, begins[:-1], singles, order[:-1])                 # (the stream is a prefix of the longer one: the same bits)
    ctx.vbx_set_dither(V.dither_stream(max(max(PARTS), max(BATCH_LENGTHS))))
    _check(ctx, begins, singles, order)


def test_batch_front_end_still_gives_its_bits(ctx):
    """iss_vbx_features_batch_pcm16 on the inputs of test_batch_front_end_equals_single_file_entry: the same frames as the
    single-file entry, file by file, and three launches per call (one fbank, the cumsum and the CMN) as before."""
    rng = np.random.default_rng(9)
    pcms = [np.clip(np.round(rng.normal(0, 0.1, n) * 32768), -32768, 32767).astype(np.int16) for n in BATCH_LENGTHS]
    V.FeatureExtractor(ctx)._ensure_dither(max(BATCH_LENGTHS))
    want = [ctx.vbx_features_pcm16(p) for p in pcms]
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        before = ctx.vbx_resident_stats()
        foff, arena = ctx.vbx_features_batch_pcm16(pcms)
        launches = ctx.prof_get(1)[1], ctx.prof_get(2)[1]
    finally:
        ctx.prof_enable(False)
    assert launches == (1, 1)                                     # two brackets: the fbank launch; cumsum + CMN
    assert ctx.vbx_resident_stats() == before
    assert list(np.diff(foff)) == [V.frame_count(n) for n in BATCH_LENGTHS]
    for f, one in enumerate(want):
        assert np.array_equal(arena[foff[f]:foff[f + 1]], one), f


# ------------------------------------------------------------------------------------------------ files
SECONDS = 13


@pytest.fixture(scope='module')
def scorer():
    v = vfs.VoiceFemininityScoring(ffmpeg=None, models='synthetic', resample=True)
    yield v
    v.vad.close()


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """name -> path: 13 s, ch0 from lamartine.wav, ch1 from musanmix.wav; the 8 kHz file takes every second sample."""
    d = tmp_path_factory.mktemp('vfs_parts')
    n = 16000 * SECONDS
    lam = np.clip(np.round(read_wav_int16(os.path.join(GOLDEN, 'lamartine.wav')).astype(np.float64) * 32768), -32768, 32767)
    mus = read_wav_int16(os.path.join(GOLDEN, 'musanmix.wav'))
    x = np.stack([lam[:n], mus[:n]], axis=1).astype('<i2')
    out = {'wav': wavgen.write_wav(d / 'two.wav', x, 16000, 'i16')}
    out['ima'] = sndgen.write(d / 'two_ima.wav', 'wav', 'ima', False, x[::2] / 32768.0, 8000, block_align=512)[0]
    out['flac'] = flacgen.write(d / 'two.flac', x.astype(np.int64), 16000, 16, blocksize=4096, subframe={'type': 'fixed', 'order': 2})
    quiet = x.copy()
    quiet[:, 1] = 0
    out['silent'] = wavgen.write_wav(d / 'silent_ch1.wav', quiet, 16000, 'i16')
    return {k: str(p) for k, p in out.items()}


# inside a hop at both ends; overlapping the first; the first again; open-ended; under 68 frames of the VAD (11 000 samples)
N16 = 16000 * SECONDS
RANGES = [(sec(1234), sec(100037)), (sec(50011), sec(150003)), (sec(1234), sec(100037)), (sec(120003), None),
          (sec(80001), sec(91001))]


def _fixed_speech(vad_tuples):
    """Stands in for vfs.speech_intervals: a fixed function of the part's duration (the end of its last segment) -- two
    stretches of speech with a gap -- and nothing for a part the energy detector found silent throughout."""
    if all(lab == 'noEnergy' for lab, _, _ in vad_tuples):
        return []
    d = max(e for _, _, e in vad_tuples)
    return [(round(0.02 * d, 2), round(0.5 * d, 2)), (round(0.52 * d, 2), round(0.98 * d, 2))]


def _recording(v, monkeypatch):
    """Every x-vector matrix that reaches the gender MLP goes to the list in sink[0] (as tests/test_gpu_vfs_batch.py)."""
    sink = [[]]
    orig = v.gender_predict

    def rec(x):
        sink[0].append(np.array(x, copy=True))
        return orig(x)
    monkeypatch.setattr(v, 'gender_predict', rec)
    return sink


def _same_matrices(got, want):
    """The same matrices, whatever the order the parts were scored in (parts that go alone are scored first)."""
    key = lambda m: (m.shape, m.tobytes())                                      # noqa: E731
    got, want = sorted(got, key=key), sorted(want, key=key)
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize('vad', ['standin', 'fixed'])
@pytest.mark.parametrize('name', ['wav', 'ima', 'flac', 'silent'])
def test_scores_equal_their_definition(scorer, files, name, vad, monkeypatch):
    """The three calls against score_signal on what load_pcm_* returns.  'standin': the seeded stand-in VAD decides.  It finds
    speech in channel 0 (lamartine.wav: 33 x-vectors, 8 to 18 per range) and none in channel 1 (musanmix.wav) nor in the
    downmix of the two, so the downmixed excerpts of the two-signal files never reach the front end in this variant and prove
    nothing beyond the VAD bookkeeping there.  'fixed':vfs.speech_intervals, which both routes call through the module, is replaced by a fixed function
    of the part's duration, so every non-silent part reaches the ResNet."""
    v, path = scorer, files[name]
    if vad == 'fixed':
        monkeypatch.setattr(vfs, 'speech_intervals', _fixed_speech)
    sink = _recording(v, monkeypatch)
    sel = [1, 0, 1]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                           # (the short range: 'duration is short')
        # channels
        want = [v.score_signal(x) for x in v.vad.load_pcm_channels(path)]
        want_x, sink[0] = sink[0], []
        got = v.score_channels(path)
        got_x, sink[0] = sink[0], []
        print(name, vad, 'channels', got)
        assert got == want and _same_matrices(got_x, want_x)
        assert v.score_channels(path, sel) == [want[c] for c in sel]
        sink[0] = []
        if name == 'silent':
            assert got[1] == (None, 0, 0)
        if vad == 'fixed':
            assert all(r[2] > 0 for c, r in enumerate(got) if not (name == 'silent' and c == 1))
        # excerpts (of the downmix)
        want = [v.score_signal(v.vad.load_pcm_excerpts(path, [r])[0]) for r in RANGES]
        want_x, sink[0] = sink[0], []
        got = v.score_excerpts(path, RANGES)
        got_x, sink[0] = sink[0], []
        print(name, vad, 'excerpts', got)
        assert got == want and _same_matrices(got_x, want_x)
        if vad == 'fixed':
            assert all(r[2] > 0 for r in got)
        # excerpts of channels
        want = [[v.score_signal(v.vad.load_pcm_channel_excerpts(path, [r], [c])[0][0]) for c in sel] for r in RANGES]
        want_x, sink[0] = sink[0], []
        got = v.score_channel_excerpts(path, RANGES, sel)
        got_x, sink[0] = sink[0], []
        print(name, vad, 'channel excerpts', got)
        assert got == want and _same_matrices(got_x, want_x)
        for row in got:
            assert row[0] == row[2]
            if name == 'silent':
                assert row[0] == (None, 0, 0)
            if vad == 'fixed':
                assert all(r[2] > 0 for c, r in zip(sel, row) if not (name == 'silent' and c == 1))


def test_nothing_leaves_the_device(scorer, files, monkeypatch):
    v = scorer
    monkeypatch.setattr(vfs, 'speech_intervals', _fixed_speech)
    want = v.score_channels(files['ima'])

    def refuse(*a, **kw):
        raise AssertionError('PCM came back to the host, or was uploaded again')
    for fn in ('get_signal_pcm16', 'vbx_features_batch_pcm16', 'vbx_features_pcm16', 'vbx_features'):
        monkeypatch.setattr(v.ctx, fn, refuse)
    before = v.ctx.adpcm_stats()[0], v.ctx.resample_stats()[0], v.ctx.vbx_resident_stats()
    got = v.score_channels(files['ima'])
    after = v.ctx.adpcm_stats()[0], v.ctx.resample_stats()[0], v.ctx.vbx_resident_stats()
    assert got == want and all(r[2] > 0 for r in got)
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)
    assert (after[2][0] - before[2][0], after[2][1] - before[2][1]) == (1, 2)    # one front-end call, both channels


def test_passes_give_the_same_results(scorer, files, monkeypatch):
    v = scorer
    monkeypatch.setattr(vfs, 'speech_intervals', _fixed_speech)
    for name in ('wav', 'ima', 'flac'):
        before = v.ctx.vbx_resident_stats()[0]
        one = v.score_channels(files[name])
        mid = v.ctx.vbx_resident_stats()[0]
        assert v.score_channels(files[name], batch_files=1) == one
        assert (mid - before, v.ctx.vbx_resident_stats()[0] - mid) == (1, 2)    # one pass; a pass per channel
    assert v.score_excerpts(files['flac'], RANGES[:2], batch_files=1) == v.score_excerpts(files['flac'], RANGES[:2])
    assert (v.score_channel_excerpts(files['ima'], RANGES[:2], batch_files=1) ==
            v.score_channel_excerpts(files['ima'], RANGES[:2]))


def test_bad_ima_block_inside_and_outside(scorer, tmp_path):
    v = scorer
    spb = sndgen.ima_samples_per_block(512, 2)
    clean = sndgen.write(tmp_path / 'clean.wav', 'wav', 'ima', False, wavgen.make_signal(spb * 60, 2, 54), 16000, block_align=512)[0]
    base = sndfmt.parse(open(clean, 'rb').read(), clean).base
    bad = bytearray(open(clean, 'rb').read())
    bad[base + 50 * 512 + 2] = 89                                                 # block 50: step index above 88
    path = tmp_path / 'bad.wav'
    path.write_bytes(bytes(bad))
    inside = (sec(spb * 20 + 10), sec(spb * 50 + 450))
    outside = [(sec(spb * 4 + 10), sec(spb * 50)), (sec(spb * 51), None)]
    assert spb * 30 > 11120 and spb * 9 < 11120                                   # a pass part, and one that goes alone
    match = r'bad\.wav: block at byte %d: step index above 88' % (base + 50 * 512)
    with pytest.raises(ValueError, match=match):
        v.score_excerpts(str(path), [outside[0], inside])
    with pytest.raises(ValueError, match=match):
        v.score_channel_excerpts(str(path), [inside], [1])
    with pytest.raises(ValueError, match=match):
        v.score_channels(str(path))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert v.score_excerpts(str(path), outside) == v.score_excerpts(clean, outside)
        assert v.score_channel_excerpts(str(path), outside) == v.score_channel_excerpts(clean, outside)


def test_batch_process_split_and_command_line(scorer, files, tmp_path, monkeypatch, capsys):
    v = scorer
    monkeypatch.setattr(vfs, 'speech_intervals', _fixed_speech)
    paths = [files['flac'], str(tmp_path / 'missing.wav'), files['silent']]
    want = [v.score_channels(paths[0]), None, v.score_channels(paths[2])]
    got = v.batch_process(paths, output_csv=str(tmp_path / 'out.tsv'), channels='split')
    assert got[0] == want[0] and got[2] == want[2]
    assert isinstance(got[1], str) and 'FileNotFoundError' in got[1]
    rows = open(tmp_path / 'out.tsv').read().splitlines()
    assert rows[0] == 'path\tchannel\tscore\tspeech_duration\tnb_vectors' and len(rows) == 6
    assert rows[1:3] == ['\t'.join([paths[0], str(k)] + [str(x) for x in want[0][k]]) for k in range(2)]
    assert rows[3] == '\t'.join([paths[1], '', got[1]])
    assert rows[4:6] == ['\t'.join([paths[2], str(k)] + [str(x) for x in want[2][k]]) for k in range(2)]
    assert rows[5] == paths[2] + '\t1\tNone\t0\t0'
    # the command line: --channels split passes through (on this module's scorer: the script builds its own from the arguments)
    spec = importlib.util.spec_from_file_location('ina_voice_femininity_amd', os.path.join(ROOT, 'scripts', 'ina_voice_femininity_amd.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    made = []
    monkeypatch.setattr(vfs, 'VoiceFemininityScoring', lambda **kw: (made.append(kw), v)[1])
    assert cli.main(['-i'] + paths + ['-o', str(tmp_path / 'cli.tsv'), '-b', 'None', '--resample', '--models', 'synthetic',
                                      '--channels', 'split']) == 0
    assert made[0]['ffmpeg'] is None and made[0]['resample'] is True
    assert open(tmp_path / 'cli.tsv').read().splitlines() == rows
    with pytest.raises(SystemExit):
        cli.main(['-i', paths[0], '-o', str(tmp_path / 'x.tsv'), '--channels', 'split'])
    assert '--channels split needs -b None' in capsys.readouterr().err
