"""CPU: file sets on the host.  io.decode_set is the set's interleaved twin -- the samples io.decode_source reads from the twin
file setgen.py writes --, every host-only call on a set equals the same call on the twin, every refusal names the set, the
member and the reason, and --sets parses its list."""
import os

import numpy as np
import pytest

import autocases
import flacgen
import setgen
import sndgen
import wavgen
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd import sources


def _script():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts', 'ina_speech_segmenter_amd.py')
    spec = importlib.util.spec_from_file_location('ina_speech_segmenter_amd_cli', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize('kind,containers,big', [('i16', ['wav', 'w64'], False), ('i24', ['aiff', 'caf'], True),
                                                 ('u8', ['wav', 'aifc'], False), ('ulaw', ['wav', 'au'], False),
                                                 ('f32', ['caf', 'au'], True)])
def test_decode_set_is_the_twin(tmp_path, kind, containers, big):
    xs = setgen.signals([700, 1000 if kind != 'ulaw' else 700], [2, 1], 3)
    members, twin = setgen.write_set(tmp_path, 's', xs, 22050, kind, containers, big)
    x, sr = iss_io.decode_set(members)
    want, wsr = iss_io.decode_source(twin)
    assert sr == wsr == 22050 and x.dtype == want.dtype and x.shape == want.shape == (max(len(a) for a in xs), 3)
    np.testing.assert_array_equal(x, want)
    np.testing.assert_array_equal(iss_io.decode_source(tuple(members))[0], want)      # a tuple or list means FileSet
    np.testing.assert_array_equal(iss_io.decode_source(iss_io.FileSet(members, name='n'))[0], want)


def test_padding_is_the_stored_zero(tmp_path):
    members, _ = setgen.mono_set(tmp_path, 'z', [10, 4], 8000, 4, kind='u8')
    x, _ = iss_io.decode_set(members)
    assert x.dtype == np.uint8 and list(x[4:, 1]) == [128] * 6     # unsigned bytes: 128 is 0.0
    members, _ = setgen.mono_set(tmp_path, 'y', [10, 4], 8000, 4, kind='f64')
    assert not np.any(iss_io.decode_set(members)[0][4:, 1])


def test_one_member_set_is_the_file(tmp_path):
    f = sndgen.write(tmp_path / 'a.wav', 'wav', 'i16', False, wavgen.make_signal(500, 2, 5), 16000)[0]
    assert iss_io.as_media((f,)) == f and iss_io.as_media(iss_io.FileSet([f])) == f
    np.testing.assert_array_equal(iss_io.decode_set([f])[0], iss_io.decode_source(f)[0])
    sel, src = iss_io.split_source([f], None)
    assert type(src) is sources.RawSource and sel == [0, 1]
    m = sndgen.write(tmp_path / 'm.wav', 'wav', 'i16', False, wavgen.make_signal(500, 1, 5), 16000)[0]
    np.testing.assert_array_equal(iss_io.set_source([m]), iss_io.decode_pcm(m, ffmpeg=None))


def test_names():
    assert iss_io.FileSet(['a.wav', 'b.wav', 'c.wav']).name == 'set(a.wav, +2)' == str(iss_io.FileSet(('a.wav', 'b.wav', 'c.wav')))
    assert iss_io.FileSet(['a.wav', 'b.wav'], name='call 7').name == 'call 7'
    assert iss_io.FileSet(['a.wav', 'b.wav']) == iss_io.FileSet(('a.wav', 'b.wav')) and len(iss_io.FileSet(['a', 'b'])) == 2
    with pytest.raises(ValueError, match='sequence of paths'):
        iss_io.FileSet('a.wav')


# ------------------------------------------------------------------------------------------------ host-only calls
def test_host_calls_equal_the_twin(tmp_path):
    x = autocases.stored('deadinv', 8000, n=6000)
    members = [wavgen.write_wav(str(tmp_path / f'{c}.wav'), np.ascontiguousarray(x[:5000 + 500 * c, c]), 8000, 'i16') for c in range(3)]
    x[5000:, 0], x[5500:, 1] = 0, 0
    twin = wavgen.write_wav(str(tmp_path / 'twin.wav'), x, 8000, 'i16')
    mixes = R.parse_mixes('0,1+2,0.5*2+1')
    for got, want in zip(iss_io.decode_mixes(members, mixes), iss_io.decode_mixes(twin, mixes)):
        np.testing.assert_array_equal(got, want)
    for got, want in zip(iss_io.decode_channels(members, [2, 0]), iss_io.decode_channels(twin, [2, 0])):
        np.testing.assert_array_equal(got, want)
    assert iss_io.survey_channels(members) == iss_io.survey_channels(twin)
    pcm, survey, mix = iss_io.decode_auto(members)
    tpcm, tsurvey, tmix = iss_io.decode_auto(twin)
    np.testing.assert_array_equal(pcm, tpcm)
    assert survey == tsurvey and mix == tmix == R.Mix(((1, 1.0), (2, -1.0)), 2.0)


def test_sources_hold_the_members_as_stored(tmp_path):
    """Nothing is interleaved on the host: the payload is the members' bytes end to end, each on a 16-byte boundary."""
    xs = setgen.signals([301, 200, 7], [1, 2, 1], 6)
    members, _ = setgen.write_set(tmp_path, 'p', xs, 48000)
    sel, src = iss_io.split_source(members, [3, 0], True)
    assert type(src) is sources.SetSource and sel == [3, 0] and src.sel == [3, 0] and src.parts == 2
    assert (src.frames, src.nch, src.size) == (301, 4, R.out_len(301, 48000))
    assert src.members == [(0, 301, 1), (608, 200, 2), (608 + 800, 7, 1)]
    stored = [iss_io.decode_source(m)[0] for m in members]
    assert src.payload.size == src.payload_size == 608 + 800 + 14
    for (off, _, _), a in zip(src.members, stored):
        np.testing.assert_array_equal(src.payload[off:off + a.nbytes], a.reshape(-1).view(np.uint8))
    assert type(iss_io.set_source(members, True)) is sources.SetSource
    mixes, msrc = iss_io.mix_source(members, [[0, 3]], True)
    assert type(msrc) is sources.SetSource and msrc.sel == mixes == [R.Mix(((0, 1.0), (3, 1.0)), 2.0)]
    auto = iss_io.auto_source(members, True)
    assert type(auto) is sources.SetAuto and auto.parts == 1 and auto.two_step
    sr, ((sv, first),) = iss_io.survey_sources(members)
    assert type(sv) is sources.SetSurvey and (sr, first) == (48000, 0) and sv.full == R.SURVEY_FULL['i16']
    assert len({sources.SetSource, sources.SetSurvey, sources.SetAuto, sources.RawSource}) == 4      # classes of their own


# ------------------------------------------------------------------------------------------------ refusals
def _wav(tmp_path, name, n=400, ch=1, sr=8000, kind='i16', container='wav', big=False):
    return sndgen.write(tmp_path / name, container, kind, big, wavgen.make_signal(n, ch, 7), sr)[0]


def test_refusals(tmp_path):
    a, b = _wav(tmp_path, 'a.wav'), _wav(tmp_path, 'b.wav', n=300)
    other_rate = _wav(tmp_path, 'r.wav', sr=16000)
    other_fmt = _wav(tmp_path, 'f.wav', kind='i32')
    swapped = _wav(tmp_path, 's.aiff', container='aiff', big=True)
    i24 = _wav(tmp_path, 't.wav', kind='i24')
    flac = flacgen.write(str(tmp_path / 'c.flac'), wavgen.encode(wavgen.make_signal(4096, 1, 8), 'i16').astype(np.int64), 8000, 16)
    ima = _wav(tmp_path, 'i.wav', kind='ima', n=2000)
    empty = wavgen.write_wav(str(tmp_path / 'e.wav'), np.zeros(0, dtype='<i2'), 8000, 'i16')
    named = iss_io.FileSet([a, other_rate], name='call 9')
    for members, match in (
            ([a, other_rate], rf'^set\({a}, \+1\): the members differ in sample rate: {a} is sampled at 8000 Hz, {other_rate} at 16000 Hz'),
            (named, r'^call 9: the members differ in sample rate'),
            ([a, b, other_fmt], rf'the members differ in stored sample format: {a} holds i16 samples, {other_fmt} holds i32'),
            ([a, swapped], rf'stored sample format: {a} holds i16 samples, {swapped} holds big-endian i16'),
            ([other_fmt, i24], rf'stored sample format: {other_fmt} holds i32 samples, {i24} holds i24'),
            ([a, flac], rf'member {flac}: FLAC is not supported in a file set'),
            ([ima, a], rf'member {ima}: IMA ADPCM is not supported in a file set'),
            ([a, empty], rf'member {empty} has no frames'),
            ([], r'^set\(\): the set is empty')):
        for call in (iss_io.decode_set, lambda m: iss_io.set_source(m, True), lambda m: iss_io.split_source(m, None, True),
                     lambda m: iss_io.mix_source(m, [0], True), lambda m: iss_io.auto_source(m, True), iss_io.survey_sources,
                     iss_io.survey_channels, iss_io.decode_auto):
            with pytest.raises(ValueError, match=match):
                call(members)
    with pytest.raises(ValueError, match=r'http://host/x.wav: .*http servers'):      # (a member on a server: as a file on one)
        iss_io.decode_set([a, 'http://host/x.wav'])
    with pytest.raises(NotImplementedError, match=r'medianame=http://host/x.wav'):
        iss_io.auto_source([a, 'http://host/x.wav'], True)
    wide = [_wav(tmp_path, f'w{k}.wav', n=2, ch=205) for k in range(5)]
    with pytest.raises(ValueError, match=r'1026 channels in all, a set holds at most 1024'):
        iss_io.decode_set(wide + [a])
    assert iss_io.decode_set(wide[:4] + [_wav(tmp_path, 'w.wav', n=2, ch=204)])[0].shape == (2, 1024)


def test_rate_and_selection_refusals(tmp_path):
    a, b = _wav(tmp_path, 'a.wav'), _wav(tmp_path, 'b.wav', n=300)
    with pytest.raises(AssertionError, match='sampled at 8000 Hz'):
        iss_io.set_source([a, b], resample=False)
    c, d = _wav(tmp_path, 'c.wav', sr=16000), _wav(tmp_path, 'd.wav', sr=16000)
    with pytest.raises(ValueError, match='2 channels; without ffmpeg only mono files are supported'):
        iss_io.set_source([c, d], resample=False)
    assert type(iss_io.split_source([c, d], None, False)[1]) is sources.SetSource      # (the channel count is not refused here)
    with pytest.raises(ValueError, match=r"channel 2 is outside the file's 2 channels"):
        iss_io.split_source([a, b], [2], True)
    with pytest.raises(ValueError, match=r'channel 5 is outside'):
        iss_io.mix_source([a, b], [[0, 5]], True)
    for call in (lambda: iss_io.excerpts([a, b], [(0, 1)]), lambda: iss_io.channel_excerpts([a, b], [(0, 1)]),
                 lambda: iss_io.mix_excerpts([a, b], [(0, 1)], [0]), lambda: iss_io.survey_sources([a, b], [(0, 1)]),
                 lambda: iss_io.survey_channels([a, b], [(0, 1)])):
        with pytest.raises(ValueError, match=r'^set\(.*\): (time )?ranges of a set are not supported'):
            call()
    with pytest.raises(ValueError, match='file sets are read without ffmpeg'):
        iss_io.decode_pcm([a, b], ffmpeg='ffmpeg')


# ------------------------------------------------------------------------------------------------ --sets
def test_sets_list_parsing(tmp_path):
    cli = _script()
    lst = tmp_path / 'sets.tsv'
    lst.write_text('call7\t/a/7-in.wav\t/a/7-out.wav\n\n# a comment\nprog\tp.A1.wav\tp.A2.wav\tp.A3.wav \r\n')
    sets = cli.read_sets(str(lst))
    assert sets == [iss_io.FileSet(['/a/7-in.wav', '/a/7-out.wav'], name='call7'), iss_io.FileSet(['p.A1.wav', 'p.A2.wav', 'p.A3.wav'], name='prog')]
    assert [s.name for s in sets] == ['call7', 'prog']
    assert cli.output_stem(sets[0]) == 'call7' and cli.output_stem('/x/y/file.one.wav') == 'file.one'
    for text, match in (('lonely\n', 'line 1: .*name<TAB>member'), ('\ta.wav\n', 'line 1: .*empty name'),
                        ('a\tx.wav\na\ty.wav\n', "line 2: .*'a' .*twice"), ('d/e\tx.wav\n', 'line 1: .*separator')):
        lst.write_text(text)
        with pytest.raises(ValueError, match=match):
            cli.read_sets(str(lst))
    args = cli.parse_args(['--sets', str(lst), '-o', str(tmp_path), '-b', 'None'])
    assert args.input == [] and args.sets == str(lst)
