"""Channel survey on the host: resample.survey_ref (the numpy statement of the survey order), io.survey_channels (the host-only
twin of Segmenter.survey_channels) on every container and encoding the generators write, ranges, and the derived figures of
survey.ChannelSurvey on constructed cases.  The sums are held to the worst-case bound of any summation order against
math.fsum, n * 2**-52 * sum|term|; peak and the counts to plain numpy, exactly."""
import math

import numpy as np
import pytest

import flacgen
import msadpcmgen
import sndgen
import wavgen
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.survey import ChannelSurvey

C = R.SURVEY_CHUNK


def _float(x):
    v = iss_io._to_float(np.asarray(x), np.float64)
    return v[:, None] if v.ndim == 1 else v


def check_against_numpy(f, x, full, a=0, b=None):
    """SurveyFields `f` of frames [a, b) of stored samples x: counts and peak exactly numpy's, sums within the fsum bound."""
    raw = _float(x)[a:b]
    bad = ~np.isfinite(raw)
    v = np.where(bad, 0.0, raw)
    n, ch = v.shape
    assert f.n == n
    np.testing.assert_array_equal(f.peak, np.abs(v).max(axis=0) if n else np.zeros(ch))
    np.testing.assert_array_equal(f.zeros, (v == 0).sum(axis=0))
    np.testing.assert_array_equal(f.fullscale, (np.abs(v) >= full).sum(axis=0))
    np.testing.assert_array_equal(f.nonfinite, bad.sum(axis=0))

    def bound(got, terms):
        terms = [float(t) for t in terms]
        assert abs(float(got) - math.fsum(terms)) <= n * 2.0 ** -52 * math.fsum(abs(t) for t in terms)

    for c in range(ch):
        bound(f.s1[c], v[:, c])
        bound(f.s2[c], v[:, c] * v[:, c])
    if ch > R.SURVEY_PAIR_CHANNELS:
        assert f.s12 is None
    else:
        assert len(f.s12) == ch * (ch - 1) // 2
        for k, (c, d) in enumerate(R.survey_pairs(ch)):
            bound(f.s12[k], v[:, c] * v[:, d])


# ------------------------------------------------------------------------------------------------ survey_ref
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, C - 1, C, C + 1, 3 * C + 17])
@pytest.mark.parametrize('ch', [1, 3])
def test_survey_ref_sums_and_counts(n, ch):
    x = wavgen.encode(wavgen.make_signal(max(n, 1), ch, 100 + n)[:n].reshape(n, ch), 'i16')
    x[::7] = 0
    x[3::11] = 32767
    x[5::13] = -32768
    check_against_numpy(R.survey_ref(x, R.SURVEY_FULL['i16']), x, R.SURVEY_FULL['i16'])


def test_survey_ref_order_is_the_stated_one():
    """The order restated by hand for one full chunk and a tail: lanes, wave trees, waves in order, chunks in order."""
    rng = np.random.default_rng(5)
    t = rng.standard_normal(C + 300)
    want = 0.0
    for chunk in (t[:C], t[C:]):
        lanes = np.zeros(256)
        for k, v in enumerate(chunk):
            lanes[k % 256] = lanes[k % 256] + v if k >= 256 else 0.0 + v
        waves = []
        for w in range(4):
            lane = list(lanes[64 * w:64 * w + 64])
            s = 32
            while s:
                lane = [lane[l] + lane[l + s] for l in range(s)]
                s //= 2
            waves.append(lane[0])
        want = want + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    assert R.survey_sum(t[:, None])[0] == want


def test_survey_ref_float_nan_and_inf():
    x = (wavgen.make_signal(700, 2, 7) * 0.5).astype(np.float32)
    x[10, 0], x[11, 0], x[12, 1], x[300, 1] = np.nan, np.inf, -np.inf, 1.0
    f = R.survey_ref(x, 1.0)
    assert list(f.nonfinite) == [2, 1] and list(f.fullscale) == [0, 1]
    assert np.isfinite(f.s1).all() and np.isfinite(f.s2).all() and np.isfinite(f.s12).all()
    check_against_numpy(f, x, 1.0)


def test_survey_ref_17_channels_has_no_pairs():
    x = wavgen.encode(wavgen.make_signal(300, 17, 9), 'i16')
    f = R.survey_ref(x, R.SURVEY_FULL['i16'])
    assert f.s12 is None and len(f.s1) == 17
    check_against_numpy(f, x, R.SURVEY_FULL['i16'])
    s = ChannelSurvey(f, 48000)
    assert s.downmix_loss_db is None and s.inverted() == [] and math.isnan(s.corr(0, 1))


def test_survey_ref_one_and_no_sample():
    f = R.survey_ref(np.array([-16384], dtype=np.int16), R.SURVEY_FULL['i16'])
    assert (f.n, f.peak[0], f.s1[0], f.s2[0], len(f.s12)) == (1, 0.5, -0.5, 0.25, 0)
    s = ChannelSurvey(f, 8000)
    assert s.downmix_loss_db == 0.0 and s.active() == [0] and s.inverted() == []
    e = ChannelSurvey(R.survey_ref(np.zeros((0, 2), dtype=np.int16), 1.0), 8000)
    assert (e.n, list(e.peak), e.dc, e.rms_db, e.active()) == (0, [0.0, 0.0], [0.0, 0.0], [-math.inf, -math.inf], [])


# ------------------------------------------------------------------------------------------------ every container and encoding
def _stored(path):
    x, _ = iss_io.decode_source(path)
    return x


SND = sndgen.cases()


@pytest.mark.parametrize('container,kind,big', SND, ids=[f'{c}-{k}-{"be" if b else "le"}' for c, k, b in SND])
def test_io_survey_every_sndgen_case(tmp_path, container, kind, big):
    x = wavgen.make_signal(1500, 2, 40)
    x[100:110, 0] = 0.0
    x[200:205, 1] = 1.0 if kind in ('f32', 'f64') else 0.99999
    path, _, _ = sndgen.write(tmp_path / f'a.{container}', container, kind, big, x, 22050)
    s = iss_io.survey_channels(path)
    full = R.SURVEY_FULL[kind]
    stored = _stored(path)
    assert s == ChannelSurvey(R.survey_ref(stored, full), 22050)
    check_against_numpy(s.fields, stored, full)
    if kind != 'ima':
        assert s.fullscale[1] >= 5                             # the right `full`: the clipped run counts


@pytest.mark.parametrize('fmt', wavgen.FORMATS)
def test_io_survey_plain_wav(tmp_path, fmt):
    x = wavgen.make_signal(C + 37, 3, 41)
    x[50:60, 2] = 1.0 if fmt in ('f32', 'f64') else 0.9999999
    path = str(tmp_path / 'a.wav')
    wavgen.write_wav(path, wavgen.encode(x, fmt), 44100, fmt)
    s = iss_io.survey_channels(path)
    stored, sr = iss_io.decode_source(path)
    assert s == ChannelSurvey(R.survey_ref(stored, R.SURVEY_FULL[fmt]), sr)
    assert s.fullscale[2] >= 10 and s.channels == 3 and s.n == C + 37


@pytest.mark.parametrize('bps,mode', [(16, 'independent'), (16, 'left_side'), (24, 'independent'), (8, 'independent')])
def test_io_survey_flac(tmp_path, bps, mode):
    x = np.rint(wavgen.make_signal(5000, 2, bps) * 0.8 * ((1 << (bps - 1)) - 1)).astype(np.int64)
    x[77:80, 0] = (1 << (bps - 1)) - 1
    path = flacgen.write(tmp_path / 'a.flac', x, 16000, bps, blocksize=1152, channel_mode=mode)
    s = iss_io.survey_channels(path)
    stored, sr = iss_io.decode_source(path)
    full = R.SURVEY_FULL[{8: 'i8', 16: 'i16', 24: 'i24'}[bps]]
    assert s == ChannelSurvey(R.survey_ref(stored, full), sr)
    assert s.fullscale[0] >= 1
    check_against_numpy(s.fields, stored, full)


def test_io_survey_msadpcm(tmp_path):
    x = wavgen.make_signal(3000, 2, 43)
    path, twin = msadpcmgen.write(tmp_path / 'a.wav', x, 8000, 256)
    s = iss_io.survey_channels(path)
    assert s == ChannelSurvey(R.survey_ref(twin, R.SURVEY_FULL['ms']), 8000)
    check_against_numpy(s.fields, twin, R.SURVEY_FULL['ms'])


# ------------------------------------------------------------------------------------------------ ranges
def test_io_survey_ranges(tmp_path):
    sr, n = 8000, 3 * C + 17
    stored = wavgen.encode(wavgen.make_signal(n, 2, 44), 'i16')
    path = str(tmp_path / 'a.wav')
    wavgen.write_wav(path, stored, sr, 'i16')
    full = R.SURVEY_FULL['i16']
    ranges = [(0.1, 0.3), (0.25, 99.0), (0.2, 0.2 + 1 / sr), (0.0, None)]
    got = iss_io.survey_channels(path, ranges)
    spans = [(800, 2400), (2000, n), (1600, 1601), (0, n)]
    for s, (a, b) in zip(got, spans):
        assert (s.first, s.n) == (a, b - a)
        assert s == ChannelSurvey(R.survey_ref(stored, full, a, b), sr, a)
        assert s == ChannelSurvey(R.survey_ref(stored[a:b], full), sr, a)          # the order depends on (a, b) alone
    with pytest.raises(ValueError, match='holds no frame'):
        iss_io.survey_channels(path, [(n / sr + 1.0, None)])
    with pytest.raises(ValueError, match='holds no frame'):
        iss_io.survey_channels(path, [(0.2, 0.2 + 0.4 / sr)])
    with pytest.raises(ValueError):
        iss_io.survey_channels(path, [(0.5, 0.25)])


# ------------------------------------------------------------------------------------------------ derived figures
def _write_i16(tmp_path, cols, sr=16000, name='a.wav'):
    path = str(tmp_path / name)
    wavgen.write_wav(path, np.stack(cols, axis=1).astype('<i2'), sr, 'i16')
    return path


def test_inverted_pair_cancels_in_the_downmix(tmp_path):
    left = wavgen.encode(wavgen.make_signal(4000, 1, 45).reshape(-1) * 0.5, 'i16')
    s = iss_io.survey_channels(_write_i16(tmp_path, [left, -left]))
    assert s.corr(0, 1) == -1.0 and s.inverted() == [(0, 1)] and s.downmix_loss_db == -math.inf
    assert s.active() == [0, 1]


def test_identical_channels_lose_nothing(tmp_path):
    left = wavgen.encode(wavgen.make_signal(4000, 1, 46).reshape(-1), 'i16')
    s = iss_io.survey_channels(_write_i16(tmp_path, [left, left]))
    assert s.downmix_loss_db == 0.0 and s.inverted() == [] and s.corr(0, 1) == 1.0


def test_active_leaves_out_silent_and_idle_channels(tmp_path):
    rng = np.random.default_rng(47)
    prog = wavgen.encode(wavgen.make_signal(8000, 2, 47) * 0.3, 'i16')
    idle = rng.integers(-4, 5, size=8000)                      # about -80 dBFS
    s = iss_io.survey_channels(_write_i16(tmp_path, [prog[:, 0], np.zeros(8000), prog[:, 1], idle]))
    assert -85 < s.rms_db[3] < -75 and s.rms_db[1] == -math.inf and s.zeros[1] == 8000
    assert s.active() == [0, 2]
    assert s.active(floor_db=-90.0) == [0, 2, 3]
    rows = s.rows()
    assert [r[0] for r in rows] == [0, 1, 2, 3] and [r[-1] for r in rows] == [True, False, True, False]


def test_tsv_rows(tmp_path):
    from inaspeechsegmenter_amd.survey import TSV_COLUMNS, write_tsv
    left = wavgen.encode(wavgen.make_signal(2000, 1, 48).reshape(-1) * 0.5, 'i16')
    path = _write_i16(tmp_path, [left, -left, np.zeros(2000)])
    out = tmp_path / 's.tsv'
    write_tsv(out, [path, 'gone.wav'], [iss_io.survey_channels(path), "error: <class 'FileNotFoundError'> gone.wav"])
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert tuple(rows[0]) == TSV_COLUMNS and all(len(r) == len(TSV_COLUMNS) for r in rows) and len(rows) == 6
    assert [r[1] for r in rows[1:]] == ['0', '1', '2', '*', '!'] and [r[-1] for r in rows[1:4]] == ['1', '1', '0']
    assert rows[1][2] == '2000' and float(rows[1][3]) == abs(left).max() / 32768 and rows[3][4] == '-inf' and rows[3][6] == '2000'
    assert rows[4][-1] == '0-1' and float(rows[4][4]) < -100 and rows[5][-1].startswith('error: ')


def test_command_line_takes_survey():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('cli', os.path.join(os.path.dirname(__file__), '..', 'scripts', 'ina_speech_segmenter_amd.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = cli.build_parser().parse_args(['-i', 'a.wav', '-o', '.', '-b', 'None', '--survey', 'out.tsv'])
    assert args.survey == 'out.tsv'
    assert cli.build_parser().parse_args(['-i', 'a.wav', '-o', '.']).survey is None
    with pytest.raises(SystemExit):
        cli.main(['-i', 'a.wav', '-o', '.', '--survey', 'out.tsv'])          # ffmpeg set: refused before anything is read
