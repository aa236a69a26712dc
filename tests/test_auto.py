"""CPU: the survey-guided downmix (channels='auto').  The rule, survey.ChannelSurvey.safe_mix, case by case on surveys of
io.survey_channels; io.decode_auto, the host-only twin of Segmenter.load_pcm_auto, against decode_mixes and the plain decode, to
the bit, for every source class; the argument errors; the command line on a fake device.  The inputs are autocases.py's."""
import importlib.util
import math
import os

import numpy as np
import pytest

import autocases
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd import survey as survey_mod
from inaspeechsegmenter_amd.resample import Mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the rule
WANT = {'inverted': Mix(((0, 1.0), (1, -1.0)), 2.0), 'healthy': None, 'dead4': Mix(((0, 1.0), (2, 1.0)), 2.0),
        'deadinv': Mix(((1, 1.0), (2, -1.0)), 2.0), 'independent': None, 'silent': None, 'mono': None,
        'twins': Mix(((0, 1.0), (1, -1.0), (2, -1.0)), 3.0), 'wide17': Mix(tuple((c, 1.0) for c in range(17) if c not in (3, 11)), 15.0)}


@pytest.mark.parametrize('sr', autocases.RATES)
@pytest.mark.parametrize('case', sorted(WANT))
def test_safe_mix_case_by_case(tmp_path, case, sr):
    s = iss_io.survey_channels(autocases.write(tmp_path / 'a.wav', case, sr))
    mix = s.safe_mix()
    assert mix == WANT[case], (case, mix)
    assert mix is None or (isinstance(mix, Mix) and all(isinstance(w, float) and isinstance(c, int) for c, w in mix.terms)
                           and isinstance(mix.divisor, float) and mix.divisor == len(mix.terms))


def test_the_inputs_decide_far_from_both_thresholds(tmp_path):
    """What the rule reads of each input, against the figures the cases were chosen for."""
    sv = {case: iss_io.survey_channels(autocases.write(tmp_path / f'{case}.wav', case, 48000)) for case in WANT if case != 'mono'}
    assert sv['inverted'].corr(0, 1) == -1.0 and sv['inverted'].downmix_loss_db == -math.inf and sv['inverted'].active() == [0, 1]
    assert 0.90 < sv['healthy'].corr(0, 1) < 0.94 and -0.4 < sv['healthy'].downmix_loss_db < -0.1
    assert sv['dead4'].active() == [0, 2] and sv['dead4'].peak[1] == 0 and -94 < sv['dead4'].rms_db[3] < -92
    assert -3.6 < sv['dead4'].downmix_loss_db < -3.0
    assert sv['deadinv'].active() == [1, 2] and -0.94 < sv['deadinv'].corr(1, 2) < -0.90 and sv['deadinv'].downmix_loss_db < -10
    assert abs(sv['independent'].corr(0, 1)) < 0.05
    assert sv['silent'].active() == []
    assert sv['twins'].s2[0] == sv['twins'].s2[1] == sv['twins'].s2[2]                 # a tie: channel 0 is the reference;
    assert sv['twins'].corr(1, 2) == 1.0 and sv['twins'].corr(0, 1) == -1.0            # channel 1 or 2 would give (-1, +1, +1)
    assert sv['inverted'].s2[0] == sv['inverted'].s2[1]                                # (and here (-1, +1) in place of (+1, -1))
    assert sv['wide17'].s12 is None and len(sv['wide17'].active()) == 15
    for s in sv.values():                                                              # every active channel far above the floor
        assert all(db > survey_mod.ACTIVE_FLOOR_DB + 20 for c, db in enumerate(s.rms_db) if c in s.active())


def test_equal_surveys_decide_equally(tmp_path):
    a = iss_io.survey_channels(autocases.write(tmp_path / 'a.wav', 'deadinv', 44100))
    b = iss_io.survey_channels(autocases.write(tmp_path / 'b.wav', 'deadinv', 44100))
    assert a == b and a.safe_mix() == b.safe_mix()


def test_nan_correlation_keeps_the_sign():
    """A constant (DC) channel has no correlation: NaN gives +1, and the channel is kept as it is."""
    n = 4096
    x = np.zeros((n, 2))
    x[:, 0] = np.random.default_rng(1).uniform(-0.5, 0.5, n)
    x[:, 1] = 0.25
    s = survey_mod.ChannelSurvey(R.survey_ref(x, 1.0), 16000)
    assert math.isnan(s.corr(0, 1)) and s.active() == [0, 1] and s.safe_mix() is None


# ------------------------------------------------------------------------------------------------ the host-only twin
CLASSES = [('i16', 44100), ('i16', 48000), ('f32', 48000), ('flac', 16000), ('ima', 8000), ('ms', 8000)]


@pytest.mark.parametrize('kind,sr', CLASSES, ids=[f'{k}-{sr}' for k, sr in CLASSES])
@pytest.mark.parametrize('case', ['deadinv', 'healthy'])
def test_decode_auto_is_the_mix_or_the_plain_decode(tmp_path, case, kind, sr):
    n = int(0.25 * sr)                                            # (one gate of noise: the rule needs no more, the host less time)
    f = autocases.write(tmp_path / 'a.bin', case, sr, kind, n=n)
    pcm, survey, mix = iss_io.decode_auto(f)
    assert survey == iss_io.survey_channels(f) and mix == survey.safe_mix()
    x, rate = iss_io.decode_source(f)
    assert rate == sr and pcm.dtype == np.int16
    if case == 'healthy':
        assert mix is None
        np.testing.assert_array_equal(pcm, R.resample_ref(x, sr))
    else:
        assert mix == WANT['deadinv']
        np.testing.assert_array_equal(pcm, iss_io.decode_mixes(f, [mix])[0])
        assert not np.array_equal(pcm, R.resample_ref(x, sr))


def test_decode_auto_saves_the_inverted_file(tmp_path):
    f = autocases.write(tmp_path / 'a.wav', 'inverted', 16000)
    pcm, survey, mix = iss_io.decode_auto(f)
    x, _ = iss_io.decode_source(f)
    assert mix == WANT['inverted'] and not np.any(R.resample_ref(x, 16000))           # the plain decode: all zeros
    np.testing.assert_array_equal(pcm, iss_io.decode_mixes(f, [[0]])[0])
    np.testing.assert_array_equal(pcm, x[:, 0])                                        # channel 0's own samples
    assert np.any(pcm)


def test_decode_auto_mono_is_the_default_read(tmp_path):
    f = autocases.write(tmp_path / 'a.wav', 'mono', 16000)
    pcm, survey, mix = iss_io.decode_auto(f)
    assert survey is None and mix is None
    np.testing.assert_array_equal(pcm, iss_io.decode_pcm(f, ffmpeg=None))
    g = autocases.write(tmp_path / 'b.wav', 'mono', 8000, n=2000)
    np.testing.assert_array_equal(iss_io.decode_auto(g)[0], R.resample_ref(iss_io.decode_source(g)[0], 8000))
    with pytest.raises(AssertionError, match='16000 Hz'):
        iss_io.decode_auto(autocases.write(tmp_path / 'c.wav', 'healthy', 8000, n=2000), resample=False)


def test_auto_source_shape(tmp_path):
    """A mono file gives what the default read gives; a file of two or more channels one signal of the downmix's length."""
    from inaspeechsegmenter_amd import flac, sndfmt, sources
    mono = iss_io.auto_source(autocases.write(tmp_path / 'm.wav', 'mono', 16000))
    assert isinstance(mono, np.ndarray) and mono.dtype == np.int16
    for kind, sr, cls in (('i16', 48000, sources.RawAuto), ('f32', 44100, sources.RawAuto), ('flac', 16000, flac.FlacAuto),
                          ('ima', 8000, sndfmt.AdpcmAuto), ('ms', 8000, sndfmt.MsAdpcmAuto)):
        n = int(0.25 * sr)
        s = iss_io.auto_source(autocases.write(tmp_path / f'a.{kind}', 'deadinv', sr, kind, n=n), resample=True)
        assert type(s) is cls and s.two_step and s.parts == 1 and s.size == R.out_len(n, sr) and s.decision is None and s.batchable
    with pytest.raises(AssertionError, match='16000 Hz'):
        iss_io.auto_source(autocases.write(tmp_path / 'r.wav', 'healthy', 8000, n=2000), resample=False)
    # a coder's one-channel files come as the coder's two-step class: a pass makes one decode call per coder, whatever it holds
    for kind, sr, cls, want in (('flac', 16000, flac.FlacAuto, 'pcm'), ('flac', 8000, flac.FlacAuto, 'stage'),
                                ('ima', 16000, sndfmt.AdpcmAuto, 'pcm'), ('ms', 8000, sndfmt.MsAdpcmAuto, 'stage')):
        s = iss_io.auto_source(autocases.write(tmp_path / f'm.{kind}', 'mono', sr, kind, n=2000), resample=True)
        assert type(s) is cls and s.kind == want and s.parts == 1 and s.size == R.out_len(2000, sr) and s.batchable
        assert type(s).pass_order == type(iss_io.auto_source(autocases.write(tmp_path / f's.{kind}', 'healthy', sr, kind, n=2000),
                                                             resample=True)).pass_order and type(s).two_step
    with pytest.raises(AssertionError, match='16000 Hz'):
        iss_io.auto_source(autocases.write(tmp_path / 'r.flac', 'mono', 8000, 'flac', n=2000), resample=False)


def test_decisions_tsv_keeps_a_path_listed_twice(tmp_path):
    f = autocases.write(tmp_path / 'a.wav', 'deadinv', 16000, n=4000)
    _, survey, mix = iss_io.decode_auto(f)
    survey_mod.write_decisions_tsv(tmp_path / 'd.tsv', [f, f, f], [(f, survey, mix), (f, survey, None)])
    rows = [line.split('\t') for line in (tmp_path / 'd.tsv').read_text().splitlines()][1:]
    assert [r[1] for r in rows] == ['mix', 'plain', '!'] and rows[2][4] == 'not processed'


# ------------------------------------------------------------------------------------------------ argument errors
class _NoDevice:
    """Segmenter.batch_process / load_pcm_auto on an object that has no device: the refusals come before any device call."""
    resample = True

    def __init__(self, ffmpeg):
        self.ffmpeg = ffmpeg

    def _no_ffmpeg_mixes(self):
        pass


def test_argument_errors(tmp_path):
    from inaspeechsegmenter_amd.segmenter import Segmenter
    with pytest.raises(ValueError, match="mixes and channels='auto' exclude each other"):
        Segmenter.batch_process(_NoDevice(None), ['a.wav'], ['a.csv'], channels='auto', mixes=[[0]])
    with pytest.raises(ValueError, match="channels='auto' reads files without ffmpeg"):
        Segmenter.batch_process(_NoDevice('ffmpeg'), ['a.wav'], ['a.csv'], channels='auto')
    with pytest.raises(ValueError, match="None, 'split' or 'auto'"):
        Segmenter.batch_process(_NoDevice(None), ['a.wav'], ['a.csv'], channels='each')
    with pytest.raises(ValueError, match="channels='auto' reads files without ffmpeg"):
        Segmenter._auto_sig(_NoDevice('ffmpeg'), 'a.wav')        # (what load_pcm_auto and segment_auto call first)


# ------------------------------------------------------------------------------------------------ the command line
def _cli():
    spec = importlib.util.spec_from_file_location('ina_cli', os.path.join(ROOT, 'scripts', 'ina_speech_segmenter_amd.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_auto_writes_the_decisions(tmp_path, monkeypatch):
    import inaspeechsegmenter_amd
    seen = {}
    names = {case: autocases.write(tmp_path / f'{case}.wav', case, 16000, n=4000) for case in ('deadinv', 'healthy', 'mono', 'silent')}

    class FakeSegmenter:
        def __init__(self, **kw):
            seen['init'] = kw

        def batch_process(self, inputs, outputs, **kw):
            seen['batch'] = (list(inputs), list(outputs), kw)
            lmsg = []
            for src, dst in zip(inputs, outputs):
                if src == names['silent']:                        # (stands for a file that failed)
                    lmsg.append((dst, 2, "error: <class 'ValueError'> bad\tframe"))
                    continue
                kw['decisions'].append((src,) + iss_io.decode_auto(src)[1:])
                lmsg.append((dst, 0, 'ok 0.0'))
            return 0.0, 3, 0.0, lmsg

    monkeypatch.setattr(inaspeechsegmenter_amd, 'Segmenter', FakeSegmenter)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    tsv = tmp_path / 'd.tsv'
    assert _cli().main(['-i', str(tmp_path / '*.wav'), '-o', str(tmp_path), '-b', 'None', '--resample', '--channels', 'auto',
                        '--decisions', str(tsv)]) == 0
    inputs, outputs, kw = seen['batch']
    assert inputs == sorted(names.values()) and kw['channels'] == 'auto' and seen['init']['ffmpeg'] is None
    rows = [line.split('\t') for line in tsv.read_text().splitlines()]
    assert rows[0] == list(survey_mod.DECISION_COLUMNS) == ['path', 'plan', 'kept', 'flipped', 'downmix_loss_db']
    by = {r[0]: r[1:] for r in rows[1:]}
    assert [r[0] for r in rows[1:]] == inputs
    assert by[names['deadinv']][:3] == ['mix', '1,2', '2'] and float(by[names['deadinv']][3]) < -10
    assert by[names['healthy']][:3] == ['plain', '0,1', ''] and -0.5 < float(by[names['healthy']][3]) < 0
    assert by[names['mono']] == ['mono', '0', '', '']
    assert by[names['silent']] == ['!', '', '', "error: <class 'ValueError'> bad frame"]


@pytest.mark.parametrize('argv,why', [(['--channels', 'auto'], 'needs -b None'),
                                      (['-b', 'None', '--channels', 'auto', '--mixes', '0+1'], 'exclude each other'),
                                      (['-b', 'None', '--decisions', 'd.tsv'], 'goes with --channels auto')])
def test_cli_refusals(tmp_path, capsys, argv, why):
    with pytest.raises(SystemExit):
        _cli().main(['-i', 'a.wav', '-o', str(tmp_path)] + argv)
    assert why in capsys.readouterr().err
