"""CPU: scheduled downmixes.  resample.Schedule / normalise_schedule / schedule_mixdown / schedule_ref: the two identities, the
host twin io.decode_schedule against a by-hand piecewise mixdown, every refusal of a bad specification, and the argument errors of
the Segmenter calls, which come before any device call."""
import numpy as np
import pytest

import autocases
import wavgen
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.resample import Mix, Schedule


@pytest.mark.parametrize('sr,fmt,ch', [(8000, 'i16', 2), (44100, 'i24', 3), (16000, 'f32', 2), (48000, 'f64', 3)])
def test_identities(sr, fmt, ch):
    x = wavgen.as_read(wavgen.encode(wavgen.make_signal(1500, ch, 400), fmt), fmt)
    np.testing.assert_array_equal(R.schedule_ref(x, sr, [(0, None)]), R.resample_ref(x, sr))
    np.testing.assert_array_equal(R.schedule_mixdown(x, [(0, None)]), R.mixdown(x, list(range(ch))))
    mix = Mix(((1, 0.7071067811865476), (0, -1.0 / 3.0)), 1.7)
    np.testing.assert_array_equal(R.schedule_ref(x, sr, [(0, mix)]), R.mix_ref(x, sr, mix))
    # a run that begins at or past the end governs nothing; two runs naming one mix are that mix throughout
    np.testing.assert_array_equal(R.schedule_ref(x, sr, [(0, mix), (1500, None), (1700, mix)]), R.mix_ref(x, sr, mix))
    np.testing.assert_array_equal(R.schedule_ref(x, sr, [(0, mix), (700, mix)]), R.mix_ref(x, sr, mix))


def test_mono_is_its_samples():
    x = wavgen.encode(wavgen.make_signal(1200, 1, 401), 'i16')
    np.testing.assert_array_equal(R.schedule_ref(x, 8000, [(0, None), (300, None)]), R.resample_ref(x, 8000))


@pytest.mark.parametrize('kind,sr', [('i16', 8000), ('f32', 44100), ('flac', 48000), ('ima', 8000), ('ms', 16000)])
def test_decode_schedule_against_a_by_hand_statement(tmp_path, kind, sr):
    path = autocases.write(tmp_path / f'a.{kind}', 'deadinv', sr, kind, n=3000)
    spec = [(0, None), (0.01, {1: 1, 2: -1}), (0.1, [2]), (0.1 + 1.0 / sr, None), (0.2, Mix(((0, 0.25), (2, -0.6), (2, 0.1)), 0.9))]
    stored, got_sr = iss_io.decode_source(path)
    assert got_sr == sr and stored.shape == (3000, 3)
    v = iss_io._to_float(stored, np.float64)
    begins = [0, int(np.floor(0.01 * sr + 0.5)), int(np.floor(0.1 * sr + 0.5)), int(np.floor((0.1 + 1.0 / sr) * sr + 0.5)),
              int(np.floor(0.2 * sr + 0.5)), 3000]
    assert begins[3] == begins[2] + 1                                           # a run of one frame
    m = np.zeros(3000)
    a, b = begins[0], begins[1]
    m[a:b] = ((1.0 * v[a:b, 0] + 1.0 * v[a:b, 1]) + 1.0 * v[a:b, 2]) / 3.0
    a, b = begins[1], begins[2]
    m[a:b] = (1.0 * v[a:b, 1] + -1.0 * v[a:b, 2]) / 1.0
    a, b = begins[2], begins[3]
    m[a:b] = (1.0 * v[a:b, 2]) / 1.0
    a, b = begins[3], begins[4]
    m[a:b] = ((1.0 * v[a:b, 0] + 1.0 * v[a:b, 1]) + 1.0 * v[a:b, 2]) / 3.0
    a, b = begins[4], begins[5]
    m[a:b] = ((0.25 * v[a:b, 0] + -0.6 * v[a:b, 2]) + 0.1 * v[a:b, 2]) / 0.9
    want = R.quantise(R.resample_float(m, sr))
    got = iss_io.decode_schedule(path, spec)
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, want)
    sched = R.normalise_schedule(spec, sr, 3)
    assert [b for b, _ in sched] == begins[:-1] and sched.runs[0][1] is None and sched.runs[2][1] == Mix(((2, 1.0),), 1.0)
    np.testing.assert_array_equal(iss_io.decode_schedule(path, sched), want)     # a Schedule counts in frames
    np.testing.assert_array_equal(iss_io.decode_schedule(path, [(0, None)]), R.resample_ref(stored, sr))


def test_decode_schedule_of_a_one_channel_file(tmp_path):
    path = autocases.write(tmp_path / 'm.wav', 'mono', 16000, n=3000)
    np.testing.assert_array_equal(iss_io.decode_schedule(path, [(0, None), (0.1, None)]), iss_io.decode_pcm(path, ffmpeg=None))
    stored, _ = iss_io.decode_source(path)
    np.testing.assert_array_equal(iss_io.decode_schedule(path, [(0, None), (0.1, {0: 0.5})]),
                                  R.schedule_ref(stored, 16000, [(0, None), (1600, Mix(((0, 0.5),), 1.0))]))


@pytest.mark.parametrize('spec,why', [
    ([(0.5, None)], r'run 0 starts at 0.5 s \(frame 4000\): the first run starts at 0'),
    ([(0, None), (0.10001, [0]), (0.10002, None)], r'run 2: starts 0.10001 s and 0.10002 s round to one frame \(800\) at 8000 Hz'),
    ([(0, None), (0.5, [0]), (0.25, None)], r'run 2: start 0.25 s lies before run 1 \(0.5 s\): starts ascend'),
    ([(0, None), (0.5, [0, 2])], r"run 1: .*channel 2 is outside the file's 2 channels"),
    ([(0, None), (-0.5, None)], r'run 1: start -0.5 s is negative or not finite'),
    ([(0, None), (float('nan'), None)], r'run 1: start nan s is negative or not finite'),
    ([(0, None), (0.5, {0: float('inf')})], r'run 1: .*weight inf of channel 0 is not finite'),
    ([(0, Mix(((0, 1.0),), 0.0))], r'run 0: .*divisor 0.0 must be finite and not zero'),
    ([(0, [])], r'run 0: .*empty mix'),
    ([], r'empty schedule'),
    ([(0, None, 1)], r'run 0 \(\(0, None, 1\)\) is not a \(start_sec, mix\) pair'),
    ('0:none', r'a schedule is a sequence of \(start_sec, mix\) runs'),
    (None, r'a schedule is a sequence of \(start_sec, mix\) runs'),
])
def test_bad_specifications(spec, why):
    with pytest.raises(ValueError, match='sched: ' + why):
        R.normalise_schedule(spec, 8000, 2, 'sched')


def test_schedule_class():
    with pytest.raises(ValueError, match='run 0 begins at frame 1, not 0'):
        Schedule([(1, None)])
    with pytest.raises(ValueError, match='run 2 begins at frame 5, run 1 at 5: begins ascend strictly'):
        Schedule([(0, None), (5, None), (5, None)])
    with pytest.raises(ValueError, match='run 1: its mix is a resample.Mix or None'):
        Schedule([(0, None), (5, [0, 1])])
    with pytest.raises(ValueError, match="s: run 1: .*channel 3 is outside the file's 2 channels"):
        R.normalise_schedule(Schedule([(0, None), (5, Mix(((3, 1.0),), 1.0))]), 8000, 2, 's')
    s = Schedule([(0, None), (5, Mix(((0, 1.0),), 1.0))])
    assert s == Schedule(list(s)) and s == [(0, None), (5, Mix(((0, 1.0),), 1.0))] and s != Schedule([(0, None)]) and len(s) == 2


def test_errors_name_the_file(tmp_path):
    path = autocases.write(tmp_path / 'a.wav', 'healthy', 8000, n=3000)
    with pytest.raises(ValueError, match=r"a\.wav: schedule: run 1: .*channel 2 is outside the file's 2 channels"):
        iss_io.decode_schedule(path, [(0, None), (0.1, [2])])
    with pytest.raises(ValueError, match='schedules of a set are not supported'):
        iss_io.decode_schedule((path, path), [(0, None)])
    with pytest.raises(ValueError, match='schedules of a set are not supported'):
        iss_io.schedule_source((path, path), [(0, None)], True)
    with pytest.raises(AssertionError, match='16000 Hz'):
        iss_io.schedule_source(path, [(0, None)], resample=False)


class _NoDevice:
    resample = True

    def __init__(self, ffmpeg):
        self.ffmpeg = ffmpeg


def test_ffmpeg_set_is_refused_before_any_device_call():
    from inaspeechsegmenter_amd.segmenter import Segmenter
    nd = _NoDevice('ffmpeg')
    nd._no_ffmpeg_schedule = lambda what: Segmenter._no_ffmpeg_schedule(nd, what)
    for call, args in ((Segmenter.load_pcm_schedule, ('a.wav', [(0, None)])), (Segmenter.segment_schedule, ('a.wav', [(0, None)])),
                       (Segmenter.survey_timeline, ('a.wav',)), (Segmenter.load_pcm_auto_timeline, ('a.wav',)),
                       (Segmenter.segment_auto_timeline, ('a.wav',))):
        with pytest.raises(ValueError, match=r"are read without ffmpeg \(Segmenter\(ffmpeg=None\)\); ffmpeg='ffmpeg'"):
            call(nd, *args)


def test_the_sources_of_a_schedule(tmp_path):
    """A scheduled source is io.auto_source's source of its class, two-step, in the same place of a pass."""
    from inaspeechsegmenter_amd import sources
    for kind in ('i16', 'flac', 'ima', 'ms'):
        path = autocases.write(tmp_path / f's.{kind}', 'healthy', 8000, kind, n=2000)
        sched, src = iss_io.schedule_source(path, [(0, None), (0.1, [1])], True)
        auto = iss_io.auto_source(path, True)
        assert isinstance(src, sources.SchedSource) and isinstance(src, type(auto)) and type(src).two_step
        assert src.sched == sched == [(0, None), (800, Mix(((1, 1.0),), 1.0))] and src.decision is None
        assert src.size == auto.size and type(src).pass_order == type(auto).pass_order
        tl = iss_io.timeline_source(path, 0.5, True)
        assert type(tl) is type(src) and tl.sched is None and tl.block_chunks == 4
    mono = autocases.write(tmp_path / 'm.wav', 'mono', 16000, n=2000)
    assert isinstance(iss_io.schedule_source(mono, [(0, None)], True)[1], np.ndarray)      # read as it always was
    assert isinstance(iss_io.schedule_source(mono, [(0, {0: 0.5})], True)[1], sources.RawSched)
    assert isinstance(iss_io.timeline_source(mono, None, True), np.ndarray)
