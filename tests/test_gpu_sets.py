"""GPU: file sets -- one file per channel or group of channels, read as the interleaved file they stand for.  Every check is an
equality with the set's interleaved TWIN (setgen.py writes it) through the calls that exist for single files: load_pcm,
load_pcm_channels, load_pcm_mixes, survey_channels, load_pcm_auto, batch_process -- arrays with assert_array_equal, surveys with
==, CSVs byte for byte.  The twin is never the code under test: it takes the interleaved readers.  The counters say that a set is
uploaded once and launched once; the planner's refusals are host-side checks, nothing here reaches a kernel with a bad row."""
import filecmp
import os

import numpy as np
import pytest

import autocases
import setgen
import sndgen
import wavgen
from inaspeechsegmenter_amd import _native, Segmenter
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.resample import Mix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype == np.int16
        np.testing.assert_array_equal(a, b)


def _twin_equalities(seg, members, twin, mixes):
    """The whole-set calls against the twin: downmix, every channel, `mixes`, the survey."""
    np.testing.assert_array_equal(seg.load_pcm(members), seg.load_pcm(twin))
    _same(seg.load_pcm_channels(members), seg.load_pcm_channels(twin))
    _same(seg.load_pcm_mixes(members, mixes), seg.load_pcm_mixes(twin, mixes))
    got, want = seg.survey_channels(members), seg.survey_channels(twin)
    assert got == want
    return got


# ------------------------------------------------------------------------------------------------ geometry
@pytest.fixture(scope='module')
def geometry(seg, tmp_path_factory):
    """8 kHz mono PCM16 members against the tile T (outputs) and the survey chunk: member 0 ends inside the third tile and is the
    longest but one, member 1 exactly on a tile boundary (T frames: 2 T outputs), member 2 inside the first tile, member 3 holds
    one frame; members 4 .. 7 hold chunk - 1, chunk, chunk + 1 and 2 chunk + 1 frames."""
    tile = seg.ctx.resample_split_geometry(8000, 8)[0]
    chunk = seg.ctx.survey_geometry()[0]
    assert chunk == 1024 and tile % 2 == 0
    lens = [tile + 300, tile, tile // 4, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    members, twin = setgen.mono_set(tmp_path_factory.mktemp('geo'), 'g', lens, 8000, 100)
    assert R.out_len(max(lens), 8000) > tile
    return members, twin, lens


def test_geometry_downmix_and_survey(seg, geometry):
    members, twin, lens = geometry
    np.testing.assert_array_equal(seg.load_pcm(members), seg.load_pcm(twin))
    np.testing.assert_array_equal(seg.load_pcm(tuple(members)), R.resample_ref(*iss_io.decode_set(members)))
    got = seg.survey_channels(iss_io.FileSet(members))
    assert got == seg.survey_channels(twin) == iss_io.survey_channels(members)
    assert got.n == max(lens) and not np.any(got.nonfinite)
    assert all(z >= max(lens) - n for z, n in zip(got.zeros, lens))      # the padding counts as digital zeros


@pytest.mark.parametrize('channels', [None, [7, 0, 3, 5, 1, 2, 6, 4], [3, 3, 0, 7, 3]], ids=['all', 'permuted', 'repeated'])
def test_geometry_channels(seg, geometry, channels):
    members, twin, _ = geometry
    _same(seg.load_pcm_channels(members, channels), seg.load_pcm_channels(twin, channels))


def test_geometry_mixes(seg, geometry):
    members, twin, _ = geometry
    group = seg.ctx.resample_split_geometry(8000, 40)[1]
    many = [[k % 8, (3 * k + 1) % 8] for k in range(group + 3)]   # more mixes than one group holds
    assert len(many) > group
    for mixes in ([0], [[0, 1]], [Mix(((0, 4.0), (7, 1.5), (1, -1.25)), 1.0)], [Mix(((2, 1.0), (2, 1.0), (3, 0.5)), 2.0)], many):
        _same(seg.load_pcm_mixes(members, mixes), seg.load_pcm_mixes(twin, mixes))
    loud = seg.load_pcm_mixes(members, [Mix(((0, 4.0), (7, 1.5), (1, -1.25)), 1.0)])[0]
    assert loud.max() == 32767 and loud.min() == -32768           # (the weighted mix saturates)
    _same(seg.load_pcm_mixes(members, [0, [0, 1]]), [R.mix_ref(*iss_io.decode_set(members), m) for m in R.normalise_mixes([0, [0, 1]])])


# ------------------------------------------------------------------------------------------------ formats
FORMATS = [('u8', 'wav', False), ('i8', 'au', True), ('i16', 'wav', False), ('i24', 'wav', False), ('i32', 'rf64', False),
           ('f32', 'wav', False), ('f64', 'w64', False), ('ulaw', 'wav', False), ('alaw', 'wav', False), ('i16', 'aiff', True),
           ('f32', 'au', True), ('i32', 'caf', True), ('f64', 'caf', True)]


@pytest.mark.parametrize('kind,container,big', FORMATS, ids=[f'{k}-{c}' for k, c, _ in FORMATS])
def test_formats(seg, tmp_path, kind, container, big):
    """One two-member set per ISS_RS_* code.  The second member is the shorter one (but for A-law, which has no code for 0.0: its
    twin needs members of one length); the float sets hold a NaN and an Inf where the shorter member has ended."""
    lens = [1500, 1500 if kind == 'alaw' else 900]
    xs = setgen.signals(lens, [1, 1], 40)
    if kind in ('f32', 'f64'):
        xs[0][1000], xs[0][1200], xs[1][10] = np.nan, np.inf, -np.inf
    members, twin = setgen.write_set(tmp_path, 'f', xs, 8000, kind, container, big)
    survey = _twin_equalities(seg, members, twin, [0, 1, [0, 1], Mix(((1, -1.0), (0, 0.5)), 1.0)])
    assert survey == iss_io.survey_channels(members)
    assert list(survey.nonfinite) == ([2, 1] if kind in ('f32', 'f64') else [0, 0])
    assert survey.zeros[1] >= lens[0] - lens[1]


def test_formats_mixed_containers(seg, tmp_path):
    """Members of one code (little-endian PCM16) in four containers."""
    xs = setgen.signals([1300, 700, 1301, 64], [1] * 4, 41)
    members, twin = setgen.write_set(tmp_path, 'c', xs, 8000, 'i16', ['wav', 'w64', 'caf', 'rf64'], False)
    _twin_equalities(seg, members, twin, [[0, 1, 2, 3], 3, Mix(((3, 2.0), (1, 1.0)), 1.0)])


# ------------------------------------------------------------------------------------------------ layout
def test_stereo_member_and_mono_member(seg, tmp_path):
    """Three channels from two members: channel 1 is c_local 1 of member 0, channel 2 lies in the longer member."""
    xs = setgen.signals([900, 1400], [2, 1], 42)
    members, twin = setgen.write_set(tmp_path, 'l', xs, 8000)
    _twin_equalities(seg, members, twin, [1, [1, 2], [2, 1, 0], Mix(((1, 1.0), (2, -1.0)), 2.0)])
    _same(seg.load_pcm_channels(members, [1, 2, 0, 1]), seg.load_pcm_channels(twin, [1, 2, 0, 1]))


def test_seventeen_members(seg, tmp_path):
    lens = [600 + 37 * k for k in range(17)]
    members, twin = setgen.mono_set(tmp_path, 'w', lens, 8000, 43)
    survey = _twin_equalities(seg, members, twin, [list(range(17)), 16, [16, 0]])
    assert survey.s12 is None and seg.survey_channels(twin).s12 is None


def test_one_member_set_is_the_file(seg, tmp_path):
    for ch, sr in ((1, 8000), (2, 48000), (1, 16000)):
        f = sndgen.write(tmp_path / f'one{ch}{sr}.wav', 'wav', 'i16', False, wavgen.make_signal(2000, ch, 44), sr)[0]
        np.testing.assert_array_equal(seg.load_pcm((f,)), seg.load_pcm(f))
        np.testing.assert_array_equal(seg.load_pcm(iss_io.FileSet([f])), seg.load_pcm(f))
        _same(seg.load_pcm_channels([f]), seg.load_pcm_channels(f))
        assert seg.survey_channels([f]) == seg.survey_channels(f)


@pytest.mark.parametrize('sr', [16000, 48000, 44100])
def test_rates(seg, tmp_path, sr):
    """The identity filter, a table that fits LDS beside the spans, and one that is read through the caches."""
    members, twin = setgen.mono_set(tmp_path, 'r', [2 * sr // 10, sr // 10, sr // 7], sr, 45)
    _twin_equalities(seg, members, twin, [2, [0, 1, 2], Mix(((0, 1.0), (1, -1.0)), 2.0)])
    if sr == 16000:                                               # (the stored PCM16 values themselves)
        np.testing.assert_array_equal(seg.load_pcm_channels(members, [0])[0], iss_io.decode_source(members[0])[0])


# ------------------------------------------------------------------------------------------------ one upload, no host interleave
def _payload_bytes(members):
    """The members' stored bytes end to end, each but the last padded to a 16-byte boundary."""
    sizes = [iss_io.decode_source(m)[0].nbytes for m in members]
    return sum(-(-n // 16) * 16 for n in sizes[:-1]) + sizes[-1]


def test_one_upload_one_launch(seg, geometry):
    members, _, _ = geometry
    ctx = seg.ctx
    up, rs, sv = ctx.upload_stats(), ctx.resample_stats(), ctx.survey_stats()
    seg.load_pcm_mixes(members, [0, [0, 1], [2, 3, 4]])
    assert ctx.upload_stats() == (up[0] + 1, up[1] + _payload_bytes(members))
    assert ctx.resample_stats() == (rs[0] + 1, rs[1] + 1) and ctx.survey_stats() == sv
    up, rs = ctx.upload_stats(), ctx.resample_stats()
    pcm, survey, mix = seg.load_pcm_auto(members)
    assert ctx.upload_stats() == (up[0] + 1, up[1] + _payload_bytes(members))
    assert ctx.survey_stats() == (sv[0] + 1, sv[1] + 1) and ctx.resample_stats() == (rs[0] + 1, rs[1] + 1)
    assert survey is not None


# ------------------------------------------------------------------------------------------------ channels='auto'
def _auto_set(folder, case, sr, n=None):
    """The columns of an autocases case as one mono WAV each, and the case's own file as the twin."""
    x = autocases.stored(case, sr, n=n)
    members = [wavgen.write_wav(os.path.join(str(folder), f'{case}.{c}.wav'), np.ascontiguousarray(x[:, c]), sr, 'i16')
               for c in range(x.shape[1])]
    return members, wavgen.write_wav(os.path.join(str(folder), f'{case}.twin.wav'), x, sr, 'i16')


def _auto_equalities(seg, members, twin):
    pcm, survey, mix = seg.load_pcm_auto(members)
    tpcm, tsurvey, tmix = seg.load_pcm_auto(twin)
    np.testing.assert_array_equal(pcm, tpcm)
    assert survey == tsurvey and mix == tmix
    hpcm, hsurvey, hmix = iss_io.decode_auto(members)
    np.testing.assert_array_equal(pcm, hpcm)
    assert hsurvey == survey and hmix == mix
    segments, s2, m2 = seg.segment_auto(members)
    assert s2 == survey and m2 == mix and segments == seg.segment_signal(pcm) == seg.segment_auto(twin)[0]
    return pcm, survey, mix, segments


def test_auto_inverted_pair_is_saved(seg, tmp_path):
    """Member 1 is the inverse of member 0: the plain downmix is silence from end to end, 'auto' hears channel 0."""
    members, twin = _auto_set(tmp_path, 'inverted', 8000)
    pcm, survey, mix, segments = _auto_equalities(seg, members, twin)
    assert mix == Mix(((0, 1.0), (1, -1.0)), 2.0)
    np.testing.assert_array_equal(pcm, seg.load_pcm_channels(members, [0])[0])
    assert not np.any(seg.load_pcm(members))
    plain = seg(members)
    assert len(plain) == 1 and plain[0][0] == 'noEnergy', plain
    assert segments != plain and any(lab != 'noEnergy' for lab, _, _ in segments), segments


def test_auto_drops_a_silent_member(seg, tmp_path):
    members, twin = _auto_set(tmp_path, 'deadinv', 48000)
    pcm, survey, mix, _ = _auto_equalities(seg, members, twin)
    assert mix == Mix(((1, 1.0), (2, -1.0)), 2.0)
    assert not np.array_equal(pcm, seg.load_pcm(members))


def test_auto_healthy_set_is_read_as_ever(seg, tmp_path):
    members, twin = _auto_set(tmp_path, 'healthy', 48000)
    pcm, survey, mix, _ = _auto_equalities(seg, members, twin)
    assert mix is None
    np.testing.assert_array_equal(pcm, seg.load_pcm(twin))
    np.testing.assert_array_equal(pcm, seg.load_pcm(members))


# ------------------------------------------------------------------------------------------------ passes
@pytest.fixture(scope='module')
def archive(tmp_path_factory):
    """Two sets of different sizes, a plain stereo WAV and a stereo FLAC file -> (the list with the sets, the list with their twins)."""
    d = tmp_path_factory.mktemp('arch')
    a, ta = _auto_set(d, 'inverted', 8000)
    x = autocases.stored('deadinv', 44100, seed=9, n=60000)
    b = [wavgen.write_wav(str(d / 'b.0.wav'), np.ascontiguousarray(x[:, 0]), 44100, 'i16'),
         wavgen.write_wav(str(d / 'b.12.wav'), np.ascontiguousarray(x[:50000, 1:]), 44100, 'i16')]      # a stereo member, shorter
    x[50000:, 1:] = 0
    tb = wavgen.write_wav(str(d / 'b.twin.wav'), x, 44100, 'i16')
    wav = autocases.write(d / 'plain.wav', 'healthy', 48000)
    fl = autocases.write(d / 'coded.flac', 'independent', 16000, 'flac')
    return [tuple(a), wav, iss_io.FileSet(b, name='tape-b'), fl], [ta, wav, tb, fl]


@pytest.mark.parametrize('mode', ['default', 'split', 'auto', 'mixes'])
def test_batch_process_equals_the_twins(seg, archive, tmp_path, mode):
    with_sets, with_twins = archive
    kw = {'default': {}, 'split': {'channels': 'split'}, 'auto': {'channels': 'auto'}, 'mixes': {'mixes': R.parse_mixes('0,1,0+1')}}[mode]
    names = ['a', 'plain', 'b', 'coded']
    outs = {}
    for tag, linput in (('set', with_sets), ('twin', with_twins)):
        os.makedirs(tmp_path / tag)
        decisions = []
        extra = {'decisions': decisions} if mode == 'auto' else {}
        lmsg = seg.batch_process(linput, [str(tmp_path / tag / f'{n}.csv') for n in names], **kw, **extra)[3]
        outs[tag] = (lmsg, decisions)
    (ls, ds), (lt, dt) = outs['set'], outs['twin']
    assert [(os.path.basename(dst), code) for dst, code, _ in ls] == [(os.path.basename(dst), code) for dst, code, _ in lt]
    assert all(code == 0 for _, code, _ in ls) and len(ls) == {'default': 4, 'split': 2 + 2 + 3 + 2, 'auto': 4, 'mixes': 12}[mode]
    for (dst, _, _), (tdst, _, _) in zip(ls, lt):
        assert filecmp.cmp(dst, tdst, shallow=False), (dst, tdst)
    if mode == 'auto':
        by = {str(src): (s, m) for src, s, m in ds}
        tby = {str(src): (s, m) for src, s, m in dt}
        assert by[str(iss_io.FileSet(with_sets[0]))] == tby[with_twins[0]] and by['tape-b'] == tby[with_twins[2]]
        assert by['tape-b'][1] == Mix(((1, 1.0), (2, -1.0)), 2.0)


def test_batch_process_bad_sets_and_a_plain_call_after(seg, archive, tmp_path):
    with_sets, with_twins = archive
    coded = (with_sets[0][0], with_sets[3])                       # a FLAC member
    rates = (with_sets[0][0], with_sets[2].members[0])            # 8 000 Hz and 44 100 Hz
    linput = [with_sets[1], coded, with_sets[0], rates, with_sets[3]]
    lmsg = seg.batch_process(linput, [str(tmp_path / f'{k}.csv') for k in range(5)])[3]
    assert [code for _, code, _ in lmsg] == [0, 2, 0, 2, 0]
    assert with_sets[3] in lmsg[1][2] and 'FLAC is not supported in a file set' in lmsg[1][2]
    assert with_sets[2].members[0] in lmsg[3][2] and 'sample rate' in lmsg[3][2]
    os.makedirs(tmp_path / 'alone')
    alone = seg.batch_process([with_twins[1], with_twins[0], with_twins[3]], [str(tmp_path / 'alone' / f'{k}.csv') for k in (0, 2, 4)])[3]
    for (dst, _, _), (tdst, _, _) in zip([lmsg[0], lmsg[2], lmsg[4]], alone):
        assert filecmp.cmp(dst, tdst, shallow=False)
    # a plain call still gives what it gave: the single-file comparison of the resampler tests, repeated last
    f = with_twins[2]
    np.testing.assert_array_equal(seg.load_pcm(f), R.resample_ref(*iss_io.decode_source(f)))


def test_out_of_scope_calls_refuse(seg, geometry):
    members, _, _ = geometry
    for call in (lambda: seg.load_pcm_excerpts(members, [(0.0, 0.1)]), lambda: seg.segment_excerpts(members, [(0.0, 0.1)]),
                 lambda: seg.load_pcm_channel_excerpts(members, [(0.0, 0.1)]), lambda: seg.load_pcm_mix_excerpts(members, [(0.0, 0.1)], [0]),
                 lambda: seg.survey_channels(members, [(0.0, 0.1)]), lambda: seg(members, 0.0, 0.1)):
        with pytest.raises(ValueError, match='of a set are not supported'):
            call()


# ------------------------------------------------------------------------------------------------ planner refusals
def test_planner_refusals(seg):
    """Every ISS_EINVAL of the three entry points is found on the host: counters and the resident signal stay as they were."""
    ctx = seg.ctx
    a = wavgen.encode(wavgen.make_signal(3000, 1, 50), 'i16')
    b = wavgen.encode(wavgen.make_signal(2000, 2, 51), 'i16')
    src = np.zeros(6000 + 8000, dtype=np.uint8)
    src[:6000], src[6000:] = a.view(np.uint8), b.reshape(-1).view(np.uint8)
    fid = ctx.resample_filter(8000)[0]
    good_job = (0, 3000, 3, _native.RS_FORMAT[np.dtype('<i2')], fid, 0, 0, 6000)
    good_members = [(0, 3000, 1, 0), (6000, 2000, 2, 0)]
    resident = wavgen.encode(wavgen.make_signal(7000, 1, 52), 'i16')
    ctx.set_signal(resident)

    def tables(job=good_job, sets=((0, 2),), members=good_members, dtype=_native.RS_JOB):
        return (np.array([job], dtype=dtype), (np.array(list(sets), dtype=_native.SET), np.array(list(members), dtype=_native.SET_MEMBER)))

    cases = [
        (r'job 0: member rows \[0, \+0\) empty', tables(sets=[(0, 0)])),
        (r'job 0: member rows \[1, \+2\) empty, above 1024 or outside the 2', tables(sets=[(1, 2)])),
        (r'job 0: member rows \[-1, \+2\)', tables(sets=[(-1, 2)])),
        (r'job 0: the members hold 3 channels, the job row states 2', tables(job=good_job[:2] + (2,) + good_job[3:])),
        (r'job 0: the longest member holds 3000 frames, the job row states 2999', tables(job=(0, 2999) + good_job[2:7] + (5998,))),
        (r'job 0: member 1: source bytes from 6004 on \(8000 of them\) outside the 14000-byte buffer', tables(members=[good_members[0], (6004, 2000, 2, 0)])),
        (r'job 0: member 0: source bytes from 1 on .* misaligned', tables(members=[(1, 2999, 1, 0), good_members[1]], job=good_job)),
        (r'job 0: member 1: 0 frames of 2 channels', tables(members=[good_members[0], (6000, 0, 2, 0)])),
        (r'job 0: member 0: 3000 frames of 0 channels', tables(members=[(0, 3000, 0, 0), good_members[1]])),
        (r'job 0: src_offset 16: a set job states 0', tables(job=(16,) + good_job[1:])),
    ]
    before = (ctx.resample_stats(), ctx.survey_stats(), ctx.upload_stats())
    for match, (jobs, members) in cases:
        with pytest.raises(_native.NativeError, match=match):
            ctx.resample_set(src, jobs, members, n_signal=6000)
        sjobs = np.array([(jobs['src_offset'][0], jobs['frames_in'][0], jobs['channels'][0], jobs['format'][0], 32767 / 32768)],
                         dtype=_native.SURVEY_JOB)
        with pytest.raises(_native.NativeError, match=match):
            ctx.survey_set(src, sjobs, members)
    jobs, members = tables()
    stride = 6080
    for match, mixes in ((r'job 0: mix 0: term 0: channel 3 of 3', [(stride, [3])]), (r'dst_stride 10 below the 6000 outputs', [(10, [0, 1])]),
                         (r'job 0: mix 0: divisor 0', [(stride, [Mix(((0, 1.0),), 0.0)])])):
        with pytest.raises(_native.NativeError, match=match):
            ctx.resample_set(src, jobs, members, n_signal=3 * stride, mixes=mixes)
    with pytest.raises(_native.NativeError, match=r'output \[0, 6000\) outside the 100-sample signal'):
        ctx.resample_set(src, jobs, members, n_signal=100)
    with pytest.raises(_native.NativeError, match=r'job 0: bad format 5'):
        ctx.resample_set(src, tables(job=good_job[:3] + (5,) + good_job[4:])[0], members, n_signal=6000)
    assert (ctx.resample_stats(), ctx.survey_stats(), ctx.upload_stats()) == before
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, resident.size), resident)

    # the staged entry point: a payload of iss_survey_set, its own id, its own members
    sjob = np.array([(0, 3000, 3, good_job[3], 32767 / 32768)], dtype=_native.SURVEY_JOB)
    with pytest.raises(_native.NativeError, match='iss_resample_staged_set: .*payload'):
        ctx.resample_staged_set(12345678, jobs, members, n_signal=6000)
    fields = ctx.survey_set(src, sjob, members)
    payload = ctx.staged_payload(None)
    mid = (ctx.resample_stats(), ctx.upload_stats())
    with pytest.raises(_native.NativeError, match='iss_resample_staged_set: job 0: no job of the last iss_survey_set held these members'):
        ctx.resample_staged_set(payload, jobs, (members[0], np.array([good_members[0], (6000, 1999, 2, 0)], dtype=_native.SET_MEMBER)), n_signal=6000)
    with pytest.raises(_native.NativeError, match='iss_resample_staged_mix: job 0: no job of the last iss_survey'):
        ctx.resample_staged(None, payload, [good_job], n_signal=6000)      # (a set's payload is not one of interleaved frames)
    with pytest.raises(_native.NativeError, match='payload .* has been replaced|holds no payload'):
        ctx.resample_staged_set(payload + 1, jobs, members, n_signal=6000)
    assert (ctx.resample_stats(), ctx.upload_stats()) == mid
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, resident.size), resident)
    # ... and the context still works: the staged downmix is the twin's, and so is the survey
    ctx.resample_staged_set(payload, jobs, members, n_signal=6000)
    twin = np.zeros((3000, 3), dtype='<i2')
    twin[:, 0], twin[:2000, 1:] = a, b
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 6000), R.resample_ref(twin, 8000))
    assert ctx.upload_stats() == mid[1] and ctx.resample_stats() == (mid[0][0] + 1, mid[0][1] + 1)
    want = R.survey_ref(twin, 32767 / 32768, 0, 3000)
    for name in want._fields:
        np.testing.assert_array_equal(getattr(fields[0], name), getattr(want, name))
