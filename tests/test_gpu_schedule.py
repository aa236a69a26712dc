"""GPU: scheduled downmixes -- a mix per stretch of a file, mixed and resampled on the device.  The SCHED instantiations of
resample_kernel through ctx.resample_sched / ctx.resample_staged_sched and Segmenter.load_pcm_schedule against
resample.schedule_ref / io.decode_schedule, to the bit.  Shapes: three tiles of output and a ragged tail (about 3 300 outputs),
run begins where staging can go wrong -- frame 1, the first staged frame of tile 1 and its neighbours, within the filter's reach
of a tile edge, the last frame, past the end, runs of one frame, 2 000 runs of 1 to 3 frames --, runs without a mix beside mixes,
two runs naming one mix; 2, 3 and 8 channels; PCM16, 24-bit, float32, mu-law and big-endian AIFF; FLAC, IMA and Microsoft ADPCM
through what their decode call staged; four unlike jobs in one launch; and every refusal of the planner with nothing launched."""
import numpy as np
import pytest

import flacgen
import msadpcmgen
import sndgen
import wavgen
from inaspeechsegmenter_amd import _native, Segmenter, sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.resample import Mix, Schedule

pytestmark = pytest.mark.gpu

NOUT = 3 * 1024 + 230                                  # three tiles of 1 024 outputs and a ragged tail


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _hop(n):
    return -(-n // 160) * 160


def _frames(sr):
    """Stored frames that give NOUT outputs at `sr`."""
    up, down, _ = R.plan(sr)
    n = NOUT * down // up
    assert R.out_len(n, sr) == NOUT
    return n


def _mixes(ch):
    """Three mixes of a file of `ch` channels: an inverted pair turned back, one channel alone, weights that are no powers of 2."""
    return [Mix(((0, 1.0), (1, -1.0)), 2.0), Mix(((ch - 1, 1.0),), 1.0), Mix(((1, 0.7071067811865476), (0, -1.0 / 3.0), (ch - 1, 0.3)), 1.7)]


def _begins(sr, n, tile):
    """Run begins where staging can go wrong, for a file of n frames at sr whose tiles hold `tile` outputs."""
    up, down, h = R.plan(sr)
    hl = (h.size - 1) // 2
    s0 = (tile * down - hl) // up                      # the first staged frame of tile 1
    edge, reach = tile * down // up, max(1, hl // up)  # the frame under tile 1's first output, and the filter's half length in frames
    edge2 = 2 * tile * down // up
    out = {1, s0 - 1, s0, s0 + 1, edge - reach // 2, edge + reach // 2, edge2 - 1, edge2 + 1, n - 1, n + 5}
    out |= {edge2 + reach + k for k in range(2, 8)}    # five consecutive one-frame runs (six begins)
    return sorted(b for b in out if b > 0)


def _schedule(sr, n, ch, tile):
    """The schedule of the kernel cases: _begins, the runs cycling through no mix, a mix, another, the first again."""
    a, b, c = _mixes(ch)
    cycle = [None, a, b, a, None, c]
    runs = [(0, b)] + [(beg, cycle[k % len(cycle)]) for k, beg in enumerate(_begins(sr, n, tile))]
    assert sum(m is None for _, m in runs) > 1 and sum(m == a for _, m in runs) > 1 and runs[-1][0] >= n
    return Schedule(runs)


def _sched_direct(ctx, raw, sr, fmt, schedule, stored=None):
    """One scheduled job on its own, checked against schedule_ref of `stored` (what the host reads for `raw`) -> the output."""
    stored = raw if stored is None else stored
    job = ctx.resample_job(raw, sr, 0, 0, fmt)
    nout = job[-1]
    before = ctx.resample_stats()
    ctx.resample_sched(raw.reshape(-1).view(np.uint8), [job], [schedule], n_signal=_hop(nout))
    sig = ctx.get_signal_pcm16(0, _hop(nout))
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)
    np.testing.assert_array_equal(sig[:nout], R.schedule_ref(stored, sr, schedule))
    assert not sig[nout:].any()
    return sig[:nout]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('sr,fmt,ch', [(8000, 'i16', 2), (48000, 'i24', 3), (44100, 'f32', 2), (16000, 'i16', 8), (48000, 'f32', 8),
                                       (44100, 'i16', 3)])
def test_runs_at_the_places_where_staging_can_go_wrong(seg, sr, fmt, ch):
    ctx = seg.ctx
    n = _frames(sr)
    tile, group = ctx.resample_split_geometry(sr, 1)
    assert (tile, group) == (1024, 1) and NOUT > 3 * tile
    if sr == 44100:
        assert R.plan(sr)[:2] == (160, 441) and R.plan(sr)[2].size == 8821
    x = wavgen.encode(wavgen.make_signal(n, ch, 300 + ch), fmt)
    raw = wavgen.as_read(x, fmt)
    sched = _schedule(sr, n, ch, tile)
    got = _sched_direct(ctx, raw, sr, _native.RS_FORMAT[raw.dtype], sched)
    assert not np.array_equal(got, R.resample_ref(raw, sr))                    # the schedule is not the plain downmix


@pytest.mark.parametrize('sr,ch', [(8000, 2), (44100, 3)])
def test_two_thousand_short_runs(seg, sr, ch):
    """A seeded schedule of 2 000 runs of 1 to 3 frames from frame 40 on: every tile searches its frames' runs one by one."""
    n = _frames(sr)
    rng = np.random.default_rng(310 + ch)
    begins = 40 + np.concatenate(([0], np.cumsum(rng.integers(1, 4, 1999))))
    pool = [None] + _mixes(ch)
    picks = rng.integers(0, len(pool), begins.size + 1)
    sched = Schedule([(0, pool[picks[-1]])] + [(int(b), pool[k]) for b, k in zip(begins, picks)])
    assert len(sched) == 2001 and (sr != 8000 or begins[-1] >= n)               # at 8 kHz the runs pass the end of the file
    x = wavgen.encode(wavgen.make_signal(n, ch, 311), 'i16')
    _sched_direct(seg.ctx, x, sr, _native.RS_FORMAT[x.dtype], sched)


@pytest.mark.parametrize('container,kind,big', [('wav', 'ulaw', False), ('aiff', 'i16', True)])
def test_ext_instantiation(seg, tmp_path, container, kind, big):
    """mu-law bytes and big-endian AIFF: the formats behind the default case of the EXT instantiation."""
    sr = 8000
    n = _frames(sr)
    path = sndgen.write(tmp_path / f'e.{container}', container, kind, big, wavgen.make_signal(n, 2, 320), sr)[0]
    snd = sndfmt.parse(open(path, 'rb').read(), path)
    raw, fmt = snd.raw()
    assert fmt > 4
    _sched_direct(seg.ctx, raw, sr, fmt, _schedule(sr, n, 2, 1024), snd.stored())


# ------------------------------------------------------------------------------------------------ identities, on the device
@pytest.mark.parametrize('sr,fmt,ch', [(44100, 'i16', 2), (48000, 'f32', 3), (16000, 'i16', 2)])
def test_identities_on_the_device(seg, sr, fmt, ch):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(_frames(sr), ch, 330), fmt)
    code = _native.RS_FORMAT[x.dtype]
    got = _sched_direct(ctx, x, sr, code, Schedule([(0, None)]))
    n = ctx.resample_signal(x, sr)
    np.testing.assert_array_equal(got, ctx.get_signal_pcm16(0, n))              # [(0, None)]: the plain call's output
    mix = _mixes(ch)[2]
    got = _sched_direct(ctx, x, sr, code, Schedule([(0, mix)]))
    job = ctx.resample_job(x, sr, 0, 0)
    ctx.resample(x.reshape(-1).view(np.uint8), [job], n_signal=_hop(n), mixes=[(_hop(n), [mix])])
    np.testing.assert_array_equal(got, ctx.get_signal_pcm16(0, n))              # [(0, mix)]: the mix call's
    np.testing.assert_array_equal(got, R.mix_ref(x, sr, mix))


# ------------------------------------------------------------------------------------------------ one launch for unlike jobs
def test_four_unlike_jobs_in_one_launch(seg):
    ctx = seg.ctx
    srs, chs = (44100, 8000, 48000, 8000), (2, 3, 2, 1)
    xs = [wavgen.encode(wavgen.make_signal(_frames(sr), ch, 340 + k), 'i16') for k, (sr, ch) in enumerate(zip(srs, chs))]
    scheds = [Schedule([(0, None)]), Schedule([(0, _mixes(3)[2])]), _schedule(48000, _frames(48000), 2, 1024), Schedule([(0, None)])]
    jobs, parts, bpos = [], [], 0
    for k, (x, sr) in enumerate(zip(xs, srs)):
        jobs.append(ctx.resample_job(x, sr, bpos, k * _hop(NOUT)))
        parts += [x.reshape(-1).view(np.uint8), np.zeros(-x.nbytes % 16, dtype=np.uint8)]
        bpos += x.nbytes + (-x.nbytes % 16)
    before = ctx.resample_stats()
    ctx.resample_sched(np.concatenate(parts), jobs, scheds, n_signal=4 * _hop(NOUT))
    sig = ctx.get_signal_pcm16(0, 4 * _hop(NOUT))
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 4)              # one launch, four jobs
    for k, (x, sr, s) in enumerate(zip(xs, srs, scheds)):
        np.testing.assert_array_equal(sig[k * _hop(NOUT):k * _hop(NOUT) + NOUT], R.schedule_ref(x, sr, s), err_msg=f'job {k}')
        assert not sig[k * _hop(NOUT) + NOUT:(k + 1) * _hop(NOUT)].any()
    np.testing.assert_array_equal(sig[:NOUT], R.resample_ref(xs[0], srs[0]))
    np.testing.assert_array_equal(sig[3 * _hop(NOUT):3 * _hop(NOUT) + NOUT], R.resample_ref(xs[3], srs[3]))      # the one-channel file


# ------------------------------------------------------------------------------------------------ planner refusals
def test_planner_refusals(seg):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(3000, 2, 350), 'i16')
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, 44100, 0, 0)
    nout = job[-1]
    one = Mix(((0, 1.0),), 1.0)
    ctx.survey(src, [(0, 3000, 2, 1, 1.0)])                                     # a payload for the staged entry point
    payload = ctx.staged_payload(None)
    before = ctx.resample_stats(), ctx.survey_stats(), ctx.upload_stats()

    def tables(scheds, runs, mixes=(), terms=()):
        return tuple(np.array(list(rows), dtype=dt).reshape(-1) if len(rows) else np.zeros(0, dtype=dt)
                     for rows, dt in ((scheds, _native.SCHED), (runs, _native.SCHED_RUN), (mixes, _native.MIX), (terms, _native.MIX_TERM)))

    def refused(match, scheds, code='ISS_EINVAL', **kw):
        with pytest.raises(_native.NativeError, match=match):
            ctx.resample_sched(src, [job], scheds, n_signal=_hop(nout), **kw)
        with pytest.raises(_native.NativeError, match=match):
            ctx.resample_staged_sched(None, payload, [job], scheds, n_signal=_hop(nout), **kw)

    refused(r'job 0: run rows \[0, \+0\)', tables([(0, 0)], [(0, -1, 0)]))
    refused(r'job 0: run rows \[0, \+-1\)', tables([(0, -1)], [(0, -1, 0)]))
    refused(r'job 0: run rows \[0, \+1048577\)', tables([(0, (1 << 20) + 1)], [(k, -1, 0) for k in range((1 << 20) + 1)]))
    refused(r'job 0: run rows \[1, \+2\) outside the 2', tables([(1, 2)], [(0, -1, 0), (5, -1, 0)]))
    refused(r'job 0: run 0 begins at frame 3, not 0', tables([(0, 1)], [(3, -1, 0)]))
    refused(r'job 0: run 0 begins at frame -1, not 0', tables([(0, 2)], [(-1, -1, 0), (0, -1, 0)]))
    refused(r'job 0: run 2 begins at frame 7, run 1 at 7: begins ascend strictly', tables([(0, 3)], [(0, -1, 0), (7, -1, 0), (7, -1, 0)]))
    refused(r'job 0: run 1 begins at frame 4, run 0 at 0: begins ascend strictly|job 0: run 2 begins at frame 3, run 1 at 4',
            tables([(0, 3)], [(0, -1, 0), (4, -1, 0), (3, -1, 0)]))
    refused(r'job 0: run 1: mix 1 outside \[-1, 1\)', tables([(0, 2)], [(0, 0, 0), (9, 1, 0)], [(0, 1, 1.0)], [(0, 0, 1.0)]))
    refused(r'job 0: run 0: mix -2 outside \[-1, 0\)', tables([(0, 1)], [(0, -2, 0)]))
    refused(r'windows passed with a schedule', [[(0, None)]], windows=[(0, 3000, 3000, 0, nout)])
    # everything the mix call refuses of a mix a run names
    refused(r'job 0: mix 0: term rows \[0, \+2\) outside the 1', tables([(0, 1)], [(0, 0, 0)], [(0, 2, 1.0)], [(0, 0, 1.0)]))
    refused(r'job 0: mix 0: term 1: channel 2 of 2', [[(0, None), (5, Mix(((1, 1.0), (2, 1.0)), 1.0))]])
    refused(r'job 0: mix 0: term 0: weight -?nan', [[(0, Mix(((0, float('nan')),), 1.0))]])
    refused(r'job 0: mix 1: divisor 0', [[(0, one), (5, Mix(((0, 1.0),), 0.0))]])
    # ... and of a job
    with pytest.raises(_native.NativeError, match=r'job 0: frames_out'):
        ctx.resample_sched(src, [job[:-1] + (nout + 1,)], [[(0, None)]], n_signal=_hop(nout) + 160)
    with pytest.raises(_native.NativeError, match=r'job 0: output \[0, %d\) outside the %d-sample signal' % (nout, nout - 1)):
        ctx.resample_sched(src, [job], [[(0, None)]], n_signal=nout - 1)
    with pytest.raises(ValueError, match='2 schedules for 1 jobs'):
        ctx.resample_sched(src, [job], [[(0, None)], [(0, None)]], n_signal=_hop(nout))
    # ISS_ESTATE as the staged mix call: a payload that is not the one the origin holds, an origin that holds none
    with pytest.raises(_native.NativeError, match=r'iss_resample_staged_sched: origin survey: payload %d has been replaced' % (payload - 1)):
        ctx.resample_staged_sched(None, payload - 1, [job], [[(0, None)]], n_signal=_hop(nout))
    with pytest.raises(_native.NativeError, match=r'iss_resample_staged_sched: job 0: no job of the last iss_survey held'):
        ctx.resample_staged_sched(None, payload, [job[:1] + (2999,) + job[2:]], [[(0, None)]], n_signal=_hop(nout))
    assert (ctx.resample_stats(), ctx.survey_stats(), ctx.upload_stats()) == before      # nothing launched, nothing uploaded
    ctx.resample_staged_sched(None, payload, [job], [[(0, None), (1000, one)]], n_signal=_hop(nout))      # the payload is still good
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, nout), R.schedule_ref(x, 44100, [(0, None), (1000, one)]))
    assert ctx.upload_stats() == before[2]
    fresh = _native.Context()
    try:
        with pytest.raises(_native.NativeError, match=r'iss_resample_staged_sched: origin flac holds no payload'):
            fresh.resample_staged_sched('flac', 1, [job[:4] + (fresh.resample_filter(44100)[0],) + job[5:]], [[(0, None)]], n_signal=_hop(nout))
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ through the Segmenter
def _stats(ctx):
    return ctx.flac_stats()[0], ctx.adpcm_stats()[0], ctx.msadpcm_stats()[0], ctx.survey_stats()[0], ctx.resample_stats()[0], ctx.upload_stats()[0]


def _coded(d, what, x, sr):
    if what == 'flac':
        return flacgen.write(d / 'a.flac', np.round(x * 32767).astype(np.int64), sr, 16, blocksize=1152, channel_mode='left_side',
                             subframe={'type': 'fixed', 'order': 2})
    if what == 'ima':
        return sndgen.write(d / 'a_ima.wav', 'wav', 'ima', False, x, sr, block_align=256)[0]
    if what == 'ms':
        return msadpcmgen.write(d / 'a_ms.wav', x, sr, 256)[0]
    return wavgen.write_wav(d / 'a.wav', wavgen.encode(x, 'i16'), sr, 'i16')


SPEC = [(0, None), (0.05, {0: 1, 1: -1}), (0.1, [1]), (0.1001, None), (0.15, {0: 1, 1: -1}), (0.2, [0, 1])]


@pytest.mark.parametrize('what,launches', [('wav', (0, 0, 0, 0, 1, 1)), ('flac', (1, 0, 0, 0, 1, 1)), ('ima', (0, 1, 0, 0, 1, 1)),
                                           ('ms', (0, 0, 1, 0, 1, 1))])
def test_load_pcm_schedule(seg, tmp_path, what, launches):
    """Coded files ride on what their decode call staged: one upload, one decode launch, one resample launch, no survey."""
    sr = 8000
    path = _coded(tmp_path, what, wavgen.make_signal(_frames(sr), 2, 360, peak=0.5), sr)
    want = iss_io.decode_schedule(path, SPEC)
    stored, _ = iss_io.decode_source(path)
    np.testing.assert_array_equal(want, R.schedule_ref(stored, sr, R.normalise_schedule(SPEC, sr, 2)))
    before = _stats(seg.ctx)
    got = seg.load_pcm_schedule(path, SPEC)
    after = _stats(seg.ctx)
    assert tuple(b - a for a, b in zip(before, after)) == launches
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(seg.load_pcm_schedule(path, [(0, None)]), seg.load_pcm(path))
    np.testing.assert_array_equal(seg.load_pcm_schedule(path, [(0, {0: 1, 1: -1})]), seg.load_pcm_mixes(path, [{0: 1, 1: -1}])[0])


def test_segment_schedule_is_segment_signal_of_the_scheduled_pcm(seg, tmp_path):
    from conftest import synth_pcm
    a = synth_pcm(1, 3 * 16000).astype(np.float64) / 32768
    x = np.stack([a, a], axis=1)
    x[16000:32000, 1] *= -1                                                      # one second out of phase
    path = wavgen.write_wav(tmp_path / 's.wav', wavgen.encode(x, 'i16'), 16000, 'i16')
    spec = [(0, None), (1.0, Mix(((0, 1.0), (1, -1.0)), 2.0)), (2.0, None)]
    pcm = seg.load_pcm_schedule(path, spec)
    np.testing.assert_array_equal(pcm, wavgen.encode(a, 'i16'))                   # the inverted second turned back
    assert not seg.load_pcm(path)[16000:32000].any()                              # ... which the plain downmix cancels
    assert seg.segment_schedule(path, spec) == seg.segment_signal(pcm)


def test_schedule_errors_through_the_segmenter(seg, tmp_path):
    x = wavgen.encode(wavgen.make_signal(4000, 2, 370), 'i16')
    path = wavgen.write_wav(tmp_path / 'e.wav', x, 8000, 'i16')
    with pytest.raises(ValueError, match='run 1.*channel 2 is outside'):
        seg.load_pcm_schedule(path, [(0, None), (0.1, [2])])
    with pytest.raises(ValueError, match='of a set are not supported'):
        seg.load_pcm_schedule((path, path), [(0, None)])
    np.testing.assert_array_equal(seg.load_pcm_schedule(path, [(0, None)]), seg.load_pcm(path))      # and the context still works
