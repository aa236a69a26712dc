"""GPU: schedules whose runs cross-fade in (include/iss.h, "Fades") -- the FADE instantiations of resample_kernel through
ctx.resample_sched / ctx.resample_staged_sched and the Segmenter's steady timeline route, everything bit-equal to
resample.schedule_ref.  Shapes as tests/test_gpu_schedule.py sizes them: three tiles of output and a ragged tail (about 3 300
outputs).  Zones are placed against the tile geometry: inside one tile's span, starting at the first staged frame of tile 1 and
either neighbour, across the frame under tile 1's first output, wider than a whole tile's span (first and last frame one run,
and still blended), from frame 0, past the last frame, for a run that begins past the end, touching, of two frames, and 200 runs
of 40 frames that leave no frame outside a zone."""
import filecmp
import os

import numpy as np
import pytest

import autocases
import flacgen
import msadpcmgen
import sndgen
import timelinecases as TC
import wavgen
from inaspeechsegmenter_amd import _native, Segmenter, pipeline, sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.export_funcs import seg2csv
from inaspeechsegmenter_amd.resample import Mix, Schedule

pytestmark = pytest.mark.gpu

NOUT = 3 * 1024 + 230                                  # three tiles of 1 024 outputs and a ragged tail
TILE = 1024


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


def _span(sr, t):
    """(first, last) staged frame of output tile t of a file of NOUT outputs at sr: resample.hip's s0 and s1."""
    up, down, h = R.plan(sr)
    hl = (h.size - 1) // 2
    return (t * TILE * down - hl) // up, ((min((t + 1) * TILE, NOUT) - 1) * down + hl) // up


def _faded(ch, zones):
    """[(begin, half)] -> a Schedule: run 0 and the runs beginning there, cycling through a mix, no mix, two other mixes."""
    a, b, c = _mixes(ch)
    cycle = [None, a, c, b]
    return Schedule([(0, b)] + [(beg, cycle[k % 4]) for k, (beg, _) in enumerate(zones)], [0] + [h for _, h in zones])


def _placements(sr, n, ch):
    """name -> Schedule: the zone placements of the module's docstring for a file of n frames at sr."""
    up, down, h = R.plan(sr)
    reach = max(1, (h.size - 1) // 2 // up)                                        # the filter's half length in frames
    (a0, _), (b0, b1), (c0, _) = _span(sr, 0), _span(sr, 1), _span(sr, 2)
    edge = TILE * down // up                                                      # the frame under tile 1's first output
    t1 = edge + 4 * reach + 60
    assert t1 + 75 < c0                                                           # (Schedule itself refuses zones that overlap)
    out = {
        # two frames; inside tile 0's span; across the frame under tile 1's first output; two touching zones; tile 2 and the tail clear
        'places': _faded(ch, [(5, 1), (b0 // 2, 8), (edge, reach + 3), (t1, 25), (t1 + 50, 25)]),
        # tile 1's span lies in run 0 from its first frame to its last, and all of it in run 1's zone
        'wide': _faded(ch, [(b1 + 10, b1 + 15 - b0)]),
        'from0': _faded(ch, [(37, 37), (n // 2, 1)]),
        'past_end': _faded(ch, [(n - 10, 30)]),                                   # ... and every tile before it between zones
        'begins_past_end': _faded(ch, [(n + 5, 40)]),
        'all_zone': Schedule([(40 * k, _mixes(ch)[k % 3] if k % 4 else None) for k in range(200)], [0] + [20] * 199),
    }
    for d in (-1, 0, 1):                                                          # zones that start at tile 1's first staged frame +- 1
        out[f'tile1{d:+d}'] = _faded(ch, [(b0 + d + 12, 12), (n - 3, 2)])
    assert b1 + 10 - (b1 + 15 - b0) == b0 - 5 >= max(a0, 0)                       # (the wide zone begins five frames before tile 1 stages)
    return out


PLACES = ['places', 'wide', 'from0', 'past_end', 'begins_past_end', 'all_zone', 'tile1-1', 'tile1+0', 'tile1+1']


def _direct(ctx, raw, sr, fmt, schedule, stored=None, **kw):
    """One scheduled job on its own, checked against schedule_ref of `stored` (what the host reads for `raw`) -> the output."""
    stored = raw if stored is None else stored
    job = ctx.resample_job(raw, sr, 0, 0, fmt)
    nout = job[-1]
    before = ctx.resample_stats()
    ctx.resample_sched(raw.reshape(-1).view(np.uint8), [job], [schedule], n_signal=_hop(nout), **kw)
    sig = ctx.get_signal_pcm16(0, _hop(nout))
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)
    np.testing.assert_array_equal(sig[:nout], R.schedule_ref(stored, sr, schedule))
    assert not sig[nout:].any()
    return sig[:nout]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('place', PLACES)
@pytest.mark.parametrize('sr,fmt,ch', [(8000, 'i16', 2), (48000, 'i24', 3), (44100, 'f32', 2), (16000, 'i16', 8)])
def test_zones_against_the_tile_geometry(seg, sr, fmt, ch, place):
    ctx = seg.ctx
    n = _frames(sr)
    assert ctx.resample_split_geometry(sr, 1) == (TILE, 1) and NOUT > 3 * TILE
    x = wavgen.encode(wavgen.make_signal(n, ch, 500 + ch), fmt)
    raw = wavgen.as_read(x, fmt)
    sched = _placements(sr, n, ch)[place]
    assert sched.faded
    got = _direct(ctx, raw, sr, _native.RS_FORMAT[raw.dtype], sched)
    hard = R.schedule_ref(raw, sr, Schedule(sched.runs))
    assert not np.array_equal(got, hard)                                          # the fades are not hard cuts


@pytest.mark.parametrize('container,kind,big', [('wav', 'ulaw', False), ('aiff', 'i16', True)])
def test_ext_instantiation(seg, tmp_path, container, kind, big):
    """mu-law bytes and big-endian AIFF: the formats behind the default case of the EXT instantiation."""
    sr = 8000
    n = _frames(sr)
    path = sndgen.write(tmp_path / f'e.{container}', container, kind, big, wavgen.make_signal(n, 2, 520), sr)[0]
    snd = sndfmt.parse(open(path, 'rb').read(), path)
    raw, fmt = snd.raw()
    assert fmt > 4
    for place in ('places', 'wide'):
        _direct(seg.ctx, raw, sr, fmt, _placements(sr, n, 2)[place], snd.stored())


# ------------------------------------------------------------------------------------------------ identities, on the device
@pytest.mark.parametrize('sr,fmt,ch', [(44100, 'i16', 2), (48000, 'f32', 3)])
def test_identities_on_the_device(seg, sr, fmt, ch):
    ctx = seg.ctx
    n = _frames(sr)
    x = wavgen.encode(wavgen.make_signal(n, ch, 530), fmt)
    code = _native.RS_FORMAT[x.dtype]
    sched = _placements(sr, n, ch)['places']
    hard = Schedule(sched.runs)
    job = ctx.resample_job(x, sr, 0, 0, code)
    ctx.resample_sched(x.reshape(-1).view(np.uint8), [job], [hard], n_signal=_hop(NOUT))      # iss_resample_pcm16_sched
    want = ctx.get_signal_pcm16(0, NOUT)
    got = _direct(ctx, x, sr, code, hard, fades=np.zeros(len(hard), dtype=np.int32))           # ..._sched_fade, every half-width 0
    np.testing.assert_array_equal(got, want)
    # equal mixes either side of a boundary: as if there were no boundary, whatever the fade
    a, b, _ = _mixes(ch)
    same = Mix(a.terms, a.divisor)
    got = _direct(ctx, x, sr, code, Schedule([(0, a), (n // 3, same), (n // 2, b), (n // 2 + 400, Mix(b.terms, b.divisor))], [0, 300, 0, 77]))
    ctx.resample_sched(x.reshape(-1).view(np.uint8), [job], [[(0, a), (n // 2, b)]], n_signal=_hop(NOUT))
    np.testing.assert_array_equal(got, ctx.get_signal_pcm16(0, NOUT))


# ------------------------------------------------------------------------------------------------ one launch for unlike jobs
def test_four_unlike_jobs_in_one_launch(seg):
    ctx = seg.ctx
    srs, chs = (44100, 8000, 48000, 8000), (2, 3, 2, 1)
    xs = [wavgen.encode(wavgen.make_signal(_frames(sr), ch, 540 + k), 'i16') for k, (sr, ch) in enumerate(zip(srs, chs))]
    scheds = [_placements(44100, _frames(44100), 2)['wide'], Schedule([(0, _mixes(3)[2]), (700, None), (900, _mixes(3)[0])]),
              _placements(48000, _frames(48000), 2)['places'], Schedule([(0, None), (800, Mix(((0, 0.5),), 1.0))], [0, 300])]
    assert [s.faded for s in scheds] == [True, False, True, True]                  # one job of the four has no fade
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


# ------------------------------------------------------------------------------------------------ planner refusals
def test_planner_refusals(seg):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(3000, 2, 550), 'i16')
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, 44100, 0, 0)
    nout = job[-1]
    ctx.survey(src, [(0, 3000, 2, 1, 1.0)])                                     # a payload for the staged entry point
    payload = ctx.staged_payload(None)
    before = ctx.resample_stats(), ctx.survey_stats(), ctx.upload_stats()

    def tables(scheds, runs, mixes=(), terms=()):
        return tuple(np.array(list(rows), dtype=dt).reshape(-1) if len(rows) else np.zeros(0, dtype=dt)
                     for rows, dt in ((scheds, _native.SCHED), (runs, _native.SCHED_RUN), (mixes, _native.MIX), (terms, _native.MIX_TERM)))

    def refused(match, scheds, fades, **kw):
        with pytest.raises(_native.NativeError, match='iss_resample_pcm16_sched_fade: ' + match):
            ctx.resample_sched(src, [job], scheds, n_signal=_hop(nout), fades=fades, **kw)
        with pytest.raises(_native.NativeError, match='iss_resample_staged_sched_fade: ' + match):
            ctx.resample_staged_sched(None, payload, [job], scheds, n_signal=_hop(nout), fades=fades, **kw)

    three = tables([(0, 3)], [(0, -1, 0), (100, -1, 0), (200, -1, 0)])
    refused(r'job 0: run 2: fade half-width -1 is negative', three, [0, 5, -1])
    refused(r'job 0: run 0: fade half-width 3: the first run has nothing to fade from', three, [3, 0, 0])
    refused(r'job 0: run 2: its fade zone, 50 frames either side of frame 200, overlaps that of run 1, 51 frames either side of frame 100',
            three, [0, 51, 50])
    refused(r'job 0: run 1: its fade zone, 101 frames either side of frame 100, overlaps that of run 0', three, [0, 101, 0])
    # ... and what the twin refuses, under the new names
    refused(r'job 0: run 2 begins at frame 7, run 1 at 7: begins ascend strictly', tables([(0, 3)], [(0, -1, 0), (7, -1, 0), (7, -1, 0)]), [0, 0, 0])
    refused(r'job 0: run 1: mix 1 outside \[-1, 1\)', tables([(0, 2)], [(0, 0, 0), (9, 1, 0)], [(0, 1, 1.0)], [(0, 0, 1.0)]), [0, 2])
    refused(r'windows passed with a schedule', [[(0, None)]], [0], windows=[(0, 3000, 3000, 0, nout)])
    with pytest.raises(ValueError, match='2 fades for 3 runs'):
        ctx.resample_sched(src, [job], three, n_signal=_hop(nout), fades=[0, 1])
    assert (ctx.resample_stats(), ctx.survey_stats(), ctx.upload_stats()) == before      # nothing launched, nothing uploaded
    sched = Schedule([(0, None), (100, Mix(((0, 1.0),), 1.0)), (200, None)], [0, 50, 50])       # touching zones are no overlap
    ctx.resample_staged_sched(None, payload, [job], [sched], n_signal=_hop(nout))               # the payload is still good
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, nout), R.schedule_ref(x, 44100, sched))
    assert ctx.upload_stats() == before[2]


# ------------------------------------------------------------------------------------------------ coded files, over what was staged
def _coded(d, what, x, sr):
    if what == 'flac':
        return flacgen.write(d / 'a.flac', np.round(x * 32767).astype(np.int64), sr, 16, blocksize=1152, channel_mode='left_side',
                             subframe={'type': 'fixed', 'order': 2})
    if what == 'ima':
        return sndgen.write(d / 'a_ima.wav', 'wav', 'ima', False, x, sr, block_align=256)[0]
    if what == 'ms':
        return msadpcmgen.write(d / 'a_ms.wav', x, sr, 256)[0]
    return wavgen.write_wav(d / 'a.wav', wavgen.encode(x, 'i16'), sr, 'i16')


def _stats(ctx):
    return ctx.flac_stats()[0], ctx.adpcm_stats()[0], ctx.msadpcm_stats()[0], ctx.survey_stats()[0], ctx.resample_stats()[0], ctx.upload_stats()[0]


SPEC = [(0, None), (0.05, {0: 1, 1: -1}), (0.1, [1]), (0.1001, None), (0.15, {0: 1, 1: -1}), (0.2, [0, 1])]


@pytest.mark.parametrize('what,launches', [('wav', (0, 0, 0, 0, 1, 1)), ('flac', (1, 0, 0, 0, 1, 1)), ('ima', (0, 1, 0, 0, 1, 1)),
                                           ('ms', (0, 0, 1, 0, 1, 1))])
def test_load_pcm_schedule_with_fades(seg, tmp_path, what, launches):
    """Coded files ride on what their decode call staged (iss_resample_staged_sched_fade): one upload, one decode launch, one
    resample launch, no survey."""
    sr = 8000
    path = _coded(tmp_path, what, wavgen.make_signal(_frames(sr), 2, 560, peak=0.5), sr)
    stored, _ = iss_io.decode_source(path)
    sched = R.normalise_schedule(SPEC, sr, 2, fade_sec=0.02)
    assert sched.fades == (0, 80, 0, 0, 80, 80)                                   # a run of one frame has nothing to give
    want = iss_io.decode_schedule(path, SPEC, fade_sec=0.02)
    np.testing.assert_array_equal(want, R.schedule_ref(stored, sr, sched))
    before = _stats(seg.ctx)
    got = seg.load_pcm_schedule(path, SPEC, fade_sec=0.02)
    assert tuple(b - a for a, b in zip(before, _stats(seg.ctx))) == launches
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(seg.load_pcm_schedule(path, sched), want)       # ... and a Schedule with its own half-widths
    assert not np.array_equal(got, seg.load_pcm_schedule(path, SPEC))


def test_segment_schedule_is_segment_signal_of_the_faded_pcm(seg, tmp_path):
    from conftest import synth_pcm
    a = synth_pcm(1, 3 * 16000).astype(np.float64) / 32768
    x = np.stack([a, a], axis=1)
    x[16000:32000, 1] *= -1                                                      # one second out of phase
    path = wavgen.write_wav(tmp_path / 's.wav', wavgen.encode(x, 'i16'), 16000, 'i16')
    spec = [(0, None), (1.0, Mix(((0, 1.0), (1, -1.0)), 2.0)), (2.0, None)]
    pcm = seg.load_pcm_schedule(path, spec, fade_sec=0.05)
    np.testing.assert_array_equal(pcm, iss_io.decode_schedule(path, spec, fade_sec=0.05))
    want = wavgen.encode(a, 'i16')
    zones = np.r_[15600:16400, 31600:32400]                                       # 400 frames either side of a begin
    assert not np.array_equal(pcm[zones], want[zones])                            # where both mixes are wrong by halves
    np.testing.assert_array_equal(np.delete(pcm, zones), np.delete(want, zones))  # the inverted second turned back
    assert seg.segment_schedule(path, spec, fade_sec=0.05) == seg.segment_signal(pcm)


# ------------------------------------------------------------------------------------------------ the steady rule, end to end
def _five(dead_channel=False):
    """tests/test_fades.py's fixture: five blocks, R = L, -1.2 L, -0.8 L, 0, L; with a channel of zeros between them on request."""
    rng = np.random.default_rng(5)
    left = rng.uniform(-0.1, 0.1, 5 * TC.B)
    right = left.copy()
    right[TC.B:2 * TC.B] *= -1.2
    right[2 * TC.B:3 * TC.B] *= -0.8
    right[3 * TC.B:4 * TC.B] = 0
    chans = [left, np.zeros_like(left), right] if dead_channel else [left, right]
    return wavgen.encode(np.stack(chans, axis=1), 'i16')


def _counters(ctx):
    return {'upload': ctx.upload_stats(), 'survey': ctx.survey_stats()[0], 'resample': ctx.resample_stats()[0],
            'flac': ctx.flac_stats()[0], 'adpcm': ctx.adpcm_stats()[0], 'msadpcm': ctx.msadpcm_stats()[0]}


def _grown(ctx, before):
    now = _counters(ctx)
    return {k: (now[k][0] - before[k][0], now[k][1] - before[k][1]) if k == 'upload' else now[k] - before[k] for k in now}


@pytest.mark.parametrize('kind,coder', [('i16', None), ('flac', 'flac'), ('ima', 'adpcm')])
@pytest.mark.parametrize('fixture', ['stored', 'five', 'five3'])
def test_steady_rule_end_to_end(seg, tmp_path, fixture, kind, coder):
    x = {'stored': TC.stored, 'five': _five, 'five3': lambda: _five(True)}[fixture]()
    path = TC.write(tmp_path / f'f.{kind}', kind, x)
    nbytes = iss_io.timeline_source(path, TC.BLOCK_SEC, True).payload.size
    before = _counters(seg.ctx)
    pcm, timeline, schedule = seg.load_pcm_auto_timeline(path, TC.BLOCK_SEC, rule='steady')
    got = _grown(seg.ctx, before)
    want = {'upload': (1, nbytes), 'survey': 1, 'resample': 1, 'flac': 0, 'adpcm': 0, 'msadpcm': 0}
    if coder:
        want[coder] = 1
    assert got == want                                                          # one payload copy, one survey launch, one resample launch
    host = iss_io.decode_auto_timeline(path, TC.BLOCK_SEC, rule='steady')
    assert timeline == host[1] and schedule == host[2] == timeline.steady_schedule() and schedule.faded
    np.testing.assert_array_equal(pcm, host[0])
    if kind != 'ima' and fixture == 'five':
        assert schedule == Schedule([(0, None), (8192, Mix(((0, 1.0), (1, -1.0)), 2.0)), (32768, None)], [0, 200, 200])
    before = _counters(seg.ctx)
    segments, t2, s2 = seg.segment_auto_timeline(path, TC.BLOCK_SEC, rule='steady')
    assert _grown(seg.ctx, before) == want
    assert t2 == timeline and s2 == schedule and segments == seg.segment_signal(pcm)
    cut = seg.load_pcm_auto_timeline(path, TC.BLOCK_SEC, rule='steady', fade_sec=0)
    assert cut[2] == timeline.steady_schedule(0) and not np.array_equal(cut[0], pcm)
    np.testing.assert_array_equal(cut[0], iss_io.decode_auto_timeline(path, TC.BLOCK_SEC, rule='steady', fade_sec=0)[0])


def test_one_steady_pass_of_mixed_classes(seg, tmp_path, monkeypatch):
    d = tmp_path
    files = [TC.write(d / 'five.wav', 'i16', _five()), TC.write(d / 'ok.wav', 'i16', TC.healthy()), TC.write(d / 'fault.flac', 'flac'),
             TC.write(d / 'five3.flac', 'flac', _five(True)), TC.write(d / 'five_ima.wav', 'ima', _five()), autocases.write(d / 'm.wav', 'mono', 8000, n=9000)]
    outs = [str(d / 'out' / (os.path.basename(f) + '.csv')) for f in files]
    passes = []
    run = pipeline._Worker.run

    def counted(self, batch):
        before = _counters(self.ctx)
        out = run(self, batch)
        passes.append(_grown(self.ctx, before))
        return out
    monkeypatch.setattr(pipeline._Worker, 'run', counted)
    decisions = []
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='auto', auto_block_sec=1.0, auto_rule='steady', auto_fade_sec=0.03, decisions=decisions)
    monkeypatch.setattr(pipeline._Worker, 'run', run)
    assert [m[1] for m in lmsg] == [0] * 6 and nb == 6, lmsg
    assert len(passes) == 1 and {k: v for k, v in passes[0].items() if k != 'upload'} == {
        'survey': 3, 'resample': 4, 'flac': 1, 'adpcm': 1, 'msadpcm': 0}, passes       # (the mono file: a plain resample launch of its own)
    by = {dec[0]: dec for dec in decisions}
    for f, o in zip(files, outs):
        segments, timeline, schedule = seg.segment_auto_timeline(f, 1.0, rule='steady', fade_sec=0.03)
        seg2csv(segments, str(d / 'alone.csv'))
        assert filecmp.cmp(o, str(d / 'alone.csv'), shallow=False), f
        assert by[f][1] == timeline and by[f][2] == schedule, f
    assert by[files[0]][2].fades == (0, 120, 120) and by[files[1]][2] == [(0, None)] and by[files[5]][2] is None
