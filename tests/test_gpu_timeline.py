"""GPU: surveys resolved in time, and the downmix they decide.  survey_reduce_blocks_kernel through ctx.survey_blocks against
resample.survey_ref block by block, the whole-file rows against the unblocked call's bytes; the three coded origins; the fault
fixture (timelinecases.py) end to end with its uploads and launches counted; one batch_process pass of six files of three source
classes.  Every comparison is exact."""
import filecmp
import os

import numpy as np
import pytest

import autocases
import timelinecases as TC
from inaspeechsegmenter_amd import Segmenter, pipeline
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.export_funcs import seg2csv
from inaspeechsegmenter_amd.survey import ChannelSurvey

pytestmark = pytest.mark.gpu

FULL = 32767 / 32768


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _same(got, want):
    return ChannelSurvey(got, 8000, 0) == ChannelSurvey(want, 8000, 0)


# ------------------------------------------------------------------------------------------------ block rows
def test_block_rows_of_many_jobs_in_one_call(seg):
    """K = 1, 2, 3; n a multiple of B, one more, one less, below one chunk, and 1; 1, 2, 16 and 17 channels (no pair sums): fifteen
    jobs with different K in ONE call."""
    ctx = seg.ctx
    rng = np.random.default_rng(500)
    jobs, ks, xs, parts, bpos = [], [], [], [], 0
    chans = [1, 2, 16, 17]
    for K in (1, 2, 3):
        per = K * 1024
        for n in (2 * per, 2 * per + 1, 2 * per - 1, 500, 1):
            ch = chans[len(jobs) % 4]
            x = rng.integers(-20000, 20000, (n, ch)).astype('<i2')
            x[rng.integers(0, n, n // 7 + 1), rng.integers(0, ch, n // 7 + 1)] = 0
            x[0, 0] = 32767
            jobs.append((bpos, n, ch, 1, FULL)); ks.append(K); xs.append(x)
            parts += [x.reshape(-1).view(np.uint8), np.zeros(-x.nbytes % 16, dtype=np.uint8)]
            bpos += x.nbytes + (-x.nbytes % 16)
    assert len(jobs) == 15 and {j[2] for j in jobs} == set(chans)
    src = np.concatenate(parts)
    before = ctx.survey_stats(), ctx.upload_stats()
    whole, blocks = ctx.survey_blocks(src, jobs, ks)
    assert (ctx.survey_stats()[0] - before[0][0], ctx.survey_stats()[1] - before[0][1]) == (1, 15)      # ONE launch of the counters
    assert ctx.upload_stats()[0] - before[1][0] == 1
    plain = ctx.survey(src, jobs)
    for k, (x, K) in enumerate(zip(xs, ks)):
        per, n = K * 1024, x.shape[0]
        assert len(blocks[k]) == -(-n // per), (k, len(blocks[k]))
        for b, got in enumerate(blocks[k]):
            want = R.survey_ref(x, FULL, b * per, min((b + 1) * per, n))
            assert got.n == want.n and _same(got, want), (k, b)
        assert _same(whole[k], plain[k]) and _same(whole[k], R.survey_ref(x, FULL)), k      # `results`: the unblocked call's


def test_block_sums_differ_from_the_whole_in_association_only(seg):
    """float32 noise, K = 1: the whole-file sums are the chunk rows in one chain from +0.0, equal to the unblocked call's to the
    bit, and the block rows ARE the chunk rows."""
    ctx = seg.ctx
    x = np.random.default_rng(501).uniform(-1, 1, (5 * 1024 + 17, 2)).astype('<f4')
    src = x.reshape(-1).view(np.uint8)
    job = [(0, x.shape[0], 2, 3, 1.0)]
    whole, blocks = ctx.survey_blocks(src, job, [1])
    assert _same(whole[0], ctx.survey(src, job)[0]) and len(blocks[0]) == 6
    acc = np.zeros(2)
    for b in blocks[0]:
        acc = acc + b.s2
    np.testing.assert_array_equal(acc, whole[0].s2)                              # six chunk rows added in ascending order


def test_refusals_launch_nothing(seg):
    from inaspeechsegmenter_amd import _native
    ctx = seg.ctx
    x = np.zeros((2000, 2), dtype='<i2')
    before = ctx.survey_stats(), ctx.upload_stats()
    with pytest.raises(_native.NativeError, match=r'iss_survey_blocks: job 1: block_chunks 0: a block holds at least one chunk'):
        ctx.survey_blocks(x.reshape(-1).view(np.uint8), [(0, 1000, 2, 1, FULL), (4000, 1000, 2, 1, FULL)], [1, 0])
    with pytest.raises(_native.NativeError, match=r'iss_survey_blocks: job 0: .*outside the 8000-byte buffer'):
        ctx.survey_blocks(x.reshape(-1).view(np.uint8), [(0, 2001, 2, 1, FULL)], [1])
    with pytest.raises(ValueError, match='2 block sizes for 1 jobs'):
        ctx.survey_blocks(x.reshape(-1).view(np.uint8), [(0, 2000, 2, 1, FULL)], [1, 1])
    assert (ctx.survey_stats(), ctx.upload_stats()) == before


# ------------------------------------------------------------------------------------------------ the fixture, end to end
def _counters(ctx):
    return {'upload': ctx.upload_stats(), 'survey': ctx.survey_stats()[0], 'resample': ctx.resample_stats()[0],
            'flac': ctx.flac_stats()[0], 'adpcm': ctx.adpcm_stats()[0], 'msadpcm': ctx.msadpcm_stats()[0]}


def _grown(ctx, before):
    now = _counters(ctx)
    return {k: (now[k][0] - before[k][0], now[k][1] - before[k][1]) if k == 'upload' else now[k] - before[k] for k in now}


@pytest.mark.parametrize('kind,coder', [('i16', None), ('flac', 'flac'), ('ima', 'adpcm')])
def test_fixture_end_to_end(seg, tmp_path, kind, coder):
    path = TC.write(tmp_path / f'f.{kind}', kind)
    stored, sr = iss_io.decode_source(path)
    nbytes = iss_io.timeline_source(path, TC.BLOCK_SEC, True).payload.size
    before = _counters(seg.ctx)
    pcm, timeline, schedule = seg.load_pcm_auto_timeline(path, TC.BLOCK_SEC)
    got = _grown(seg.ctx, before)
    want = {'upload': (1, nbytes), 'survey': 1, 'resample': 1, 'flac': 0, 'adpcm': 0, 'msadpcm': 0}
    if coder:
        want[coder] = 1
    assert got == want                                                          # one payload copy, one survey launch, one resample launch
    if kind != 'ima':
        assert schedule == TC.SCHEDULE
        np.testing.assert_array_equal(pcm, R.schedule_ref(stored, sr, TC.SCHEDULE))
        assert not seg.load_pcm(path)[2 * TC.B + 100:4 * TC.B - 100].any()        # block 1 (at 16 kHz, a filter length from its edges): the plain downmix is silence
        assert pcm[2 * TC.B + 100:4 * TC.B - 100].any()
    np.testing.assert_array_equal(pcm, R.schedule_ref(stored, sr, schedule))
    host = iss_io.survey_timeline(path, TC.BLOCK_SEC)
    assert timeline == host and schedule == host.safe_schedule() and timeline.whole == seg.survey_channels(path)
    assert seg.survey_timeline(path, TC.BLOCK_SEC) == host
    before = _counters(seg.ctx)
    segments, t2, s2 = seg.segment_auto_timeline(path, TC.BLOCK_SEC)
    assert _grown(seg.ctx, before) == want
    assert t2 == timeline and s2 == schedule and segments == seg.segment_signal(pcm)
    np.testing.assert_array_equal(seg.load_pcm_schedule(path, schedule), pcm)


def test_coded_origins_block_by_block(seg, tmp_path):
    """FLAC, IMA and Microsoft ADPCM: iss_<coder>_survey_blocks over what the decode call staged, K = 2 at 8 kHz, three channels."""
    for kind in ('flac', 'ima', 'ms'):
        path = autocases.write(tmp_path / f'a.{kind}', 'deadinv', 8000, kind, n=5 * 1024 + 300)
        got = seg.survey_timeline(path, 0.25)
        assert got.block_frames == 2048 and len(got.blocks) == 3 and got == iss_io.survey_timeline(path, 0.25), kind


def test_mono_takes_the_default_path(seg, tmp_path):
    launches = seg.ctx.survey_stats()[0]
    for kind, sr in (('i16', 16000), ('i16', 8000), ('flac', 8000), ('ima', 16000)):
        f = autocases.write(tmp_path / f'm{sr}.{kind}', 'mono', sr, kind)
        pcm, timeline, schedule = seg.load_pcm_auto_timeline(f)
        assert timeline is None and schedule is None
        np.testing.assert_array_equal(pcm, seg.load_pcm(f))
        assert seg.segment_auto_timeline(f) == (seg(f), None, None)
    assert seg.ctx.survey_stats()[0] == launches


# ------------------------------------------------------------------------------------------------ one batch_process pass
def test_one_pass_of_six_files(seg, tmp_path, monkeypatch):
    d = tmp_path
    files = [TC.write(d / 'fault.wav'), TC.write(d / 'ok.wav', 'i16', TC.healthy()), TC.write(d / 'fault.flac', 'flac'),
             TC.write(d / 'ok.flac', 'flac', TC.healthy()), TC.write(d / 'fault_ima.wav', 'ima'), TC.write(d / 'ok_ima.wav', 'ima', TC.healthy())]
    outs = [str(d / 'out' / (os.path.basename(f) + '.csv')) for f in files]
    passes = []
    run = pipeline._Worker.run

    def counted(self, batch):
        before = _counters(self.ctx)
        out = run(self, batch)
        passes.append(([type(s).__name__ for s in batch.sigs], _grown(self.ctx, before)))
        return out
    monkeypatch.setattr(pipeline._Worker, 'run', counted)
    decisions = []
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='auto', auto_block_sec=1.0, decisions=decisions)
    monkeypatch.setattr(pipeline._Worker, 'run', run)
    assert [m[1] for m in lmsg] == [0] * 6 and nb == 6 and [m[0] for m in lmsg] == outs, lmsg
    assert len(passes) == 1, passes                                             # six files, one pass, one launch of each per class
    names, grown = passes[0]
    assert sorted(names) == ['AdpcmSched', 'AdpcmSched', 'FlacSched', 'FlacSched', 'RawSched', 'RawSched']
    assert grown['upload'][0] == 3 and {k: v for k, v in grown.items() if k != 'upload'} == {
        'survey': 3, 'resample': 3, 'flac': 1, 'adpcm': 1, 'msadpcm': 0}
    by = {dec[0]: dec for dec in decisions}
    assert sorted(by) == sorted(files)
    for f, o in zip(files, outs):
        segments, timeline, schedule = seg.segment_auto_timeline(f, 1.0)
        seg2csv(segments, str(d / 'alone.csv'))
        assert filecmp.cmp(o, str(d / 'alone.csv'), shallow=False), f
        assert by[f][1] == timeline and by[f][2] == schedule, f
    assert by[files[0]][2] == TC.SCHEDULE and by[files[2]][2] == TC.SCHEDULE and len(by[files[4]][2]) > 1
    plain = [o + '.auto.csv' for o in outs]
    seg.batch_process(files, plain, channels='auto')
    for k in (1, 3, 5):                                                         # a healthy file: what plain 'auto' writes
        assert by[files[k]][2] == [(0, None)] and filecmp.cmp(outs[k], plain[k], shallow=False), files[k]
