"""CPU: surveys resolved in time and the schedules they decide.  io.survey_timeline against resample.survey_ref block by block;
the rule survey.SurveyTimeline.safe_schedule on the fault fixture (timelinecases.py), from active(), corr() and the tie rule alone;
io.decode_auto_timeline; the bytes of the per-run decisions table; the argument errors; the command line on a fake device."""
import importlib.util
import math
import os

import numpy as np
import pytest

import autocases
import timelinecases as TC
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd import survey as survey_mod
from inaspeechsegmenter_amd.resample import Mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_chunks_is_the_definition():
    assert survey_mod.DEFAULT_BLOCK_SEC == 10.0
    assert survey_mod.block_chunks(TC.BLOCK_SEC, TC.SR) == TC.K == 8 and TC.B == 8192
    assert survey_mod.block_chunks(10.0, 48000) == 469 == math.floor(10.0 * 48000 / 1024 + 0.5)
    assert survey_mod.block_chunks(10.0, 44100) == 431 and survey_mod.block_chunks(0.001, 8000) == 1
    assert survey_mod.block_chunks(0.064, 8000) == 1 and survey_mod.block_chunks(0.192, 8000) == 2      # 0.5 and 1.5 chunks: up
    for bad in (0, -1.0, float('nan'), float('inf'), None, '10', True):
        with pytest.raises(ValueError, match='block_sec='):
            survey_mod.block_chunks(bad, 8000)


@pytest.mark.parametrize('kind', ['i16', 'flac', 'ima'])
def test_timeline_twin_block_by_block(tmp_path, kind):
    path = TC.write(tmp_path / f'f.{kind}', kind)
    tl = iss_io.survey_timeline(path, TC.BLOCK_SEC)
    x, sr = iss_io.decode_source(path)
    full = R.SURVEY_FULL['ima' if kind == 'ima' else 'i16']
    assert sr == TC.SR and tl.block_frames == TC.B and len(tl.blocks) == 4 and tl.n == TC.N and tl.channels == 2
    for b, blk in enumerate(tl.blocks):
        want = survey_mod.ChannelSurvey(R.survey_ref(x, full, b * TC.B, min((b + 1) * TC.B, TC.N)), sr, b * TC.B)
        assert blk == want and blk.first == b * TC.B and blk.n == (TC.B if b < 3 else TC.B // 2)
    assert tl.whole == iss_io.survey_channels(path)
    assert tl == iss_io.survey_timeline(path, 1.02) and tl != iss_io.survey_timeline(path, 0.5)      # 1.02 s is K = 8 too
    # the whole file's sums are its chunk rows in one chain, not the block sums added up
    assert tl.whole.n == sum(b.n for b in tl.blocks) and np.array_equal(tl.whole.zeros, sum(b.zeros for b in tl.blocks))


def test_default_block_is_ten_seconds(tmp_path):
    path = TC.write(tmp_path / 'f.wav')
    tl = iss_io.survey_timeline(path)
    assert tl.block_frames == 78 * 1024 and len(tl.blocks) == 1 and tl.blocks[0] == tl.whole


def test_the_fixture_decides_from_active_corr_and_the_tie_rule(tmp_path):
    path = TC.write(tmp_path / 'f.wav')
    tl = iss_io.survey_timeline(path, TC.BLOCK_SEC)
    b0, b1, b2, b3 = tl.blocks
    assert b0.active() == [0, 1] and b0.corr(0, 1) == 1.0 and b0.safe_mix() is None
    assert b1.active() == [0, 1] and b1.corr(0, 1) == -1.0 and b1.s2[0] == b1.s2[1]      # a tie: channel 0 is the reference
    assert b1.downmix_loss_db == -math.inf
    assert b2.active() == [0] and b2.peak[1] == 0 and b3.active() == [0] and b3.zeros[1] == TC.B // 2
    assert all(db > survey_mod.ACTIVE_FLOOR_DB + 20 for blk in tl.blocks for c, db in enumerate(blk.rms_db) if c in blk.active())
    sched = tl.safe_schedule()
    assert isinstance(sched, R.Schedule) and sched == TC.SCHEDULE
    assert sched.runs == ((0, None), (8192, Mix(((0, 1.0), (1, -1.0)), 2.0)), (16384, Mix(((0, 1.0),), 1.0)))
    assert [blocks for _, blocks, _ in tl.runs()] == [[0], [1], [2, 3]]           # equal neighbours merge
    # over the whole file the fault is averaged away: nothing is done, and the plain downmix of block 1 is digital silence
    assert tl.whole.safe_mix() is None and abs(tl.whole.corr(0, 1)) < 0.05
    x = TC.stored()
    assert not R.mixdown(x[TC.B:2 * TC.B], [0, 1]).any() and R.schedule_mixdown(x, sched)[TC.B:2 * TC.B].any()
    np.testing.assert_array_equal(R.schedule_mixdown(x, sched), x[:, 0] / 32768.0)      # the left channel throughout


def test_equal_timelines_decide_equally(tmp_path):
    a = iss_io.survey_timeline(TC.write(tmp_path / 'a.wav'), TC.BLOCK_SEC)
    b = iss_io.survey_timeline(TC.write(tmp_path / 'b.flac', 'flac'), TC.BLOCK_SEC)
    assert a == b and a.safe_schedule() == b.safe_schedule()
    assert a != 'a' and (a == 'a') is False


@pytest.mark.parametrize('kind', ['i16', 'flac', 'ima'])
def test_decode_auto_timeline(tmp_path, kind):
    path = TC.write(tmp_path / f'f.{kind}', kind)
    pcm, tl, sched = iss_io.decode_auto_timeline(path, TC.BLOCK_SEC)
    x, sr = iss_io.decode_source(path)
    assert tl == iss_io.survey_timeline(path, TC.BLOCK_SEC) and sched == tl.safe_schedule()
    np.testing.assert_array_equal(pcm, R.schedule_ref(x, sr, sched))
    np.testing.assert_array_equal(pcm, iss_io.decode_schedule(path, sched))
    if kind != 'ima':
        assert sched == TC.SCHEDULE
        assert not np.array_equal(pcm, iss_io.decode_auto(path)[0])               # the file-level decision cancels block 1
    healthy = TC.write(tmp_path / f'h.{kind}', kind, TC.healthy())
    pcm, tl, sched = iss_io.decode_auto_timeline(healthy, TC.BLOCK_SEC)
    assert sched == [(0, None)] and len(tl.blocks) == 4
    np.testing.assert_array_equal(pcm, iss_io.decode_auto(healthy)[0])
    mono = autocases.write(tmp_path / 'm.wav', 'mono', 8000, n=3000)
    pcm, tl, sched = iss_io.decode_auto_timeline(mono, TC.BLOCK_SEC)
    assert tl is None and sched is None
    np.testing.assert_array_equal(pcm, iss_io.decode_auto(mono)[0])


def test_out_of_scope_calls_are_refused(tmp_path):
    path = TC.write(tmp_path / 'f.wav')
    for call in (lambda: iss_io.survey_timeline((path, path)), lambda: iss_io.decode_auto_timeline((path, path)),
                 lambda: iss_io.timeline_source((path, path), None, True)):
        with pytest.raises(ValueError, match='timelines of a set are not supported'):
            call()
    with pytest.raises(ValueError, match='block_sec=0'):
        iss_io.survey_timeline(path, 0)


# ------------------------------------------------------------------------------------------------ the decisions table
def test_schedule_decisions_tsv_bytes(tmp_path):
    path = TC.write(tmp_path / 'f.wav')
    mono = autocases.write(tmp_path / 'm.wav', 'mono', 8000, n=3000)
    _, tl, sched = iss_io.decode_auto_timeline(path, TC.BLOCK_SEC)
    survey_mod.write_schedule_decisions_tsv(tmp_path / 'd.tsv', [path, mono, 'gone.wav', 'bad.wav', path],
                                            [(path, tl, sched), (mono, None, None)], {'bad.wav': "error: bad\tframe\n"})
    loss0, loss2 = tl.blocks[0].downmix_loss_db, min(tl.blocks[2].downmix_loss_db, tl.blocks[3].downmix_loss_db)
    assert loss0 == 0.0 and -3.1 < loss2 < -2.9
    want = ('path\tstart\tstop\tblocks\tplan\tkept\tflipped\tdownmix_loss_db\n'
            f'{path}\t0.000000\t1.024000\t1\tplain\t0,1\t\t{loss0!r}\n'
            f'{path}\t1.024000\t2.048000\t1\tmix\t0,1\t1\t-inf\n'
            f'{path}\t2.048000\t3.584000\t2\tmix\t0\t\t{loss2!r}\n'
            f'{mono}\t\t\t\tmono\t0\t\t\n'
            'gone.wav\t\t\t\t!\t\t\tnot processed\n'
            'bad.wav\t\t\t\t!\t\t\terror: bad frame \n'
            f'{path}\t\t\t\t!\t\t\tnot processed\n')
    assert (tmp_path / 'd.tsv').read_bytes() == want.encode()
    assert survey_mod.SCHEDULE_DECISION_COLUMNS == ('path', 'start', 'stop', 'blocks', 'plan', 'kept', 'flipped', 'downmix_loss_db')


# ------------------------------------------------------------------------------------------------ argument errors
class _NoDevice:
    resample = True

    def __init__(self, ffmpeg):
        self.ffmpeg = ffmpeg

    def _no_ffmpeg_mixes(self):
        pass


def test_batch_process_argument_errors():
    from inaspeechsegmenter_amd.segmenter import Segmenter
    for kw in ({}, {'channels': 'split'}, {'mixes': [[0]]}):
        with pytest.raises(ValueError, match="auto_block_sec=10 needs channels='auto'"):
            Segmenter.batch_process(_NoDevice(None), ['a.wav'], ['a.csv'], auto_block_sec=10, **kw)
    with pytest.raises(ValueError, match='block_sec=0'):
        Segmenter.batch_process(_NoDevice(None), ['a.wav'], ['a.csv'], channels='auto', auto_block_sec=0)
    with pytest.raises(ValueError, match="channels='auto' reads files without ffmpeg"):
        Segmenter.batch_process(_NoDevice('ffmpeg'), ['a.wav'], ['a.csv'], channels='auto', auto_block_sec=10)
    with pytest.raises(ValueError, match="None, 'split' or 'auto'"):             # the existing values and their text stay
        Segmenter.batch_process(_NoDevice(None), ['a.wav'], ['a.csv'], channels='each', auto_block_sec=10)


# ------------------------------------------------------------------------------------------------ the command line
def _cli():
    spec = importlib.util.spec_from_file_location('ina_cli', os.path.join(ROOT, 'scripts', 'ina_speech_segmenter_amd.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fake(monkeypatch, seen, fail):
    import inaspeechsegmenter_amd

    class FakeSegmenter:
        def __init__(self, **kw):
            seen['init'] = kw

        def batch_process(self, inputs, outputs, **kw):
            seen['batch'] = (list(inputs), list(outputs), kw)
            lmsg = []
            for src, dst in zip(inputs, outputs):
                if src == fail:                                    # (stands for a file that failed)
                    lmsg.append((dst, 2, "error: <class 'ValueError'> bad\tframe"))
                    continue
                if 'auto_block_sec' in kw:
                    kw['decisions'].append((src,) + iss_io.decode_auto_timeline(src, kw['auto_block_sec'])[1:])
                else:
                    kw['decisions'].append((src,) + iss_io.decode_auto(src)[1:])
                lmsg.append((dst, 0, 'ok 0.0'))
            return 0.0, len(lmsg), 0.0, lmsg

    monkeypatch.setattr(inaspeechsegmenter_amd, 'Segmenter', FakeSegmenter)
    monkeypatch.delenv('WORLD_SIZE', raising=False)


def test_cli_auto_block_writes_one_row_per_run(tmp_path, monkeypatch):
    seen = {}
    fault, mono = TC.write(tmp_path / 'a_fault.wav'), autocases.write(tmp_path / 'b_mono.wav', 'mono', 8000, n=3000)
    bad = TC.write(tmp_path / 'c_bad.wav', 'i16', TC.healthy())
    _fake(monkeypatch, seen, bad)
    tsv = tmp_path / 'd.tsv'
    assert _cli().main(['-i', str(tmp_path / '*.wav'), '-o', str(tmp_path), '-b', 'None', '--resample', '--channels', 'auto',
                        '--auto-block', '1.0', '--decisions', str(tsv)]) == 0
    inputs, _, kw = seen['batch']
    assert inputs == [fault, mono, bad] and kw['channels'] == 'auto' and kw['auto_block_sec'] == 1.0
    rows = [line.split('\t') for line in tsv.read_text().split('\n')[:-1]]
    assert rows[0] == list(survey_mod.SCHEDULE_DECISION_COLUMNS)
    assert [r[:7] for r in rows[1:4]] == [[fault, '0.000000', '1.024000', '1', 'plain', '0,1', ''],
                                          [fault, '1.024000', '2.048000', '1', 'mix', '0,1', '1'],
                                          [fault, '2.048000', '3.584000', '2', 'mix', '0', '']]
    assert rows[2][7] == '-inf' and rows[4] == [mono, '', '', '', 'mono', '0', '', '']
    assert rows[5] == [bad, '', '', '', '!', '', '', "error: <class 'ValueError'> bad frame"] and len(rows) == 6


def test_cli_decisions_without_auto_block_are_the_table_they_were(tmp_path, monkeypatch):
    seen = {}
    fault, mono = TC.write(tmp_path / 'a_fault.wav'), autocases.write(tmp_path / 'b_mono.wav', 'mono', 8000, n=3000)
    inv = autocases.write(tmp_path / 'c_inv.wav', 'deadinv', 8000, n=4000)
    bad = TC.write(tmp_path / 'd_bad.wav', 'i16', TC.healthy())
    _fake(monkeypatch, seen, bad)
    tsv = tmp_path / 'd.tsv'
    assert _cli().main(['-i', str(tmp_path / '*.wav'), '-o', str(tmp_path), '-b', 'None', '--resample', '--channels', 'auto',
                        '--decisions', str(tsv)]) == 0
    assert 'auto_block_sec' not in seen['batch'][2]
    loss_f, loss_i = iss_io.survey_channels(fault).downmix_loss_db, iss_io.survey_channels(inv).downmix_loss_db
    want = ('path\tplan\tkept\tflipped\tdownmix_loss_db\n'
            f'{fault}\tplain\t0,1\t\t{loss_f!r}\n'
            f'{mono}\tmono\t0\t\t\n'
            f'{inv}\tmix\t1,2\t2\t{loss_i!r}\n'
            f"{bad}\t!\t\t\terror: <class 'ValueError'> bad frame\n")
    assert tsv.read_bytes() == want.encode()


@pytest.mark.parametrize('argv,why', [(['-b', 'None', '--auto-block', '10'], '--auto-block goes with --channels auto'),
                                      (['-b', 'None', '--channels', 'split', '--auto-block', '10'], '--auto-block goes with --channels auto'),
                                      (['-b', 'None', '--channels', 'auto', '--auto-block', '0'], 'a number of seconds above 0'),
                                      (['-b', 'None', '--channels', 'auto', '--auto-block', 'nan'], 'a number of seconds above 0'),
                                      (['--channels', 'auto', '--auto-block', '10'], 'needs -b None')])
def test_cli_refusals(tmp_path, capsys, argv, why):
    with pytest.raises(SystemExit):
        _cli().main(['-i', 'a.wav', '-o', str(tmp_path)] + argv)
    assert why in capsys.readouterr().err


def test_cli_flag_defaults():
    cli = _cli()
    assert cli.build_parser().parse_args(['-i', 'a.wav', '-o', '.']).auto_block is None
    assert cli.build_parser().parse_args(['-i', 'a.wav', '-o', '.', '--auto-block', '2.5']).auto_block == 2.5
