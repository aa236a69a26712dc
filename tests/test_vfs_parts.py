"""CPU: the host side of voice femininity per channel and per time range -- argument checks that need no device, the TSV
layouts of batch_process with the scoring stubbed, and the part table pipeline._Worker.run leaves on its batch."""
import numpy as np
import pytest

import wavgen
from inaspeechsegmenter_amd import Segmenter, pipeline, vfs


def _scorer(ffmpeg, resample=True):
    """A scorer with no device behind it: what the argument checks and the TSV writers reach."""
    v = object.__new__(vfs.VoiceFemininityScoring)
    v.ffmpeg = ffmpeg
    v.vad = object.__new__(Segmenter)
    v.vad.ffmpeg, v.vad.resample = ffmpeg, resample
    v.resample = resample
    return v


@pytest.fixture(scope='module')
def stereo(tmp_path_factory):
    x = wavgen.encode(wavgen.make_signal(16000, 2, 5), 'i16')
    return wavgen.write_wav(tmp_path_factory.mktemp('vfs_parts') / 'stereo.wav', x, 16000, 'i16')


def test_ffmpeg_set_is_refused_as_the_segmenter_refuses_it(stereo):
    v = _scorer('ffmpeg')
    for call, args, text in ((v.score_channels, (stereo,), 'channels are split without ffmpeg'),
                             (v.score_excerpts, (stereo, [(0, 0.5)]), 'excerpts are read without ffmpeg'),
                             (v.score_channel_excerpts, (stereo, [(0, 0.5)]), 'excerpts of channels are read without ffmpeg')):
        with pytest.raises(ValueError, match=text) as e:
            call(*args)
        with pytest.raises(ValueError) as want:                # the Segmenter call of the same shape: the same words
            getattr(v.vad, call.__name__.replace('score', 'segment'))(*args)
        assert str(e.value) == str(want.value) and "ffmpeg='ffmpeg'" in str(e.value)
    with pytest.raises(ValueError, match=r"channels='split' reads files without ffmpeg .*ffmpeg='ffmpeg' downmixes"):
        v.batch_process([stereo], channels='split')
    with pytest.raises(ValueError, match=r"channels='both': None or 'split'"):
        _scorer(None).batch_process([stereo], channels='both')


def test_channel_and_range_errors_name_the_file(stereo):
    v = _scorer(None)
    for call, args in ((v.score_channels, ([2],)), (v.score_channels, ([],)), (v.score_channels, ([0, -1],)),
                       (v.score_excerpts, ([(1.0, 2.0)],)),            # starts at the end of a 1 s file
                       (v.score_excerpts, ([(0.5, 0.25)],)),
                       (v.score_channel_excerpts, ([(0, 0.5)], [2])),
                       (v.score_channel_excerpts, ([(1.5, None)],)),
                       (v.score_channel_excerpts, ([(0.25, 0.26)], [0]))):   # 160 samples: less than one analysis window
        with pytest.raises(ValueError, match=r'stereo\.wav'):
            call(stereo, *args)
    with pytest.raises(FileNotFoundError, match=r'missing\.wav'):  # (a missing file: the error of the read, as in Segmenter)
        v.score_channels('/nowhere/missing.wav')


def test_split_tsv_layout(tmp_path):
    v = _scorer(None)
    table = {'a.wav': [(0.25, 3.5, 12), (None, 0, 0)], 'c.flac': [(1.0, 0.98, 1)]}
    calls = []

    def score_channels(fpath, channels=None, batch_files=None, batch_seconds=None):
        calls.append((fpath, channels, batch_files, batch_seconds))
        if fpath not in table:
            raise FileNotFoundError(2, 'No such file or directory', fpath)
        return table[fpath]
    v.score_channels = score_channels
    out = tmp_path / 'split.tsv'
    res = v.batch_process(['a.wav', 'b.wav', 'c.flac'], output_csv=str(out), batch_seconds=600, channels='split')
    assert res == [table['a.wav'], "FileNotFoundError: [Errno 2] No such file or directory: 'b.wav'", table['c.flac']]
    assert calls == [(p, None, None, 600) for p in ('a.wav', 'b.wav', 'c.flac')]
    assert out.read_bytes() == (b'path\tchannel\tscore\tspeech_duration\tnb_vectors\n'
                                b'a.wav\t0\t0.25\t3.5\t12\n'
                                b'a.wav\t1\tNone\t0\t0\n'
                                b"b.wav\t\tFileNotFoundError: [Errno 2] No such file or directory: 'b.wav'\n"
                                b'c.flac\t0\t1.0\t0.98\t1\n')
    assert v.batch_process([], channels='split') == []


def test_default_tsv_is_unchanged(tmp_path):
    """channels=None: the code path, the header and the rows batch_process has always written, for a scorer whose decode, VAD
    and scoring are stubbed (the bytes below are what the version before the `channels` argument wrote for this stub)."""
    v = _scorer(None)
    pcm = {'a.wav': np.full(16000, 100, np.int16), 'quiet.wav': np.zeros(32000, np.int16), 'c.wav': np.full(8000, 7, np.int16)}

    def decode(fpath, nbtry, trydelay):
        if fpath not in pcm:
            raise FileNotFoundError(2, 'No such file or directory', fpath)
        return pcm[fpath]
    v._decode = decode
    v.vad.segment_signal = lambda a, start_sec=0: ([('speech', 0.0, len(a) / 32000), ('noEnergy', len(a) / 32000, len(a) / 16000)]
                                                   if a.any() else [('noEnergy', 0.0, len(a) / 16000)])
    v._score_batch = lambda batch: {b[0]: (0.5, b[5], len(b[2]) // 4000) for b in batch}
    out = tmp_path / 'plain.tsv'
    for kw in ({}, {'channels': None}):
        res = v.batch_process(['a.wav', 'b.wav', 'quiet.wav', 'c.wav'], output_csv=str(out), **kw)
        assert res == [(0.5, 0.5, 4), "FileNotFoundError: [Errno 2] No such file or directory: 'b.wav'", (None, 0, 0), (0.5, 0.25, 2)]
        assert out.read_bytes() == (b'path\tscore\tspeech_duration\tnb_vectors\n'
                                    b'a.wav\t0.5\t0.5\t4\n'
                                    b"b.wav\tFileNotFoundError: [Errno 2] No such file or directory: 'b.wav'\n"
                                    b'quiet.wav\tNone\t0\t0\n'
                                    b'c.wav\t0.5\t0.25\t2\n')


def test_worker_run_leaves_the_part_table():
    """Per part of a pass: its offset in the resident signal (a multiple of 160) and its samples, on the fake device of
    tests/test_host.py; what `run` returns is what it returned without them."""
    from inaspeechsegmenter_amd import segmenter as S
    from test_host import _FakeDevice

    def predict(nclass):
        def run(batch):
            out = np.full((len(batch), nclass), 0.1 / (nclass - 1), np.float32)
            out[:, 0] = 0.9
            return out
        return run

    fake = _FakeDevice({0: predict(3)}, {0: 21})
    seg = object.__new__(S.Segmenter)
    seg.energy_ratio, seg.detect_gender, seg.ctx, seg.ffmpeg = 0.03, False, fake, None
    seg.vad = object.__new__(S.SpeechMusicNoise)
    seg.vad.ctx, seg.vad.compiled = fake, None
    rng = np.random.default_rng(3)
    sizes = [70001, 11120, 160 * 300, 40333]
    batch = pipeline._Batch()
    assert batch.poffs is None and batch.psize is None
    batch.sigs = [np.round(rng.normal(0, 1000, n)).astype(np.int16) for n in sizes]
    batch.idx, batch.names = list(range(len(sizes))), ['m%d' % k for k in range(len(sizes))]
    lsegs = pipeline._Worker(seg, fake).run(batch)
    assert batch.psize == sizes
    assert batch.poffs == [0, 70080, 70080 + 11200, 70080 + 11200 + 48000]
    assert all(o % 160 == 0 for o in batch.poffs) and fake.sig.size == batch.poffs[-1] + 40480
    for o, n, x in zip(batch.poffs, batch.psize, batch.sigs):     # the parts are where the table says, zeros between them
        assert np.array_equal(fake.sig[o:o + n], x) and not fake.sig[o + n:o + -(-n // 160) * 160].any()
    assert len(lsegs) == len(sizes) and not batch.errs
    for lseg in lsegs:                                            # one contiguous labelling per part, from its slot 0
        assert lseg[0][1] == 0 and all(a[2] == b[1] for a, b in zip(lseg, lseg[1:]))
