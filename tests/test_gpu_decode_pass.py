"""GPU: the host side of a decode pass (iss_flac_decode, iss_adpcm_decode, iss_resample_pcm16 and the two stage read-backs)
refuses a bad call with the code and the text recorded in tests/golden/decode_refusals.json, and a refused call changes
nothing: the launch counters, the resident signal and the staged job of the call before it stay what they were."""
import json
import os
import re

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from conftest import GOLDEN
from inaspeechsegmenter_amd import _native, flac, sndfmt

pytestmark = pytest.mark.gpu

N_SIGNAL = 4096          # the signal every edited call asks for: none of them gets it
TO_SIGNAL, TO_STAGE = 0, 1


def _pcm(n, ch, seed, bps=16):
    return np.round(wavgen.make_signal(n, ch, seed, peak=0.5) * 2 ** (bps - 1)).astype(np.int64)


def _ima(n, ch, sr, seed):
    data, _, twin, frames = sndgen.encode(wavgen.make_signal(n, ch, seed), 'ima', False, 256)
    s = sndfmt.Sound(f'i{seed}.wav', sr, ch, 'ima', False, np.frombuffer(data, np.uint8), 0, frames=frames, block_align=256,
                     spb=sndgen.ima_samples_per_block(256, ch))
    assert s.nblocks == 2
    return s


def _cat(parts):
    """Payloads end to end, each at a multiple of 16 bytes -> (bytes, offset of every part)."""
    out, offs, pos = [], [], 0
    for p in parts:
        pad = -p.size % 16
        offs.append(pos)
        out += [p, np.zeros(pad, np.uint8)]
        pos += p.size + pad
    return np.concatenate(out), offs


def _outcome(fn):
    """(return code, error text) of one call through _native.Context: (0, '') when it is accepted."""
    try:
        fn()
    except _native.NativeError as e:
        m = re.fullmatch(r'\w+ failed \((-?\d+)\): (.*)', str(e), re.S)
        return int(m.group(1)), m.group(2)
    return 0, ''


class _Inputs:
    """The streams of the issue's list, and per decoder one good call with a job of every kind it takes."""

    def __init__(self):
        self.f16 = flac.FlacStream(flacgen.encode(_pcm(1152, 1, 1), 16000, 16, blocksize=576), 'f16.flac')
        self.fst = flac.FlacStream(flacgen.encode(_pcm(1152, 2, 2), 44100, 16, blocksize=576), 'fst.flac')
        self.f24 = flac.FlacStream(flacgen.encode(_pcm(1152, 1, 3, 24), 16000, 24, blocksize=576), 'f24.flac')
        assert [len(s.frames) for s in (self.f16, self.fst, self.f24)] == [2, 2, 2]
        self.a1 = _ima(1010, 1, 16000, 4)
        self.a2 = _ima(498, 2, 22050, 5)
        self.raw = wavgen.encode(wavgen.make_signal(441, 2, 6), 'i16')
        self.known = (np.arange(1000) * 31 % 2001 - 1000).astype(np.int16)

    def flac_call(self, ctx, streams=None):
        """(src, frames, jobs): f16 to the signal, fst staged and resampled behind it, f24 staged."""
        streams = streams or (self.f16, self.fst, self.f24)
        src, offs = _cat([s.audio for s in streams])
        fid = ctx.resample_filter(44100)[0]
        jobs, fb, dst = [], 0, 0
        for s, o in zip(streams, offs):
            if s.bps > 16:
                jobs.append((o, fb, len(s.frames), s.n, s.ch, s.bps, TO_STAGE, -1, 0, 0))
            elif s.ch == 1:
                jobs.append((o, fb, len(s.frames), s.n, 1, s.bps, TO_SIGNAL, -1, dst, 0))
                dst += 1200
            else:
                nout = -(-s.n * 160 // 441)
                jobs.append((o, fb, len(s.frames), s.n, s.ch, s.bps, TO_STAGE, fid, dst, nout))
                dst += 1200
            fb += len(s.frames)
        return src, np.concatenate([s.frames for s in streams]), np.array(jobs, dtype=_native.FLAC_JOB)

    def adpcm_call(self, ctx, sounds=None):
        """(src, jobs, nblocks): a1 to the signal, a2 staged and resampled behind it."""
        sounds = sounds or (self.a1, self.a2)
        src, offs = _cat([s.data for s in sounds])
        fid = ctx.resample_filter(22050)[0]
        jobs, bb, dst = [], 0, 0
        for s, o in zip(sounds, offs):
            if s.ch == 1:
                jobs.append((o, bb, s.nblocks, s.n, 1, 256, TO_SIGNAL, -1, dst, 0))
            else:
                jobs.append((o, bb, s.nblocks, s.n, s.ch, 256, TO_STAGE, fid, dst, -(-s.n * 320 // 441)))
            bb += s.nblocks
            dst += 1200
        return src, np.array(jobs, dtype=_native.ADPCM_JOB), bb

    def raw_call(self, ctx):
        job = np.array([ctx.resample_job(self.raw, 44100, 0, 0)], dtype=_native.RS_JOB)
        return self.raw.reshape(-1).view(np.uint8), job


def _edit(jobs, j, **fields):
    out = jobs.copy()
    for k, v in fields.items():
        out[k][j] = v
    return out


def _flac_cases(I, ctx):
    src, fr, jobs = I.flac_call(ctx)
    call = lambda jb, s=src, f=fr, n=N_SIGNAL: (lambda: ctx.flac_decode(s, f, jb, n))
    j0 = lambda **kw: call(_edit(jobs, 0, **kw))
    j1 = lambda **kw: call(_edit(jobs, 1, **kw))
    yield 'dst_past_signal', j0(dst_offset=N_SIGNAL - 1151)
    s2, f2, jb2 = I.flac_call(ctx, (I.f16, I.f16))
    yield 'two_jobs_overlap', call(_edit(jb2, 1, dst_offset=1000), s2, f2)
    yield 'resample_overlaps_signal', j1(dst_offset=1000)
    yield 'unknown_filter', j1(filter=99)
    yield 'frames_out_off_by_one', j1(frames_out=jobs['frames_out'][1] + 1)
    yield 'channels_0', j0(channels=0)
    yield 'channels_9', j0(channels=9)
    yield 'bps_12', j0(bps=12)
    yield 'nframes_0', j0(nframes=0)
    yield 'frame_begin_past_table', j0(frame_begin=len(fr))
    yield 'frames_total_0', j0(frames_total=0)
    yield 'frames_total_not_tiled', j0(frames_total=1151)
    yield 'src_offset_negative', j0(src_offset=-1)
    yield 'src_offset_beyond', j0(src_offset=src.size + 1)
    long_row = fr.copy()
    long_row['length'][-1] += 64
    yield 'row_past_src', call(jobs, src, long_row)
    s1, f1, jb1 = I.flac_call(ctx, (I.f16,))
    yield 'row_in_two_jobs', call(np.concatenate([jb1, _edit(jb1, 0, dst_offset=2000)]), s1, f1)
    yield 'row_in_no_job', call(jobs[:2])
    yield 'to_signal_stereo', j1(output=TO_SIGNAL)
    yield 'to_signal_24_bit', call(_edit(jobs, 2, output=TO_SIGNAL, dst_offset=2400))
    yield 'output_2', j0(output=2)


def _adpcm_cases(I, ctx):
    src, jobs, nb = I.adpcm_call(ctx)
    call = lambda jb, s=src, b=nb, n=N_SIGNAL: (lambda: ctx.adpcm_decode(s, jb, b, n))
    j0 = lambda **kw: call(_edit(jobs, 0, **kw))
    j1 = lambda **kw: call(_edit(jobs, 1, **kw))
    yield 'dst_past_signal', j0(dst_offset=N_SIGNAL - 1009)
    s2, jb2, nb2 = I.adpcm_call(ctx, (I.a1, I.a1))
    yield 'two_jobs_overlap', call(_edit(jb2, 1, dst_offset=1000), s2, nb2)
    yield 'resample_overlaps_signal', j1(dst_offset=1000)
    yield 'unknown_filter', j1(filter=99)
    yield 'frames_out_off_by_one', j1(frames_out=jobs['frames_out'][1] + 1)
    yield 'block_align_not_multiple', j0(block_align=258)
    yield 'block_align_is_header_only', j0(block_align=4)
    yield 'block_align_above_32768', j0(block_align=32772)
    yield 'nblocks_0', j0(nblocks=0)
    yield 'frames_total_below', j0(frames_total=505)
    yield 'frames_total_above', j0(frames_total=1011)
    yield 'block_begin_breaks_tiling', j1(block_begin=3)
    yield 'src_offset_misaligned', j0(src_offset=2)
    yield 'src_offset_beyond', j1(src_offset=src.size)
    yield 'nblocks_total_not_the_sum', call(jobs, src, nb + 1)
    yield 'to_signal_stereo', j1(output=TO_SIGNAL)
    yield 'output_2', j0(output=2)


def _raw_cases(I, ctx):
    src, job = I.raw_call(ctx)
    call = lambda jb, n=N_SIGNAL: (lambda: ctx.resample(src, jb, n))
    j0 = lambda **kw: call(_edit(job, 0, **kw))
    yield 'dst_past_signal', j0(dst_offset=N_SIGNAL - 159)
    yield 'two_jobs_overlap', call(np.concatenate([job, _edit(job, 0, dst_offset=100)]))
    yield 'unknown_filter', j0(filter=99)
    yield 'frames_out_off_by_one', j0(frames_out=161)
    yield 'format_7', j0(format=7)
    yield 'frames_out_10', j0(frames_out=10)
    yield 'src_offset_2', j0(src_offset=2)
    yield 'src_offset_4', j0(src_offset=4)
    yield 'dst_offset_1e9', j0(dst_offset=10 ** 9)


def _stage_cases(I, ctx):
    """Read-backs after the good calls of _good_calls: FLAC job 1 (stereo, 1152 frames) and ADPCM job 1 (stereo, 498 frames)
    were staged, job 0 of each went to the signal."""
    yield 'flac_get_stage/job_minus_1', lambda: ctx.flac_get_stage(-1, 1152, 2, 16)
    yield 'flac_get_stage/job_past_the_end', lambda: ctx.flac_get_stage(3, 1152, 2, 16)
    yield 'flac_get_stage/job_went_to_signal', lambda: ctx.flac_get_stage(0, 1152, 1, 16)
    yield 'flac_get_stage/bytes_off_by_2', lambda: ctx.flac_get_stage(1, 2 * 1152 + 1, 1, 16)
    yield 'adpcm_get_stage/job_minus_1', lambda: ctx.adpcm_get_stage(-1, 498, 2)
    yield 'adpcm_get_stage/job_past_the_end', lambda: ctx.adpcm_get_stage(2, 498, 2)
    yield 'adpcm_get_stage/job_went_to_signal', lambda: ctx.adpcm_get_stage(0, 1010, 1)
    yield 'adpcm_get_stage/bytes_off_by_2', lambda: ctx.adpcm_get_stage(1, 2 * 498 + 1, 1)


def _good_calls(I, ctx):
    """One good call per decoder with a staged job, then the known signal.  -> the state a refused call has to leave."""
    src, fr, jobs = I.flac_call(ctx)
    st = ctx.flac_decode(src, fr, jobs, N_SIGNAL)
    fstage = ctx.flac_get_stage(1, I.fst.n, 2, 16).copy()
    assert not st.any()
    np.testing.assert_array_equal(fstage, I.fst.decode_host())
    src, jobs, nb = I.adpcm_call(ctx)
    st = ctx.adpcm_decode(src, jobs, nb, N_SIGNAL)
    astage = ctx.adpcm_get_stage(1, I.a2.n, 2).copy()
    assert not st.any()
    np.testing.assert_array_equal(astage, I.a2.stored())
    ctx.set_signal(I.known)
    return {'stats': (ctx.flac_stats(), ctx.adpcm_stats(), ctx.resample_stats()), 'flac': fstage, 'adpcm': astage}


def _unchanged(I, ctx, before, name):
    assert (ctx.flac_stats(), ctx.adpcm_stats(), ctx.resample_stats()) == before['stats'], name
    np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 1000), I.known, err_msg=name)
    np.testing.assert_array_equal(ctx.flac_get_stage(1, I.fst.n, 2, 16), before['flac'], err_msg=name)
    np.testing.assert_array_equal(ctx.adpcm_get_stage(1, I.a2.n, 2), before['adpcm'], err_msg=name)


def _entry_points(I, ctx):
    """(name, the same good call with n_signal < 0) of the three entry points."""
    fs, ff, fj = I.flac_call(ctx)
    as_, aj, ab = I.adpcm_call(ctx)
    rs, rj = I.raw_call(ctx)
    return (('flac_decode', lambda: ctx.flac_decode(fs, ff, fj, -1)), ('adpcm_decode', lambda: ctx.adpcm_decode(as_, aj, ab, -1)),
            ('resample', lambda: ctx.resample(rs, rj, -1)))


def decode_refusals():
    """Yields (case name, return code, error text or '') of a fixed list of calls, one defect each, and asserts around every
    refused call on the main context that it changed nothing."""
    import torch
    I = _Inputs()
    # n_signal < 0 without an own PCM16 signal: a fresh context, and one whose signal is the caller's device memory
    ctx = _native.Context(0)
    try:
        for name, fn in _entry_points(I, ctx):
            rc, text = _outcome(fn)
            assert (ctx.flac_stats(), ctx.adpcm_stats(), ctx.resample_stats()) == ((0, 0), (0, 0), (0, 0)), name
            yield f'{name}/n_signal_negative_fresh_context', rc, text
        yield ('flac_get_stage/before_any_decode',) + _outcome(lambda: ctx.flac_get_stage(0, 1152, 1, 16))
        yield ('adpcm_get_stage/before_any_decode',) + _outcome(lambda: ctx.adpcm_get_stage(0, 1010, 1))
        t = torch.from_numpy(I.known).cuda()
        torch.cuda.synchronize()
        ctx.set_signal_device(t.data_ptr(), t.numel())
        for name, fn in _entry_points(I, ctx):
            rc, text = _outcome(fn)
            assert (ctx.flac_stats(), ctx.adpcm_stats(), ctx.resample_stats()) == ((0, 0), (0, 0), (0, 0)), name
            np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 1000), I.known, err_msg=name)
            yield f'{name}/n_signal_negative_device_signal', rc, text
    finally:
        ctx.close()
    # every other refusal: on a context holding one good staged decode per decoder and a known signal
    ctx = _native.Context(0)
    try:
        before = _good_calls(I, ctx)
        for prefix, cases in (('flac_decode', _flac_cases), ('adpcm_decode', _adpcm_cases), ('resample', _raw_cases), ('', _stage_cases)):
            for name, fn in cases(I, ctx):
                name = f'{prefix}/{name}' if prefix else name
                rc, text = _outcome(fn)
                assert rc != 0, name
                _unchanged(I, ctx, before, name)
                yield name, rc, text
        # accepted: no jobs and a signal of 64 samples, which then reads as zeros
        none = np.zeros(0, np.uint8)
        for name, fn in (('flac_decode', lambda: ctx.flac_decode(none, np.zeros(0, _native.FLAC_FRAME), [], 64)),
                         ('adpcm_decode', lambda: ctx.adpcm_decode(none, [], 0, 64)), ('resample', lambda: ctx.resample(none, [], 64))):
            ctx.set_signal(I.known)
            rc, text = _outcome(fn)
            if rc == 0:
                np.testing.assert_array_equal(ctx.get_signal_pcm16(0, 64), np.zeros(64, np.int16), err_msg=name)
                assert _outcome(lambda: ctx.get_signal_pcm16(0, 65))[0] != 0, name
            yield f'{name}/no_jobs_n_signal_64', rc, text
    finally:
        ctx.close()


def test_decode_refusals_are_pinned():
    """Code and text of every refusal equal the record made with the library as it was before the three entry points shared
    one decode pass (tests/golden/decode_refusals.json), and the calls without jobs are still accepted."""
    with open(os.path.join(GOLDEN, 'decode_refusals.json')) as f:
        want = json.load(f)
    got = json.loads(json.dumps(list(decode_refusals())))
    assert [g[0] for g in got] == [w[0] for w in want]
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff
    assert [g[0] for g in got if g[1] == 0] == [f'{p}/no_jobs_n_signal_64' for p in ('flac_decode', 'adpcm_decode', 'resample')]
