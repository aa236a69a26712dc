"""GPU: weighted channel mixes of a file, mixed and resampled on the device.  The MIX instantiations of resample_kernel through
ctx.resample(..., mixes=...), plain and windowed, against resample.mix_ref of the stored samples; the two identities on the device
(a one-term mix is the split's output, the all-channel mean is the plain entry point's); the planner's refusals; FLAC, IMA and
Microsoft ADPCM through Segmenter.load_pcm_mixes; segment_mixes and segment_mix_excerpts against segment_signal of each mix;
batch_process(mixes=...) against the mono twins; score_mixes; and the calls without mixes afterwards.  Every comparison is exact.
The shapes are the smallest at which a mix can go wrong: more than one tile per mix (a tile boundary and the last output
inside every case), more mixes than one group holds, weights that are no powers of two, a repeated channel, saturation, the
16 kHz identity filter, a filter table too large for LDS, windows at both ends of the file and across a tile boundary."""
import os

import numpy as np
import pytest

import flacgen
import msadpcmgen
import sndgen
import wavgen
from conftest import synth_pcm
from inaspeechsegmenter_amd import _native, Segmenter, sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.resample import Mix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    yield s
    s.close()


def _hop(n):
    return -(-n // 160) * 160


def _mix_direct(ctx, raw, sr, fmt, spec, stored=None):
    """One mixed job on its own: -> (the whole signal, len(spec) strides; the references), checked against mix_ref of `stored`
    (what the host reads for `raw`) for every mix, with the samples between a mix's end and the next stride still zero."""
    stored = raw if stored is None else stored
    mixes = R.normalise_mixes(spec, raw.shape[1])
    job = ctx.resample_job(raw, sr, 0, 0, fmt)
    nout, stride = job[-1], _hop(job[-1])
    before = ctx.resample_stats()
    ctx.resample(raw.reshape(-1).view(np.uint8), [job], n_signal=len(mixes) * stride, mixes=[(stride, mixes)])
    sig = ctx.get_signal_pcm16(0, len(mixes) * stride)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)            # a mixed job counts as one job
    tile, _ = ctx.resample_split_geometry(sr, len(mixes))
    assert nout > tile                                                          # more than one tile per mix
    refs = [R.mix_ref(stored, sr, m) for m in mixes]
    for k, want in enumerate(refs):
        np.testing.assert_array_equal(sig[k * stride:k * stride + nout], want, err_msg=f'mix {k} = {mixes[k]}')
        assert not sig[k * stride + nout:(k + 1) * stride].any()
    return sig, refs


def _split(ctx, raw, sr, fmt, sel):
    job = ctx.resample_job(raw, sr, 0, 0, fmt)
    stride = _hop(job[-1])
    ctx.resample(raw.reshape(-1).view(np.uint8), [job], n_signal=len(sel) * stride, splits=[(stride, sel)])
    return ctx.get_signal_pcm16(0, len(sel) * stride)


def _plain(ctx, raw, sr, fmt=None):
    n = ctx.resample_signal(raw, sr, fmt)
    return ctx.get_signal_pcm16(0, n)


# ------------------------------------------------------------------------------------------------ kernel
def test_mix_plain_instantiation_i16(seg):
    x = wavgen.encode(wavgen.make_signal(6000, 2, 61), 'i16')
    _, refs = _mix_direct(seg.ctx, x, 44100, _native.RS_FORMAT[x.dtype], [0, 1, [0, 1], {0: 1, 1: -1}])
    assert not np.array_equal(refs[2], refs[3]) and not np.array_equal(refs[0], refs[1])


def test_mix_plain_instantiation_f32(seg):
    """Weights that are no powers of two, a mix that repeats a channel, a divisor that is neither 1 nor a count."""
    x = wavgen.encode(wavgen.make_signal(5000, 3, 62), 'f32')
    spec = [{0: 0.7071067811865476, 2: 0.7071067811865476, 1: 1.0}, Mix(((1, 1.0 / 3.0), (1, 1.0 / 3.0), (0, -1.0 / 3.0)), 1.0),
            Mix(((2, 0.7071067811865476), (0, 1.0 / 3.0), (2, 3.0)), 1.7), [2, 1, 0]]
    _mix_direct(seg.ctx, x, 48000, _native.RS_FORMAT[x.dtype], spec)


def test_mix_identity_filter_saturates_at_both_ends(seg):
    """16 kHz: the mix itself, quantised.  {0: 1, 1: 1} on frames that sum past +1 and below -1."""
    x = wavgen.encode(wavgen.make_signal(2000, 2, 63, peak=0.4), 'i16')
    x[100:110] = 30000
    x[1500:1510] = -30000
    x[1900] = (-32768, -32768)
    sig, refs = _mix_direct(seg.ctx, x, 16000, _native.RS_FORMAT[x.dtype], [{0: 1, 1: 1}, [0, 1], 1, {0: 1, 1: -1}])
    assert (refs[0][100:110] == 32767).all() and (refs[0][1500:1510] == -32768).all() and refs[0][1900] == -32768
    assert (refs[1][100:110] == 30000).all() and refs[1][1900] == -32768       # the mean does not saturate
    np.testing.assert_array_equal(sig[2 * _hop(2000):2 * _hop(2000) + 2000], x[:, 1])      # the stored column itself


def test_mix_ext_instantiation(seg, tmp_path):
    path = sndgen.write(tmp_path / 'u.wav', 'wav', 'ulaw', False, wavgen.make_signal(3000, 2, 64), 8000)[0]
    snd = sndfmt.parse(open(path, 'rb').read(), path)
    raw, fmt = snd.raw()
    assert fmt == _native.RS_ULAW
    _mix_direct(seg.ctx, raw, 8000, fmt, [[0, 1], {1: 0.6, 0: -0.8}, 1], snd.stored())


def test_mix_table_read_through_cache(seg):
    """44 056 Hz: 110 141 taps, more than LDS holds next to the spans."""
    assert R.plan(44056)[2].size == 110141
    x = wavgen.encode(wavgen.make_signal(30000, 2, 65), 'i16')
    _mix_direct(seg.ctx, x, 44056, _native.RS_FORMAT[x.dtype], [[0, 1], {0: 0.3, 1: 0.9}])


def test_more_mixes_than_a_group(seg):
    """22 050 Hz, 11 mixes of 2 .. 11 terms: a tile's span is 11.5 KB of float64, so 64 KiB hold 5 mixes side by side."""
    ctx = seg.ctx
    tile, group = ctx.resample_split_geometry(22050, 11)
    assert group < 11 and -(-11 // group) > 1                                   # 11 mixes need more than one group
    x = wavgen.encode(wavgen.make_signal(3000, 11, 66), 'i16')
    rng = np.random.default_rng(67)
    spec = []
    for k in range(11):
        nterms = min(11, 2 + k)
        chans = rng.permutation(11)[:nterms] if k % 2 else rng.integers(0, 11, nterms)
        spec.append(Mix(tuple((int(c), float(w)) for c, w in zip(chans, rng.uniform(-0.4, 0.4, nterms))), float(rng.uniform(0.5, 2))))
    assert sorted(len(m.terms) for m in spec) == [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11]
    _mix_direct(ctx, x, 22050, _native.RS_FORMAT[x.dtype], spec)


# ------------------------------------------------------------------------------------------------ identities, on the device
@pytest.mark.parametrize('sr,fmt,ch,n', [(44100, 'i16', 2, 6000), (48000, 'f32', 3, 5000), (22050, 'f64', 9, 3000)])
def test_identities_on_the_device(seg, sr, fmt, ch, n):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(n, ch, 68), fmt)
    code = _native.RS_FORMAT[x.dtype]
    sel = [ch - 1, 0, 1]
    sig, refs = _mix_direct(ctx, x, sr, code, sel + [list(range(ch))])
    nout, stride = refs[0].size, _hop(refs[0].size)
    np.testing.assert_array_equal(sig[:3 * stride], _split(ctx, x, sr, code, sel))       # one-term mixes: the split call's output
    np.testing.assert_array_equal(sig[3 * stride:3 * stride + nout], _plain(ctx, x, sr))      # the mean of all: the plain call's
    if ch == 9:                                                                 # the reference was the in-order loop, not numpy's
        acc = x[:, 0].copy()
        for c in range(1, 9):
            acc = acc + x[:, c]
        np.testing.assert_array_equal(refs[3], R.quantise(R.resample_float(acc / 9.0, sr)))


def test_mixed_and_downmixed_jobs_in_one_call(seg):
    ctx = seg.ctx
    a = wavgen.encode(wavgen.make_signal(6000, 2, 69), 'i16')
    b = wavgen.encode(wavgen.make_signal(5000, 3, 70), 'f32')
    ja = ctx.resample_job(a, 44100, 0, 0)
    sa = _hop(ja[-1])
    jb = ctx.resample_job(b, 48000, a.nbytes, 3 * sa)
    staged = np.concatenate([a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)])
    nsig = 3 * sa + _hop(jb[-1])
    mixes = R.normalise_mixes([[0, 1], {0: 0.25, 1: -0.6}], 2) + [1]            # (a channel index stands for that channel alone)
    before = ctx.resample_stats()
    ctx.resample(staged, [ja, jb], n_signal=nsig, mixes=[(sa, mixes), None])
    sig = ctx.get_signal_pcm16(0, nsig)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 2)              # one launch, two jobs
    for k, m in enumerate(mixes):
        np.testing.assert_array_equal(sig[k * sa:k * sa + ja[-1]], R.mix_ref(a, 44100, m))
        assert not sig[k * sa + ja[-1]:(k + 1) * sa].any()
    np.testing.assert_array_equal(sig[3 * sa:3 * sa + jb[-1]], R.resample_ref(b, 48000))
    assert not sig[3 * sa + jb[-1]:].any()


# ------------------------------------------------------------------------------------------------ windows
def test_windowed_mixes(seg):
    """44.1 kHz, 3 channels, 20 000 frames -> 7 257 outputs, tile 1 024.  Three windows of two mixes each in ONE launch: at the
    file's start, ending at its last output, and an interior one across tile boundaries whose staged slice is exactly
    input_span -- a frame outside the slice but inside the file would be read as zero only by mistake."""
    ctx = seg.ctx
    sr, n = 44100, 20000
    x = wavgen.encode(wavgen.make_signal(n, 3, 71), 'i16')
    n16 = R.out_len(n, sr)
    fid = ctx.resample_filter(sr)[0]
    tile, _ = ctx.resample_split_geometry(sr, 2)
    assert n16 == 7257 and tile == 1024
    wins = [(0, 1500), (n16 - 1300, 1300), (900, 2300)]
    specs = [[[0, 1], {2: 0.7071067811865476, 0: -1.0 / 3.0}], [{0: 1, 1: 1, 2: 1}, 2], [Mix(((1, 0.3), (1, 0.3), (2, -0.9)), 0.9), [2, 0]]]
    whole = [[R.mix_ref(x, sr, m) for m in spec] for spec in specs]
    jobs, rows, mixes, parts, pos, bpos = [], [], [], [], 0, 0
    for (a, count), spec in zip(wins, specs):
        assert count > tile                                                     # more than one tile per mix
        j_lo, j_hi = R.input_span(sr, n, a, count)
        part = np.ascontiguousarray(x[j_lo:j_hi + 1])                           # exactly input_span
        jobs.append((bpos, part.shape[0], 3, _native.RS_FORMAT[x.dtype], fid, 0, pos, count))
        rows.append((j_lo, j_hi + 1, n, a, count))
        mixes.append((_hop(count), R.normalise_mixes(spec, 3)))
        parts += [part.reshape(-1).view(np.uint8), np.zeros(-part.nbytes % 16, dtype=np.uint8)]      # each on a 16-byte boundary
        bpos += part.nbytes + (-part.nbytes % 16)
        pos += 2 * _hop(count)
    assert rows[2][0] > 0 and rows[2][1] < n and (wins[2][0] // tile) != ((wins[2][0] + wins[2][1] - 1) // tile)
    before = ctx.resample_stats()
    ctx.resample(np.concatenate(parts), jobs, n_signal=pos, windows=rows, mixes=mixes)
    sig = ctx.get_signal_pcm16(0, pos)
    after = ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 3)
    for (a, count), job, win, full, spec in zip(wins, jobs, rows, whole, specs):
        for k in range(2):
            o = job[6] + k * _hop(count)
            np.testing.assert_array_equal(sig[o:o + count], full[k][a:a + count], err_msg=f'window [{a}, +{count}) mix {k}')
            np.testing.assert_array_equal(sig[o:o + count], R.mix_ref(x[win[0]:win[1]], sr, spec[k], a, count, win[0], n))
            assert not sig[o + count:o + _hop(count)].any()


# ------------------------------------------------------------------------------------------------ planner refusals
def test_planner_refusals(seg, tmp_path):
    ctx = seg.ctx
    x = wavgen.encode(wavgen.make_signal(3000, 2, 72), 'i16')
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, 44100, 0, 0)
    nout, stride = job[-1], _hop(job[-1])
    one = Mix(((0, 1.0),), 1.0)
    before = ctx.resample_stats(), ctx.adpcm_stats(), ctx.flac_stats(), ctx.msadpcm_stats()

    def tables(sets, mixes, terms):
        return (np.array(sets, dtype=_native.MIXSET), np.array(mixes, dtype=_native.MIX).reshape(-1),
                np.array(terms, dtype=_native.MIX_TERM).reshape(-1))

    def refused(match, mixes, jobs=(job,), staged=src, n_signal=2 * stride):
        with pytest.raises(_native.NativeError, match=match):
            ctx.resample(staged, list(jobs), n_signal=n_signal, mixes=mixes)

    refused(r'job 0: mix rows \[1, \+2\) outside the 2', tables([(stride, 1, 2)], [(0, 1, 1.0)] * 2, [(0, 0, 1.0)]))
    refused(r'job 0: mix rows \[0, \+-1\)', tables([(stride, 0, -1)], [(0, 1, 1.0)], [(0, 0, 1.0)]))
    refused(r'job 0: mix 1: term rows \[1, \+2\) outside the 2', tables([(stride, 0, 2)], [(0, 1, 1.0), (1, 2, 1.0)], [(0, 0, 1.0)] * 2))
    refused(r'job 0: mix 0: term rows \[0, \+0\) outside the 1 of the call, or no term', tables([(stride, 0, 1)], [(0, 0, 1.0)], [(0, 0, 1.0)]))
    refused(r'job 0: mix 1: term 1: channel 2 of 2', [(stride, [one, Mix(((1, 1.0), (2, 1.0)), 1.0)])])
    refused(r'job 0: mix 0: term 0: channel -1 of 2', [(stride, [Mix(((-1, 1.0),), 1.0)])])
    refused(r'job 0: mix 0: term 1: weight -?nan', [(stride, [Mix(((0, 1.0), (1, float('nan'))), 1.0)])])
    refused(r'job 0: mix 1: term 0: weight -?inf', [(stride, [one, Mix(((0, float('-inf')),), 1.0)])])
    refused(r'job 0: mix 1: divisor 0', [(stride, [one, Mix(((0, 1.0),), 0.0)])])
    refused(r'job 0: mix 0: divisor inf', [(stride, [Mix(((0, 1.0),), float('inf'))])])
    refused(r'job 0: mix 0: divisor -?nan', [(stride, [Mix(((0, 1.0),), float('nan'))])])
    refused(r'job 0: dst_stride %d below the %d outputs' % (nout - 1, nout), [(nout - 1, [one, one])])
    refused(r'job 0: output of mix 1, .* outside the %d-sample signal' % (2 * stride - 200), [(stride, [one, one])], n_signal=2 * stride - 200)
    job2 = ctx.resample_job(x, 44100, src.size, stride)                          # on top of job 0's second mix
    refused('overlap', [(stride, [one, one]), (stride, [one])], jobs=(job, job2), staged=np.concatenate([src, src]), n_signal=4 * stride)
    with pytest.raises(ValueError, match='2 mix sets for 1 jobs'):
        ctx.resample(src, [job], n_signal=2 * stride, mixes=[(stride, [one]), None])
    with pytest.raises(ValueError, match='splits or mixes'):
        ctx.resample(src, [job], n_signal=2 * stride, mixes=[(stride, [one])], splits=[(stride, [0])])
    path = sndgen.write(tmp_path / 'm.wav', 'wav', 'ima', False, wavgen.make_signal(3000, 1, 73), 16000, block_align=256)[0]
    s = sndfmt.AdpcmSource(sndfmt.parse(open(path, 'rb').read(), path), 'pcm')
    with pytest.raises(_native.NativeError, match=r'job 0: mixes need a TO_STAGE job with a filter'):
        ctx.adpcm_decode(s.payload, [s.job(ctx, 0, 0, 0).row], s.units, n_signal=s.size, mixes=[(_hop(s.size), [one])])
    assert (ctx.resample_stats(), ctx.adpcm_stats(), ctx.flac_stats(), ctx.msadpcm_stats()) == before      # nothing launched
    _mix_direct(ctx, wavgen.encode(wavgen.make_signal(6000, 2, 74), 'i16'), 44100, 1, [[1, 0]])       # and the context still works


# ------------------------------------------------------------------------------------------------ through the Segmenter
SPEC = [1, [0, 1], {0: 0.7071067811865476, 1: -1.0 / 3.0}]


def _stats(ctx):
    return ctx.flac_stats()[0], ctx.adpcm_stats()[0], ctx.msadpcm_stats()[0], ctx.resample_stats()[0]


def _coded(d, what, x, sr):
    if what == 'flac':
        return flacgen.write(d / 'a.flac', np.round(x * 32767).astype(np.int64), sr, 16, blocksize=1152, channel_mode='left_side',
                             subframe={'type': 'fixed', 'order': 2})
    if what == 'ima':
        return sndgen.write(d / 'a_ima.wav', 'wav', 'ima', False, x, sr, block_align=256)[0]
    return msadpcmgen.write(d / 'a_ms.wav', x, sr, 256)[0]


@pytest.mark.parametrize('what,launches', [('flac', (1, 0, 0, 1)), ('ima', (0, 1, 0, 1)), ('ms', (0, 0, 1, 1))])
def test_load_pcm_mixes_of_coded_files(seg, tmp_path, what, launches):
    path = _coded(tmp_path, what, wavgen.make_signal(5000, 2, 75, peak=0.5), 8000)
    want = iss_io.decode_mixes(path, SPEC)
    before = _stats(seg.ctx)
    got = seg.load_pcm_mixes(path, SPEC)
    after = _stats(seg.ctx)
    assert tuple(b - a for a, b in zip(before, after)) == launches              # all mixes: one decode launch, one resample launch
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(got[0], seg.load_pcm_channels(path, [1])[0])
    ranges = [(0.0, 0.21), (0.3, None)]
    before = _stats(seg.ctx)
    ex = seg.load_pcm_mix_excerpts(path, ranges, SPEC)
    after = _stats(seg.ctx)
    assert tuple(b - a for a, b in zip(before, after)) == launches              # all (range, mix) pairs likewise
    for r, (start, stop) in enumerate(ranges):
        a, b = iss_io.excerpt_bounds(path, want[0].size, start, stop)
        for k in range(3):
            np.testing.assert_array_equal(ex[r][k], want[k][a:b], err_msg=f'range {r} mix {k}')


def _pair(n):
    """Two channels that the energy detector alone tells apart: each silent where the other sounds."""
    a, b = synth_pcm(1, n), synth_pcm(2, n)
    a[:n // 2] = 0
    b[n // 2:] = 0
    return np.stack([a, b], axis=1)


@pytest.fixture(scope='module')
def pair44(tmp_path_factory):
    import scipy.signal
    x = _pair(48000)
    up = np.stack([scipy.signal.resample_poly(x[:, c] / 32768.0, 441, 160) for c in range(2)], axis=1)
    return wavgen.write_wav(tmp_path_factory.mktemp('mixpair') / 'p44.wav', wavgen.encode(up, 'i16'), 44100, 'i16')


def test_segment_mixes_equal_segment_signal(seg, pair44):
    spec = [0, 1, [0, 1]]
    pcm = seg.load_pcm_mixes(pair44, spec)
    before = seg.ctx.resample_stats()
    got = seg.segment_mixes(pair44, spec)
    after = seg.ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)              # all mixes: one launch, one job
    assert len(got) == 3
    for k in range(3):
        assert got[k] == seg.segment_signal(pcm[k]), k
        assert got[k] == seg.segment_signal(seg.load_pcm_mixes(pair44, [spec[k]])[0])
    assert got[0] == seg.segment_channels(pair44, [0])[0] and got[0] != got[1] and got[2] not in (got[0], got[1])
    assert got[0][0][0] == 'noEnergy' and got[1][-1][0] == 'noEnergy'
    assert seg.segment_mixes(pair44, spec, batch_files=1) == got               # one mix per pass


def test_segment_mix_excerpts_equal_segment_signal(seg, pair44):
    spec = [[0, 1], 1]
    ranges = [(0.5, 2.25), (1.0, None)]
    pcm = seg.load_pcm_mix_excerpts(pair44, ranges, spec)
    whole = seg.load_pcm_mixes(pair44, spec)
    before = seg.ctx.resample_stats()
    got = seg.segment_mix_excerpts(pair44, ranges, spec)
    after = seg.ctx.resample_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 2)              # both ranges: one launch, one job per range
    for r, (start, stop) in enumerate(ranges):
        a, b = iss_io.excerpt_bounds(pair44, whole[0].size, start, stop)
        for k in range(2):
            np.testing.assert_array_equal(pcm[r][k], whole[k][a:b])
            assert got[r][k] == seg.segment_signal(pcm[r][k], start_sec=start), (r, k)
    assert got[0][0] != got[0][1]


def test_batch_process_mixes(seg, tmp_path):
    n = 16000
    spec = [[0, 1], 1, {0: 1, 1: -0.5}]
    files = {
        'wav48': wavgen.write_wav(tmp_path / 'wav48.wav', wavgen.encode(wavgen.make_signal(3 * n, 2, 76, peak=0.3), 'i16'), 48000, 'i16'),
        'mono': wavgen.write_wav(tmp_path / 'mono.wav', synth_pcm(3, n).astype('<i2'), 16000, 'i16'),      # too few channels
        'flac': flacgen.write(tmp_path / 'flac.flac', _pair(n).astype(np.int64), 16000, 16, blocksize=1152, channel_mode='left_side',
                              subframe={'type': 'fixed', 'order': 2}),
    }
    names = ['wav48', 'mono', 'flac']
    inputs = [files[k] for k in names]
    outputs = [str(tmp_path / 'out' / f'{k}.csv') for k in names]
    _, nb, _, lmsg = seg.batch_process(inputs, outputs, mixes=spec, workers=1, batch_files=16)
    want_dst = [iss_io.mix_name(outputs[0], k) for k in range(3)] + [outputs[1]] + [iss_io.mix_name(outputs[2], k) for k in range(3)]
    assert [m[0] for m in lmsg] == want_dst and nb == 6
    assert [m[1] for m in lmsg] == [0, 0, 0, 2, 0, 0, 0]
    assert 'ValueError' in lmsg[3][2]                                           # (a decode error's text is its class, as the reference's)
    assert not os.path.exists(outputs[1]) and not os.path.exists(iss_io.mix_name(outputs[1], 0))
    # every CSV against batch_process on the mono twin of that mix, written from the host-only read
    twins, touts, souts = [], [], []
    for k in ('wav48', 'flac'):
        for q, pcm in enumerate(iss_io.decode_mixes(files[k], spec)):
            twins.append(wavgen.write_wav(tmp_path / f'twin_{k}_{q}.wav', pcm.astype('<i2'), 16000, 'i16'))
            touts.append(str(tmp_path / 'twin_out' / f'{k}_{q}.csv'))
            souts.append(iss_io.mix_name(str(tmp_path / 'out' / f'{k}.csv'), q))
    assert seg.batch_process(twins, touts, workers=1)[1] == 6
    for s, t in zip(souts, touts):
        assert open(s, 'rb').read() == open(t, 'rb').read(), s
    assert open(souts[3], 'rb').read() != open(souts[4], 'rb').read()            # the FLAC pair's mean and its channel 1 differ
    # skipifexist goes by .mix0
    os.remove(iss_io.mix_name(outputs[0], 2))
    os.remove(iss_io.mix_name(outputs[2], 0))
    _, nb, _, lmsg = seg.batch_process([inputs[0], inputs[2]], [outputs[0], outputs[2]], mixes=spec, workers=1, skipifexist=True)
    assert [(m[0], m[1]) for m in lmsg] == [(iss_io.mix_name(outputs[0], 0), 1)] + [(iss_io.mix_name(outputs[2], k), 0) for k in range(3)]


def test_score_mixes(pair44):
    from inaspeechsegmenter_amd.vfs import VoiceFemininityScoring
    vfs = VoiceFemininityScoring(ffmpeg=None, models='synthetic', resample=True)
    try:
        spec = [[0, 1], 0]
        got = vfs.score_mixes(pair44, spec)
        pcm = vfs.vad.load_pcm_mixes(pair44, spec)
        assert len(got) == 2
        for k in range(2):
            assert got[k] == vfs.score_signal(pcm[k]), k
        ex = vfs.score_mix_excerpts(pair44, [(0.5, 2.5)], spec)
        pcm = vfs.vad.load_pcm_mix_excerpts(pair44, [(0.5, 2.5)], spec)
        for k in range(2):
            assert ex[0][k] == vfs.score_signal(pcm[0][k]), k
    finally:
        vfs.vad.close()


# ------------------------------------------------------------------------------------------------ afterwards
def test_calls_without_mixes_afterwards(seg):
    """The plain, split, windowed and windowed-split calls of one small case after mixed launches on the same context: what
    resample_ref gives, one launch and one job each."""
    ctx = seg.ctx
    sr, n = 44100, 6000
    x = wavgen.encode(wavgen.make_signal(n, 2, 77), 'i16')
    code = _native.RS_FORMAT[x.dtype]
    _mix_direct(ctx, x, sr, code, [[0, 1], {0: 0.5, 1: 2.0}])
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, sr, 0, 0)
    nout, stride = job[-1], _hop(job[-1])
    a, count = 300, 1500
    j_lo, j_hi = R.input_span(sr, n, a, count)
    part = np.ascontiguousarray(x[j_lo:j_hi + 1])
    wjob = (0, part.shape[0], 2, code, job[4], 0, 0, count)
    win = (j_lo, j_hi + 1, n, a, count)
    calls = [
        (lambda: ctx.resample(src, [job], n_signal=nout), [R.resample_ref(x, sr)], nout),
        (lambda: ctx.resample(src, [job], n_signal=2 * stride, splits=[(stride, [1, 0])]), [R.resample_ref(x[:, c], sr) for c in (1, 0)], stride),
        (lambda: ctx.resample(part.reshape(-1).view(np.uint8), [wjob], n_signal=count, windows=[win]), [R.resample_ref(x, sr)[a:a + count]], count),
        (lambda: ctx.resample(part.reshape(-1).view(np.uint8), [wjob], n_signal=2 * _hop(count), windows=[win], splits=[(_hop(count), [1, 0])]),
         [R.resample_ref(x[:, c], sr)[a:a + count] for c in (1, 0)], _hop(count)),
    ]
    for call, wants, step in calls:
        before = ctx.resample_stats()
        call()
        got = ctx.get_signal_pcm16(0, step * (len(wants) - 1) + wants[0].size)
        after = ctx.resample_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (1, 1)
        for k, w in enumerate(wants):
            np.testing.assert_array_equal(got[k * step:k * step + w.size], w)
