"""Microsoft ADPCM (WAVE format tag 2) without ffmpeg, on the CPU: the host build of the device's block decoder
(iss_msadpcm_decode_host, through io.decode_source) against the plain Python decoder of msadpcmgen.py, every sample; crafted
blocks for saturation, the delta floor and the delta cap; `fact` counts; the refusals; the host-only twins of the device cuts;
and the bytes a ranged read fetches.  Every comparison is exact: the decode is integer arithmetic.

Both decoders implement this project's own statement of the format (include/iss.h: floor rounding of the prediction, the
header delta raised to 16, delta capped at 2^21); no libsndfile was at hand to pin it."""
import os

import numpy as np
import pytest

import msadpcmgen as M
import wavgen
from inaspeechsegmenter_amd import _native, sndfmt
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'msadpcm_vectors.npz')
# (channels, block_align) -> 500, 500, 128, 20 and 4 samples per block; 3 and 5 channels alternate a channel's nibble and put
# blocks off 4-byte alignment, 64 channels give the shortest legal walk
MATRIX = [(1, 256), (2, 512), (3, 210), (5, 80), (64, 512)]
SPB = {(1, 256): 500, (2, 512): 500, (3, 210): 128, (5, 80): 20, (64, 512): 4}


def sec(k):
    return k / 16000.0


def _host(blocks, ch, align, frames=None):
    nb = len(blocks) // align
    spb = M.samples_per_block(align, ch)
    n = nb * spb if frames is None else frames
    return _native.msadpcm_decode_host(np.frombuffer(blocks, np.uint8), -(-n // spb), ch, align, n)


def test_samples_per_block_of_the_matrix():
    for ch, align in MATRIX:
        assert M.samples_per_block(align, ch) == SPB[ch, align]


@pytest.mark.parametrize('ch,align', MATRIX)
@pytest.mark.parametrize('container', ['wav', 'rf64', 'w64'])
def test_host_decoder_equals_python_decoder(tmp_path, ch, align, container):
    n = SPB[ch, align] * 5 + 3 if ch < 64 else 4 * 30 + 1
    p, twin = M.write(tmp_path / f'a.{container}', wavgen.make_signal(n, ch, 100 + ch), 16000, align, container)
    got, sr = iss_io.decode_source(p)
    assert sr == 16000 and got.dtype == np.int16 and got.shape == twin.shape and len(twin) == n
    np.testing.assert_array_equal(got, twin)


def test_encoder_round_trip_is_an_encoder():
    """The helper's encoder tracks its input (tens of dB): the formulas hang together.  Not a pin of the rounding rule."""
    x = wavgen.make_signal(4000, 1, 3)
    pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    got = M.decode(M.encode(pcm, 256), 1, 256, 4000).astype(np.float64)
    err = got - pcm
    assert 10 * np.log10((pcm.astype(np.float64) ** 2).mean() / (err ** 2).mean()) > 20


@pytest.mark.parametrize('predictor', range(7))
def test_every_predictor(tmp_path, predictor):
    p, twin = M.write(tmp_path / f'p{predictor}.wav', wavgen.make_signal(1300, 2, 40 + predictor), 16000, 420,
                      predictor=predictor)
    data = open(p, 'rb').read()
    base = M.data_offset(p)
    assert set(data[base:base + 2]) == {predictor}
    np.testing.assert_array_equal(iss_io.decode_source(p)[0], twin)


def _crafted():
    """name -> (block bytes, channels): the blocks of the golden file."""
    out = {}
    out['saturate_high'] = (M.block([7] * 20, predictor=0, delta=3000, samp1=30000, samp2=29000), 1)
    out['saturate_low'] = (M.block([8] * 20, predictor=0, delta=3000, samp1=-30000, samp2=-29000), 1)
    out['delta_floor'] = (M.block([0, 1, 15, 0] * 20, predictor=1, delta=5, samp1=100, samp2=90), 1)
    out['negative_header_delta'] = (M.block([1, 15, 2, 14] * 5, predictor=3, delta=-300, samp1=-5, samp2=7), 1)
    out['delta_cap'] = (M.block([7, 8] * 40, predictor=2, delta=32767, samp1=0, samp2=0), 1)
    out['floor_not_truncation'] = (M.block([0] * 10, predictor=5, delta=16, samp1=-1, samp2=3), 1)
    rng = np.random.default_rng(5)
    out['three_channels'] = (M.block(rng.integers(0, 16, (22, 3)), predictor=[6, 4, 1], delta=[16, 900, 40],
                                     samp1=[-3000, 12, 32767], samp2=[-2900, -12, -32768]), 3)
    return out


def test_crafted_blocks():
    c = _crafted()
    for name, (blk, ch) in c.items():
        want = np.array(M.decode_block(blk, ch)[0], dtype=np.int16)
        got, st = _host(blk, ch, len(blk))
        assert not st.any(), name
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=name)
    hi = np.array(M.decode_block(c['saturate_high'][0], 1)[0])
    lo = np.array(M.decode_block(c['saturate_low'][0], 1)[0])
    assert hi.max() == 32767 and (hi[-5:] == 32767).all() and lo.min() == -32768 and (lo[-5:] == -32768).all()
    # the floor of 16: predictor 1 extrapolates the line through the last two samples, so a code s bends it by s * delta; from a
    # header delta of 5 and through codes that shrink it (230 / 256), every bend is s * 16
    fl = np.array(M.decode_block(c['delta_floor'][0], 1)[0])[:, 0]
    assert list(np.diff(fl, 2)) == [0, 16, -16, 0] * 20
    # floor, not truncation: predictor 5 on (-1, 3) gives (-460 - 624) >> 8 = -5 (C division would give -4)
    assert M.decode_block(c['floor_not_truncation'][0], 1)[0][2][0] == -5


def test_delta_cap_is_reached():
    """Forty codes 7 and forty codes 8 in turn from the largest header delta: every one grows delta by 614/256 or 768/256, so
    the cap of 2^21 holds it from the fifth code on, and both decoders apply it (no 32-bit overflow in the host build)."""
    blk = _crafted()['delta_cap'][0]
    d = 32767
    trace = []
    for code in [7, 8] * 40:
        d = max(16, (M.ADAPT[code] * d) >> 8)
        trace.append(d)
    assert max(trace) > M.DELTA_MAX * 1000                        # uncapped, it would leave 32 bits
    want = np.array(M.decode_block(blk, 1)[0], dtype=np.int16)[:, 0]
    got, st = _host(blk, 1, len(blk))
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(want[6:])) <= {-32768, 32767}


@pytest.mark.parametrize('ch,align', [(1, 256), (3, 210)])
def test_fact_and_partial_blocks(tmp_path, ch, align):
    spb = SPB[ch, align]
    x = wavgen.make_signal(spb * 4, ch, 9)
    pcm = np.round(x * 32767).astype(np.int16)
    blocks = M.encode(pcm, align)
    full = M.decode(blocks, ch, align)
    assert len(full) == spb * 4
    f = M.fmt(16000, ch, align)

    def read(data, fact):
        return iss_io.decode_source(M.write_riff(tmp_path / 'f.wav', f, data, fact=fact))[0]
    for cut in (1, 2, 3):                                         # the last block gives iSamp2 alone, both seeds, one code
        np.testing.assert_array_equal(read(blocks, spb * 3 + cut), full[:spb * 3 + cut])
    np.testing.assert_array_equal(read(blocks, None), full)
    np.testing.assert_array_equal(read(blocks, spb * 4 + 1), full)                 # a count past the blocks: ignored
    np.testing.assert_array_equal(read(blocks + blocks[:align - 1], None), full)   # a trailing partial block: ignored
    np.testing.assert_array_equal(read(blocks + blocks[:9], spb * 2 + 5), full[:spb * 2 + 5])
    assert len(read(blocks, 0)) == 0


def test_bad_predictor_names_file_offset_and_reason(tmp_path):
    x = wavgen.make_signal(500 * 6, 1, 2)
    blocks = bytearray(M.encode(np.round(x * 32767).astype(np.int16), 256))
    blocks[3 * 256] = 7
    p = M.write_riff(tmp_path / 'pred.wav', M.fmt(16000, 1, 256), bytes(blocks), fact=3000)
    at = M.data_offset(p) + 3 * 256
    for fn in (iss_io.decode_source, lambda q: iss_io.decode_pcm(q, ffmpeg=None)):
        with pytest.raises(ValueError, match=rf'pred\.wav: block at byte {at}: predictor'):
            fn(p)
    # garbage in that block only: the others decode as in the clean file
    got, st = _host(bytes(blocks), 1, 256)
    assert list(st) == [0, 0, 0, 2, 0, 0] and _native.ADPCM_STATUS[2].startswith('predictor')
    blocks[3 * 256] = 0
    clean, _ = _host(bytes(blocks), 1, 256)
    np.testing.assert_array_equal(got[:1500], clean[:1500])
    np.testing.assert_array_equal(got[2000:], clean[2000:])


REFUSALS = [
    ('short.wav', lambda: M.short_fmt(8000, 1, 256), 'without the 32-byte extension'),
    ('cbsize.wav', lambda: M.fmt(8000, 1, 256, cbsize=4), 'cbSize 4'),
    ('bits.wav', lambda: M.fmt(8000, 1, 256, bits=8), '8 bits per sample'),
    ('spb.wav', lambda: M.fmt(8000, 1, 256, spb=505), '505 samples per block'),
    ('ncoef.wav', lambda: M.fmt(8000, 1, 256, ncoef=8, coefs=[v for pr in zip(M.C1 + (1,), M.C2 + (2,)) for v in pr]), 'coefficient'),
    ('coefs.wav', lambda: M.fmt(8000, 1, 256, coefs=[256, 0, 512, -256, 0, 0, 192, 64, 240, 0, 460, -208, 392, -231]), 'coefficient'),
    ('extensible.wav', lambda: M.extensible_fmt(8000, 1, 256), 'WAVE_FORMAT_EXTENSIBLE'),
    ('header_only.wav', lambda: M.fmt(8000, 2, 14), 'block size 14'),
    ('under_header.wav', lambda: M.fmt(8000, 2, 9, spb=2), 'block size 9'),
    ('ragged.wav', lambda: M.fmt(8000, 3, 22), 'block size 22'),
]


@pytest.mark.parametrize('name,make,why', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_header_refusals(tmp_path, name, make, why):
    for k, writer in enumerate((M.write_riff, M.write_w64, lambda p, f, d, fact=None: M.write_rf64(p, f, d, 1000))):
        p = writer(tmp_path / name, make(), b'\0' * 1024, fact=None)
        for fn in (iss_io.decode_source, lambda q: iss_io.decode_pcm(q, ffmpeg=None)):
            with pytest.raises(ValueError, match=name.replace('.', r'\.') + r': .*WAVE format tag 2 \(MS ADPCM\).*' + why):
                fn(p)
        if k == 0:                                                # the ranged read leaves the wording to the whole-file read
            assert sndfmt.read_header(p) is None
            with pytest.raises(ValueError, match=r'WAVE format tag 2 \(MS ADPCM\)'):
                iss_io.decode_excerpts(p, [(0, None)])


def test_limits(tmp_path):
    p = M.write_riff(tmp_path / 'wide.wav', M.fmt(8000, 65, 7 * 65 + 65), b'\0' * 2080)
    with pytest.raises(ValueError, match=r'wide\.wav: MS ADPCM with 65 channels .* is not supported'):
        iss_io.decode_source(p)
    p = M.write_riff(tmp_path / 'big.wav', M.fmt(8000, 1, 32769, spb=65526), b'\0' * 32769)
    with pytest.raises(ValueError, match=r'big\.wav: MS ADPCM .*32769-byte blocks is not supported'):
        iss_io.decode_source(p)


def test_largest_block(tmp_path):
    x = wavgen.make_signal(65524 + 100, 1, 8)
    p, twin = M.write(tmp_path / 'big.wav', x, 16000, 32768)
    assert M.samples_per_block(32768, 1) == 65524
    np.testing.assert_array_equal(iss_io.decode_pcm(p, ffmpeg=None), twin)


def test_without_resample_only_16k_mono(tmp_path):
    p, _ = M.write(tmp_path / 'a8.wav', wavgen.make_signal(2000, 1, 1), 8000, 256)
    with pytest.raises(AssertionError, match='can only take files sampled at 16000 Hz'):
        iss_io.decode_pcm(p, ffmpeg=None)
    p, _ = M.write(tmp_path / 'a2.wav', wavgen.make_signal(2000, 2, 1), 16000, 512)
    with pytest.raises(ValueError, match='2 channels; without ffmpeg only mono files are supported'):
        iss_io.decode_pcm(p, ffmpeg=None)
    p, twin = M.write(tmp_path / 'a1.wav', wavgen.make_signal(2000, 1, 1), 16000, 256)
    np.testing.assert_array_equal(iss_io.media2sig16kmono(p, ffmpeg=None), twin / 32768.0)
    src = sndfmt.parse(open(p, 'rb').read(), p).source()
    assert type(src) is sndfmt.MsAdpcmSource and src.kind == 'pcm' and src.pass_order > sndfmt.AdpcmSource.pass_order


# ------------------------------------------------------------------------------------------------ golden
def test_golden_vectors():
    """tests/golden/msadpcm_vectors.npz: the crafted blocks above and their samples, produced by THIS project's own definition
    of the format (msadpcmgen.decode_block; no libsndfile or other outside decoder made them).  A regression pin: the definition
    may not drift without this file being remade on purpose."""
    g = np.load(GOLDEN)
    c = _crafted()
    assert sorted(k[:-7] for k in g.files if k.endswith('_blocks')) == sorted(c)
    for name, (blk, ch) in c.items():
        assert g[name + '_blocks'].tobytes() == blk, name
        want = g[name + '_samples']
        assert want.dtype == np.int16 and want.shape == (M.samples_per_block(len(blk), ch), ch)
        got, st = _host(blk, ch, len(blk))
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=name)
        np.testing.assert_array_equal(np.array(M.decode_block(blk, ch)[0], dtype=np.int16), want, err_msg=name)


# ------------------------------------------------------------------------------------------------ host-only twins of the device cuts
@pytest.fixture(scope='module')
def stereo8k(tmp_path_factory):
    d = tmp_path_factory.mktemp('ms')
    p, twin = M.write(d / 's.wav', wavgen.make_signal(500 * 9 + 77, 2, 21), 8000, 512)
    return p, twin


def test_decode_channels_are_columns(stereo8k):
    p, twin = stereo8k
    x, sr = iss_io.decode_source(p)
    np.testing.assert_array_equal(x, twin)
    got = iss_io.decode_channels(p, [1, 0, 1])
    for g, c in zip(got, (1, 0, 1)):
        np.testing.assert_array_equal(g, R.resample_ref(twin[:, c], 8000))


def _edge_ranges(spb, n):
    """Excerpts beginning on sample 0, 1 and 2 of a block (the header samples and the first code) and one ending on a block's
    first sample -> [(a, b)] in stored samples."""
    return [(spb * 2, spb * 2 + 700), (spb * 2 + 1, spb * 3 + 450), (spb * 2 + 2, spb * 4), (spb - 450, spb * 3 + 1), (0, n)]


def test_decode_excerpts_are_slices_16k_mono(tmp_path):
    spb = 500
    n = spb * 8 + 250
    p, twin = M.write(tmp_path / 'm.wav', wavgen.make_signal(n, 1, 22), 16000, 256)
    ab = _edge_ranges(spb, n)
    srcs = iss_io.excerpts(p, [(sec(a), sec(b)) for a, b in ab])
    assert all(type(s) is sndfmt.MsAdpcmExcerpt and s.kind == 'pcm' for s in srcs)
    assert [s.s.nblocks for s in srcs] == [2, 2, 2, 4, 9]
    for got, (a, b) in zip(iss_io.decode_excerpts(p, [(sec(a), sec(b)) for a, b in ab]), ab):
        np.testing.assert_array_equal(got, twin[a:b])


def test_decode_excerpts_and_channel_excerpts_resampled(stereo8k):
    p, twin = stereo8k
    whole = R.resample_ref(twin, 8000)
    cols = [R.resample_ref(twin[:, c], 8000) for c in (0, 1)]
    ab = [(2 * a, 2 * b) for a, b in _edge_ranges(500, len(twin))]             # 16 kHz outputs of those 8 kHz samples
    ranges = [(sec(a), sec(b)) for a, b in ab]
    for got, (a, b) in zip(iss_io.decode_excerpts(p, ranges, resample=True), ab):
        np.testing.assert_array_equal(got, whole[a:b])
    sel = [1, 1, 0]
    srcs = iss_io.channel_excerpts(p, ranges, sel, resample=True)[1]
    assert all(type(s) is sndfmt.MsAdpcmExcerpt and s.sel == sel for s in srcs)
    for got, (a, b) in zip(iss_io.decode_channel_excerpts(p, ranges, sel), ab):
        assert len(got) == 3
        for g, c in zip(got, sel):
            np.testing.assert_array_equal(g, cols[c][a:b])


def test_bad_block_outside_an_excerpt_is_not_read(tmp_path):
    x = wavgen.make_signal(500 * 8, 1, 23)
    blocks = bytearray(M.encode(np.round(x * 32767).astype(np.int16), 256))
    twin = M.decode(bytes(blocks), 1, 256)
    blocks[5 * 256] = 9
    p = M.write_riff(tmp_path / 'bad.wav', M.fmt(16000, 1, 256), bytes(blocks), fact=4000)
    np.testing.assert_array_equal(iss_io.decode_excerpts(p, [(sec(600), sec(2400))])[0], twin[600:2400])
    with pytest.raises(ValueError, match=rf'bad\.wav: block at byte {M.data_offset(p) + 5 * 256}: predictor'):
        iss_io.decode_excerpts(p, [(sec(2400), sec(2900))])


# ------------------------------------------------------------------------------------------------ bytes read
def test_an_excerpt_reads_only_its_blocks(tmp_path, monkeypatch):
    blocks = M.encode(np.round(wavgen.make_signal(500 * 32, 1, 3) * 32767).astype(np.int16), 256)
    data = bytes(blocks) * 300                                                    # 9600 blocks of 500 samples: 5 min at 16 kHz
    path = M.write_riff(tmp_path / 'long.wav', M.fmt(16000, 1, 256), data, fact=500 * 9600)
    calls = []
    real = iss_io._read_range

    def counting(p, offset, size):
        calls.append((offset, size))
        return real(p, offset, size)
    monkeypatch.setattr(iss_io, '_read_range', counting)
    a, b = 150 * 16000 + 123, 152 * 16000 + 123
    got = iss_io.decode_excerpts(path, [(sec(a), sec(b))])[0]
    k0, k1 = a // 500, (b - 1) // 500
    base = M.data_offset(path)
    assert calls[-1] == (base + k0 * 256, (k1 - k0 + 1) * 256)                    # exactly the covering blocks ...
    assert sum(s for _, s in calls[:-1]) < 200                                    # ... after the chunk headers (fmt: 50 bytes)
    assert sum(s for _, s in calls) < 0.01 * os.path.getsize(path)
    del calls[:]
    np.testing.assert_array_equal(got, iss_io.decode_pcm(path, ffmpeg=None)[a:b])
    assert not calls
