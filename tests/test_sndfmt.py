"""CPU: G.711, IMA ADPCM, AIFF / AIFF-C, AU, CAF, Wave64 and RF64 files read without ffmpeg exactly like their WAV twins
(inaspeechsegmenter_amd/sndfmt.py, the host build of csrc/adpcm.hip).  Every comparison is exact.  The outside reference is
tests/golden/sndfmt_vectors.npz (CPython's audioop, see make_sndfmt_golden.py); the files come from tests/sndgen.py."""
import os
import shutil
import struct

import numpy as np
import pytest

import sndgen
import wavgen
from conftest import GOLDEN
from inaspeechsegmenter_amd import _native, sndfmt
from inaspeechsegmenter_amd import io as iss_io

VEC = np.load(os.path.join(GOLDEN, 'sndfmt_vectors.npz'))
CASES = sndgen.cases()


# ------------------------------------------------------------------------------------------------ the decoders themselves
def test_g711_tables_equal_audioop():
    np.testing.assert_array_equal(sndfmt.ULAW_TABLE, VEC['ulaw'])
    np.testing.assert_array_equal(sndfmt.ALAW_TABLE, VEC['alaw'])
    np.testing.assert_array_equal(sndgen.ULAW, VEC['ulaw'])
    np.testing.assert_array_equal(sndgen.ALAW, VEC['alaw'])
    assert (VEC['ulaw'][0], VEC['ulaw'][255], VEC['alaw'][0]) == (-32124, 0, -5504)


def test_ima_step_equals_audioop():
    nib, pred, index, out = VEC['ima_nibbles'], VEC['ima_pred'], VEC['ima_index'], VEC['ima_out']
    assert nib.shape[0] >= 100 and nib.shape[1] % 8 == 0
    align = 4 + nib.shape[1] // 2
    blocks = b''.join(sndgen.ima_block(nib[k], pred[k], index[k]) for k in range(len(nib)))
    want = np.concatenate((pred[:, None], out), axis=1).reshape(-1)
    got, st = _native.adpcm_decode_host(np.frombuffer(blocks, np.uint8), len(nib), 1, align, want.size)
    assert not st.any()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(sndgen.ima_decode(blocks, 1, align), want)


# ------------------------------------------------------------------------------------------------ every file like its twin
def _outcome(fn, path):
    """('ok', result) or ('err', exception type, its text with the file's name taken out)."""
    try:
        return ('ok', fn(path))
    except (AssertionError, ValueError, NotImplementedError) as exc:
        return ('err', type(exc), str(exc).replace(str(path), '<file>'))


def _same(a, b):
    assert a[0] == b[0], (a, b)
    if a[0] == 'err':
        assert a[1:] == b[1:]
        return
    ra, rb = a[1], b[1]
    if isinstance(ra, tuple):                                     # decode_source: (samples, rate)
        assert ra[1] == rb[1]
        ra, rb = ra[0], rb[0]
    assert ra.dtype == rb.dtype and ra.shape == rb.shape, (ra.dtype, rb.dtype, ra.shape, rb.shape)
    np.testing.assert_array_equal(ra, rb)


def _like_twin(path, twin):
    _same(_outcome(iss_io.decode_source, path), _outcome(iss_io.decode_source, twin))
    _same(_outcome(lambda p: iss_io.decode_pcm(p, ffmpeg=None), path), _outcome(lambda p: iss_io.decode_pcm(p, ffmpeg=None), twin))
    for dt in ('float64', 'float32'):
        fn = lambda p: iss_io.media2sig16kmono(p, ffmpeg=None, dtype=dt)      # noqa: E731
        _same(_outcome(fn, path), _outcome(fn, twin))


@pytest.mark.parametrize('container,kind,big', CASES, ids=['%s-%s-%s' % (c, k, 'be' if b else 'le') for c, k, b in CASES])
def test_reads_like_wav_twin(tmp_path, container, kind, big):
    for ch in (1, 2, 5):
        for sr in (8000, 16000, 44100):
            x = wavgen.make_signal(2500 + 131 * ch + sr // 1000, ch, 7 * ch + sr % 97)
            p, tfmt, twin = sndgen.write(tmp_path / f'{container}_{ch}_{sr}.snd', container, kind, big, x, sr)
            w = sndgen.wav_twin(tmp_path / f'{container}_{ch}_{sr}.wav', twin, sr, tfmt)
            a, rate = iss_io.decode_source(p)
            assert rate == sr and a.dtype == wavgen.as_read(twin, tfmt).dtype
            np.testing.assert_array_equal(a, wavgen.as_read(twin, tfmt))
            _like_twin(p, w)
            if ch == 1 and sr == 16000:
                assert _outcome(lambda q: iss_io.decode_pcm(q, ffmpeg=None), p)[0] == 'ok'


def test_renamed_files_are_read_by_their_bytes(tmp_path):
    x = wavgen.make_signal(4000, 1, 3)
    for container, kind, big in (('aiff', 'i16', True), ('au', 'ulaw', True), ('caf', 'f32', False), ('w64', 'ima', False)):
        p, tfmt, twin = sndgen.write(tmp_path / f'{container}.wav', container, kind, big, x, 16000)
        w = sndgen.wav_twin(tmp_path / f'{container}_twin.wav', twin, 16000, tfmt)
        _like_twin(p, w)
        q = str(shutil.copy(p, tmp_path / f'{container}.flac'))
        _like_twin(q, w)


def test_start_stop_stay_not_implemented(tmp_path):
    p, _, _ = sndgen.write(tmp_path / 'a.au', 'au', 'ulaw', True, wavgen.make_signal(4000, 1, 3), 16000)
    with pytest.raises(NotImplementedError):
        iss_io.decode_pcm(p, start_sec=1.0, ffmpeg=None)


# ------------------------------------------------------------------------------------------------ IMA ADPCM geometry
@pytest.mark.parametrize('block_align', [256, 512, 1024, 2048])
@pytest.mark.parametrize('ch', [1, 2, 3, 5])
def test_ima_block_sizes_and_channels(tmp_path, block_align, ch):
    x = wavgen.make_signal(9000, ch, block_align + ch)
    p, tfmt, twin = sndgen.write(tmp_path / 'a.wav', 'wav', 'ima', False, x, 16000, block_align=block_align)
    assert len(twin) == 9000
    _like_twin(p, sndgen.wav_twin(tmp_path / 't.wav', twin, 16000, tfmt))


def test_ima_fact_and_partial_blocks(tmp_path):
    x = wavgen.make_signal(5050, 2, 1)                            # 2 channels, 256-byte blocks: 249 samples per block
    pcm = wavgen.encode(x, 'i16')
    blocks = sndgen.ima_encode(pcm, 256)
    spb = sndgen.ima_samples_per_block(256, 2)
    nb = len(blocks) // 256
    full = sndgen.ima_decode(blocks, 2, 256)
    assert nb * spb > 5050 and len(full) == nb * spb
    fmt = sndgen.wav_fmt('ima', 16000, 2, 256)

    def read(**kw):
        sndgen.write_riff(tmp_path / 'f.wav', fmt, **kw)
        return iss_io.decode_source(str(tmp_path / 'f.wav'))[0]
    np.testing.assert_array_equal(read(data=blocks, fact=5050), full[:5050])               # a count that cuts the last block
    np.testing.assert_array_equal(read(data=blocks, fact=None), full)                      # no fact: whole blocks
    np.testing.assert_array_equal(read(data=blocks, fact=nb * spb + 1), full)              # a count past the blocks: ignored
    np.testing.assert_array_equal(read(data=blocks + blocks[:100], fact=None), full)       # a trailing partial block: ignored
    np.testing.assert_array_equal(read(data=blocks + blocks[:100], fact=5050), full[:5050])
    np.testing.assert_array_equal(read(data=blocks, fact=spb * 3 - 7), full[:spb * 3 - 7])  # a count several blocks short
    np.testing.assert_array_equal(read(data=blocks, fact=0), full[:0])


def test_ima_refusals(tmp_path):
    x = wavgen.make_signal(3000, 1, 1)
    blocks = bytearray(sndgen.ima_encode(wavgen.encode(x, 'i16'), 256))
    fmt = sndgen.wav_fmt('ima', 16000, 1, 256)
    blocks[2 * 256 + 2] = 89                                      # third block's step index
    p = sndgen.write_riff(tmp_path / 'idx.wav', fmt, bytes(blocks), fact=3000)
    base = open(p, 'rb').read().index(b'data') + 8
    with pytest.raises(ValueError, match=rf'idx\.wav: block at byte {base + 512}: step index above 88'):
        iss_io.decode_source(p)
    for name, kw, why in (('spb.wav', dict(spb=500), 'samples per block'), ('align.wav', dict(block_align=258), 'block size 258'),
                          ('bits.wav', dict(bits=3), '3-bit IMA ADPCM')):
        args = dict(kind='ima', sr=16000, ch=1, block_align=256)
        args.update(kw)
        p = sndgen.write_riff(tmp_path / name, sndgen.wav_fmt(**args), bytes(blocks[:512]))
        with pytest.raises(ValueError, match=name.replace('.', r'\.') + ': .*' + why):
            iss_io.decode_source(p)


# ------------------------------------------------------------------------------------------------ container details
def test_rf64_chunk_after_the_samples_is_not_audio(tmp_path):
    x = wavgen.make_signal(4000, 2, 5)
    for kind in ('i16', 'ulaw', 'f32'):
        data, tfmt, twin, n = sndgen.encode(x, kind)
        fmt = sndgen.wav_fmt(kind, 16000, 2)
        p = sndgen.write_riff(tmp_path / 'r.wav', fmt, data, magic=b'RF64', ds64=(len(data), n),
                              after=[(b'LIST', b'INFOISFT' + struct.pack('<I', 8) + b'sndgen\0\0'), (b'junk', b'\x11' * 4001)])
        a, sr = iss_io.decode_source(p)
        assert a.shape == (4000, 2)
        np.testing.assert_array_equal(a, wavgen.as_read(twin, tfmt))
    # a plain RIFF file with the same size field keeps its meaning: a piped WAV, to the end of the buffer
    data, tfmt, twin, n = sndgen.encode(x, 'i16')
    p = sndgen.write_riff(tmp_path / 'pipe.wav', sndgen.wav_fmt('i16', 16000, 2), data, unknown_size=True, after=[(b'junk', b'\0' * 40)])
    assert iss_io.decode_source(p)[0].shape == (4000 + 12, 2)


def test_odd_sized_chunks_before_the_audio(tmp_path):
    x = wavgen.make_signal(3001, 1, 9)
    for kind in ('i16', 'alaw', 'ima'):
        data, tfmt, twin, n = sndgen.encode(x, kind)
        p = sndgen.write_w64(tmp_path / 'o.w64', sndgen.wav_fmt(kind, 16000, 1), data, fact=n if kind != 'i16' else None,
                             before=[(b'junk', b'\x07' * 13), (b'LIST', b'\x01' * 3)])
        _like_twin(p, sndgen.wav_twin(tmp_path / 'o.wav', twin, 16000, tfmt))
    for kind, big in (('i16', True), ('i8', True), ('ulaw', False)):
        data, tfmt, twin, n = sndgen.encode(x, kind, big)
        w = sndgen.wav_twin(tmp_path / 'o.wav', twin, 16000, tfmt)
        p = sndgen.write_aiff(tmp_path / 'o.aif', kind, big, data, 16000, 1, n, before=[(b'NAME', b'odd'), (b'ANNO', b'seven b')])
        _like_twin(p, w)
        p = sndgen.write_aiff(tmp_path / 'o2.aif', kind, big, data, 16000, 1, n, ssnd_offset=6, ssnd_first=True)
        _like_twin(p, w)


def test_aiff_sample_size_is_left_justified_in_its_container(tmp_path):
    x = wavgen.make_signal(3000, 2, 2)
    s = (wavgen.encode(x, 'i16').astype(np.int32) >> 4) << 4      # 12 bits in 2 bytes
    p = sndgen.write_aiff(tmp_path / 'a12.aif', 'i16', True, s.astype('>i2').tobytes(), 16000, 2, 3000, bits=12)
    a, _ = iss_io.decode_source(p)
    assert a.dtype == np.int16
    np.testing.assert_array_equal(a, s.astype(np.int16))
    s = (wavgen.encode(x, 'i24') >> 4) << 4                       # 20 bits in 3 bytes
    raw = np.ascontiguousarray(s.astype('<i4').reshape(-1, 1).view(np.uint8)[:, 2::-1]).tobytes()
    p = sndgen.write_aiff(tmp_path / 'a20.aif', 'i24', True, raw, 16000, 2, 3000, bits=20)
    np.testing.assert_array_equal(iss_io.decode_source(p)[0], s.astype(np.int32) << 8)


def test_unknown_sizes_run_to_the_end(tmp_path):
    x = wavgen.make_signal(3000, 1, 4)
    data, tfmt, twin, n = sndgen.encode(x, 'ulaw')
    for p in (sndgen.write_au(tmp_path / 'u.au', 'ulaw', data, 16000, 1, unknown_size=True),
              sndgen.write_caf(tmp_path / 'u.caf', 'ulaw', True, data, 16000, 1, unknown_size=True)):
        np.testing.assert_array_equal(iss_io.decode_source(p)[0], twin)


REFUSALS = [
    ('gsm.w64', lambda p: sndgen.write_w64(p, sndgen.wav_fmt(None, 8000, 1, tag=0x31, bits=0), b'\0' * 650), r'format tag 49 \(GSM 06\.10\)'),
    ('msadpcm.rf64', lambda p: sndgen.write_riff(p, sndgen.wav_fmt(None, 8000, 1, tag=2, bits=4), b'\0' * 512, magic=b'RF64',
                                                 ds64=(512, 1000)), r'format tag 2 \(MS ADPCM\)'),
    ('msadpcm.wav', lambda p: sndgen.write_riff(p, sndgen.wav_fmt(None, 8000, 1, tag=2, bits=4), b'\0' * 512), 'format tag 2'),
    ('g726.wav', lambda p: sndgen.write_riff(p, sndgen.wav_fmt(None, 8000, 1, tag=0x45, bits=4), b'\0' * 512), 'format tag 69'),
    ('ima4.aifc', lambda p: sndgen.write_aiff(p, 'i16', True, b'\0' * 340, 44100, 1, 640, aifc=True, ctype=b'ima4'), "compression type 'ima4'"),
    ('mace.aifc', lambda p: sndgen.write_aiff(p, 'i16', True, b'\0' * 340, 22050, 1, 640, aifc=True, ctype=b'MAC3'), "compression type 'MAC3'"),
    ('gsm.aifc', lambda p: sndgen.write_aiff(p, 'i16', True, b'\0' * 330, 8000, 1, 1600, aifc=True, ctype=b'GSM '), "compression type 'GSM '"),
    ('ima4.caf', lambda p: sndgen.write_caf(p, 'i16', True, b'\0' * 340, 44100, 1, fmtid=b'ima4'), "CAF format 'ima4'"),
    ('alac.caf', lambda p: sndgen.write_caf(p, 'i16', True, b'\0' * 340, 44100, 2, fmtid=b'alac'), "CAF format 'alac'"),
    ('v2.caf', lambda p: sndgen.write_caf(p, 'i16', True, b'\0' * 340, 44100, 2, version=2), 'CAF version 2'),
    ('g721.au', lambda p: sndgen.write_au(p, 'ulaw', b'\0' * 400, 8000, 1, enc=23), r'AU encoding 23 \(G\.721 ADPCM\)'),
    ('g723.au', lambda p: sndgen.write_au(p, 'ulaw', b'\0' * 400, 8000, 1, enc=25), 'AU encoding 25'),
    ('rate.aif', lambda p: sndgen.write_aiff(p, 'i16', True, b'\0' * 400, '44100.5', 1, 200), r'sample rate 44100\.5 Hz is not a whole number'),
    ('rate.caf', lambda p: sndgen.write_caf(p, 'i16', True, b'\0' * 400, 44100.5, 1), r'sample rate 44100\.5 Hz is not a whole number'),
]


@pytest.mark.parametrize('name,make,why', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_file_and_the_encoding(tmp_path, name, make, why):
    p = make(tmp_path / name)
    for fn in (iss_io.decode_source, lambda q: iss_io.decode_pcm(q, ffmpeg=None), lambda q: iss_io.media2sig16kmono(q, ffmpeg=None)):
        with pytest.raises(ValueError, match=name.replace('.', r'\.') + ': .*' + why):
            fn(p)


def test_truncated_headers(tmp_path):
    x = wavgen.make_signal(2000, 1, 1)
    for container, kind, big, cut, what in (('aiff', 'i16', True, 30, 'AIFF'), ('au', 'ulaw', True, 14, 'AU'), ('caf', 'i16', True, 40, 'CAF'),
                                            ('w64', 'ulaw', False, 70, 'Wave64'), ('rf64', 'i16', False, 30, 'WAVE')):
        p, _, _ = sndgen.write(tmp_path / f't.{container}', container, kind, big, x, 16000)
        q = tmp_path / f'cut.{container}'
        q.write_bytes(open(p, 'rb').read()[:cut])
        with pytest.raises(ValueError, match=rf'cut\.{container}: (truncated {what} header|missing .* chunk)'):
            iss_io.decode_source(str(q))


def test_bytes_of_no_container_keep_their_error(tmp_path):
    for name, data in (('a.bin', b'\x00' * 64), ('b.aif', b'FORM\0\0\0\x10WAVEfmt \0\0\0\0'), ('c.mp3', b'ID3\x03' + b'\0' * 60),
                       ('d.caf', b'caf')):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError, match='not a RIFF/WAVE file'):
            iss_io.decode_source(str(tmp_path / name))


def test_truncated_plain_wav_keeps_its_error(tmp_path):
    x = wavgen.encode(wavgen.make_signal(500, 1, 1), 'i16')
    data = open(wavgen.write_wav(tmp_path / 'full.wav', x, 16000, 'i16'), 'rb').read()
    for cut in (22, 30):                                          # inside the fmt chunk
        (tmp_path / 'cut.wav').write_bytes(data[:cut])
        with pytest.raises(Exception) as want:
            iss_io._parse_wav(data[:cut], 'cut.wav')
        with pytest.raises(type(want.value)) as got:
            iss_io.decode_source(str(tmp_path / 'cut.wav'))
        assert str(got.value) == str(want.value)


def test_float_of_another_width_is_refused(tmp_path):
    p = sndgen.write_w64(tmp_path / 'f16.w64', sndgen.wav_fmt(None, 16000, 1, tag=3, bits=16), b'\0' * 400)
    with pytest.raises(ValueError, match=r'f16\.w64: unsupported IEEE float width 16'):
        iss_io.decode_source(p)


@pytest.mark.parametrize('block_align', [16380, 32768])
def test_ima_largest_blocks(tmp_path, block_align):
    x = wavgen.make_signal(70000, 1, block_align)
    p, tfmt, twin = sndgen.write(tmp_path / 'big.wav', 'wav', 'ima', False, x, 16000, block_align=block_align)
    _like_twin(p, sndgen.wav_twin(tmp_path / 't.wav', twin, 16000, tfmt))
    fmt = sndgen.wav_fmt('ima', 16000, 2, 32776)
    q = sndgen.write_riff(tmp_path / 'over.wav', fmt, b'\0' * 32776)
    with pytest.raises(ValueError, match=r'over\.wav: IMA ADPCM .* is not supported'):
        iss_io.decode_source(q)
