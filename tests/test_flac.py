"""FLAC read without ffmpeg (CPU): the host build of the frame decoder against tests/flacgen.py over the syntax matrix,
hand-assembled frames, malformed streams, and the io entry points against each file's WAV twin."""
import os

import numpy as np
import pytest

import flacgen
from conftest import GOLDEN, synth_pcm
from inaspeechsegmenter_amd import flac, _native
from inaspeechsegmenter_amd import io as iss_io


def _signal(n, ch, bps, seed):
    """Integer samples within `bps` bits: speech-like synthetic audio, one column per channel."""
    base = synth_pcm(seed, n).astype(np.int64)
    cols = [np.roll(base, 31 * c) + (c * 97 % 200 - 100) for c in range(ch)]
    x = np.stack(cols, axis=1)
    x = (x << 8) + np.random.default_rng(seed).integers(-128, 128, x.shape) if bps == 24 else x >> (16 - bps)
    x = np.clip(x, -(1 << (bps - 1)), (1 << (bps - 1)) - 1)
    return x[:, 0] if ch == 1 else x


def _stored(x, bps):
    """What the decoder returns (the WAV twin's stored samples): int16 x << (16 - bps), or int32 x << 8."""
    x = np.asarray(x, dtype=np.int64)
    return (x << 8).astype(np.int32) if bps == 24 else (x << (16 - bps)).astype(np.int16)


def _roundtrip(data, x, bps, sr=None):
    y, rate = flac.read_host(data, 'mem.flac')
    assert y.dtype == (np.int32 if bps == 24 else np.int16)
    np.testing.assert_array_equal(y, _stored(x, bps))
    if sr is not None:
        assert rate == sr


def test_crc_check_values():
    assert flacgen.crc8(b'123456789') == 0xF4
    assert flacgen.crc16(b'123456789') == 0xFEE8
    assert _native.flac_crc(b'123456789') == (0xF4, 0xFEE8)


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize('ch', range(1, 9))
@pytest.mark.parametrize('bps', [8, 16, 24])
def test_roundtrip_channels_and_widths(ch, bps):
    x = _signal(5000, ch, bps, seed=ch)
    _roundtrip(flacgen.encode(x, 16000, bps, blocksize=1152), x, bps, 16000)


@pytest.mark.parametrize('mode', ['left_side', 'side_right', 'mid_side'])
@pytest.mark.parametrize('bps', [8, 16, 24])
def test_roundtrip_stereo_decorrelation(mode, bps):
    x = _signal(6000, 2, bps, seed=5)
    x[:, 1] = np.clip(-x[:, 0] + 3, -(1 << (bps - 1)), (1 << (bps - 1)) - 1)     # wide side channel, odd sides
    x[100:200, 1] = -(1 << (bps - 1))
    x[100:200, 0] = (1 << (bps - 1)) - 1
    for sub in ({'type': 'realistic'}, {'type': 'verbatim'}, {'type': 'fixed', 'order': 2}):
        _roundtrip(flacgen.encode(x, 44100, bps, blocksize=2048, channel_mode=mode, subframe=sub), x, bps)


SUBFRAMES = ([{'type': 'verbatim'}] + [{'type': 'fixed', 'order': o} for o in range(5)] +
             [{'type': 'lpc', 'order': o, 'precision': p} for o in (1, 2, 3, 5, 8, 9, 12, 16, 17, 24, 31, 32)
              for p in (5, 12, 15)] +
             [{'type': 'lpc', 'order': 8, 'precision': 15, 'shift': 0}, {'type': 'lpc', 'order': 4, 'precision': 15, 'shift': 15}])


@pytest.mark.parametrize('spec', SUBFRAMES, ids=lambda s: '-'.join(f'{k}{v}' for k, v in s.items()))
@pytest.mark.parametrize('bps', [16, 24])
def test_roundtrip_subframe_types(spec, bps):
    x = _signal(8192, 1, bps, seed=11)
    _roundtrip(flacgen.encode(x, 16000, bps, blocksize=4096, subframe=spec), x, bps)


def test_roundtrip_constant_wasted_rice2_escape_partitions():
    x = _signal(8192, 1, 16, seed=3)
    x[:4096] = -1234
    _roundtrip(flacgen.encode(x, 16000, 16, subframe=lambda f, c: {'type': 'constant'} if f == 0 else {'type': 'realistic'}),
               x, 16)
    for k in (1, 3, 7):
        w = (x >> k) << k
        _roundtrip(flacgen.encode(w, 16000, 16, subframe={'type': 'fixed', 'order': 2}), w, 16)
        _roundtrip(flacgen.encode(w, 16000, 16, subframe={'type': 'lpc', 'order': 6, 'precision': 14}), w, 16)
    for porder in range(0, 9):
        for rice2 in (False, True):
            for esc in (False, True):
                spec = {'type': 'fixed', 'order': 1, 'porder': porder, 'rice2': rice2, 'escape': esc}
                _roundtrip(flacgen.encode(x, 16000, 16, subframe=spec), x, 16)
    z = np.zeros(4096, np.int64)
    z[2000:2100] = 5
    _roundtrip(flacgen.encode(z, 16000, 16, subframe={'type': 'fixed', 'order': 0, 'porder': 4, 'escape': True}), z, 16)
    _roundtrip(flacgen.encode(x, 16000, 16, subframe={'type': 'fixed', 'order': 1, 'ks': [14]}), x, 16)
    _roundtrip(flacgen.encode(x, 16000, 16, subframe={'type': 'fixed', 'order': 1, 'rice2': True, 'ks': [0]}), x, 16)


BLOCKS = [192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 100, 3000]


@pytest.mark.parametrize('bs', BLOCKS)
def test_roundtrip_block_size_codes(bs):
    x = _signal(2 * bs + 77, 1, 16, seed=bs)                      # two full frames and a short last one
    data = flacgen.encode(x, 16000, 16, blocksize=bs)
    _roundtrip(data, x, 16)
    _roundtrip(flacgen.encode(x, 16000, 16, blocksize=bs, bs_code=7), x, 16)
    if bs <= 256:
        _roundtrip(flacgen.encode(x, 16000, 16, blocksize=bs, bs_code=6), x, 16)


@pytest.mark.parametrize('sr,code', [(88200, None), (176400, None), (192000, None), (8000, None), (16000, None),
                                     (22050, None), (24000, None), (32000, None), (44100, None), (48000, None),
                                     (96000, None), (16000, 0), (16000, 12), (16000, 13), (16000, 14), (11025, 13),
                                     (37000, 12), (96010, 14), (100001, 0)])
def test_roundtrip_rate_codes(sr, code):
    x = _signal(3000, 1, 16, seed=7)
    data = flacgen.encode(x, sr, 16, blocksize=1024, rate_code=code)
    _roundtrip(data, x, 16, sr)


def test_roundtrip_variable_blocking_short_last_frame_and_numbers():
    x = _signal(50000, 2, 16, seed=9)
    sizes = [192, 4096, 17, 1, 1000, 4608, 256] * 4
    sizes.append(x.shape[0] - sum(sizes))
    _roundtrip(flacgen.encode(x, 16000, 16, blocksize=sizes, variable=True, channel_mode='mid_side'), x, 16)
    y = _signal(16 * 300 + 5, 1, 16, seed=1)                       # 301 frames: 2-byte frame numbers
    _roundtrip(flacgen.encode(y, 16000, 16, blocksize=16), y, 16)
    _roundtrip(flacgen.encode(y, 16000, 16, blocksize=16, ss_code=0, rate_code=0), y, 16)
    _roundtrip(flacgen.encode(y, 16000, 16, blocksize=16, total_in_streaminfo=False), y, 16)


@pytest.mark.parametrize('meta', [(1,), (2,), (3,), (4,), (5,), (6,), (3, 4, 6, 1), (7, 2)])
def test_roundtrip_metadata_blocks_and_id3(meta):
    x = _signal(5000, 1, 16, seed=2)
    _roundtrip(flacgen.encode(x, 16000, 16, metadata=meta), x, 16)
    _roundtrip(flacgen.encode(x, 16000, 16, metadata=meta, id3=True), x, 16)


# ------------------------------------------------------------------------------------------------ hand-assembled frames
def _b(bits):
    bits = bits.replace(' ', '')
    return int(bits, 2).to_bytes(len(bits) // 8, 'big') if bits else b''


def _s(v, w):
    return format(v & ((1 << w) - 1), f'0{w}b') if w else ''


def _stream(frame_bits_after_header, bs, ch_code, ch, bps=16, sr=16000):
    """fLaC + STREAMINFO + one frame: header (16 kHz code, explicit 8-bit block size, frame 0), the given subframe bits,
    zero padding, CRC-16."""
    ss = {8: '001', 16: '100', 24: '110'}[bps]
    hdr = _b('11111111 11111000' + '0110' + '0101' + _s(ch_code, 4) + ss + '0' + '00000000' + _s(bs - 1, 8))
    hdr += bytes([flacgen.crc8(hdr)])
    body = frame_bits_after_header.replace(' ', '')
    body += '0' * (-len(body) % 8)
    frame = hdr + _b(body)
    frame += flacgen.crc16(frame).to_bytes(2, 'big')
    return b'fLaC' + bytes([0x80, 0, 0, 34]) + flacgen.streaminfo(bs, bs, sr, ch, bps, bs) + frame


def test_hand_frame_mid_side_odd_side():
    L, R = [10, -3, 7, 0], [5, -8, 2, 1]
    mid, side = [7, -6, 4, 0], [5, 5, 5, -1]
    bits = '0 000001 0' + ''.join(_s(v, 16) for v in mid) + '0 000001 0' + ''.join(_s(v, 17) for v in side)
    y, _ = flac.read_host(_stream(bits, 4, 10, 2), 'ms.flac')
    np.testing.assert_array_equal(y, np.array([L, R]).T)


def test_hand_frame_lpc_negative_coefficients_and_shift():
    # order 2, precision 4, shift 2, coefficients (-3, 2): the first multiplies the most recent sample; floor(sum >> 2)
    bits = ('0 100001 0' + _s(100, 16) + _s(-50, 16) + '0011' + '00010' + _s(-3, 4) + _s(2, 4) +
            '00 0000 0001' + '010' + '011' + '10' + '00010')              # Rice k=1: residuals 1, -2, 0, 3
    y, _ = flac.read_host(_stream(bits, 6, 0, 1), 'lpc.flac')
    np.testing.assert_array_equal(y, [100, -50, 88, -93, 113, -129])


def test_hand_frame_fixed4_with_wasted_bits():
    # wasted k = 2 (flag, one zero, a one): 14-bit warm-up 1 2 4 8, residuals 0 1 -1 2 with k = 0
    bits = '0 001100 1 01' + ''.join(_s(v, 14) for v in (1, 2, 4, 8)) + '00 0000 0000' + '1' + '001' + '01' + '00001'
    y, _ = flac.read_host(_stream(bits, 8, 0, 1), 'w.flac')
    np.testing.assert_array_equal(y, [4, 8, 16, 32, 60, 108, 180, 288])


def test_hand_frame_escape_width_zero():
    bits = '0 001001 0' + _s(500, 16) + '00 0000 1111 00000'
    y, _ = flac.read_host(_stream(bits, 4, 0, 1), 'e.flac')
    np.testing.assert_array_equal(y, [500] * 4)
    bits = '0 001001 0' + _s(-7, 16) + '01 0000 11111 00000'                  # Rice2 escape
    y, _ = flac.read_host(_stream(bits, 4, 0, 1), 'e2.flac')
    np.testing.assert_array_equal(y, [-7] * 4)


def _coded(v, n):
    if n == 1:
        return _s(v, 8)
    first = '1' * n + '0' + _s(v >> (6 * (n - 1)), 7 - n)
    return first + ''.join('10' + _s(v >> (6 * k), 6) for k in range(n - 2, -1, -1))


@pytest.mark.parametrize('n,v', [(1, 5), (2, 0x7FF), (3, 0xFFFF), (4, 0x1FFFFF), (5, 0x3FFFFFF), (6, 0x7FFFFFFF),
                                 (7, 0xFFFFFFFFF)])
def test_hand_coded_numbers(n, v):
    """1..7-byte coded numbers: the index parses the number and reports it as a sequence break of a first frame."""
    for variable in ((False, True) if n < 7 else (True,)):
        hdr = _b('11111111 1111100' + str(int(variable)) + '0110 0101 0000 100 0' + _coded(v, n) + _s(3, 8))
        hdr += bytes([flacgen.crc8(hdr)])
        body = hdr + _b('0 000000 0' + _s(0, 16) + '')
        frame = body + flacgen.crc16(body).to_bytes(2, 'big')
        data = b'fLaC' + bytes([0x80, 0, 0, 34]) + flacgen.streaminfo(4, 4, 16000, 1, 16, 0) + frame
        what = 'sample number' if variable else 'frame number'
        with pytest.raises(ValueError, match=rf'x.flac: frame at byte 42: frame-sequence break \({what} {v}, expected 0\)'):
            flac.read_host(data, 'x.flac')
    bad = _b('11111111 11111000 0110 0101 0000 100 0' + '11111110' + '10000000' * 6 + _s(3, 8))      # 7 bytes, fixed
    bad += bytes([flacgen.crc8(bad)])
    data = b'fLaC' + bytes([0x80, 0, 0, 34]) + flacgen.streaminfo(4, 4, 16000, 1, 16, 0) + bad + b'\0' * 8
    with pytest.raises(ValueError, match='frame at byte 42: invalid coded number'):
        flac.read_host(data, 'x.flac')


# ------------------------------------------------------------------------------------------------ malformed streams
def _plain(n=4096 * 5, seed=4):
    x = _signal(n, 1, 16, seed)
    data, offs = flacgen.encode(x, 16000, 16, blocksize=4096, return_offsets=True)
    return x, bytearray(data), offs


def _raises(data, pattern):
    with pytest.raises(ValueError, match=pattern):
        flac.read_host(bytes(data), 'bad.flac')


def test_malformed_crc8_crc16_reserved_sequence():
    x, d, offs = _plain()
    b = bytearray(d); b[offs[2] + 5] ^= 0x01                                       # frame 2's CRC-8 byte
    _raises(b, rf'bad.flac: frame at byte {offs[2]}: header CRC-8 mismatch')
    b = bytearray(d); b[offs[2] - 1] ^= 0x40                                       # frame 1's CRC-16
    _raises(b, rf'bad.flac: frame at byte {offs[1]}: CRC-16 mismatch')
    b = bytearray(d); b[offs[3] + 100] ^= 0x10                                     # frame 3's data
    with pytest.raises(ValueError, match=rf'bad.flac: frame at byte {offs[3]}: '):
        flac.read_host(bytes(b), 'bad.flac')
    b = bytearray(d); b[offs[0] + 2] &= 0x0F                                       # block size code 0000
    b[offs[0] + 5] = flacgen.crc8(bytes(b[offs[0]:offs[0] + 5]))
    _raises(b, rf'bad.flac: frame at byte {offs[0]}: reserved block size code')
    b = bytearray(d); b[offs[0] + 3] = (b[offs[0] + 3] & 0xF1) | (3 << 1)          # sample size code 011
    b[offs[0] + 5] = flacgen.crc8(bytes(b[offs[0]:offs[0] + 5]))
    _raises(b, rf'frame at byte {offs[0]}: reserved sample size code')
    b = d[:offs[1]] + d[offs[2]:]                                                 # frame 1 missing
    _raises(b, rf'bad.flac: frame at byte {offs[1]}: frame-sequence break')


def test_malformed_totals_and_truncation():
    x, d, offs = _plain()
    si = 8 + 10                                                                   # STREAMINFO's rate/ch/bps/total field
    for total in (x.size + 1, x.size - 1):
        b = bytearray(d)
        v = int.from_bytes(b[si:si + 8], 'big') & ~((1 << 36) - 1) | total
        b[si:si + 8] = v.to_bytes(8, 'big')
        _raises(b, rf'frame at byte {offs[-1]}: .*STREAMINFO total')
    for cut in (1, 2, 10, 300):
        with pytest.raises(ValueError, match=rf'bad.flac: frame at byte {offs[-1]}: '):
            flac.read_host(bytes(d[:-cut]), 'bad.flac')


def test_malformed_residual_overrun_footer_and_codes():
    with pytest.raises(ValueError, match='frame at byte 42: residual overruns the frame'):
        flac.read_host(_stream('0 001001 0' + _s(500, 16) + '00 0000 0000', 4, 0, 1), 'o.flac')
    with pytest.raises(ValueError, match='frame at byte 42: subframes end before the footer'):
        flac.read_host(_stream('0 001001 0' + _s(500, 16) + '00 0000 1111 00000' + '0' * 16, 4, 0, 1), 'f.flac')
    cases = {'0 000010 0': 'reserved subframe type', '0 001101 0': 'reserved subframe type',
             '1 000001 0': 'subframe header padding bit set',
             '0 001001 0' + _s(5, 16) + '10 0000': 'reserved residual coding method',
             '0 001001 0' + _s(5, 16) + '00 0011 0000': 'residual partition order does not fit the block',
             '0 100000 0' + _s(5, 16) + '1111 00000': 'invalid LPC precision',
             '0 100000 0' + _s(5, 16) + '0011 11110 0001': 'negative LPC shift',
             '0 000000 1' + '0' * 16 + '1' + _s(5, 1): 'wasted bits exceed the sample size',
             '0 001000 0' + '00 0000 1111 00000' + '1': 'nonzero padding before the footer'}
    for bits, why in cases.items():
        with pytest.raises(ValueError, match=f'frame at byte 42: {why}'):
            flac.read_host(_stream(bits, 4, 0, 1), 'c.flac')


def test_false_sync_inside_verbatim_is_not_a_frame():
    x = _signal(8192, 1, 16, seed=6).astype(np.int64)
    fake = flacgen.frame_header(4096, 16000, 0, 16, 0, False)                      # a valid header of frame 0, again
    assert len(fake) == 6
    words = np.frombuffer(fake, dtype='>i2').astype(np.int64)
    x[1000:1003] = words
    data = flacgen.encode(x, 16000, 16, blocksize=4096, subframe={'type': 'verbatim'})
    assert data.count(fake) == 2
    _roundtrip(data, x, 16)


def test_unsupported_widths_and_ogg():
    x = _signal(3000, 1, 16, seed=1) >> 4
    for bps in (12, 20):
        with pytest.raises(ValueError, match=f'{bps}-bit FLAC is not supported'):
            flac.read_host(flacgen.encode(x, 16000, bps), 'w.flac')
    hdr = b'fLaC' + bytes([0x80, 0, 0, 34]) + flacgen.streaminfo(4096, 4096, 16000, 1, 32, 0)
    with pytest.raises(ValueError, match='32-bit FLAC is not supported'):
        flac.read_host(hdr, 'w.flac')


# ------------------------------------------------------------------------------------------------ io semantics (WAV twins)
def _twins(tmp_path, x, sr, bps, name, **kw):
    f = flacgen.write(tmp_path / f'{name}.flac', x, sr, bps, **kw)
    w = flacgen.wav_twin(tmp_path / f'{name}.wav', x, sr, bps)
    return f, w


@pytest.mark.parametrize('bps', [8, 16, 24])
def test_io_16k_mono_reads_like_wav_twin(tmp_path, bps):
    x = _signal(20000, 1, bps, seed=bps)
    f, w = _twins(tmp_path, x, 16000, bps, 'm')
    a, b = iss_io.decode_pcm(f, ffmpeg=None), iss_io.decode_pcm(w, ffmpeg=None)
    assert a.dtype == b.dtype == (np.float32 if bps == 24 else np.int16)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(iss_io.media2sig16kmono(f, ffmpeg=None), iss_io.media2sig16kmono(w, ffmpeg=None))
    np.testing.assert_array_equal(iss_io.media2sig16kmono(f, ffmpeg=None, dtype='float32'),
                                  iss_io.media2sig16kmono(w, ffmpeg=None, dtype='float32'))
    (sa, ra), (sb, rb) = iss_io.decode_source(f), iss_io.decode_source(w)
    assert ra == rb == 16000 and sa.dtype == sb.dtype
    np.testing.assert_array_equal(sa, sb)


@pytest.mark.parametrize('sr,ch,bps', [(44100, 1, 16), (48000, 2, 24), (16000, 2, 16), (22050, 3, 8)])
def test_io_other_rates_and_channels_like_wav_twin(tmp_path, sr, ch, bps):
    x = _signal(9000, ch, bps, seed=sr % 97)
    f, w = _twins(tmp_path, x, sr, bps, 'o', channel_mode='mid_side' if ch == 2 else 'independent')
    for fn in (lambda p: iss_io.decode_pcm(p, ffmpeg=None), lambda p: iss_io.media2sig16kmono(p, ffmpeg=None)):
        with pytest.raises(Exception) as ef:
            fn(f)
        with pytest.raises(Exception) as ew:
            fn(w)
        assert type(ef.value) is type(ew.value)
        assert str(ef.value).replace('o.flac', 'o.wav') == str(ew.value)
    (sa, ra), (sb, rb) = iss_io.decode_source(f), iss_io.decode_source(w)
    assert ra == rb == sr and sa.dtype == sb.dtype and sa.shape == sb.shape
    np.testing.assert_array_equal(sa, sb)


def test_io_golden_twins_and_no_ffmpeg_limits(tmp_path):
    pcms = {}
    for name in ('musanmix.wav', 'silence2sec.wav'):
        pcms[name] = pcm = iss_io.decode_pcm(os.path.join(GOLDEN, name), ffmpeg=None)
        f = flacgen.write(tmp_path / (name + '.flac'), pcm, 16000, 16)
        np.testing.assert_array_equal(iss_io.decode_pcm(f, ffmpeg=None), pcm)
    g = str(tmp_path / 'renamed.wav')                                   # the bytes decide, not the extension
    os.rename(str(tmp_path / 'musanmix.wav.flac'), g)
    np.testing.assert_array_equal(iss_io.decode_pcm(g, ffmpeg=None), pcms['musanmix.wav'])
    with pytest.raises(NotImplementedError):
        iss_io.decode_pcm(g, start_sec=1.0, ffmpeg=None)
    with pytest.raises(NotImplementedError):
        iss_io.media2sig16kmono('http://a/b.flac', ffmpeg=None)
    ogg = tmp_path / 'x.oga'
    ogg.write_bytes(b'OggS' + b'\0' * 24 + b'\x7fFLAC\x01\x00' + b'\0' * 64)
    with pytest.raises(ValueError, match='Ogg-FLAC'):
        iss_io.decode_pcm(str(ogg), ffmpeg=None)
    with pytest.raises(ValueError, match='not a RIFF/WAVE file'):              # anything else: as before
        (tmp_path / 'y.bin').write_bytes(b'junk' * 10)
        iss_io.decode_pcm(str(tmp_path / 'y.bin'), ffmpeg=None)
