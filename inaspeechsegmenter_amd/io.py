"""Media decode boundary: anything -> 16 kHz mono samples on the host.

Mirrors io.py:32-79 `media2sig16kmono(medianame, start_sec, stop_sec, ffmpeg, dtype)`:
  * ffmpeg given  -> `ffmpeg -i <media> -f wav -acodec pcm_s16le -ar 16000 -ac 1 [-ss] [-to] pipe:1`
    (same command line, io.py:61-68); non-zero exit raises Exception(stderr) (io.py:72-75).
    The PCM is taken straight from the pipe instead of a TemporaryFile + soundfile.
  * ffmpeg=None   -> direct read; start/stop and http(s) sources raise NotImplementedError
    with the reference's wording (io.py:37-50); the file must already be 16 kHz (io.py:53-55).
Decode stays on the host (north star); soundfile/libsndfile is not available in the target
image, so RIFF/WAVE is parsed here with libsndfile's conversion rules (PCM16 -> x/32768,
unknown chunks skipped).  FLAC (flac.py) reads exactly like its WAV twin, decoded here by the host build of the
device's frame decoder; so do G.711 and IMA ADPCM in WAV, RF64 / BW64, Wave64, AIFF / AIFF-C, AU and CAF (sndfmt.py: numpy
tables, byte swaps and the host build of the device's IMA decoder).  A file is read once (`_read_file`) and `_classify` says
from its bytes which parser takes it: a new format is one line there.  `decode_pcm` is the entry the native pipeline uses: it keeps
PCM16 as int16 so the device does the x/32768 scaling (2 B/sample over PCIe, not 4).
"""
import os
import struct
import subprocess

import numpy as np

from . import resample as R
from .sources import RawSource


def _parse_wav(buf, name='<buffer>'):
    """-> (samples ndarray shaped (n,) or (n,ch), sr).  dtype int16 / uint8 / int32 / float32 / float64
    exactly as stored (24-bit widened to int32 << 8)."""
    if len(buf) < 12 or buf[:4] not in (b'RIFF', b'RF64') or buf[8:12] != b'WAVE':
        raise ValueError(f'{name}: not a RIFF/WAVE file')
    pos, fmt, data = 12, None, None
    n = len(buf)
    while pos + 8 <= n:
        cid, size = buf[pos:pos + 4], struct.unpack_from('<I', buf, pos + 4)[0]
        body = pos + 8
        if cid == b'fmt ':
            tag, ch, sr, _, _, bits = struct.unpack_from('<HHIIHH', buf, body)
            if tag == 0xFFFE and size >= 26:                      # WAVE_FORMAT_EXTENSIBLE
                tag = struct.unpack_from('<H', buf, body + 24)[0]
            fmt = (tag, ch, sr, bits)
        elif cid == b'data':
            end = n if (size == 0xFFFFFFFF or body + size > n) else body + size   # piped WAVs carry no length
            data = buf[body:end]
            break
        pos = body + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f'{name}: missing fmt or data chunk')
    tag, ch, sr, bits = fmt
    if tag == 1:
        if bits == 16:
            a = np.frombuffer(data, dtype='<i2', count=len(data) // 2)
        elif bits == 8:
            a = np.frombuffer(data, dtype=np.uint8)
        elif bits == 32:
            a = np.frombuffer(data, dtype='<i4', count=len(data) // 4)
        elif bits == 24:
            raw = np.frombuffer(data, dtype=np.uint8, count=(len(data) // 3) * 3).reshape(-1, 3)
            a = ((raw[:, 0].astype(np.int32) << 8) | (raw[:, 1].astype(np.int32) << 16) | (raw[:, 2].astype(np.int32) << 24))
        else:
            raise ValueError(f'{name}: unsupported PCM width {bits}')
    elif tag == 3:
        a = np.frombuffer(data, dtype='<f4' if bits == 32 else '<f8', count=len(data) // (bits // 8))
    else:
        raise ValueError(f'{name}: unsupported WAVE format tag {tag}')
    if ch > 1:
        a = a[:(len(a) // ch) * ch].reshape(-1, ch)
    return a, sr


def _read_file(medianame):
    with open(medianame, 'rb') as f:
        return f.read()


def _classify(buf, name):
    """What the bytes of a file are to the ffmpeg-free read: a flac.FlacStream, a sndfmt.Sound (G.711 / IMA ADPCM WAV, RF64,
    Wave64, AIFF, AU, CAF), or None for what _parse_wav reads or refuses.  One line per format; what comes back has `sr`,
    `stored()` (the host decode) and `source(resample)` (what Segmenter reads).  (flac and sndfmt import this
    module for need_16k_mono and _to_float, so they are imported here and not at the top.)"""
    from . import flac, sndfmt
    if flac.is_flac(buf):
        return flac.FlacStream(buf, name)
    if flac.is_ogg_flac(buf):
        raise ValueError(f'{name}: Ogg-FLAC (FLAC in an Ogg container) is not supported without ffmpeg')
    return sndfmt.parse(buf, name)


def _stored(what, buf, name):
    """what = _classify(buf, name) -> (samples as stored, sr) as _parse_wav returns them (for the WAV twin), decoded on the host."""
    return _parse_wav(buf, name) if what is None else (what.stored(), what.sr)


def _to_float(a, dtype):
    """libsndfile's integer -> float scaling."""
    if a.dtype == np.int16:
        return (a.astype(np.float64) / 32768.0).astype(dtype)
    if a.dtype == np.uint8:
        return ((a.astype(np.float64) - 128.0) / 128.0).astype(dtype)
    if a.dtype == np.int32:
        return (a.astype(np.float64) / 2147483648.0).astype(dtype)
    return a.astype(dtype)


def _run_ffmpeg(medianame, start_sec, stop_sec, ffmpeg):
    cmd = [ffmpeg, '-i', medianame, '-f', 'wav', '-acodec', 'pcm_s16le', '-ar', '16000', '-ac', '1']
    if start_sec is not None:
        cmd += ['-ss', '%f' % start_sec]
    if stop_sec is not None:
        cmd += ['-to', '%f' % stop_sec]
    cmd += ['pipe:1']
    ret = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if ret.returncode != 0:
        raise Exception(ret.stderr)
    a, fs = _parse_wav(ret.stdout, medianame)
    assert fs == 16000
    return a


def _check_no_ffmpeg(medianame, start_sec, stop_sec):
    if start_sec is not None or stop_sec is not None:
        raise NotImplementedError(
            f'start_sec={start_sec} and stop_sec={stop_sec} cannot be set '
            f' when running inaSpeechSegmenter without ffmpeg. Please cut '
            f'down your audio files beforehand or use ffmpeg.')
    if medianame.startswith('http://') or medianame.startswith('https://'):
        raise NotImplementedError(
            f'Without ffmpeg you cannot process media content on http '
            f'servers. You need to download your audio files beforehand '
            f'or use ffmpeg. You gave medianame={medianame}.')


def need_16k_mono(name, sr, channels):
    """The refusal of the ffmpeg-free read without `resample` (io.py:53-55), the same for every format: rate first."""
    assert sr == 16_000, \
        f'Without ffmpeg, inaSpeechSegmenter can only take files sampled ' \
        f'at 16000 Hz. The file {name} is sampled at {sr} Hz.'
    if channels != 1:
        raise ValueError(f'{name}: {channels} channels; without ffmpeg only mono files are supported')


def source_of(x, sr, name, resample=False):
    """What Segmenter reads for samples as stored on the host: the 16 kHz mono array (int16, or float32 for the float path);
    anything else is refused without `resample` and handed to the device resampler as a RawSource with it."""
    if sr == R.SR_OUT and x.ndim == 1:
        return np.ascontiguousarray(x) if x.dtype == np.int16 else np.ascontiguousarray(_to_float(x, np.float32))
    if not resample:
        need_16k_mono(name, sr, 1 if x.ndim == 1 else x.shape[1])
    R.check_rate(sr)
    return RawSource(x, sr)


def decode_pcm(medianame, start_sec=None, stop_sec=None, ffmpeg='ffmpeg'):
    """16 kHz mono samples for the device: int16 when the source is PCM16 (always, through
    ffmpeg), else float32 holding exactly what soundfile's float32 read would return."""
    if ffmpeg is None:
        _check_no_ffmpeg(medianame, start_sec, stop_sec)
        a, sr = decode_source(medianame)
        need_16k_mono(medianame, sr, 1 if a.ndim == 1 else a.shape[1])
    else:
        a = _run_ffmpeg(medianame, start_sec, stop_sec, ffmpeg)
    if a.dtype == np.int16:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(_to_float(a, np.float32))


def decode_source(medianame):
    """ffmpeg-free read of a WAV, FLAC or sndfmt.py file: -> (samples as stored, (n,) or (n, C), sr).  Nothing is converted:
    the device downmixes, resamples and quantises (inaspeechsegmenter_amd/resample.py)."""
    buf = _read_file(medianame)
    return _stored(_classify(buf, medianame), buf, medianame)


def media2sig16kmono(medianame, start_sec=None, stop_sec=None, ffmpeg='ffmpeg', dtype='float64'):
    """Reference-compatible signature and result (float array of `dtype`)."""
    a = decode_pcm(medianame, start_sec, stop_sec, ffmpeg)
    return _to_float(a, np.dtype(dtype)) if a.dtype == np.int16 else a.astype(dtype)
