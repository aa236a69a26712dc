"""WAV files of every sample format the ffmpeg-free reader takes, for the resampler tests (no soundfile / scipy needed)."""
import struct

import numpy as np

FORMATS = ('u8', 'i16', 'i24', 'i32', 'f32', 'f64')
_BITS = {'u8': 8, 'i16': 16, 'i24': 24, 'i32': 32, 'f32': 32, 'f64': 64}


def encode(x, fmt):
    """float samples (n,) or (n, C), nominally in [-1, 1) -> the stored array of `fmt` (i24: int32 holding 24-bit values)."""
    x = np.asarray(x, dtype=np.float64)
    if fmt == 'u8':
        return np.clip(np.round(x * 128) + 128, 0, 255).astype(np.uint8)
    if fmt == 'i16':
        return np.clip(np.round(x * 32768), -32768, 32767).astype('<i2')
    if fmt == 'i24':
        return np.clip(np.round(x * 2 ** 23), -2 ** 23, 2 ** 23 - 1).astype('<i4')
    if fmt == 'i32':
        return np.clip(np.round(x * 2 ** 31), -2 ** 31, 2 ** 31 - 1).astype('<i4')
    return x.astype('<f4' if fmt == 'f32' else '<f8')


def as_read(stored, fmt):
    """What io._parse_wav returns for the stored array (24-bit PCM is widened to int32 << 8)."""
    return (stored.astype('<i4') << 8) if fmt == 'i24' else stored


def write_wav(path, stored, sr, fmt):
    """Write `stored` (from `encode`) as a RIFF/WAVE file -> path."""
    ch = 1 if stored.ndim == 1 else stored.shape[1]
    bits = _BITS[fmt]
    if fmt == 'i24':
        data = stored.astype('<i4').reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    else:
        data = np.ascontiguousarray(stored).tobytes()
    tag = 3 if fmt in ('f32', 'f64') else 1
    fmt_chunk = struct.pack('<HHIIHH', tag, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt_chunk)) + fmt_chunk + b'data' + struct.pack('<I', len(data)) + data
    if len(data) & 1:
        body += b'\0'
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)
    return str(path)


def make_signal(n, ch, seed, peak=0.9):
    """Tones plus noise, (n,) or (n, ch), peaks just over `peak` so that filtered outputs also exercise saturation."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    cols = []
    for c in range(ch):
        f1, f2 = 0.001 + 0.013 * rng.random(), 0.05 + 0.4 * rng.random()
        cols.append(peak * np.sin(2 * np.pi * f1 * t) + 0.1 * np.sin(2 * np.pi * f2 * t) + 0.05 * rng.standard_normal(n))
    x = np.clip(np.stack(cols, axis=1), -1.0, 1.0 - 2 ** -31)
    return x[:, 0] if ch == 1 else x
