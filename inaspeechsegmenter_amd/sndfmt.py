"""Telephony and studio containers without ffmpeg: G.711, IMA and Microsoft ADPCM, AIFF / AIFF-C, AU, CAF, Wave64, RF64 / BW64.

The reference's ffmpeg-free read is `soundfile.read` (io.py:36-55), and libsndfile opens all of these.  Here a file is
recognised by its leading bytes and then reads exactly like its WAV twin: the little-endian RIFF/WAVE file of the same rate
and channel count that holds

    G.711 mu-law / A-law, IMA ADPCM (WAV tag 0x11),  PCM16, the decoded value (include/iss.h states the four decoders)
    Microsoft ADPCM (WAV tag 2)
    signed 8-bit (AIFF, AU, CAF)                     8-bit WAV (unsigned), x + 128
    unsigned 8-bit (AIFF-C `raw `)                   8-bit WAV, as stored
    16 / 24 / 32-bit integer, either byte order      PCM of the same width, same values
    float32 / float64, either byte order             IEEE-float WAV, same values

This module parses the containers (the device never sees a header) into a `Sound`: the stored bytes plus what they mean.
`Sound.stored()` expands them on the host into the array io._parse_wav returns for the twin (numpy tables, and the host
build of the device's IMA decoder); `source()` hands them to the device as they are, as one of the sources of sources.py: G.711
bytes, signed bytes and big-endian samples to the resample kernel (a `RawSource` with ISS_RS_I8 / ISS_RS_ULAW / ISS_RS_ALAW /
ISS_RS_SWAP), IMA blocks to adpcm_decode_kernel (`AdpcmSource`).  The frame count of an IMA file is its `fact` count when present and not larger than whole blocks *
samples per block, else that product; a trailing partial block is ignored (a definition: libsndfile was not at hand to pin it).
Microsoft ADPCM (kind 'ms') is the second block-coded kind and follows IMA through every branch: `_BLOCK` below is the table of what
tells the two apart (samples-per-block rule, host decoder, source classes), and the same frame-count rule holds.  Only files whose
`fmt ` chunk carries the 32-byte extension with the seven standard coefficient pairs are read (what libsndfile decodes: it
uses its own table); its decode rules, floor rounding among them, are definitions stated in include/iss.h.
"""
import struct
from typing import NamedTuple

import numpy as np

from . import _native
from . import flac
from . import resample as R
from .io import _to_float, need_16k_mono
from .sources import SCHED_OF, CodedAuto, CodedSched, CodedSource, RawAuto, RawSource, host_window, selection

# benchmark switch (tools/bench_sndfmt.py), not a user option: True makes the ffmpeg-free read expand G.711 and ADPCM on
# the host (numpy table / iss_adpcm_decode_host, iss_msadpcm_decode_host in the decode threads) instead of handing the stored bytes to the device
_HOST_DECODE = False

_WIDTH = {'u8': 1, 'i8': 1, 'ulaw': 1, 'alaw': 1, 'i16': 2, 'i24': 3, 'i32': 4, 'f32': 4, 'f64': 8}
_RS_CODE = {'u8': 0, 'i16': 1, 'i32': 2, 'f32': 3, 'f64': 4, 'i8': _native.RS_I8, 'ulaw': _native.RS_ULAW, 'alaw': _native.RS_ALAW}
_W64_TAIL = bytes.fromhex('f3acd3118cd100c04f8edb8a')            # GUID tail of the Wave64 chunk ids 'wave', 'fmt ', 'data', 'fact'
_W64_RIFF = b'riff' + bytes.fromhex('2e91cf11a5d628db04c10000')
_MS_TAG = 'WAVE format tag 2 (MS ADPCM)'                        # every refusal of such a file says this
_MS_COEFS = (256, 0, 512, -256, 0, 0, 192, 64, 240, 0, 460, -208, 392, -232)
_WAV_TAGS = {2: 'MS ADPCM', 0x10: 'OKI ADPCM', 0x14: 'G.723 ADPCM', 0x31: 'GSM 06.10', 0x40: 'G.721 ADPCM', 0x45: 'G.726 ADPCM',
             0x50: 'MPEG', 0x55: 'MPEG Layer III', 0x64: 'G.726 ADPCM'}
_AU_ENC = {1: 'ulaw', 2: 'i8', 3: 'i16', 4: 'i24', 5: 'i32', 6: 'f32', 7: 'f64', 27: 'alaw'}
_AU_NAMES = {23: 'G.721 ADPCM', 24: 'G.722', 25: 'G.723 3-bit ADPCM', 26: 'G.723 5-bit ADPCM'}
_AIFC = {b'NONE': None, b'twos': None, b'in24': 'i24', b'in32': 'i32', b'fl32': 'f32', b'FL32': 'f32', b'fl64': 'f64', b'FL64': 'f64',
         b'ulaw': 'ulaw', b'ULAW': 'ulaw', b'alaw': 'alaw', b'ALAW': 'alaw'}
_INT_OF_BYTES = {1: 'i8', 2: 'i16', 3: 'i24', 4: 'i32'}
MAX_ADPCM_CHANNELS, MAX_ADPCM_ALIGN = 64, 32768                  # adpcm.hip's limits


def _g711_tables():
    b = np.arange(256, dtype=np.int64)
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    ulaw = np.where(u & 0x80, 0x84 - t, t - 0x84)
    a = b ^ 0x55
    t = (a & 15) << 4
    s = (a >> 4) & 7
    t = np.where(s == 0, t + 8, np.where(s == 1, t + 0x108, (t + 0x108) << np.maximum(s - 1, 0)))
    alaw = np.where(a & 0x80, t, -t)
    return ulaw.astype(np.int16), alaw.astype(np.int16)


ULAW_TABLE, ALAW_TABLE = _g711_tables()
for _t in (ULAW_TABLE, ALAW_TABLE):
    _t.setflags(write=False)


class Sound:
    """A parsed file: `data` = the stored sample bytes (uint8, exactly the frames that count), `kind` one of u8 i8 i16 i24
    i32 f32 f64 ulaw alaw ima ms, `big` = stored big-endian, `base` = byte offset of `data` in the file.  ima, ms (the
    block-coded kinds of _BLOCK): `block_align` bytes per block, `spb` samples per block, `data` = whole blocks."""
    __slots__ = ('name', 'sr', 'ch', 'n', 'kind', 'big', 'data', 'base', 'block_align', 'spb')

    def __init__(self, name, sr, ch, kind, big, data, base, frames=None, block_align=0, spb=0):
        if ch < 1:
            raise ValueError(f'{name}: {ch} channels')
        if sr < 1:
            raise ValueError(f'{name}: sample rate {sr} Hz')
        self.name, self.sr, self.ch, self.kind, self.big, self.base = name, int(sr), int(ch), kind, bool(big), int(base)
        self.block_align, self.spb = int(block_align), int(spb)
        if kind in _BLOCK:
            if ch > MAX_ADPCM_CHANNELS or block_align > MAX_ADPCM_ALIGN:
                raise ValueError(f'{name}: {_BLOCK[kind].label} with {ch} channels in {block_align}-byte blocks is not supported '
                                 f'(at most {MAX_ADPCM_CHANNELS} channels, {MAX_ADPCM_ALIGN}-byte blocks)')
            nblocks = len(data) // block_align
            n = nblocks * spb
            if frames is not None and frames <= n:
                n = int(frames)
            nblocks = -(-n // spb)
            self.n, self.data = n, data[:nblocks * block_align]
        else:
            fb = _WIDTH[kind] * ch
            n = len(data) // fb
            if frames is not None and frames < n:
                n = int(frames)
            self.n, self.data = n, data[:n * fb]

    @property
    def nblocks(self):
        return len(self.data) // self.block_align if self.kind in _BLOCK else 0

    def fetch(self, byte0, byte1):
        """Bytes [byte0, byte1) of `data` (what a SoundHeader reads from the file)."""
        return self.data[byte0:byte1]

    def _shape(self, a):
        return a.reshape(-1, self.ch) if self.ch > 1 else a.reshape(-1)

    def check(self, status):
        """Raise ValueError for the first ADPCM block whose decode status (ISS_ADPCM_*) is not 0."""
        bad = np.flatnonzero(np.asarray(status))
        if bad.size:
            k = int(bad[0])
            why = _native.ADPCM_STATUS.get(int(status[k]), f'status {int(status[k])}')
            raise ValueError(f'{self.name}: block at byte {self.base + k * self.block_align}: {why}')

    def source(self, resample=False):
        return source(self, resample)

    def split_source(self, sel):
        """What Segmenter reads for the channels `sel` of a multi-channel file, each on its own (io.split_source)."""
        host = _HOST_DECODE and self.kind in _HOST_KINDS
        if self.kind in _BLOCK and not host and self.n > 0:
            return _BLOCK[self.kind].source(self, 'resample', sel)
        if host or self.kind in _BLOCK:
            return RawSource(self.stored(), self.sr, sel=sel)
        x, fmt = self.raw()
        return RawSource(x, self.sr, fmt, sel)

    def auto_source(self, full):
        """What Segmenter reads for a multi-channel file with channels='auto' (io.auto_source)."""
        host = _HOST_DECODE and self.kind in _HOST_KINDS
        if self.kind in _BLOCK and not host:
            return _BLOCK[self.kind].auto(self, 'pcm' if self.ch == 1 and self.sr == R.SR_OUT else 'stage')
        if self.ch == 1:                                          # stored samples of one channel: nothing to survey
            return source(self, True)
        if host or self.kind in _BLOCK:
            return RawAuto(self.stored(), self.sr, full=full)
        x, fmt = self.raw()
        return RawAuto(x, self.sr, fmt, full)

    def stored(self):
        """The array io._parse_wav returns for the WAV twin: (n,) or (n, ch), uint8 / int16 / int32 / float32 / float64."""
        d, k = self.data, self.kind
        if k == 'u8':
            a = d
        elif k == 'i8':
            a = d ^ np.uint8(0x80)
        elif k == 'ulaw':
            a = ULAW_TABLE[d]
        elif k == 'alaw':
            a = ALAW_TABLE[d]
        elif k in _BLOCK:
            if self.n == 0:
                return self._shape(np.empty(0, dtype=np.int16))
            a, st = _BLOCK[k].host(d, self.nblocks, self.ch, self.block_align, self.n)
            self.check(st)
            return a
        elif k == 'i24':
            raw = d.reshape(-1, 3)
            lo, mid, hi = (raw[:, 2], raw[:, 1], raw[:, 0]) if self.big else (raw[:, 0], raw[:, 1], raw[:, 2])
            a = (lo.astype(np.int32) << 8) | (mid.astype(np.int32) << 16) | (hi.astype(np.int32) << 24)
        else:
            code = {'i16': 'i2', 'i32': 'i4', 'f32': 'f4', 'f64': 'f8'}[k]
            a = d.view(('>' if self.big else '<') + code).astype('<' + code, copy=False)
        return self._shape(a)

    def raw(self):
        """-> (x, ISS_RS_* format): the samples for the resample kernel, as stored ((n,) or (n, ch); an unsigned integer
        of the sample's width where the bytes are not a little-endian number).  24-bit is widened to int32 << 8 here."""
        k = self.kind
        if k == 'i24':
            return self.stored(), _native.RS_FORMAT[np.dtype('<i4')]
        if k in _BLOCK:
            raise ValueError(f'{self.name}: {_BLOCK[k].label} blocks are decoded by their own kernel')
        w = _WIDTH[k]
        if w == 1 or not self.big:
            x = self.data if w == 1 else self.data.view({'i16': '<i2', 'i32': '<i4', 'f32': '<f4', 'f64': '<f8'}[k])
            return self._shape(x), _RS_CODE[k]
        return self._shape(self.data.view('<u%d' % w)), _RS_CODE[k] | _native.RS_SWAP


class SoundHeader:
    """What a Sound says of a file before any sample is read: the same fields but `data`, and `fetch` reads the bytes from
    the file at `path` (io._read_range).  read_header makes one from the chunk headers of a RIFF/WAVE file."""
    __slots__ = ('name', 'path', 'sr', 'ch', 'n', 'kind', 'big', 'base', 'block_align', 'spb')

    def fetch(self, byte0, byte1):
        from .io import _read_range
        buf = _read_range(self.path, self.base + byte0, byte1 - byte0)
        if len(buf) != byte1 - byte0:
            raise ValueError(f'{self.name}: the file ends inside bytes [{self.base + byte0}, {self.base + byte1})')
        return np.frombuffer(buf, dtype=np.uint8)


def sub_sound(h, f0, f1):
    """-> (the Sound of frames [f0, f1) of `h` -- of the whole ADPCM blocks they lie in --, the file's frame number of its first
    frame).  `h` is a Sound or a SoundHeader; only those bytes are fetched, and `base` stays an offset in the file."""
    if h.kind in _BLOCK:
        k0, k1 = f0 // h.spb, (f1 - 1) // h.spb
        data = h.fetch(k0 * h.block_align, (k1 + 1) * h.block_align)
        return Sound(h.name, h.sr, h.ch, h.kind, False, data, h.base + k0 * h.block_align,
                     frames=min(h.n, (k1 + 1) * h.spb) - k0 * h.spb, block_align=h.block_align, spb=h.spb), k0 * h.spb
    fb = _WIDTH[h.kind] * h.ch
    return Sound(h.name, h.sr, h.ch, h.kind, h.big, h.fetch(f0 * fb, f1 * fb), h.base + f0 * fb), f0


# ------------------------------------------------------------------------------------------------ containers
def _wav_kind(name, tag, bits):
    if tag == 1:
        kind = {8: 'u8', 16: 'i16', 24: 'i24', 32: 'i32'}.get(bits)
        if kind is None:
            raise ValueError(f'{name}: unsupported PCM width {bits}')
        return kind
    if tag == 3:
        if bits not in (32, 64):
            raise ValueError(f'{name}: unsupported IEEE float width {bits}')
        return 'f32' if bits == 32 else 'f64'
    if tag in (6, 7):
        if bits != 8:
            raise ValueError(f'{name}: {bits}-bit G.711 (8 bits are)')
        return 'alaw' if tag == 6 else 'ulaw'
    if tag == 0x11:
        if bits != 4:
            raise ValueError(f'{name}: {bits}-bit IMA ADPCM is not supported (4 bits are)')
        return 'ima'
    if tag == 2:
        return 'ms'                                               # (_block_geometry judges its `fmt ` extension)
    what = _WAV_TAGS.get(tag)
    raise ValueError(f'{name}: unsupported WAVE format tag {tag}' + (f' ({what})' if what else ''))


def _parse_fmt(buf, body, size, name):
    """A `fmt ` chunk body -> (tag, ch, sr, block_align, bits, samples per block | None).  Format tag 2: samples per block =
    (wSamplesPerBlock, cbSize, wNumCoef, the coefficients), or a str saying what its extension lacks."""
    tag, ch, sr, _, align, bits = struct.unpack_from('<HHIIHH', buf, body)
    spb = None
    if size >= 20 and tag == 0x11:
        spb = struct.unpack_from('<H', buf, body + 18)[0]
    if tag == 2:
        if size < 50 or len(buf) < body + 50:
            spb = f'a {size}-byte fmt chunk without the 32-byte extension (wSamplesPerBlock, wNumCoef, 7 coefficient pairs)'
        else:
            ext = struct.unpack_from('<HHH14h', buf, body + 16)
            spb = (ext[1], ext[0], ext[2], ext[3:])
    if tag == 0xFFFE and size >= 26:                              # WAVE_FORMAT_EXTENSIBLE
        tag = struct.unpack_from('<H', buf, body + 24)[0]
        if tag == 2:
            spb = 'wrapped in WAVE_FORMAT_EXTENSIBLE, which has no room for the coefficient table'
    return tag, ch, sr, align, bits, spb


def _block_geometry(kind, ch, align, bits, spb):
    """-> (samples per block, None) of a block-coded `fmt `, or (None, why it is refused): the rules of adpcm.hip's
    geometry_ok and, for Microsoft ADPCM, of the extension -- one place for the whole-file read and read_header."""
    if kind == 'ima':
        if ch < 1 or align % (4 * ch) != 0 or align <= 4 * ch:
            return None, f'IMA ADPCM block size {align} is not a multiple of 4 * {ch} channels above one header'
        want = _BLOCK[kind].spb(align, ch)
        if spb is not None and spb != want:
            return None, f'IMA ADPCM {spb} samples per block, {align}-byte blocks of {ch} channels hold {want}'
        return want, None
    if isinstance(spb, str):
        return None, f'{_MS_TAG}: {spb}'
    stated, cb, ncoef, coefs = spb
    if cb < 32:
        return None, f'{_MS_TAG}: cbSize {cb}, the extension takes 32 bytes'
    if bits != 4:
        return None, f'{_MS_TAG}: {bits} bits per sample (4 are)'
    if ch < 1 or align <= 7 * ch or (align - 7 * ch) * 2 % ch != 0:
        return None, f'{_MS_TAG}: block size {align} does not hold a 7-byte header and whole samples of {ch} channels'
    want = _BLOCK[kind].spb(align, ch)
    if stated != want:
        return None, f'{_MS_TAG}: {stated} samples per block, {align}-byte blocks of {ch} channels hold {want}'
    if ncoef != 7 or tuple(coefs) != _MS_COEFS:
        return None, f'{_MS_TAG}: {ncoef} coefficient pairs {list(coefs[:2 * min(ncoef, 7)])}, only the 7 standard pairs are decoded'
    return want, None


def _wav_sound(buf, name, fmt, fact, body, end):
    tag, ch, sr, align, bits, spb = fmt
    kind = _wav_kind(name, tag, bits)
    data = np.frombuffer(buf, dtype=np.uint8, count=end - body, offset=body)
    if kind not in _BLOCK:
        return Sound(name, sr, ch, kind, False, data, body)       # (`fact` is advisory for sample-per-byte formats, as for PCM)
    want, why = _block_geometry(kind, ch, align, bits, spb)
    if why:
        raise ValueError(f'{name}: {why}')
    return Sound(name, sr, ch, kind, False, data, body, frames=fact, block_align=align, spb=want)


def _parse_riff(buf, name):
    """RIFF / RF64 / BW64 WAVE -> Sound, or None for what io._parse_wav reads (plain RIFF holding PCM or float)."""
    rf64 = buf[:4] in (b'RF64', b'BW64')
    pos, fmt, fact, ds64 = 12, None, None, None
    n = len(buf)
    while pos + 8 <= n:
        cid, size = buf[pos:pos + 4], struct.unpack_from('<I', buf, pos + 4)[0]
        body = pos + 8
        if cid == b'ds64' and rf64:
            ds64 = struct.unpack_from('<QQQ', buf, body)
        elif cid == b'fmt ':
            fmt = _parse_fmt(buf, body, size, name)
            if not rf64 and fmt[0] not in (6, 7, 0x11, 2):
                return None
        elif cid == b'fact' and size >= 4:
            fact = struct.unpack_from('<I', buf, body)[0]
        elif cid == b'data':
            if fmt is None:
                break
            if size == 0xFFFFFFFF:
                size = ds64[1] if ds64 is not None else n         # (no ds64: a piped WAV, to the end of the buffer)
            if fact == 0xFFFFFFFF:
                fact = ds64[2] if ds64 is not None else None
            return _wav_sound(buf, name, fmt, fact, body, min(n, body + size))
        pos = body + size + (size & 1)
    if not rf64:
        return None                                               # _parse_wav words the error
    raise ValueError(f'{name}: missing fmt or data chunk')


def _parse_w64(buf, name):
    pos, fmt, fact, n = 40, None, None, len(buf)
    if buf[24:28] != b'wave' or buf[28:40] != _W64_TAIL:
        raise ValueError(f'{name}: Wave64 file without a wave GUID')
    while pos + 24 <= n:
        cid, tail, size = buf[pos:pos + 4], buf[pos + 4:pos + 16], struct.unpack_from('<Q', buf, pos + 16)[0]
        if size < 24:
            raise ValueError(f'{name}: Wave64 chunk of {size} bytes at byte {pos}')
        body = pos + 24
        if tail == _W64_TAIL and cid == b'fmt ':
            fmt = _parse_fmt(buf, body, size - 24, name)
        elif tail == _W64_TAIL and cid == b'fact' and size >= 28:
            fact = struct.unpack_from('<Q', buf, body)[0] if size >= 32 else struct.unpack_from('<I', buf, body)[0]
        elif tail == _W64_TAIL and cid == b'data':
            if fmt is None:
                break
            return _wav_sound(buf, name, fmt, fact, body, min(n, pos + size))
        pos += (size + 7) & ~7
    raise ValueError(f'{name}: missing fmt or data chunk')


def _extended(b):
    """80-bit IEEE extended -> (the value when it is a whole number >= 0, else None; the value as float)."""
    import math
    exp, mant = struct.unpack('>HQ', b)
    e = (exp & 0x7FFF) - 16383 - 63
    val = math.ldexp(float(mant), e)
    if exp & 0x8000 and mant:
        return None, -val
    if e >= 0:
        return (mant << e if e < 64 else None), val
    if -e >= 64:
        return (None if mant else 0), val
    if mant & ((1 << -e) - 1):
        return None, val
    return mant >> -e, val


def _parse_aiff(buf, name):
    aifc = buf[8:12] == b'AIFC'
    pos, comm, ssnd, n = 12, None, None, len(buf)
    while pos + 8 <= n:
        cid, size = buf[pos:pos + 4], struct.unpack_from('>I', buf, pos + 4)[0]
        body = pos + 8
        if cid == b'COMM':
            ch, frames, bits = struct.unpack_from('>hIh', buf, body)
            sr, val = _extended(buf[body + 8:body + 18])
            ctype = bytes(buf[body + 18:body + 22]) if aifc else b'NONE'
            if aifc and len(ctype) < 4:
                raise struct.error
            comm = (ch, frames, bits, sr, val, ctype)
        elif cid == b'SSND':
            off = struct.unpack_from('>II', buf, body)[0]
            ssnd = (body + 8 + off, min(n, body + size))
        pos = body + size + (size & 1)
    if comm is None or ssnd is None:
        raise ValueError(f'{name}: missing COMM or SSND chunk')
    ch, frames, bits, sr, val, ctype = comm
    if sr is None:
        raise ValueError(f'{name}: AIFF sample rate {val!r} Hz is not a whole number of Hz')
    if ctype not in _AIFC and ctype not in (b'sowt', b'raw '):
        raise ValueError(f'{name}: unsupported AIFF-C compression type {ctype.decode("latin-1")!r}')
    big = True
    if ctype in (b'NONE', b'twos', b'sowt'):
        if not 1 <= bits <= 32:
            raise ValueError(f'{name}: AIFF sample size of {bits} bits')
        kind = _INT_OF_BYTES[(bits + 7) // 8]                     # left-justified in ceil(bits / 8) bytes: the width decides
        big = ctype != b'sowt'
    elif ctype == b'raw ':
        if bits != 8:
            raise ValueError(f'{name}: AIFF-C raw samples of {bits} bits (8 are)')
        kind = 'u8'
    else:
        kind = _AIFC[ctype]
    a, b = ssnd
    data = np.frombuffer(buf, dtype=np.uint8, count=max(b - a, 0), offset=min(a, n))
    return Sound(name, sr, ch, kind, big, data, a, frames=frames)


def _parse_au(buf, name):
    e = '>' if buf[:4] == b'.snd' else '<'
    off, size, enc, sr, ch = struct.unpack_from(e + 'IIIII', buf, 4)
    kind = _AU_ENC.get(enc)
    if kind is None:
        what = _AU_NAMES.get(enc)
        raise ValueError(f'{name}: unsupported AU encoding {enc}' + (f' ({what})' if what else ''))
    if off < 24:
        raise ValueError(f'{name}: AU data offset {off}')
    n = len(buf)
    end = n if size == 0xFFFFFFFF else min(n, off + size)
    data = np.frombuffer(buf, dtype=np.uint8, count=max(end - off, 0), offset=min(off, n))
    return Sound(name, sr, ch, kind, e == '>', data, off)


def _parse_caf(buf, name):
    version = struct.unpack_from('>H', buf, 4)[0]
    if version != 1:
        raise ValueError(f'{name}: CAF version {version}')
    pos, desc, n = 8, None, len(buf)
    while pos + 12 <= n:
        cid, size = buf[pos:pos + 4], struct.unpack_from('>q', buf, pos + 4)[0]
        body = pos + 12
        if cid == b'desc':
            desc = struct.unpack_from('>d4sIIIII', buf, body)
        elif cid == b'data':
            if desc is None:
                break
            rate, fid, flags, bpp, fpp, ch, bits = desc
            if rate != int(rate) or rate < 1:
                raise ValueError(f'{name}: CAF sample rate {rate!r} Hz is not a whole number of Hz')
            if fid == b'lpcm':
                kind = ({32: 'f32', 64: 'f64'} if flags & 1 else {8: 'i8', 16: 'i16', 24: 'i24', 32: 'i32'}).get(bits)
                if kind is None or ch < 1 or bpp != _WIDTH[kind] * ch:
                    raise ValueError(f'{name}: unsupported CAF lpcm layout ({bits} bits, {bpp} bytes per packet of {ch} channels)')
                big = not flags & 2
            elif fid in (b'ulaw', b'alaw'):
                kind, big = fid.decode(), True
            else:
                raise ValueError(f'{name}: unsupported CAF format {fid.decode("latin-1")!r}')
            end = n if size < 0 else min(n, body + size)
            a = body + 4                                          # the edit count
            data = np.frombuffer(buf, dtype=np.uint8, count=max(end - a, 0), offset=min(a, n))
            return Sound(name, int(rate), ch, kind, big, data, a)
        if size < 0:
            break
        pos = body + size
    raise ValueError(f'{name}: missing desc or data chunk')


def read_header(path, name=None):
    """The SoundHeader of a plain RIFF/WAVE file (PCM, float, G.711, IMA or Microsoft ADPCM), from its chunk headers alone: 12 bytes, then
    8 per chunk and the bodies of `fmt ` and `fact`; a `data` chunk behind a large unknown chunk costs one more 8-byte read.
    None for every other container and for whatever needs the whole file to be judged (RF64 sizes, a piped WAV without a length, a
    file cut short): io.excerpts then reads the file as the whole-file read does."""
    import os
    from .io import _read_range
    name = path if name is None else name
    size_file = os.path.getsize(path)
    head = _read_range(path, 0, 12)
    if head[:4] != b'RIFF' or head[8:12] != b'WAVE':
        return None
    pos, fmt, fact = 12, None, None
    while pos + 8 <= size_file:
        head = _read_range(path, pos, 8)
        if len(head) < 8:
            return None
        cid, size = head[:4], struct.unpack('<I', head[4:])[0]
        body = pos + 8
        if cid == b'fmt ':
            chunk = _read_range(path, body, min(size, 64))
            if len(chunk) < 16:
                return None
            fmt = _parse_fmt(chunk, 0, size, name)
        elif cid == b'fact' and size >= 4:
            fact = struct.unpack('<I', _read_range(path, body, 4))[0]
        elif cid == b'data':
            if fmt is None or size == 0xFFFFFFFF or fact == 0xFFFFFFFF or body + size > size_file:
                return None
            tag, ch, sr, align, bits, spb = fmt
            h = SoundHeader()
            try:
                kind = _wav_kind(name, tag, bits)
            except ValueError:
                return None                                       # (the whole-file read words the refusal)
            h.name, h.path, h.sr, h.ch, h.kind, h.big, h.base = name, path, int(sr), int(ch), kind, False, body
            h.block_align = h.spb = 0
            if ch < 1 or sr < 1:
                return None
            if h.kind in _BLOCK:
                # (the rules of _wav_sound and Sound.__init__, on the header's numbers)
                want, why = _block_geometry(h.kind, ch, align, bits, spb)
                if why or ch > MAX_ADPCM_CHANNELS or align > MAX_ADPCM_ALIGN:
                    return None
                n = size // align * want
                h.n, h.block_align, h.spb = (int(fact) if fact is not None and fact <= n else n), int(align), want
            else:
                h.n = size // (_WIDTH[h.kind] * ch)
            return h
        pos = body + size + (size & 1)
    return None


def _container(head):
    """The parser of these leading bytes, with the container's name; None when they start none of them."""
    if head[:4] in (b'RIFF', b'RF64', b'BW64') and head[8:12] == b'WAVE':
        return _parse_riff, 'WAVE'
    if head[:16] == _W64_RIFF:
        return _parse_w64, 'Wave64'
    if head[:4] == b'FORM' and head[8:12] in (b'AIFF', b'AIFC'):
        return _parse_aiff, 'AIFF'
    if head[:4] in (b'.snd', b'dns.'):
        return _parse_au, 'AU'
    if head[:4] == b'caff':
        return _parse_caf, 'CAF'
    return None


def parse(buf, name='<buffer>'):
    """-> the Sound of a file's bytes, or None when io._parse_wav reads (or refuses) them as before."""
    c = _container(buf[:16])
    if c is None:
        return None
    try:
        return c[0](buf, name)
    except struct.error:
        if buf[:4] == b'RIFF':                                    # a plain RIFF file cut short: io._parse_wav words it as before
            return None
        raise ValueError(f'{name}: truncated {c[1]} header') from None


def _ours(head):
    """Do these leading bytes (4 KiB) start a file this module reads?  A plain RIFF/WAVE file holding PCM or float is not:
    io._parse_wav reads it as before."""
    if _container(head[:16]) is None:
        return False
    if head[:4] == b'RIFF':
        pos = 12
        while pos + 8 <= len(head):
            cid, size = head[pos:pos + 4], struct.unpack_from('<I', head, pos + 4)[0]
            if cid == b'fmt ' and pos + 10 <= len(head):
                tag = struct.unpack_from('<H', head, pos + 8)[0]
                if tag == 0xFFFE and size >= 26 and pos + 34 <= len(head):
                    tag = struct.unpack_from('<H', head, pos + 32)[0]
                return tag in (6, 7, 0x11, 2)
            if cid == b'data':
                return False
            pos += 8 + size + (size & 1)
    # a `fmt ` chunk past the first 4 KiB (a large bext / LIST / JUNK chunk in front): parse() decides on the whole file
    return True


def device_decoded(path):
    """One look at the first bytes of the file at `path` (whatever its name): 'flac' for a native FLAC stream, 'snd' for a
    file this module reads, None for anything else (a plain PCM / float WAV among them)."""
    with open(path, 'rb') as f:
        head = f.read(4096)
        p = flac._id3_end(head)
        if p:                                                     # behind an ID3v2 tag of any length
            f.seek(p)
            return 'flac' if f.read(4) == flac.MAGIC else None
    if head[:4] == flac.MAGIC:
        return 'flac'
    return 'snd' if _ours(head) else None


# ------------------------------------------------------------------------------------------------ device sources
class AdpcmSource(CodedSource):
    """An IMA ADPCM file for the device decoder (sources.py states what it answers).  kind: 'pcm' or 'resample'."""
    __slots__ = ()
    pass_order = 2
    coder = 'adpcm'                                              # iss_adpcm_survey surveys what this class's launch staged
    stage_format = _native.RS_FORMAT[np.dtype('<i2')]
    full = R.SURVEY_FULL['ima']
    payload = property(lambda self: self.s.data)
    units = property(lambda self: self.s.nblocks)

    def row(self, ctx, src_offset, block_begin, dst_offset):
        """Its ADPCM_JOB row: into the signal at dst_offset ('pcm') or staged and resampled to dst_offset ('resample'); the
        sample count is the whole file's, also where `s` holds the blocks of an excerpt."""
        s, total = self.s, self.s.n if self.win is None else self.win[2]
        to, fid, nout = _native.ADPCM_TO_SIGNAL, -1, 0
        if self.kind == 'stage':                                  # (io.survey_sources: staged for the survey kernel, no filter)
            to = _native.ADPCM_TO_STAGE
        elif self.kind != 'pcm':
            to, fid, nout = _native.ADPCM_TO_STAGE, ctx.resample_filter(s.sr)[0], self.size
        return (src_offset, block_begin, s.nblocks, total, s.ch, s.block_align, to, fid, dst_offset, nout)

    @staticmethod
    def tables(group):
        return sum(g.units for g in group)

    @staticmethod
    def launch(ctx, staged, rows, nblocks, n_signal=-1, **kw):
        return ctx.adpcm_decode(staged, rows, nblocks, n_signal, **kw)


class AdpcmExcerpt(AdpcmSource):
    """Outputs [a, b) of an IMA (or, as MsAdpcmExcerpt, Microsoft) ADPCM file for the windowed decode: `s` = the sub_sound of the blocks that hold the
    stored-rate samples the excerpt needs ('pcm': [a, b); 'resample': resample.input_span of them), `first` the file's sample
    number of its first sample.  kind 'stage' (io.survey_sources): a and b count stored frames, staged for the survey kernel.
    A bad block is named by its byte offset in the file (s.base is one).  `sel` ('resample' only):
    the channels to write apart (None: their average)."""
    __slots__ = ('first', 'win')

    def __init__(self, h, kind, a, b, sel=None):
        self.kind, self.size = kind, b - a
        self.sel = selection(sel)
        s0, s1 = (a, b) if kind in ('pcm', 'stage') else (lambda lo, hi: (lo, hi + 1))(*R.input_span(h.sr, h.n, a, b - a))
        self.s, self.first = sub_sound(h, s0, s1)
        self.win = (s0, s1, h.n, a, b - a)
        self.nbytes = self.s.data.nbytes

    def host(self):
        """The same samples by the host build of the decoder, on the same blocks (and resample.resample_ref)."""
        s0, s1, total, a, count = self.win
        x = self.s.stored()[s0 - self.first:s1 - self.first]
        return np.ascontiguousarray(x) if self.kind == 'pcm' else host_window(x, self.s.sr, self.win, self.sel)


class AdpcmAuto(CodedAuto, AdpcmSource):
    """An IMA ADPCM file for channels='auto' (sources.CodedAuto): kind 'stage' for two or more channels, and for one channel
    at another rate; 'pcm' for one channel at 16 kHz."""
    __slots__ = ('decision',)

    def __init__(self, snd, kind='stage'):
        AdpcmSource.__init__(self, snd, kind)
        self.size, self.decision = snd.n if kind == 'pcm' else R.out_len(snd.n, snd.sr), None


class MsAdpcmSource(AdpcmSource):
    """A Microsoft ADPCM file for the device decoder: AdpcmSource's rows, its own launch (iss_msadpcm_decode) after IMA's."""
    __slots__ = ()
    pass_order = 3
    coder = 'msadpcm'

    @staticmethod
    def launch(ctx, staged, rows, nblocks, n_signal=-1, **kw):
        return ctx.msadpcm_decode(staged, rows, nblocks, n_signal, **kw)


class MsAdpcmExcerpt(AdpcmExcerpt, MsAdpcmSource):
    """Outputs [a, b) of a Microsoft ADPCM file: AdpcmExcerpt's window on MsAdpcmSource's launch."""
    __slots__ = ()


class MsAdpcmAuto(AdpcmAuto, MsAdpcmSource):
    """A Microsoft ADPCM file for channels='auto'."""
    __slots__ = ()


class AdpcmSched(CodedSched, AdpcmAuto):
    """An IMA ADPCM file with a schedule, given or decided from its blocked survey (sources.CodedSched)."""
    __slots__ = ('sched', 'block_chunks', 'rule', 'fade_sec')


class MsAdpcmSched(CodedSched, MsAdpcmAuto):
    """A Microsoft ADPCM file with a schedule."""
    __slots__ = ('sched', 'block_chunks', 'rule', 'fade_sec')


SCHED_OF[AdpcmAuto], SCHED_OF[MsAdpcmAuto] = AdpcmSched, MsAdpcmSched


class _BlockKind(NamedTuple):
    """What tells the block-coded kinds apart; every `kind in _BLOCK` branch of this module reads its columns."""
    label: str
    spb: object            # (block_align, channels) -> samples per block
    host: object           # the host build of the decoder (_native)
    source: type
    excerpt: type
    auto: type


_BLOCK = {'ima': _BlockKind('IMA ADPCM', lambda align, ch: (align // ch - 4) * 2 + 1, _native.adpcm_decode_host,
                            AdpcmSource, AdpcmExcerpt, AdpcmAuto),
          'ms': _BlockKind('MS ADPCM', lambda align, ch: (align - 7 * ch) * 2 // ch + 2, _native.msadpcm_decode_host,
                           MsAdpcmSource, MsAdpcmExcerpt, MsAdpcmAuto)}
_HOST_KINDS = ('ulaw', 'alaw') + tuple(_BLOCK)                   # what _HOST_DECODE expands on the host


def block_excerpt(h, kind, a, b, sel=None):
    """The windowed source of outputs [a, b) of a block-coded file `h` (io.excerpts, io.channel_excerpts), or None for any
    other kind."""
    return _BLOCK[h.kind].excerpt(h, kind, a, b, sel) if h.kind in _BLOCK else None


def decode_on(ctx, src):
    """One ADPCM file on its own: the resident signal becomes its 16 kHz PCM16 -> the per-block status, valid after the
    context's next synchronising call (check it with src.check)."""
    return src.place(ctx)


def source(snd, resample=False):
    """What Segmenter reads for a parsed file under the WAV-twin rules of the ffmpeg-free read: the twin's int16 / float32
    array (16 kHz mono), an AdpcmSource / MsAdpcmSource, or a sources.RawSource holding the bytes as stored.  Without `resample`, anything but
    16 kHz mono is refused as the WAV path refuses it (io.need_16k_mono)."""
    mono16k = snd.sr == R.SR_OUT and snd.ch == 1
    if not mono16k and not resample:
        need_16k_mono(snd.name, snd.sr, snd.ch)
    host = _HOST_DECODE and snd.kind in _HOST_KINDS
    if snd.kind in _BLOCK and not host and snd.n > 0:
        if mono16k:
            return _BLOCK[snd.kind].source(snd, 'pcm')
        R.check_rate(snd.sr)
        return _BLOCK[snd.kind].source(snd, 'resample')
    if mono16k:
        if snd.kind == 'i16' and snd.big and snd.n > 0:           # swapped on the device, through the identity filter
            x, fmt = snd.raw()
            return RawSource(x, snd.sr, fmt)
        x = snd.stored()                                          # G.711: the 256-entry table; the float path's conversions
        return np.ascontiguousarray(x) if x.dtype == np.int16 else np.ascontiguousarray(_to_float(x, np.float32))
    R.check_rate(snd.sr)
    if host or snd.kind in _BLOCK:
        return RawSource(snd.stored(), snd.sr)
    x, fmt = snd.raw()
    return RawSource(x, snd.sr, fmt)
