"""Writers for the containers and encodings of inaspeechsegmenter_amd/sndfmt.py, their WAV twins, and G.711 / IMA ADPCM
encoders and decoders written from the definitions (no audioop, no soundfile): the decoders here are the tests' own statement
of what a file holds, checked against the audioop-generated vectors in tests/golden/sndfmt_vectors.npz."""
import struct

import numpy as np

import wavgen

IMA_STEP = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
    130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
    1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132,
    7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], dtype=np.int64)
IMA_ADJ = np.array([-1, -1, -1, -1, 2, 4, 6, 8] * 2, dtype=np.int64)

KINDS = ('u8', 'i8', 'i16', 'i24', 'i32', 'f32', 'f64', 'ulaw', 'alaw', 'ima')
_WIDTH = {'u8': 1, 'i8': 1, 'ulaw': 1, 'alaw': 1, 'i16': 2, 'i24': 3, 'i32': 4, 'f32': 4, 'f64': 8}


# ------------------------------------------------------------------------------------------------ G.711
def ulaw_value(b):
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return 0x84 - t if u & 0x80 else t - 0x84


def alaw_value(b):
    a = b ^ 0x55
    t = (a & 15) << 4
    s = (a >> 4) & 7
    if s == 0:
        t += 8
    elif s == 1:
        t += 0x108
    else:
        t = (t + 0x108) << (s - 1)
    return t if a & 0x80 else -t


ULAW = np.array([ulaw_value(b) for b in range(256)], dtype=np.int16)
ALAW = np.array([alaw_value(b) for b in range(256)], dtype=np.int16)


def g711_encode(pcm16, law):
    """int16 samples -> the code whose decoded value is nearest (an encoder: only the decoded values are compared)."""
    tab = (ULAW if law == 'ulaw' else ALAW).astype(np.int64)
    order = np.argsort(tab, kind='stable')
    vals = tab[order]
    x = np.asarray(pcm16, dtype=np.int64)
    k = np.clip(np.searchsorted(vals, x), 1, 255)
    k = np.where(np.abs(vals[k - 1] - x) <= np.abs(vals[k] - x), k - 1, k)
    return order[k].astype(np.uint8)


# ------------------------------------------------------------------------------------------------ IMA ADPCM
def ima_samples_per_block(block_align, ch):
    return (block_align // ch - 4) * 2 + 1


def ima_encode(pcm16, block_align):
    """(n,) or (n, ch) int16 -> whole blocks (bytes); the last block is filled by repeating the last frame."""
    x = np.asarray(pcm16, dtype=np.int64)
    x = x.reshape(len(x), -1)
    n, ch = x.shape
    assert block_align % (4 * ch) == 0 and block_align > 4 * ch
    spb = ima_samples_per_block(block_align, ch)
    nb = max(1, -(-n // spb))
    x = np.concatenate((x, np.repeat(x[-1:], nb * spb - n, axis=0))).reshape(nb, spb, ch)
    pred = x[:, 0, :].copy()
    idx = np.clip(np.searchsorted(IMA_STEP, np.abs(x[:, 1, :] - x[:, 0, :])), 0, 88)
    hdr = np.zeros((nb, ch, 4), dtype=np.uint8)
    hdr[:, :, 0] = pred & 0xFF
    hdr[:, :, 1] = (pred >> 8) & 0xFF
    hdr[:, :, 2] = idx
    nib = np.zeros((nb, spb - 1, ch), dtype=np.int64)
    for s in range(1, spb):
        step = IMA_STEP[idx]
        diff = x[:, s, :] - pred
        d = np.abs(diff)
        code = np.zeros_like(d)
        vp = step >> 3
        m = d >= step
        code |= m * 4; d = d - m * step; vp = vp + m * step
        m = d >= (step >> 1)
        code |= m * 2; d = d - m * (step >> 1); vp = vp + m * (step >> 1)
        m = d >= (step >> 2)
        code |= m * 1; vp = vp + m * (step >> 2)
        pred = np.clip(np.where(diff < 0, pred - vp, pred + vp), -32768, 32767)
        idx = np.clip(idx + IMA_ADJ[code], 0, 88)
        nib[:, s - 1, :] = code | ((diff < 0) * 8)
    w = nib.reshape(nb, (spb - 1) // 8, 8, ch)
    words = np.zeros((nb, (spb - 1) // 8, ch), dtype=np.int64)
    for k in range(8):
        words |= w[:, :, k, :] << (4 * k)
    body = words.astype('<u4').reshape(nb, -1).view(np.uint8)
    return np.concatenate((hdr.reshape(nb, -1), body), axis=1).tobytes()


def ima_decode(blocks, ch, block_align, frames=None):
    """Whole blocks -> (n,) or (n, ch) int16 by the issue's definition (vectorised over blocks and channels)."""
    b = np.frombuffer(blocks, dtype=np.uint8)
    nb = len(b) // block_align
    spb = ima_samples_per_block(block_align, ch)
    b = b[:nb * block_align].reshape(nb, block_align)
    hdr = b[:, :4 * ch].reshape(nb, ch, 4).astype(np.int64)
    pred = hdr[:, :, 0] | (hdr[:, :, 1] << 8)
    pred = np.where(pred >= 32768, pred - 65536, pred)
    idx = hdr[:, :, 2]
    assert (idx <= 88).all()
    words = b[:, 4 * ch:].copy().view('<u4').reshape(nb, -1, ch).astype(np.int64)
    out = np.zeros((nb, spb, ch), dtype=np.int64)
    out[:, 0, :] = pred
    for s in range(1, spb):
        n = (words[:, (s - 1) // 8, :] >> (4 * ((s - 1) % 8))) & 15
        step = IMA_STEP[idx]
        d = (step >> 3) + np.where(n & 1, step >> 2, 0) + np.where(n & 2, step >> 1, 0) + np.where(n & 4, step, 0)
        pred = np.clip(np.where(n & 8, pred - d, pred + d), -32768, 32767)
        idx = np.clip(idx + IMA_ADJ[n], 0, 88)
        out[:, s, :] = pred
    out = out.reshape(nb * spb, ch).astype(np.int16)
    if frames is not None:
        out = out[:frames]
    return out[:, 0] if ch == 1 else out


def ima_block(nibbles, pred, index):
    """One mono block from a nibble stream (a multiple of 8 nibbles, stream order = low nibble first) and a start state."""
    nib = np.asarray(nibbles, dtype=np.uint8).reshape(-1, 2)
    return struct.pack('<hBB', int(pred), int(index), 0) + (nib[:, 0] | (nib[:, 1] << 4)).astype(np.uint8).tobytes()


# ------------------------------------------------------------------------------------------------ samples of every encoding
def encode(x, kind, big=False, block_align=256):
    """float samples (wavgen.make_signal) -> (stored bytes, twin fmt of wavgen, twin's stored array, frames)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if kind == 'u8':
        s = wavgen.encode(x, 'u8')
        return s.tobytes(), 'u8', s, n
    if kind == 'i8':
        s = wavgen.encode(x, 'u8')
        return (s.astype(np.int16) - 128).astype(np.int8).tobytes(), 'u8', s, n
    if kind in ('ulaw', 'alaw'):
        codes = g711_encode(wavgen.encode(x, 'i16'), kind)
        return codes.tobytes(), 'i16', (ULAW if kind == 'ulaw' else ALAW)[codes].astype('<i2'), n
    if kind == 'ima':
        ch = 1 if x.ndim == 1 else x.shape[1]
        blocks = ima_encode(wavgen.encode(x, 'i16'), block_align)
        return blocks, 'i16', ima_decode(blocks, ch, block_align, n).astype('<i2'), n
    s = wavgen.encode(x, kind)
    if kind == 'i24':
        raw = s.astype('<i4').reshape(-1, 1).view(np.uint8)[:, :3]
        raw = raw[:, ::-1] if big else raw
        return np.ascontiguousarray(raw).tobytes(), kind, s, n
    return s.astype(s.dtype.newbyteorder('>' if big else '<')).tobytes(), kind, s, n


def wav_twin(path, twin, sr, fmt):
    """The WAV twin (wavgen.write_wav) of a file whose twin array is `twin` (from `encode`)."""
    return wavgen.write_wav(path, twin, sr, fmt)


# ------------------------------------------------------------------------------------------------ containers
_WAV_TAG = {'u8': (1, 8), 'i16': (1, 16), 'i24': (1, 24), 'i32': (1, 32), 'f32': (3, 32), 'f64': (3, 64), 'alaw': (6, 8), 'ulaw': (7, 8),
            'ima': (0x11, 4)}


def wav_fmt(kind, sr, ch, block_align=256, extensible=False, tag=None, bits=None, spb=None):
    t, b = _WAV_TAG.get(kind, (tag, bits))
    t = t if tag is None else tag
    b = b if bits is None else bits
    if kind == 'ima':
        spb = ima_samples_per_block(block_align, ch) if spb is None else spb
        return struct.pack('<HHIIHHHH', t, ch, sr, sr * block_align // spb, block_align, b, 2, spb)
    align = ch * max(b, 8) // 8
    if extensible:
        guid = struct.pack('<H', t) + bytes.fromhex('000000001000800000aa00389b71')
        return struct.pack('<HHIIHHHHI', 0xFFFE, ch, sr, sr * align, align, b, 22, b, 0) + guid
    body = struct.pack('<HHIIHH', t, ch, sr, sr * align, align, b)
    return body + (struct.pack('<H', 0) if t not in (1, 3) else b'')


def _chunk(cid, body, e='<'):
    return cid + struct.pack(e + 'I', len(body)) + body + (b'\0' if len(body) & 1 else b'')


def write_riff(path, fmt, data, fact=None, before=(), after=(), magic=b'RIFF', unknown_size=False, ds64=None):
    """RIFF / RF64 / BW64: chunks `before` the fmt chunk, fmt, [fact], data, chunks `after`.  ds64 = (data bytes, frames):
    the data chunk then says 0xFFFFFFFF; unknown_size: it says 0xFFFFFFFF with no ds64 (a piped WAV)."""
    body = b'WAVE'
    if ds64 is not None:
        body += _chunk(b'ds64', struct.pack('<QQQI', 0, ds64[0], ds64[1], 0))
    for cid, c in before:
        body += _chunk(cid, c)
    body += _chunk(b'fmt ', fmt)
    if fact is not None:
        body += _chunk(b'fact', struct.pack('<I', fact))
    big = ds64 is not None or unknown_size
    body += b'data' + struct.pack('<I', 0xFFFFFFFF if big else len(data)) + data + (b'\0' if len(data) & 1 else b'')
    for cid, c in after:
        body += _chunk(cid, c)
    with open(path, 'wb') as f:
        f.write(magic + struct.pack('<I', 0xFFFFFFFF if ds64 is not None else len(body)) + body)
    return str(path)


_W64_TAIL = bytes.fromhex('f3acd3118cd100c04f8edb8a')


def _w64_chunk(cid, body):
    c = cid + _W64_TAIL + struct.pack('<Q', 24 + len(body)) + body
    return c + b'\0' * (-len(c) % 8)


def write_w64(path, fmt, data, fact=None, before=()):
    body = b'wave' + _W64_TAIL
    for cid, c in before:
        body += _w64_chunk(cid, c)
    body += _w64_chunk(b'fmt ', fmt)
    if fact is not None:
        body += _w64_chunk(b'fact', struct.pack('<Q', fact))
    body += _w64_chunk(b'data', data)
    with open(path, 'wb') as f:
        f.write(b'riff' + bytes.fromhex('2e91cf11a5d628db04c10000') + struct.pack('<Q', 24 + len(body)) + body)
    return str(path)


def extended(v):
    """A non-negative number -> 80-bit IEEE extended (exact for values with at most 64 significant bits)."""
    from fractions import Fraction
    v = Fraction(v)
    if v == 0:
        return bytes(10)
    e = 0
    while v >= 2 ** 64:
        v /= 2; e += 1
    while v < 2 ** 63:
        v *= 2; e -= 1
    assert v.denominator == 1
    return struct.pack('>HQ', 16383 + 63 + e, int(v))


def _aifc_type(kind, big):
    if kind in ('ulaw', 'alaw'):
        return kind.encode()
    if kind in ('f32', 'f64'):
        return b'fl32' if kind == 'f32' else b'fl64'
    if kind == 'u8':
        return b'raw '
    return b'NONE' if big or kind == 'i8' else b'sowt'


def write_aiff(path, kind, big, data, sr, ch, frames, aifc=None, ctype=None, bits=None, before=(), ssnd_offset=0, ssnd_first=False):
    """AIFF (aifc False: big-endian integers only) or AIFF-C.  bits: the COMM sample size (default: the container width)."""
    aifc = (kind not in ('i8', 'i16', 'i24', 'i32') or not big) if aifc is None else aifc
    bits = (8 * _WIDTH[kind] if kind not in ('ulaw', 'alaw') else 16) if bits is None else bits
    comm = struct.pack('>hIh', ch, frames, bits) + extended(sr)
    if aifc:
        ctype = _aifc_type(kind, big) if ctype is None else ctype
        comm += ctype + b'\x00\x00'                                # an empty pascal string, padded to even
    ssnd = _chunk(b'SSND', struct.pack('>II', ssnd_offset, 0) + b'\xAA' * ssnd_offset + data, '>')
    body = (b'AIFC' if aifc else b'AIFF')
    if aifc:
        body += _chunk(b'FVER', struct.pack('>I', 0xA2805140), '>')
    for cid, c in before:
        body += _chunk(cid, c, '>')
    body += (ssnd + _chunk(b'COMM', comm, '>')) if ssnd_first else (_chunk(b'COMM', comm, '>') + ssnd)
    with open(path, 'wb') as f:
        f.write(b'FORM' + struct.pack('>I', len(body)) + body)
    return str(path)


_AU_CODE = {'ulaw': 1, 'i8': 2, 'i16': 3, 'i24': 4, 'i32': 5, 'f32': 6, 'f64': 7, 'alaw': 27}


def write_au(path, kind, data, sr, ch, swapped=False, unknown_size=False, enc=None, info=b'sndgen\0\0'):
    """Sun/NeXT AU (`.snd`, big-endian samples) or its byte-swapped form (`dns.`, little-endian header and samples)."""
    e = '<' if swapped else '>'
    hdr = struct.pack(e + 'IIIII', 24 + len(info), 0xFFFFFFFF if unknown_size else len(data), _AU_CODE[kind] if enc is None else enc, sr, ch)
    with open(path, 'wb') as f:
        f.write((b'dns.' if swapped else b'.snd') + hdr + info + data)
    return str(path)


def write_caf(path, kind, big, data, sr, ch, unknown_size=False, fmtid=None, version=1, before=()):
    w = _WIDTH[kind]
    if kind in ('ulaw', 'alaw'):
        fid, flags, bits = kind.encode(), 0, 8
    else:
        fid, flags, bits = b'lpcm', (1 if kind in ('f32', 'f64') else 0) | (0 if big else 2), 8 * w
    desc = struct.pack('>d4sIIIII', float(sr), fid if fmtid is None else fmtid, flags, w * ch, 1, ch, bits)
    body = b'desc' + struct.pack('>q', len(desc)) + desc
    for cid, c in before:
        body += cid + struct.pack('>q', len(c)) + c
    body += b'data' + struct.pack('>q', -1 if unknown_size else 4 + len(data)) + struct.pack('>I', 0) + data
    with open(path, 'wb') as f:
        f.write(b'caff' + struct.pack('>HH', version, 0) + body)
    return str(path)


# every (container, kind, big) the reader takes, by the name the tests use
def cases():
    out = []
    for kind in ('ulaw', 'alaw', 'ima'):
        out += [('wav', kind, False), ('wavx', kind, False)] if kind != 'ima' else [('wav', kind, False)]
    for kind in ('u8', 'i16', 'i24', 'i32', 'f32', 'f64', 'ulaw', 'alaw', 'ima'):
        out += [('rf64', kind, False), ('w64', kind, False)]
    out += [('bw64', 'i16', False)]
    out += [('aiff', k, True) for k in ('i8', 'i16', 'i24', 'i32')]
    out += [('aifc', k, True) for k in ('i8', 'i16', 'i24', 'i32', 'f32', 'f64')]
    out += [('aifc', k, False) for k in ('i16', 'i24', 'i32', 'u8', 'ulaw', 'alaw')]
    out += [('aifc-in24', 'i24', True), ('aifc-in32', 'i32', True), ('aifc-FL32', 'f32', True), ('aifc-ULAW', 'ulaw', False)]
    out += [('au', k, True) for k in ('ulaw', 'i8', 'i16', 'i24', 'i32', 'f32', 'f64', 'alaw')]
    out += [('dns', k, False) for k in ('ulaw', 'i16', 'i24', 'f32')]
    out += [('caf', k, True) for k in ('i8', 'i16', 'i24', 'i32', 'f32', 'f64', 'ulaw', 'alaw')]
    out += [('caf', k, False) for k in ('i16', 'i24', 'i32', 'f32', 'f64')]
    return out


def write(path, container, kind, big, x, sr, block_align=256, **kw):
    """Write float samples x ((n,) or (n, ch)) as `container` / `kind` -> (path, twin fmt, twin array)."""
    ch = 1 if np.ndim(x) == 1 else np.shape(x)[1]
    if kind == 'ima':
        block_align = -(-block_align // (4 * ch)) * 4 * ch
    data, tfmt, twin, n = encode(x, kind, big, block_align)
    fact = n if kind in ('ima', 'ulaw', 'alaw') else None
    if container in ('wav', 'wavx'):
        write_riff(path, wav_fmt(kind, sr, ch, block_align, extensible=container == 'wavx'), data, fact=fact, **kw)
    elif container in ('rf64', 'bw64'):
        write_riff(path, wav_fmt(kind, sr, ch, block_align), data, fact=fact, magic=container.upper().encode(), ds64=(len(data), n), **kw)
    elif container == 'w64':
        write_w64(path, wav_fmt(kind, sr, ch, block_align), data, fact=fact, **kw)
    elif container.startswith('aif'):
        ctype = container[5:].encode() if '-' in container else None
        write_aiff(path, kind, big, data, sr, ch, n, aifc=container != 'aiff', ctype=ctype, **kw)
    elif container in ('au', 'dns'):
        write_au(path, kind, data, sr, ch, swapped=container == 'dns', **kw)
    elif container == 'caf':
        write_caf(path, kind, big, data, sr, ch, **kw)
    else:
        raise ValueError(container)
    return str(path), tfmt, twin
