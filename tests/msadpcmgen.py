"""Microsoft ADPCM (WAVE format tag 2) for the tests, written from the text of include/iss.h and sharing no code with the
package: an encoder (nearest code), a plain sample-at-a-time decoder, a block builder for crafted code sequences, the `fmt `
chunk with its 32-byte extension and writers for RIFF, RF64 and Wave64.  No libsndfile was at hand: what these decode is this
project's own definition of the format (floor rounding, delta raised to 16 and capped at 2^21)."""
import struct

import numpy as np

C1 = (256, 512, 0, 192, 240, 460, 392)
C2 = (0, -256, 0, 64, 0, -208, -232)
ADAPT = (230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230)
DELTA_MIN, DELTA_MAX = 16, 1 << 21


def samples_per_block(block_align, ch):
    return (block_align - 7 * ch) * 2 // ch + 2


# ------------------------------------------------------------------------------------------------ decoder
def decode_block(blk, ch, n=None):
    """One block (bytes) -> (its samples [n, ch] as Python ints in int16 range, the bPredictor values as stored)."""
    spb = samples_per_block(len(blk), ch)
    n = spb if n is None else n
    out = [[0] * ch for _ in range(n)]
    preds = list(blk[:ch])
    for c in range(ch):
        p = preds[c] if preds[c] < 7 else 0
        delta = struct.unpack_from('<h', blk, ch + 2 * c)[0]
        delta = max(delta, DELTA_MIN)
        samp1 = struct.unpack_from('<h', blk, 3 * ch + 2 * c)[0]
        samp2 = struct.unpack_from('<h', blk, 5 * ch + 2 * c)[0]
        if n > 0:
            out[0][c] = samp2
        if n > 1:
            out[1][c] = samp1
        for s in range(2, n):
            k = (s - 2) * ch + c
            byte = blk[7 * ch + (k >> 1)]
            code = (byte >> 4) if k % 2 == 0 else (byte & 15)
            signed = code - 16 if code >= 8 else code
            pred = (samp1 * C1[p] + samp2 * C2[p]) >> 8            # Python's >> is floor
            v = min(32767, max(-32768, pred + signed * delta))
            samp2, samp1 = samp1, v
            out[s][c] = v
            delta = min(DELTA_MAX, max(DELTA_MIN, (ADAPT[code] * delta) >> 8))
    return out, preds


def decode(blocks, ch, block_align, frames=None):
    """Whole blocks -> (n,) or (n, ch) int16; `frames` cuts the last block as a `fact` count does."""
    nb = len(blocks) // block_align
    spb = samples_per_block(block_align, ch)
    total = nb * spb if frames is None or frames > nb * spb else frames
    rows = []
    for b in range(-(-total // spb)):
        rows += decode_block(blocks[b * block_align:(b + 1) * block_align], ch, min(spb, total - b * spb))[0]
    out = np.array(rows, dtype=np.int16).reshape(total, ch)
    return out[:, 0] if ch == 1 else out


# ------------------------------------------------------------------------------------------------ encoder
def encode(pcm16, block_align, predictor=None, delta=None):
    """(n,) or (n, ch) int16 -> whole blocks (bytes); the last block is filled by repeating the last frame.  Per block and
    channel: the predictor with the smallest summed |error| on the block's own samples (or the forced index `predictor`), the
    seeds samp2 = x[0], samp1 = x[1], the header delta from the first residual (or the forced `delta`), then the nearest code
    in [-8, 7] against the decoder's own state."""
    x = np.asarray(pcm16, dtype=np.int64)
    x = x.reshape(len(x), -1)
    n, ch = x.shape
    assert block_align > 7 * ch and (block_align - 7 * ch) * 2 % ch == 0
    spb = samples_per_block(block_align, ch)
    nb = max(1, -(-n // spb))
    x = np.concatenate((x, np.repeat(x[-1:], nb * spb - n, axis=0))).reshape(nb, spb, ch)
    c1, c2 = np.array(C1, dtype=np.int64), np.array(C2, dtype=np.int64)
    adapt = np.array(ADAPT, dtype=np.int64)
    if predictor is None:
        err = np.stack([np.abs(x[:, 2:] - ((x[:, 1:-1] * c1[p] + x[:, :-2] * c2[p]) >> 8)).sum(axis=1) for p in range(7)]) \
            if spb > 2 else np.zeros((7, nb, ch))
        pidx = np.argmin(err, axis=0)
    else:
        pidx = np.full((nb, ch), int(predictor), dtype=np.int64)
    s2, s1 = x[:, 0].copy(), x[:, 1].copy()
    if delta is None:
        first = np.abs(x[:, 2] - ((s1 * c1[pidx] + s2 * c2[pidx]) >> 8)) if spb > 2 else np.zeros((nb, ch), dtype=np.int64)
        hdelta = np.clip(first // 4, DELTA_MIN, 32767)
    else:
        hdelta = np.full((nb, ch), int(delta), dtype=np.int64)
    d = np.maximum(hdelta, DELTA_MIN)
    codes = np.zeros((nb, spb - 2, ch), dtype=np.int64)
    for s in range(2, spb):
        pred = (s1 * c1[pidx] + s2 * c2[pidx]) >> 8
        q = np.clip(np.floor_divide(2 * (x[:, s] - pred) + d, 2 * d), -8, 7)
        v = np.clip(pred + q * d, -32768, 32767)
        s2, s1 = s1, v
        code = q & 15
        codes[:, s - 2] = code
        d = np.clip((adapt[code] * d) >> 8, DELTA_MIN, DELTA_MAX)
    flat = codes.reshape(nb, -1)
    body = ((flat[:, 0::2] << 4) | flat[:, 1::2]).astype(np.uint8)
    hdr = np.concatenate((pidx.astype(np.uint8), hdelta.astype('<i2').view(np.uint8).reshape(nb, -1),
                          x[:, 1].astype('<i2').view(np.uint8).reshape(nb, -1),
                          x[:, 0].astype('<i2').view(np.uint8).reshape(nb, -1)), axis=1)
    return np.concatenate((hdr, body), axis=1).tobytes()


def block(codes, predictor=0, delta=16, samp1=0, samp2=0):
    """One block from explicit code sequences: `codes` (ncodes,) for mono or (ncodes, ch), values 0 .. 15 in stream order per
    channel; predictor / delta / samp1 / samp2 scalars or one per channel.  ncodes * ch must be even."""
    codes = np.asarray(codes, dtype=np.int64)
    codes = codes.reshape(len(codes), -1)
    ch = codes.shape[1]
    per = lambda v: [int(v)] * ch if np.ndim(v) == 0 else [int(t) for t in v]
    flat = codes.reshape(-1)
    assert flat.size % 2 == 0 and ((flat >= 0) & (flat < 16)).all()
    body = ((flat[0::2] << 4) | flat[1::2]).astype(np.uint8).tobytes()
    return (bytes(per(predictor)) + struct.pack(f'<{ch}h', *per(delta)) + struct.pack(f'<{ch}h', *per(samp1)) +
            struct.pack(f'<{ch}h', *per(samp2)) + body)


# ------------------------------------------------------------------------------------------------ containers
def fmt(sr, ch, block_align, spb=None, ncoef=7, coefs=None, cbsize=32, bits=4, tag=2):
    """The 50-byte `fmt ` body: WAVEFORMATEX, then wSamplesPerBlock, wNumCoef and the coefficient pairs."""
    spb = samples_per_block(block_align, ch) if spb is None else spb
    coefs = [v for pair in zip(C1, C2) for v in pair] if coefs is None else list(coefs)
    return (struct.pack('<HHIIHHH', tag, ch, sr, sr * block_align // max(spb, 1), block_align, bits, cbsize) +
            struct.pack('<HH', spb, ncoef) + struct.pack(f'<{len(coefs)}h', *coefs))


def short_fmt(sr, ch, block_align):
    """An 18-byte `fmt ` body (cbSize 0): what a writer that forgot the extension leaves."""
    return struct.pack('<HHIIHHH', 2, ch, sr, sr * block_align // 2, block_align, 4, 0)


def extensible_fmt(sr, ch, block_align):
    """WAVE_FORMAT_EXTENSIBLE whose sub-format GUID says tag 2."""
    guid = struct.pack('<H', 2) + bytes.fromhex('000000001000800000aa00389b71')
    return struct.pack('<HHIIHHHHI', 0xFFFE, ch, sr, sr * block_align // 2, block_align, 4, 22, 4, 0) + guid


def _chunk(cid, body):
    return cid + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')


def write_riff(path, fmt_body, data, fact=None, before=()):
    body = b'WAVE' + b''.join(_chunk(c, b) for c, b in before) + _chunk(b'fmt ', fmt_body)
    if fact is not None:
        body += _chunk(b'fact', struct.pack('<I', fact))
    body += _chunk(b'data', data)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)
    return str(path)


def write_rf64(path, fmt_body, data, fact):
    body = b'WAVE' + _chunk(b'ds64', struct.pack('<QQQI', 0, len(data), fact, 0)) + _chunk(b'fmt ', fmt_body)
    body += _chunk(b'fact', struct.pack('<I', 0xFFFFFFFF))
    body += b'data' + struct.pack('<I', 0xFFFFFFFF) + data + (b'\0' if len(data) & 1 else b'')
    with open(path, 'wb') as f:
        f.write(b'RF64' + struct.pack('<I', 0xFFFFFFFF) + body)
    return str(path)


_W64_TAIL = bytes.fromhex('f3acd3118cd100c04f8edb8a')


def _w64_chunk(cid, body):
    c = cid + _W64_TAIL + struct.pack('<Q', 24 + len(body)) + body
    return c + b'\0' * (-len(c) % 8)


def write_w64(path, fmt_body, data, fact=None):
    body = b'wave' + _W64_TAIL + _w64_chunk(b'fmt ', fmt_body)
    if fact is not None:
        body += _w64_chunk(b'fact', struct.pack('<Q', fact))
    body += _w64_chunk(b'data', data)
    with open(path, 'wb') as f:
        f.write(b'riff' + bytes.fromhex('2e91cf11a5d628db04c10000') + struct.pack('<Q', 24 + len(body)) + body)
    return str(path)


def data_offset(path):
    """Byte offset of the first block in a RIFF file written here."""
    return open(path, 'rb').read().index(b'data') + 8


def write(path, x, sr, block_align, container='wav', predictor=None, delta=None):
    """float samples x ((n,) or (n, ch), within +-1) -> (path, the PCM16 twin array (n,) or (n, ch) by `decode`)."""
    x = np.asarray(x, dtype=np.float64)
    pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    n = len(pcm)
    blocks = encode(pcm, block_align, predictor, delta)
    f = fmt(sr, ch, block_align)
    if container == 'wav':
        write_riff(path, f, blocks, fact=n)
    elif container == 'rf64':
        write_rf64(path, f, blocks, n)
    elif container == 'w64':
        write_w64(path, f, blocks, fact=n)
    else:
        raise ValueError(container)
    return str(path), decode(blocks, ch, block_align, n)
