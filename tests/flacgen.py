"""A numpy FLAC encoder (RFC 9639) for the tests and tools/bench_flac.py: every subframe type, order, precision, shift,
wasted bits, Rice / Rice2 parameters, escapes, partition order, block-size and sample-rate code, blocking strategy, channel
mode and metadata mix can be chosen, plus an ID3v2 prefix.  The default `realistic` mode picks the smallest of FIXED 0-4
and LPC 1-8 (Levinson-Durbin, quantised coefficients) per block, like an ordinary encoder.

It shares no code with the decoder under test: its CRCs, bit packing and predictors are written here.
"""
import struct

import numpy as np

_CRC16_TAB = None
_CRC16_POS = None        # _CRC16_POS[d, b]: CRC-16 of byte b followed by d zero bytes (the CRC is linear in the message)


def crc8(data):
    c = 0
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _crc16_tab():
    global _CRC16_TAB
    if _CRC16_TAB is None:
        t = np.zeros(256, dtype=np.uint32)
        for b in range(256):
            c = b << 8
            for _ in range(8):
                c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
            t[b] = c
        _CRC16_TAB = t
    return _CRC16_TAB


def crc16(data):
    """Poly 0x8005, init 0, unreflected: XOR of every byte's contribution at its distance from the end."""
    global _CRC16_POS
    m = np.frombuffer(bytes(data), dtype=np.uint8)
    n = m.size
    if n == 0:
        return 0
    tab = _crc16_tab()
    if _CRC16_POS is None or _CRC16_POS.shape[0] < n:
        rows = max(n, 2 * (0 if _CRC16_POS is None else _CRC16_POS.shape[0]), 4096)
        P = np.empty((rows, 256), dtype=np.uint32)
        P[0] = tab                                           # CRC of the single byte b
        for d in range(1, rows):
            prev = P[d - 1]
            P[d] = ((prev << 8) ^ tab[prev >> 8]) & 0xFFFF   # one more zero byte
        _CRC16_POS = P
    d = np.arange(n - 1, -1, -1)
    return int(np.bitwise_xor.reduce(_CRC16_POS[d, m]))


class Bits:
    """MSB-first bit fields (value, width), packed with numpy.  Widths may exceed 64 (unary codes): the value's bits are the
    low ones of the field."""

    def __init__(self):
        self.v, self.w = [], []

    def add(self, value, width):
        self.v.append(np.atleast_1d(np.asarray(value, dtype=np.int64)).astype(np.uint64))
        self.w.append(np.broadcast_to(np.asarray(width, dtype=np.int64), self.v[-1].shape))

    def sadd(self, value, width):
        """signed values in two's complement of `width` bits"""
        v = np.atleast_1d(np.asarray(value, dtype=np.int64))
        w = int(width)
        self.add(v & ((1 << w) - 1) if w < 63 else v, w)

    def nbits(self):
        return int(sum(int(w.sum()) for w in self.w))

    def tobytes(self, align=True):
        v = np.concatenate(self.v) if self.v else np.zeros(0, np.uint64)
        w = np.concatenate(self.w).astype(np.int64) if self.w else np.zeros(0, np.int64)
        ends = np.cumsum(w)
        total = int(ends[-1]) if ends.size else 0
        if align:
            total = -(-total // 8) * 8
        bits = np.zeros(total, dtype=np.uint8)
        L = int(v.max()).bit_length() if v.size else 0
        for j in range(L):
            sel = (((v >> np.uint64(j)) & np.uint64(1)) == 1) & (w > j)
            bits[ends[sel] - 1 - j] = 1
        return np.packbits(bits).tobytes()


def coded_number(v):
    """UTF-8-style frame / sample number (1..7 bytes)."""
    if v < 0x80:
        return bytes([v])
    for n in range(2, 8):
        if v < (1 << (5 * n + 1)):
            out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
            for k in range(n - 2, -1, -1):
                out.append(0x80 | ((v >> (6 * k)) & 0x3F))
            return bytes(out)
    raise ValueError(v)


_RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_SS = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def bs_code_auto(bs):
    if bs == 192:
        return 1
    for k in range(4):
        if bs == 576 << k:
            return 2 + k
    for k in range(8):
        if bs == 256 << k:
            return 8 + k
    return 6 if bs <= 256 else 7


def rate_code_auto(sr):
    if sr in _RATES:
        return _RATES[sr]
    if sr % 1000 == 0 and sr // 1000 < 256:
        return 12
    if sr < 65536:
        return 13
    if sr % 10 == 0 and sr // 10 < 65536:
        return 14
    return 0


def frame_header(bs, sr, ch_code, bps, number, variable, bs_code=None, rate_code=None, ss_code=None):
    bs_code = bs_code_auto(bs) if bs_code is None else bs_code
    rate_code = rate_code_auto(sr) if rate_code is None else rate_code
    ss_code = _SS[bps] if ss_code is None else ss_code
    h = bytearray([0xFF, 0xF8 | int(variable), (bs_code << 4) | rate_code, (ch_code << 4) | (ss_code << 1)])
    h += coded_number(number)
    if bs_code == 6:
        h += bytes([bs - 1])
    elif bs_code == 7:
        h += struct.pack('>H', bs - 1)
    if rate_code == 12:
        h += bytes([sr // 1000])
    elif rate_code == 13:
        h += struct.pack('>H', sr)
    elif rate_code == 14:
        h += struct.pack('>H', sr // 10)
    h.append(crc8(h))
    return bytes(h)


# ------------------------------------------------------------------------------------------------ residuals and predictors
def zigzag(r):
    r = np.asarray(r, dtype=np.int64)
    return np.where(r >= 0, 2 * r, -2 * r - 1).astype(np.int64)


def rice_plan(u, porder, order, maxk, near=False):
    """-> (ks, bits) of the best Rice parameter per partition (exact bit counts; near: only around log2 of the mean)."""
    bs = u.size + order
    psize = bs >> porder
    ks, total = [], 0
    kk = np.arange(maxk + 1, dtype=np.int64)
    start = 0
    for p in range(1 << porder):
        n = psize - (order if p == 0 else 0)
        seg = u[start:start + n]
        start += n
        cand = kk
        if near and n:
            k0 = int(np.log2(seg.mean() + 1))
            cand = kk[max(0, k0 - 1):k0 + 2]
        bits = (seg[None, :] >> cand[:, None]).sum(axis=1) + n * (cand + 1) if n else np.zeros(cand.size, np.int64)
        j = int(np.argmin(bits))
        ks.append(int(cand[j]))
        total += int(bits[j])
    return ks, total


def write_residual(B, r, order, bs, porder=0, rice2=False, escape=False, ks=None):
    """Residual of a FIXED / LPC subframe.  escape: every partition escaped (width = what its values need; 0 if all 0).
    ks: explicit parameters per partition (else the best)."""
    r = np.asarray(r, dtype=np.int64)
    u = zigzag(r)
    pbits = 5 if rice2 else 4
    esc = (1 << pbits) - 1
    B.add(1 if rice2 else 0, 2)
    B.add(porder, 4)
    if ks is None and not escape:
        ks, _ = rice_plan(u, porder, order, esc - 1)
    psize = bs >> porder
    start = 0
    for p in range(1 << porder):
        n = psize - (order if p == 0 else 0)
        seg, useg = r[start:start + n], u[start:start + n]
        start += n
        if escape:
            w = 0 if not n or not np.any(seg) else int(max(int(seg.max()).bit_length(), int((-seg - 1).max()).bit_length())) + 1
            B.add(esc, pbits)
            B.add(w, 5)
            if w:
                B.sadd(seg, w)
            continue
        k = ks[p]
        B.add(k, pbits)
        if n:
            q = useg >> k
            B.add((1 << k) | (useg & ((1 << k) - 1)), q + 1 + k)


def fixed_residual(x, order):
    return np.diff(x, n=order) if order else x.copy()


def levinson_all(x, order):
    """Predictor coefficients of every order 1..order (x[n] ~ sum a[j] x[n-1-j]) of a Welch-windowed block."""
    n = x.size
    w = 1.0 - ((np.arange(n) - (n - 1) / 2) / ((n + 1) / 2)) ** 2
    y = x.astype(np.float64) * w
    R = np.array([np.dot(y[:n - k], y[k:]) for k in range(order + 1)])
    out = [np.zeros(i + 1) for i in range(order)]
    if R[0] == 0:
        return out
    R[0] *= 1.0 + 1e-9
    a = np.zeros(0)
    err = R[0]
    for i in range(order):
        k = (R[i + 1] - np.dot(a, R[i:0:-1])) / err
        a = np.concatenate((a - k * a[::-1], [k]))
        out[i] = a
        err *= (1 - k * k)
        if err <= 0:
            for j in range(i + 1, order):
                out[j] = np.concatenate((a, np.zeros(j - i)))
            break
    return out


def levinson(x, order):
    return levinson_all(x, order)[order - 1]


def quantise_lpc(a, precision, shift=None):
    lim = 1 << (precision - 1)
    m = float(np.max(np.abs(a))) if a.size else 0.0
    if shift is None:
        shift = precision - 1 - (int(np.ceil(np.log2(m))) if m > 0 else 0)
        shift = int(min(max(shift, 0), 15))
    q = np.clip(np.round(a * (1 << shift)), -lim, lim - 1).astype(np.int64)
    return q, shift


def lpc_residual(x, q, shift):
    order = q.size
    acc = np.zeros(x.size - order, dtype=np.int64)
    for j in range(order):
        acc += q[j] * x[order - 1 - j:x.size - 1 - j]
    return x[order:] - (acc >> shift)


# ------------------------------------------------------------------------------------------------ subframes
def write_subframe(B, x, sbps, spec):
    """One subframe of the int64 samples x at sbps bits.  spec: {'type': 'constant' | 'verbatim' | 'fixed' | 'lpc' |
    'realistic', 'order', 'precision', 'shift', 'coefs', 'wasted' (True: detect), 'porder', 'rice2', 'escape'}."""
    x = np.asarray(x, dtype=np.int64)
    bs = x.size
    k = 0
    if spec.get('wasted', True) and np.any(x):
        nz = x[x != 0]
        tz = (nz & -nz)
        k = int(np.log2(int(np.min(tz))))
        k = min(k, sbps - 1)
    xs = x >> k
    sb = sbps - k
    typ = spec.get('type', 'realistic')
    if typ == 'realistic':
        typ, order, q, shift, porder = _choose(xs, sb)
    else:
        order = spec.get('order', 0)
        q, shift, porder = None, 0, spec.get('porder', 0)
        if typ == 'lpc':
            if spec.get('coefs') is not None:
                q, shift = np.asarray(spec['coefs'], dtype=np.int64), spec['shift']
            else:
                q, shift = quantise_lpc(levinson(xs, order), spec.get('precision', 12), spec.get('shift'))
    code = {'constant': 0, 'verbatim': 1}.get(typ, 8 + order if typ == 'fixed' else 31 + order)
    B.add(0, 1)
    B.add(code, 6)
    if k:
        B.add(1, 1)
        B.add(1, k)                  # k-1 zeros and a one
    else:
        B.add(0, 1)
    if typ == 'constant':
        assert np.all(xs == xs[0])
        B.sadd(xs[0], sb)
        return
    if typ == 'verbatim':
        B.sadd(xs, sb)
        return
    B.sadd(xs[:order], sb)
    if typ == 'fixed':
        r = fixed_residual(xs, order)
    else:
        prec = spec.get('precision', 12) if spec.get('type') != 'realistic' else _REAL_PREC
        B.add(prec - 1, 4)
        B.sadd(shift, 5)
        B.sadd(q, prec)
        r = lpc_residual(xs, q, shift)
    while porder and (((bs >> porder) << porder) != bs or (bs >> porder) < order):
        porder -= 1                          # (a short last block cannot take the requested partition order)
    write_residual(B, r, order, bs, porder=porder, rice2=spec.get('rice2', False) or sb > 16,
                   escape=spec.get('escape', False), ks=spec.get('ks'))


_REAL_PREC = 12


def _choose(x, sbps):
    """realistic mode: the smallest of FIXED 0-4 and LPC 1-8 (precision 12), partition order 0-4."""
    bs = x.size
    maxk = 30 if sbps > 16 else 14
    best = None
    for order in range(min(5, bs)):
        r = fixed_residual(x, order)
        _, bits = rice_plan(zigzag(r), 0, order, maxk, near=True)
        if best is None or bits + sbps * order < best[0]:
            best = (bits + sbps * order, 'fixed', order, None, 0)
    if bs > 32:
        coefs = levinson_all(x, 8)
        for order in (2, 4, 8):
            q, shift = quantise_lpc(coefs[order - 1], _REAL_PREC)
            r = lpc_residual(x, q, shift)
            _, bits = rice_plan(zigzag(r), 0, order, maxk, near=True)
            cost = bits + sbps * order + 9 + _REAL_PREC * order
            if cost < best[0]:
                best = (cost, 'lpc', order, q, shift)
    _, typ, order, q, shift = best
    r = fixed_residual(x, order) if typ == 'fixed' else lpc_residual(x, q, shift)
    u = zigzag(r)
    porder, pbits = 0, None
    for p in range(5):
        if (bs >> p) << p != bs or (bs >> p) < order or (bs >> p) < 16:
            break
        _, bits = rice_plan(u, p, order, maxk, near=True)
        bits += (4 if maxk == 14 else 5) << p
        if pbits is None or bits < pbits:
            porder, pbits = p, bits
    return typ, order, q, shift, porder


# ------------------------------------------------------------------------------------------------ stream
def streaminfo(minb, maxb, sr, ch, bps, total):
    v = (sr << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | total
    return struct.pack('>HH', minb, maxb) + b'\0' * 6 + v.to_bytes(8, 'big') + b'\0' * 16


def metadata_block(typ, last=False, size=None):
    if typ == 1:
        body = b'\0' * (size or 37)
    elif typ == 2:
        body = b'test' + b'application data'
    elif typ == 3:
        body = struct.pack('>QQH', 0, 0, 4096) + struct.pack('>QQH', 0xFFFFFFFFFFFFFFFF, 0, 0)
    elif typ == 4:
        vendor, com = b'flacgen', [b'TITLE=synthetic', b'ARTIST=none']
        body = struct.pack('<I', len(vendor)) + vendor + struct.pack('<I', len(com)) + b''.join(struct.pack('<I', len(c)) + c for c in com)
    elif typ == 5:
        body = b'\0' * 128 + struct.pack('>Q', 0) + b'\0' * 259 + b'\x01' + b'\0' * 36
    elif typ == 6:
        mime, desc, img = b'image/png', b'cover', b'\x89PNG\r\n\x1a\n' + b'\xff\xf8' * 20
        body = (struct.pack('>II', 3, len(mime)) + mime + struct.pack('>I', len(desc)) + desc + struct.pack('>IIIII', 1, 1, 24, 0, len(img)) + img)
    else:
        body = b'\0' * (size or 8)
    return bytes([(0x80 if last else 0) | typ]) + len(body).to_bytes(3, 'big') + body


def id3v2(size=100):
    syncsafe = bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F])
    return b'ID3\x04\x00\x00' + syncsafe + b'\0' * size


def stereo_transform(L, R, mode):
    if mode == 'left_side':
        return [L, L - R], 8
    if mode == 'side_right':
        return [L - R, R], 9
    if mode == 'mid_side':
        return [(L + R) >> 1, L - R], 10
    raise ValueError(mode)


def encode(x, sr, bps, blocksize=4096, subframe=None, channel_mode='independent', variable=False, bs_code=None,
           rate_code=None, ss_code=None, metadata=(), id3=False, total_in_streaminfo=True, max_block=None,
           return_offsets=False):
    """x: integer samples (n,) or (n, C) within `bps` bits.  blocksize: an int, or a list of block sizes (their sum = n;
    with variable=True the sample-number strategy).  subframe: a spec dict for every subframe (write_subframe) or a
    function (frame index, channel) -> spec; default realistic.  -> the bytes of a .flac file (and with return_offsets the
    byte offset of every frame in them)."""
    x = np.asarray(x, dtype=np.int64)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    if isinstance(blocksize, int):
        sizes = [blocksize] * (n // blocksize) + ([n % blocksize] if n % blocksize else [])
    else:
        sizes = list(blocksize)
        assert sum(sizes) == n
    spec_of = subframe if callable(subframe) else (lambda f, c: subframe or {'type': 'realistic'})
    frames = []
    pos = 0
    for f, bs in enumerate(sizes):
        blk = x[pos:pos + bs]
        if ch == 2 and channel_mode != 'independent':
            chans, ch_code = stereo_transform(blk[:, 0], blk[:, 1], channel_mode)
            side = {8: 1, 9: 0, 10: 1}[ch_code]
        else:
            chans, ch_code, side = [blk[:, c] for c in range(ch)], ch - 1, -1
        hdr = frame_header(bs, sr, ch_code, bps, pos if variable else f, variable,
                           bs_code=bs_code if (bs_code is not None and f < len(sizes) - 1) or (bs_code in (6, 7)) else None,
                           rate_code=rate_code, ss_code=ss_code)
        B = Bits()
        for c, xc in enumerate(chans):
            write_subframe(B, xc, bps + (1 if c == side else 0), spec_of(f, c))
        body = hdr + B.tobytes(align=True)
        frames.append(body + struct.pack('>H', crc16(body)))
        pos += bs
    maxb = max_block if max_block is not None else max(sizes)
    meta = [bytes([0]) + (34).to_bytes(3, 'big') + streaminfo(min(sizes), min(maxb, 65535), sr, ch, bps,
                                                              n if total_in_streaminfo else 0)]
    for t in metadata:
        meta.append(metadata_block(t))
    meta[-1] = bytes([meta[-1][0] | 0x80]) + meta[-1][1:]
    head = (id3v2() if id3 else b'') + b'fLaC' + b''.join(meta)
    data = head + b''.join(frames)
    if return_offsets:
        return data, list(len(head) + np.concatenate(([0], np.cumsum([len(f) for f in frames])[:-1])))
    return data


def write(path, x, sr, bps, **kw):
    with open(path, 'wb') as f:
        f.write(encode(x, sr, bps, **kw))
    return str(path)


def wav_twin(path, x, sr, bps):
    """The WAV twin of a FLAC of integer samples x at `bps` bits: 16-bit (8-bit widened x << 8) or 24-bit PCM."""
    import wavgen
    x = np.asarray(x, dtype=np.int64)
    if bps <= 16:
        return wavgen.write_wav(path, (x << (16 - bps)).astype('<i2'), sr, 'i16')
    return wavgen.write_wav(path, x.astype('<i4'), sr, 'i24')
