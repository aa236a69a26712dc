"""FLAC without ffmpeg: the container, the frame index and the sources the device decodes.

The reference's ffmpeg-free read is `soundfile.read` (io.py:36-55), and libsndfile decodes FLAC.  Here a FLAC file (bytes
starting with `fLaC`, optionally behind an ID3v2 tag) reads exactly like its WAV twin -- the PCM WAV of the same samples,
rate and channels, 16 bits for 8/16-bit streams and 24 bits for 24-bit streams.  This module parses the metadata blocks
(STREAMINFO used; PADDING, APPLICATION, SEEKTABLE, VORBIS_COMMENT, CUESHEET, PICTURE and reserved types skipped) and has the
compiled host code index the frames (iss_flac_index); the samples are decoded by flac_decode_kernel on the device
(`FlacSource`, one of the sources of sources.py) or by the host build of the same decoder (`FlacStream.stored`, io.py).
"""
import struct

import numpy as np

from . import _native
from . import resample as R
from .io import need_16k_mono, source_of
from .sources import SCHED_OF, CodedAuto, CodedSched, CodedSource, RawAuto, RawSource, host_window, selection

MAGIC = b'fLaC'
# benchmark switch (tools/bench_flac.py), not a user option: True makes the ffmpeg-free read decode FLAC on the host
# (iss_flac_decode_host in the decode threads) instead of handing the compressed frames to the device
_HOST_DECODE = False
_METADATA = {0: 'STREAMINFO', 1: 'PADDING', 2: 'APPLICATION', 3: 'SEEKTABLE', 4: 'VORBIS_COMMENT', 5: 'CUESHEET', 6: 'PICTURE'}


def _id3_end(buf):
    """Offset after a leading ID3v2 tag (0 if there is none)."""
    if len(buf) >= 10 and buf[:3] == b'ID3':
        size = 0
        for b in buf[6:10]:
            size = (size << 7) | (b & 0x7F)
        return 10 + size + (10 if buf[5] & 0x10 else 0)          # footer flag
    return 0


def is_flac(buf):
    """Do these (leading) bytes start a native FLAC stream?"""
    p = _id3_end(buf)
    return buf[p:p + 4] == MAGIC


def is_ogg_flac(buf):
    return buf[:4] == b'OggS' and b'\x7fFLAC' in buf[:128]


class FlacStream:
    """A parsed FLAC file: STREAMINFO, and the frames indexed by iss_flac_index (offsets relative to `audio`)."""
    __slots__ = ('name', 'audio', 'base', 'frames', 'sr', 'ch', 'bps', 'n')

    def __init__(self, buf, name='<buffer>'):
        buf = bytes(buf)
        p = _id3_end(buf)
        if buf[p:p + 4] != MAGIC:
            raise ValueError(f'{name}: not a FLAC stream')
        p += 4
        info, first = None, True
        while True:
            if p + 4 > len(buf):
                raise ValueError(f'{name}: truncated metadata at byte {p}')
            hdr = buf[p]
            typ, size = hdr & 0x7F, int.from_bytes(buf[p + 1:p + 4], 'big')
            if typ == 127:
                raise ValueError(f'{name}: invalid metadata block type 127 at byte {p}')
            if first and typ != 0:
                raise ValueError(f'{name}: the first metadata block at byte {p} is {_METADATA.get(typ, typ)}, not STREAMINFO')
            if p + 4 + size > len(buf):
                raise ValueError(f'{name}: truncated metadata block at byte {p}')
            if typ == 0:
                if size != 34 or not first:
                    raise ValueError(f'{name}: bad STREAMINFO block at byte {p}')
                b = buf[p + 4:p + 4 + 34]
                minb, maxb = struct.unpack('>HH', b[:4])
                v = int.from_bytes(b[10:18], 'big')
                sr, ch, bps, total = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
                info = (sr, ch, bps, minb, maxb, 0, total)
            first = False
            p += 4 + size
            if hdr & 0x80:
                break
        sr, ch, bps = info[0], info[1], info[2]
        if bps not in (8, 16, 24):
            raise ValueError(f'{name}: {bps}-bit FLAC is not supported without ffmpeg (8, 16 and 24 bits are)')
        if sr < 1:
            raise ValueError(f'{name}: STREAMINFO sample rate {sr}')
        arr = np.frombuffer(buf, dtype=np.uint8)
        try:
            frames = _native.flac_index(arr, p, info)
        except ValueError as exc:
            off, why = exc.args
            raise ValueError(f'{name}: frame at byte {off}: {why}') from None
        frames['offset'] -= p
        self.name, self.audio, self.base, self.frames = name, arr[p:], p, frames
        self.sr, self.ch, self.bps = sr, ch, bps
        self.n = int(frames['first_sample'][-1] + frames['block_size'][-1])

    def check(self, status, first=0):
        """Raise ValueError for the first frame whose decode status (ISS_FLAC_*) is not 0; status[0] is frame `first`'s."""
        bad = np.flatnonzero(np.asarray(status))
        if bad.size:
            k = int(bad[0])
            why = _native.FLAC_STATUS.get(int(status[k]), f'status {int(status[k])}')
            raise ValueError(f'{self.name}: frame at byte {self.base + int(self.frames["offset"][first + k])}: {why}')

    def decode_host(self):
        """The stored samples ((n,) or (n, ch) int16 / int32 << 8) by the host build of the decoder."""
        x, st = _native.flac_decode_host(self.audio, self.frames, self.ch, self.bps, self.n)
        self.check(st)
        return x

    stored = decode_host                                         # (the name sndfmt.Sound has for it: io._stored)

    def source(self, resample=False):
        return source(self, resample)

    def split_source(self, sel):
        """What Segmenter reads for the channels `sel` of a multi-channel stream, each on its own (io.split_source)."""
        if _HOST_DECODE:
            return RawSource(self.decode_host(), self.sr, sel=sel)
        return FlacSource(self, 'resample', sel)

    def auto_source(self, full):
        """What Segmenter reads for a multi-channel stream with channels='auto' (io.auto_source)."""
        if _HOST_DECODE:
            return RawAuto(self.decode_host(), self.sr, full=full) if self.ch > 1 else source(self, True)
        if self.ch == 1 and self.sr == R.SR_OUT:                     # (24-bit: the float path, which shares no pass)
            return FlacSource(self, 'float') if self.bps > 16 else FlacAuto(self, 'pcm')
        return FlacAuto(self)


class FlacSource(CodedSource):
    """A FLAC file for the device decoder (sources.py states what it answers).  kind: 'pcm' (mono 8/16-bit at 16 kHz), 'float'
    (mono 24-bit at 16 kHz: the float path of a 24-bit WAV, so it goes alone and its samples come back to the host) or
    'resample'."""
    __slots__ = ()
    pass_order = 1
    coder = 'flac'                                               # iss_flac_survey surveys what this class's launch staged
    stage_format = property(lambda self: _native.RS_FORMAT[np.dtype('<i4' if self.s.bps > 16 else '<i2')])
    full = property(lambda self: R.SURVEY_FULL[{8: 'i8', 16: 'i16', 24: 'i24'}[self.s.bps]])
    batchable = property(lambda self: self.kind != 'float')
    payload = property(lambda self: self.s.audio)
    frames = property(lambda self: self.s.frames)
    units = property(lambda self: len(self.frames))

    def row(self, ctx, src_offset, frame_begin, dst_offset):
        """Its FLAC_JOB row: into the signal at dst_offset ('pcm'), resampled to dst_offset ('resample'), or staged ('float')."""
        s = self.s
        to, fid, dst, nout = _native.FLAC_TO_STAGE, -1, 0, 0
        if self.kind == 'pcm':
            to, dst = _native.FLAC_TO_SIGNAL, dst_offset
        elif self.kind == 'resample':
            fid, dst, nout = ctx.resample_filter(s.sr)[0], dst_offset, self.size
        return (src_offset, frame_begin, self.units, s.n, s.ch, s.bps, to, fid, dst, nout)

    @staticmethod
    def tables(group):
        return np.concatenate([g.frames for g in group])

    @staticmethod
    def launch(ctx, staged, rows, frames, n_signal=-1, **kw):
        return ctx.flac_decode(staged, frames, rows, n_signal, **kw)

    def samples(self, ctx):
        """'float', on its own: decoded to the staging buffer -> the stored int32 samples on the host (checked)."""
        s = self.s
        st = self.launch(ctx, s.audio, [self.row(ctx, 0, 0, 0)], s.frames, 0)
        x = ctx.flac_get_stage(0, s.n, s.ch, s.bps)
        s.check(st)
        return x


class FlacAuto(CodedAuto, FlacSource):
    """A FLAC file for channels='auto' (sources.CodedAuto): kind 'stage' for two or more channels, and for one channel at
    another rate; 'pcm' for one 8/16-bit channel at 16 kHz.  `full` as the survey's sources state it."""
    __slots__ = ('decision',)

    def __init__(self, stream, kind='stage'):
        FlacSource.__init__(self, stream, kind)
        self.size, self.decision = stream.n if kind == 'pcm' else R.out_len(stream.n, stream.sr), None


class FlacSched(CodedSched, FlacAuto):
    """A FLAC file with a schedule, given or decided from its blocked survey (sources.CodedSched)."""
    __slots__ = ('sched', 'block_chunks', 'rule', 'fade_sec')


SCHED_OF[FlacAuto] = FlacSched


class FlacExcerpt(FlacSource):
    """Outputs [a, b) of a FLAC file for the windowed decode: the frames that cover the stored-rate samples the excerpt needs
    ('pcm': [a, b) themselves; 'resample': resample.input_span of them) and their bytes only.  kind 'stage' (io.survey_sources):
    a and b count stored frames, and those are staged for the survey kernel (TO_STAGE, no filter).  Its `frames` keep the file's sample
    numbering; a malformed frame is named by its byte offset in the file.  Frames outside the run are not decoded, so not checked.
    `sel` ('resample' only): the channels to write apart (None: their average)."""
    __slots__ = ('k0', 'rows', 'win', '_payload')
    payload = property(lambda self: self._payload)
    frames = property(lambda self: self.rows)

    def __init__(self, stream, kind, a, b, sel=None):
        self.s, self.kind, self.size = stream, kind, b - a
        self.sel = selection(sel)
        if kind in ('pcm', 'stage'):
            s0, s1 = a, b
        else:
            j_lo, j_hi = R.input_span(stream.sr, stream.n, a, b - a)
            s0, s1 = j_lo, j_hi + 1
        fr = stream.frames
        k0 = int(np.searchsorted(fr['first_sample'] + fr['block_size'], s0, side='right'))
        k1 = int(np.searchsorted(fr['first_sample'], s1, side='left')) - 1
        rows = fr[k0:k1 + 1].copy()
        byte0 = int(rows['offset'][0])
        rows['offset'] -= byte0
        self.k0, self.rows, self.win = k0, rows, (s0, s1, stream.n, a, b - a)
        self._payload = stream.audio[byte0:byte0 + int(rows['offset'][-1] + rows['length'][-1])]
        self.nbytes = self._payload.nbytes

    def check(self, status):
        self.s.check(status, self.k0)

    def host(self):
        """The same samples by the host build of the decoder, on the same frames (and resample.resample_ref)."""
        s, (s0, s1, total, a, count) = self.s, self.win
        rows = self.rows.copy()
        first = int(rows['first_sample'][0])
        rows['first_sample'] -= first                            # the run alone tiles [0, its samples)
        x, st = _native.flac_decode_host(self._payload, rows, s.ch, s.bps, int(rows['first_sample'][-1] + rows['block_size'][-1]))
        self.check(st)
        x = x[s0 - first:s1 - first]
        return np.ascontiguousarray(x) if self.kind == 'pcm' else host_window(x, s.sr, self.win, self.sel)


def source(stream, resample=False):
    """The FlacSource of a parsed stream under the WAV-twin rules of the ffmpeg-free read (io.need_16k_mono without
    `resample`); 16 kHz mono reads the same either way.  (_HOST_DECODE: the samples decoded here, as the WAV twin reads.)"""
    if _HOST_DECODE:
        return source_of(stream.decode_host(), stream.sr, stream.name, resample)
    if stream.sr == R.SR_OUT and stream.ch == 1:
        return FlacSource(stream, 'float' if stream.bps > 16 else 'pcm')
    if not resample:
        need_16k_mono(stream.name, stream.sr, stream.ch)
    R.check_rate(stream.sr)
    return FlacSource(stream, 'resample')


def decode_on(ctx, src):
    """One file on its own.  'pcm' / 'resample': the resident signal becomes its 16 kHz PCM16 -> the per-frame status, valid
    after the context's next synchronising call (check it with src.check).  'float': -> the stored int32 samples (checked)."""
    return src.place(ctx) if src.batchable else src.samples(ctx)


def read_host(buf, name='<buffer>'):
    """ffmpeg-free host read: -> (stored samples, (n,) or (n, C), sr), the arrays io._parse_wav returns for the WAV twin."""
    stream = FlacStream(buf, name)
    return stream.stored(), stream.sr
