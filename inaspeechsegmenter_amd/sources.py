"""Decoded sources the device finishes: what every kind of them answers, and the one written for the resample kernel.

The ffmpeg-free read hands on a plain numpy array (16 kHz mono samples: int16, or float32 for the float path) or a `Source`:
bytes as stored, which a kernel turns into 16 kHz mono PCM16 inside the resident signal.  A source answers

    size, held, batchable   its length at 16 kHz (it stands where a signal's `size` is read); what it holds while it waits for
                            the packer, in 16-bit sample units; may it share a device pass with other files?
    payload, units          the bytes to stage (a 1-D uint8 view); status entries the device writes for it (frames, blocks)
    job(ctx, src_offset, unit_begin, dst_offset)   its job row: payload at byte `src_offset` of the staged bytes, status from
                            entry `unit_begin`, samples to `dst_offset` of the signal
    check(status)           ValueError for a malformed file, from its slice of the status array
    tables(group), launch(ctx, staged, jobs, tables, n_signal)   (of the class) ONE launch for a group of sources of this
                            class: what it needs besides bytes and rows (built while packing), and the launch -> the status
                            array (valid after the context's next synchronising call) or None
    place(ctx)              that launch for this file alone: the resident signal becomes its `size` samples

An excerpt of a file (io.excerpts) is a source too: its `size` is the excerpt's, its `payload` only the bytes the excerpt needs,
and its job row comes with the window row (iss_window) that its class's launch hands to the windowed entry point.

`pass_order` places a class's launch among the device calls of a pass.  pipeline._Worker.run and segmenter._place are written
against this and nothing else: a new format is one class, and one line in io._classify.
"""
import numpy as np

from . import _native
from . import resample


class Source:
    __slots__ = ()
    batchable = True
    units = 0

    def check(self, status):
        pass

    @staticmethod
    def tables(group):
        return None

    def place(self, ctx):
        return self.launch(ctx, self.payload, [self.job(ctx, 0, 0, 0)], self.tables([self]), self.size)


class RawSource(Source):
    """Samples at another rate or channel count, as stored, for the device resampler (Segmenter(ffmpeg=None, resample=True)).
    `fmt` is the ISS_RS_* format of the stored bytes: the dtype's by default; explicit for signed bytes, G.711 and big-endian
    samples."""
    __slots__ = ('x', 'sr', 'size', 'fmt')
    pass_order = 0

    def __init__(self, x, sr, fmt=None):
        self.x, self.sr = np.ascontiguousarray(x), sr
        self.fmt = _native.RS_FORMAT[self.x.dtype] if fmt is None else int(fmt)
        self.size = resample.out_len(x.shape[0], sr)

    @property
    def held(self):
        return max(self.size, self.x.nbytes // 2)

    @property
    def payload(self):
        return self.x.reshape(-1).view(np.uint8)

    def job(self, ctx, src_offset, unit_begin, dst_offset):
        return ctx.resample_job(self.x, self.sr, src_offset, dst_offset, self.fmt)

    @staticmethod
    def launch(ctx, staged, jobs, tables, n_signal=-1):
        ctx.resample(staged, jobs, n_signal)


class RawExcerpt(Source):
    """Outputs [a, b) of a file at another rate or channel count, for the windowed resample kernel: `x` = the stored frames
    j_lo .. j_hi that carry a tap of those outputs (resample.input_span) and nothing else of the file, `sub` the parsed slice
    they came from (its host decode is what `host()` resamples), `win` the iss_window row."""
    __slots__ = ('sub', 'x', 'sr', 'fmt', 'size', 'win')
    pass_order = 0

    def __init__(self, sub, x, fmt, a, b, j_lo, frames_total):
        self.sub, self.x, self.sr, self.fmt = sub, np.ascontiguousarray(x), sub.sr, int(fmt)
        self.size = b - a
        self.win = (j_lo, j_lo + self.x.shape[0], frames_total, a, b - a)

    @property
    def held(self):
        return max(self.size, self.x.nbytes // 2)

    @property
    def payload(self):
        return self.x.reshape(-1).view(np.uint8)

    def job(self, ctx, src_offset, unit_begin, dst_offset):
        fid, _, _ = ctx.resample_filter(self.sr)
        x = self.x
        return (src_offset, x.shape[0], 1 if x.ndim == 1 else x.shape[1], self.fmt, fid, 0, dst_offset, self.size), self.win

    @staticmethod
    def launch(ctx, staged, jobs, tables, n_signal=-1):
        ctx.resample(staged, [j for j, _ in jobs], n_signal, windows=[w for _, w in jobs])

    def host(self):
        """The same samples by resample.resample_ref on the host decode of the slice."""
        j_lo, _, total, a, count = self.win
        return resample.resample_ref(self.sub.stored(), self.sr, a, count, j_lo, total)


class CodedSource(Source):
    """A compressed file for its decode kernel: `s` the parsed file, `kind` where its samples go ('pcm': PCM16 straight into the
    signal, mono at 16 kHz; 'resample': staged, downmixed and resampled in the same call), `nbytes` of payload."""
    __slots__ = ('s', 'kind', 'size', 'nbytes')

    def __init__(self, parsed, kind):
        self.s, self.kind = parsed, kind
        self.size = resample.out_len(parsed.n, parsed.sr) if kind == 'resample' else parsed.n
        self.nbytes = self.payload.nbytes

    @property
    def held(self):
        return max(1, self.nbytes // 2)

    def check(self, status):
        self.s.check(status)


def held(sig):
    """What a decoded signal holds, in 16-bit sample units: an array its samples, a source what it says."""
    return sig.held if isinstance(sig, Source) else sig.size


def batchable(sig):
    """May it go into a super-batch?  A float array may not (re-quantised is not exact), nor a source that says so."""
    return sig.batchable if isinstance(sig, Source) else sig.dtype == np.int16
