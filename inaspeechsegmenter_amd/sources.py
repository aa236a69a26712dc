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
    parts                   how many consecutive signals it writes (default 1): `parts` signals of `size` samples each, signal k at
                            dst_offset + k * `stride`, stride = `size` rounded up to FRAME_HOP

A source made with a channel selection `sel` (RawSource, flac.FlacSource, sndfmt.AdpcmSource) writes one signal per selected
channel instead of their average: `parts` = len(sel), and its job row comes as a SplitJob with the split row (iss_split) that its
class's launch hands to the split entry point -- downmixed and split files of a pass in the same launch.

An excerpt of a file (io.excerpts) is a source too: its `size` is the excerpt's, its `payload` only the bytes the excerpt needs,
and its job row comes with the window row (iss_window) that its class's launch hands to the windowed entry point.

`pass_order` places a class's launch among the device calls of a pass.  pipeline._Worker.run and segmenter._place are written
against this and nothing else: a new format is one class, and one line in io._classify.
"""
import numpy as np

from . import _native
from . import resample


FRAME_HOP = 160


class SplitJob(tuple):
    """(job row, (dst_stride, [channels])): what `job` returns for a source with a channel selection."""
    __slots__ = ()
    row = property(lambda self: self[0])
    split = property(lambda self: self[1])


def rows_splits(jobs):
    """-> (the job rows of a launch, its keyword arguments): nothing for plain jobs -- the call every launch made before there
    were splits --, else `splits`: the split of every SplitJob among them, None beside a plain job."""
    if not any(isinstance(j, SplitJob) for j in jobs):
        return jobs, {}
    return ([j.row if isinstance(j, SplitJob) else j for j in jobs],
            {'splits': [j.split if isinstance(j, SplitJob) else None for j in jobs]})


class Source:
    __slots__ = ()
    batchable = True
    units = 0
    sel = None                                       # the channel selection, where the class takes one and one was given

    @property
    def parts(self):
        sel = getattr(self, 'sel', None)             # (a subclass's slot that its own __init__ never set: no selection)
        return 1 if sel is None else len(sel)

    @property
    def stride(self):
        return -(-self.size // FRAME_HOP) * FRAME_HOP

    def with_split(self, row):
        """The job `row` as it stands, or with this source's split row beside it."""
        sel = getattr(self, 'sel', None)
        return row if sel is None else SplitJob((row, (self.stride, sel)))

    def reselect(self, sel):
        """This source with another selection of its channels (the file is not read again)."""
        import copy
        other = copy.copy(self)
        other.sel = [int(ch) for ch in sel]
        return other

    def check(self, status):
        pass

    @staticmethod
    def tables(group):
        return None

    def place(self, ctx):
        return self.launch(ctx, self.payload, [self.job(ctx, 0, 0, 0)], self.tables([self]),
                           (self.parts - 1) * self.stride + self.size)


class RawSource(Source):
    """Samples at another rate or channel count, as stored, for the device resampler (Segmenter(ffmpeg=None, resample=True)).
    `fmt` is the ISS_RS_* format of the stored bytes: the dtype's by default; explicit for signed bytes, G.711 and big-endian
    samples.  `sel`: the channels to write apart (None: their average)."""
    __slots__ = ('x', 'sr', 'size', 'fmt', 'sel')
    pass_order = 0

    def __init__(self, x, sr, fmt=None, sel=None):
        self.x, self.sr = np.ascontiguousarray(x), sr
        self.sel = None if sel is None else [int(ch) for ch in sel]
        self.fmt = _native.RS_FORMAT[self.x.dtype] if fmt is None else int(fmt)
        self.size = resample.out_len(x.shape[0], sr)

    @property
    def held(self):
        return max(self.size * self.parts, self.x.nbytes // 2)

    @property
    def payload(self):
        return self.x.reshape(-1).view(np.uint8)

    def job(self, ctx, src_offset, unit_begin, dst_offset):
        return self.with_split(ctx.resample_job(self.x, self.sr, src_offset, dst_offset, self.fmt))

    @staticmethod
    def launch(ctx, staged, jobs, tables, n_signal=-1):
        rows, kw = rows_splits(jobs)
        ctx.resample(staged, rows, n_signal, **kw)


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
    signal, mono at 16 kHz; 'resample': staged, downmixed and resampled in the same call), `nbytes` of payload.  `sel` ('resample'
    only): the channels to write apart (None: their average)."""
    __slots__ = ('s', 'kind', 'size', 'nbytes', 'sel')

    def __init__(self, parsed, kind, sel=None):
        self.s, self.kind = parsed, kind
        self.sel = None if sel is None else [int(ch) for ch in sel]
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
