"""Decoded sources the device finishes: what every kind of them answers, the one launch a group of them shares, and the
kind written for the resample kernel.

The ffmpeg-free read hands on a plain numpy array (16 kHz mono samples: int16, or float32 for the float path) or a `Source`:
bytes as stored, which a kernel turns into 16 kHz mono PCM16 inside the resident signal.  A source answers

    size, held, batchable   its length at 16 kHz (it stands where a signal's `size` is read); what it holds while it waits for
                            the packer, in 16-bit sample units; may it share a device pass with other files?
    payload, units          the bytes to stage (a 1-D uint8 view); status entries the device writes for it (frames, blocks)
    row(ctx, src_offset, unit_begin, dst_offset)   its job row, written once per format: payload at byte `src_offset` of the
                            staged bytes, status from entry `unit_begin`, samples to `dst_offset` of the signal
    job(...)                that row as a `Job`, with what the source carries beside it: its window row or its split row
    check(status)           ValueError for a malformed file, from its slice of the status array
    tables(group), launch(ctx, staged, rows, tables, n_signal, **kw)   (of the class) what ONE launch for a group of sources of
                            this class needs besides bytes and rows, and the launch -> the status array (valid after the
                            context's next synchronising call) or None; kw: `windows=`, `splits=` or both, only where some job has one
                            (`mixes=` in place of `splits=` where some selection holds a mix)
    parts                   how many consecutive signals it writes (default 1): `parts` signals of `size` samples each, signal k at
                            dst_offset + k * `stride`, stride = `size` rounded up to FRAME_HOP

A source made with a channel selection `sel` (RawSource, flac.FlacSource, sndfmt.AdpcmSource and its Microsoft twin) writes one signal per selected
channel instead of their average: `parts` = len(sel), and its job carries the split row (iss_split) for the split entry point
-- downmixed and split files of a pass in the same launch.

An entry of `sel` may be a `resample.Mix` in place of a channel index (io.mix_source, io.mix_excerpts): that signal is the
weighted sum of channels the mix states, staged by the resample kernel's MIX instantiations.  Everything that holds for a
selected channel holds for a mix -- `parts`, `stride`, `reselect`, `host()` --, and a launch whose jobs carry any mix goes to
the *_mix entry point (`mixes=`), plain channels beside them as one-term mixes, which are the same samples to the bit.  A launch
without a mix is the launch it always was.

An excerpt of a file (io.excerpts) is a source too, of a class of its own below its format's: its `size` is the excerpt's, its
`payload` only the bytes the excerpt needs, and its job carries the window row (iss_window) for the windowed entry point.  A
windowed launch needs a window beside every job, so whole files and excerpts never share one: launches go by class.

An excerpt made with a channel selection (io.channel_excerpts: RawExcerpt, flac.FlacExcerpt, sndfmt.AdpcmExcerpt) is both: its
job carries the window row AND the split row, for the *_windows_split entry point, which writes the window's outputs of each
selected channel apart -- `parts`, `stride`, `held` and `reselect` as on a whole file with a selection, `size` the excerpt's.
Excerpts with and without a selection share a launch (the downmixed ones with no split beside them), and `host()` of one with
a selection gives one array per selected channel.

A survey (io.survey_sources, Segmenter.survey_channels / survey_files) measures what the channels of stored frames [a, b) hold
instead of writing a signal: its sources are `RawSurvey` (stored bytes for iss_survey) and the 'stage' kind of the decoders'
excerpt classes (decoded to the staging buffer without a filter, then iss_<coder>_survey), and `Group.survey` is their one
launch per class, the class's `survey(ctx, staged, jobs, tables, sources)` -> (status, one resample.SurveyFields per source).

A source of io.auto_source (channels='auto': RawAuto, flac.FlacAuto, sndfmt.AdpcmAuto and its Microsoft twin) is staged once and
read twice on the device: surveyed, then resampled from the bytes that are there.  Its `parts` is 1 and its `size` the downmix's
length, so a pass is laid out before any survey is known; its class is `two_step`, and `Group.launch` then runs the class's
`launch_auto(ctx, staged, jobs, tables, sources, n_signal)`: the decode launch for a coder, ONE survey launch, every source told
its `decision` = (survey.ChannelSurvey, its safe_mix()), ONE resample launch over the staged bytes -- files with a mix and files
with the plain downmix in the same launch.  A file whose decode status is not clean decides nothing and writes nothing.

A scheduled source (io.schedule_source, io.timeline_source: RawSched, flac.FlacSched, sndfmt.AdpcmSched and its Microsoft twin) is
the two-step source of its format with a downmix that differs from one stretch of the file to the next (include/iss.h,
"Schedules"): a resample.Schedule the caller gave, or -- `sched` None -- the one its own timeline decides, the file surveyed in
blocks by ONE iss_*survey_blocks call of its class and resampled by ONE iss_resample_staged_sched launch from the bytes that are
there.  `parts` 1, `size` the downmix's length, `decision` = (survey.SurveyTimeline or None, the schedule) once launched.

A file set (io.FileSet: one file per channel or group of channels; io.set_source and the calls above given a tuple or list of
paths) is a source of three classes of its own -- `SetSource`, `SetSurvey`, `SetAuto` (two_step) --, which stand to the
interleaved twin of the set as RawSource, RawSurvey and RawAuto stand to a file: the same rows, selections, mixes and decisions,
channels counted across the members.  Their payload is the members' bytes end to end (`stage_into` writes them into the staged
buffer piece by piece: nothing is interleaved or joined on the host), their class's `tables` the member rows, and their launches
the *_set entry points, whose kernels read every channel where its member lies.  Whole sets only: no window row.

`Group` is the only place that stages payloads, numbers job rows, launches and hands the status back; `pass_order` places a
class's launch among the device calls of a pass.  pipeline._Worker.run, Segmenter.load_pcm_excerpts and Source.place (one file
alone: segmenter._place) are written against this and nothing else: a new format is one class, and one line in io._classify.
"""
import copy
from typing import NamedTuple

import numpy as np

from . import _native
from . import resample


FRAME_HOP = 160


def selection(sel):
    """A channel selection as the sources keep it: None, or a list of channel indices and / or `resample.Mix`."""
    return None if sel is None else [ch if isinstance(ch, resample.Mix) else int(ch) for ch in sel]


class Job(NamedTuple):
    """What `Source.job` returns: the job row, and the window row or the split `(dst_stride, [channels or mixes])` that goes
    beside it."""
    row: tuple
    window: tuple = None
    split: tuple = None


class AutoJob(NamedTuple):
    """What a two-step source's `job` returns: the row of its FIRST step (survey row, or decode-to-stage row) and where its
    signal goes, for the resample row of the second."""
    row: tuple
    dst: int


class Source:
    __slots__ = ()
    batchable = True
    units = 0
    sel = None                                       # the channel selection, where the class takes one and one was given
    win = None                                       # the window row, of an excerpt

    @property
    def parts(self):
        sel = getattr(self, 'sel', None)             # (a subclass's slot that its own __init__ never set: no selection)
        return 1 if sel is None else len(sel)

    @property
    def stride(self):
        return -(-self.size // FRAME_HOP) * FRAME_HOP

    def job(self, ctx, src_offset, unit_begin, dst_offset):
        sel = getattr(self, 'sel', None)
        return Job(self.row(ctx, src_offset, unit_begin, dst_offset), self.win, None if sel is None else (self.stride, sel))

    def reselect(self, sel):
        """This source with another selection of its channels (the file is not read again)."""
        other = copy.copy(self)
        other.sel = selection(sel)
        return other

    def check(self, status):
        pass

    @property
    def payload_size(self):
        """Bytes of `payload`; `stage_into(dst)` writes them to dst[:payload_size] (a source whose payload lies in several
        pieces -- SetSource -- writes them there without joining them first)."""
        return self.payload.size

    def stage_into(self, dst):
        dst[:] = self.payload

    @staticmethod
    def tables(group):
        return None

    def place(self, ctx):
        """The launch for this file alone (its payload handed on where it lies): the resident signal becomes its samples ->
        the status, or None."""
        return Group(ctx, type(self), [(self, 0)], in_place=True).launch((self.parts - 1) * self.stride + self.size).status


class Group:
    """ONE launch for sources of one class, `placed` = [(source, dst_offset)], in the two steps a pass takes it.  Made while
    the pass is packed: the payloads staged end to end, each on a 16-byte boundary -- in `into(nbytes)`, a page-locked buffer
    of the caller's, else a zeroed array; in_place: one source, not copied --, the jobs with running byte and unit offsets, the
    class's tables.  `launch`ed once
    the signal is there (n_signal >= 0: the launch creates it); `check` after the context's next synchronising read-back."""
    __slots__ = ('ctx', 'cls', 'placed', 'staged', 'jobs', 'tables', 'status')

    def __init__(self, ctx, cls, placed, into=None, in_place=False):
        self.ctx, self.cls, self.placed, self.jobs, self.status = ctx, cls, placed, [], None
        if in_place:                                 # one source alone: nothing to lay out, its payload as it stands
            (only, _), = placed
            self.staged = only.payload
        else:
            nbytes = sum(-(-s.payload_size // 16) * 16 for s, _ in placed)
            self.staged = np.zeros(nbytes, dtype=np.uint8) if into is None else into(nbytes)[:nbytes]
        bpos = ubeg = 0
        for s, dst in placed:
            size = s.payload_size
            if not in_place:
                s.stage_into(self.staged[bpos:bpos + size])
            self.jobs.append(s.job(ctx, bpos, ubeg, dst))
            bpos += -(-size // 16) * 16
            ubeg += s.units
        self.tables = cls.tables([s for s, _ in placed])

    def launch(self, n_signal=-1):
        if getattr(self.cls, 'two_step', False):     # survey, decide, resample what is staged (AutoSource)
            self.status = self.cls.launch_auto(self.ctx, self.staged, self.jobs, self.tables, [s for s, _ in self.placed], n_signal)
            return self
        kw = {}                                      # (a plain launch: the call every launch made before there were any)
        if any(j.window is not None for j in self.jobs):
            kw['windows'] = [j.window for j in self.jobs]
        if any(j.split is not None and any(isinstance(ch, resample.Mix) for ch in j.split[1]) for j in self.jobs):
            kw['mixes'] = [j.split for j in self.jobs]
        elif any(j.split is not None for j in self.jobs):
            kw['splits'] = [j.split for j in self.jobs]
        self.status = self.cls.launch(self.ctx, self.staged, [j.row for j in self.jobs], self.tables, n_signal, **kw)
        return self

    def survey(self):
        """ONE survey launch for the group in place of `launch` (sources of io.survey_sources: every job a TO_STAGE decode
        without a filter, or stored bytes) -> one resample.SurveyFields per source, valid on return; `check` as after `launch`."""
        self.status, fields = self.cls.survey(self.ctx, self.staged, self.jobs, self.tables, [s for s, _ in self.placed])
        return fields

    def check(self, on_error=None):
        """Every source checks its slice of the status.  A ValueError goes to on_error(index in `placed`, exception) and the
        others are still checked; without on_error the first is raised."""
        ubeg = 0
        for k, (s, _) in enumerate(self.placed):
            if self.status is not None:
                try:
                    s.check(self.status[ubeg:ubeg + s.units])
                except ValueError as exc:
                    if on_error is None:
                        raise
                    on_error(k, exc)
            ubeg += s.units


class RawSource(Source):
    """Samples at another rate or channel count, as stored, for the device resampler (Segmenter(ffmpeg=None, resample=True)).
    `fmt` is the ISS_RS_* format of the stored bytes: the dtype's by default; explicit for signed bytes, G.711 and big-endian
    samples.  `sel`: the channels (or mixes of them) to write apart (None: their average)."""
    __slots__ = ('x', 'sr', 'size', 'fmt', 'sel')
    pass_order = 0

    def __init__(self, x, sr, fmt=None, sel=None):
        self.x, self.sr = np.ascontiguousarray(x), sr
        self.sel = selection(sel)
        self.fmt = _native.RS_FORMAT[self.x.dtype] if fmt is None else int(fmt)
        self.size = resample.out_len(x.shape[0], sr)

    @property
    def held(self):
        return max(self.size * self.parts, self.x.nbytes // 2)

    @property
    def payload(self):
        return self.x.reshape(-1).view(np.uint8)

    def row(self, ctx, src_offset, unit_begin, dst_offset):
        """Its RS_JOB row: `size` is ceil(frames * up / down) for a whole file, the window's count for an excerpt."""
        fid, _, _ = ctx.resample_filter(self.sr)
        x = self.x
        return (src_offset, x.shape[0], 1 if x.ndim == 1 else x.shape[1], self.fmt, fid, 0, dst_offset, self.size)

    @staticmethod
    def launch(ctx, staged, rows, tables, n_signal=-1, **kw):
        ctx.resample(staged, rows, n_signal, **kw)


class AutoSource:
    """What the sources of io.auto_source share (a mixin in front of a source class of its format): `full`, the fullscale
    threshold of the survey; `decision`, None until the launch, then (survey.ChannelSurvey, resample.Mix or None)."""
    __slots__ = ()
    two_step = True

    def job(self, ctx, src_offset, unit_begin, dst_offset):
        return AutoJob(self.row(ctx, src_offset, unit_begin, dst_offset), dst_offset)

    def decide(self, fields, sr):
        from .survey import ChannelSurvey
        survey = ChannelSurvey(fields, sr, 0)
        self.decision = (survey, survey.safe_mix())
        return None if self.decision[1] is None else (self.stride, [self.decision[1]])


class RawAuto(AutoSource, RawSource):
    """A file of two or more channels as stored, for channels='auto': surveyed by iss_survey, then downmixed -- by the mix its
    survey suggests, or plainly -- and resampled from the survey's upload (iss_resample_staged_mix)."""
    __slots__ = ('full', 'decision')

    def __init__(self, x, sr, fmt=None, full=1.0):
        RawSource.__init__(self, x, sr, fmt)
        self.full, self.decision = float(full), None

    def row(self, ctx, src_offset, unit_begin, dst_offset):
        """Its SURVEY_JOB row (the first step); `staged_row` is the RS_JOB row over the same bytes."""
        return (src_offset, self.x.shape[0], self.x.shape[1], self.fmt, self.full)

    def staged_row(self, ctx, src_offset, dst_offset):
        return RawSource.row(self, ctx, src_offset, 0, dst_offset)

    @staticmethod
    def launch_auto(ctx, staged, jobs, tables, srcs, n_signal=-1):
        fields = ctx.survey(staged, [j.row for j in jobs])            # the one upload; valid on return
        payload = ctx.staged_payload(None)
        mixes = [s.decide(f, s.sr) for s, f in zip(srcs, fields)]
        ctx.resample_staged(None, payload, [s.staged_row(ctx, j.row[0], j.dst) for s, j in zip(srcs, jobs)], n_signal, mixes=mixes)


class RawExcerpt(RawSource):
    """Outputs [a, b) of a file at another rate or channel count, for the windowed resample kernel: `x` = the stored frames
    j_lo .. j_hi that carry a tap of those outputs (resample.input_span) and nothing else of the file, `sub` the parsed slice
    they came from (its host decode is what `host()` resamples), `win` the iss_window row."""
    __slots__ = ('sub', 'win')

    def __init__(self, sub, x, fmt, a, b, j_lo, frames_total, sel=None):
        self.sub, self.x, self.sr, self.fmt = sub, np.ascontiguousarray(x), sub.sr, int(fmt)
        self.sel = selection(sel)
        self.size = b - a
        self.win = (j_lo, j_lo + self.x.shape[0], frames_total, a, b - a)

    def host(self):
        """The same samples by resample.resample_ref on the host decode of the slice (one array per selected channel)."""
        return host_window(self.sub.stored(), self.sr, self.win, self.sel)


class RawSurvey(RawSource):
    """Stored frames for the survey kernel (io.survey_sources): `x` = frames [first, first + len(x)) of a file of `total`
    frames, of which frames [a, b) are surveyed against the fullscale threshold `full`.  `size` (what packs it into a pass) is
    the length of those frames at 16 kHz.  Its job row is a SURVEY_JOB row, its window row says which frames `x` holds."""
    __slots__ = ('full', 'win')

    def __init__(self, x, sr, fmt, full, a, b, first=0, total=None):
        self.x, self.sr, self.fmt, self.full, self.sel = np.ascontiguousarray(x), sr, int(fmt), float(full), None
        n = self.x.shape[0]
        self.win = (first, first + n, first + n if total is None else total, a, b - a)
        self.size = -(-(b - a) * resample.SR_OUT // sr)

    def row(self, ctx, src_offset, unit_begin, dst_offset):
        x = self.x
        return (src_offset, x.shape[0], 1 if x.ndim == 1 else x.shape[1], self.fmt, self.full)

    @staticmethod
    def survey(ctx, staged, jobs, tables, srcs):
        return None, ctx.survey(staged, [j.row for j in jobs], [j.window for j in jobs])


class SetSource(RawSource):
    """A file set (io.FileSet: one file per channel or per group of channels) as stored, for the SET instantiations of the
    resample kernel: `xs` = the members' stored samples, each (n_m,) or (n_m, ch_m), all of the ISS_RS_* format `fmt` at `sr` Hz.
    It reads like the set's interleaved twin -- the members' channels side by side, a shorter member continued with zeros --,
    which is never built: `payload` is the members' bytes end to end, each on a 16-byte boundary, and `members` says where.
    `sel` as for a RawSource, channels counted across the members; sets of a pass share one launch, as a class of their own."""
    __slots__ = ('xs', 'name', 'frames', 'nch', '_payload')

    def __init__(self, xs, sr, fmt, sel=None, name='<set>'):
        self.xs, self.sr, self.fmt, self.name = [np.ascontiguousarray(x) for x in xs], sr, int(fmt), name
        self.sel = selection(sel)
        self.frames = max(x.shape[0] for x in self.xs)
        self.nch = sum(1 if x.ndim == 1 else x.shape[1] for x in self.xs)
        self.size = resample.out_len(self.frames, sr)
        self._payload = None

    @property
    def held(self):
        return max(self.size * self.parts, sum(x.nbytes for x in self.xs) // 2)

    @property
    def members(self):
        """[(byte offset in `payload`, frames, channels) per member]."""
        out, pos = [], 0
        for x in self.xs:
            out.append((pos, x.shape[0], 1 if x.ndim == 1 else x.shape[1]))
            pos += -(-x.nbytes // 16) * 16
        return out

    @property
    def payload(self):
        if self._payload is None:
            if len(self.xs) == 1:
                self._payload = self.xs[0].reshape(-1).view(np.uint8)
            else:
                self._payload = np.zeros(self.payload_size, dtype=np.uint8)
                self.stage_into(self._payload)
        return self._payload

    @property
    def payload_size(self):
        return sum(-(-x.nbytes // 16) * 16 for x in self.xs[:-1]) + self.xs[-1].nbytes

    def stage_into(self, dst):
        for x, (pos, _, _) in zip(self.xs, self.members):
            dst[pos:pos + x.nbytes] = x.reshape(-1).view(np.uint8)

    def row(self, ctx, src_offset, unit_begin, dst_offset):
        """Its RS_JOB row, the twin's: src_offset is where its payload lies (the launch hands it on to the member rows)."""
        fid, _, _ = ctx.resample_filter(self.sr)
        return (src_offset, self.frames, self.nch, self.fmt, fid, 0, dst_offset, self.size)

    @staticmethod
    def tables(group):
        return [s.members for s in group]

    @staticmethod
    def launch(ctx, staged, rows, tables, n_signal=-1, mixes=None, splits=None):
        ctx.resample_set(staged, rows, tables, n_signal, mixes if splits is None else splits)      # (a split: one-term mixes)


class SetSurvey(SetSource):
    """A file set for the survey kernel's SET instantiation (io.survey_sources): the whole set, against the fullscale threshold
    `full`.  Its job row is a SURVEY_JOB row, the twin's."""
    __slots__ = ('full',)

    def __init__(self, xs, sr, fmt, full, name='<set>'):
        SetSource.__init__(self, xs, sr, fmt, None, name)
        self.full = float(full)
        self.size = -(-self.frames * resample.SR_OUT // sr)

    def row(self, ctx, src_offset, unit_begin, dst_offset):
        return (src_offset, self.frames, self.nch, self.fmt, self.full)

    @staticmethod
    def survey(ctx, staged, jobs, tables, srcs):
        return None, ctx.survey_set(staged, [j.row for j in jobs], tables)


class SetAuto(AutoSource, SetSource):
    """A file set for channels='auto': RawAuto for sets -- surveyed by iss_survey_set, then downmixed by the mix its survey
    suggests, or plainly, from the survey's upload (iss_resample_staged_set)."""
    __slots__ = ('full', 'decision')

    def __init__(self, xs, sr, fmt, full=1.0, name='<set>'):
        SetSource.__init__(self, xs, sr, fmt, None, name)
        self.full, self.decision = float(full), None

    def row(self, ctx, src_offset, unit_begin, dst_offset):
        """Its SURVEY_JOB row (the first step); `staged_row` is the RS_JOB row over the same bytes."""
        return (src_offset, self.frames, self.nch, self.fmt, self.full)

    def staged_row(self, ctx, src_offset, dst_offset):
        return SetSource.row(self, ctx, src_offset, 0, dst_offset)

    @staticmethod
    def launch_auto(ctx, staged, jobs, tables, srcs, n_signal=-1):
        fields = ctx.survey_set(staged, [j.row for j in jobs], tables)      # the one upload; valid on return
        payload = ctx.staged_payload(None)
        mixes = [s.decide(f, s.sr) for s, f in zip(srcs, fields)]
        ctx.resample_staged_set(payload, [s.staged_row(ctx, j.row[0], j.dst) for s, j in zip(srcs, jobs)], tables, n_signal, mixes)


def host_window(x, sr, win, sel=None):
    """What an excerpt's `host()` gives for x = the stored frames [s_begin, s_end) of its window row `win`: their downmix's
    outputs, or with a selection one array per selected channel, each resample.resample_ref on that channel's column
    (resample.mix_ref for an entry that is a mix)."""
    s0, _, total, a, count = win
    if sel is None:
        return resample.resample_ref(x, sr, a, count, s0, total)
    return [resample.mix_ref(x, sr, ch, a, count, s0, total) if isinstance(ch, resample.Mix) else
            resample.resample_ref(x[:, ch], sr, a, count, s0, total) for ch in sel]


class CodedSource(Source):
    """A compressed file for its decode kernel: `s` the parsed file, `kind` where its samples go ('pcm': PCM16 straight into the
    signal, mono at 16 kHz; 'resample': staged, downmixed and resampled in the same call), `nbytes` of payload.  `sel` ('resample'
    only): the channels to write apart (None: their average)."""
    __slots__ = ('s', 'kind', 'size', 'nbytes', 'sel')

    def __init__(self, parsed, kind, sel=None):
        self.s, self.kind = parsed, kind
        self.sel = selection(sel)
        self.size = resample.out_len(parsed.n, parsed.sr) if kind == 'resample' else parsed.n
        self.nbytes = self.payload.nbytes

    @property
    def held(self):
        return max(1, self.nbytes // 2)

    def check(self, status):
        self.s.check(status)

    @classmethod
    def survey(cls, ctx, staged, jobs, tables, srcs):
        """The decode launch of a group of 'stage' excerpts (every job TO_STAGE without a filter, its window the frames [a, b)
        it stages), then ONE survey launch over what it staged -> (the decode status, one resample.SurveyFields per source)."""
        status = cls.launch(ctx, staged, [j.row for j in jobs], tables, 0, windows=[j.window for j in jobs])
        rows = [(k, s.win[4], s.s.ch, s.stage_format, s.full) for k, s in enumerate(srcs)]
        return status, ctx.survey(None, rows, coder=cls.coder)


class CodedAuto(AutoSource):
    """The mixin of a coder's source for channels='auto' (flac.FlacAuto, sndfmt.AdpcmAuto, sndfmt.MsAdpcmAuto).  kind 'stage':
    decoded to the staging buffer without a filter, as a survey's sources are, and resampled from there -- a file of two or more
    channels surveyed there first (iss_<coder>_survey) and told its mix, a one-channel file at another rate resampled as it is.
    kind 'pcm' (one channel at 16 kHz): PCM16 straight into the signal, as ever.  The one-channel files of a coder are of this
    class so that a pass makes ONE decode call per coder: a call's status array and staging buffer are the coder's only ones."""
    __slots__ = ()

    @classmethod
    def launch_auto(cls, ctx, staged, jobs, tables, srcs, n_signal=-1):
        status = cls.launch(ctx, staged, [j.row for j in jobs], tables, n_signal)      # the one decode call (n_signal >= 0: a zeroed signal)
        to_stage = [k for k, s in enumerate(srcs) if s.kind == 'stage']
        if not to_stage:
            return status
        payload = ctx.staged_payload(cls.coder)
        multi = [k for k in to_stage if srcs[k].s.ch > 1]
        fields = {}
        if multi:                                                     # (the survey synchronises: the status is valid after it)
            rows = [(k, srcs[k].s.n, srcs[k].s.ch, srcs[k].stage_format, srcs[k].full) for k in multi]
            fields = dict(zip(multi, ctx.survey(None, rows, coder=cls.coder)))
        ubeg = np.concatenate(([0], np.cumsum([s.units for s in srcs])))
        rows, mixes = [], []
        for k in to_stage:
            s = srcs[k]
            if multi and np.any(status[ubeg[k]:ubeg[k + 1]]):         # a malformed file decides nothing and writes nothing
                continue
            mixes.append(s.decide(fields[k], s.s.sr) if k in fields else None)
            rows.append((k, s.s.n, s.s.ch, s.stage_format, ctx.resample_filter(s.s.sr)[0], 0, jobs[k].dst, s.size))
        if rows:
            ctx.resample_staged(cls.coder, payload, rows, -1, mixes=mixes)
        return status


# ---------------------------------------------------------------------------------------------- schedules and timelines
class SchedSource:
    """What the scheduled sources share (a mixin in front of a two-step class of its format: RawSched, flac.FlacSched,
    sndfmt.AdpcmSched and its Microsoft twin; io.schedule_source, io.timeline_source).  `sched`: a resample.Schedule the caller
    gave, or None for "decide it": the file is then surveyed in blocks of `block_chunks` chunks (include/iss.h, "Survey blocks")
    and its schedule is survey.SurveyTimeline.schedule(rule, fade_sec): safe_schedule() by default, steady_schedule() for rule
    'steady', the run boundaries cross-faded over fade_sec seconds.  `decision`: None until the launch, then (timeline, schedule)
    -- (None, schedule) for a schedule that was given."""
    __slots__ = ()

    def blocks_of(self, frames):
        """K of this source's job of a blocked survey: its block_chunks, or for a given schedule all its chunks (one block)."""
        return self.block_chunks if self.sched is None else max(1, -(-frames // resample.SURVEY_CHUNK))

    def decide_blocks(self, whole, blocks, sr):
        """-> the schedule: the one given, or the one the timeline of these survey fields suggests."""
        from .survey import ChannelSurvey, SurveyTimeline
        if self.sched is not None:
            self.decision = (None, self.sched)
            return self.sched
        per = self.block_chunks * resample.SURVEY_CHUNK
        timeline = SurveyTimeline(ChannelSurvey(whole, sr, 0), [ChannelSurvey(f, sr, b * per) for b, f in enumerate(blocks)], per)
        self.decision = (timeline, timeline.schedule(self.rule, self.fade_sec))
        return self.decision[1]


SCHED_OF = {}                                         # two-step class of channels='auto' -> its scheduled class


def scheduled(auto, sched=None, block_chunks=None, rule='safe', fade_sec=None):
    """The source `auto` of io.auto_source as a scheduled source of its format: the same file, bytes and rows.  rule, fade_sec:
    how a schedule that is to be decided is decided (survey.SurveyTimeline.schedule)."""
    cls = SCHED_OF[type(auto)]
    other = cls.__new__(cls)
    for klass in type(auto).__mro__:
        for name in getattr(klass, '__slots__', ()):
            if hasattr(auto, name):
                setattr(other, name, getattr(auto, name))
    other.sched, other.block_chunks, other.decision = sched, block_chunks, None
    other.rule, other.fade_sec = rule, fade_sec
    return other


class RawSched(SchedSource, RawAuto):
    """A file as stored with a schedule: given (iss_resample_pcm16_sched: one upload, one launch), or decided from its blocked
    survey (iss_survey_blocks, then iss_resample_staged_sched over the survey's upload).  The files of a pass share the launches:
    where any of them is to be decided, all ride on the survey's upload."""
    __slots__ = ('sched', 'block_chunks', 'rule', 'fade_sec')

    @staticmethod
    def launch_auto(ctx, staged, jobs, tables, srcs, n_signal=-1):
        rows = [s.staged_row(ctx, j.row[0], j.dst) for s, j in zip(srcs, jobs)]
        if all(s.sched is not None for s in srcs):
            ctx.resample_sched(staged, rows, [s.decide_blocks(None, None, s.sr) for s in srcs], n_signal)
            return
        whole, blocks = ctx.survey_blocks(staged, [j.row for j in jobs], [s.blocks_of(s.x.shape[0]) for s in srcs])      # the one upload
        payload = ctx.staged_payload(None)
        scheds = [s.decide_blocks(w, b, s.sr) for s, w, b in zip(srcs, whole, blocks)]
        ctx.resample_staged_sched(None, payload, rows, scheds, n_signal)


SCHED_OF[RawAuto] = RawSched


class CodedSched(SchedSource, CodedAuto):
    """The mixin of a coder's scheduled source (flac.FlacSched, sndfmt.AdpcmSched, sndfmt.MsAdpcmSched): CodedAuto's decode call,
    then for the staged files of two or more channels without a schedule ONE blocked survey (iss_<coder>_survey_blocks), and ONE
    iss_resample_staged_sched over what the decode call staged -- a one-channel file by the schedule [(0, None)], which is its
    samples resampled as they are."""
    __slots__ = ()

    @classmethod
    def launch_auto(cls, ctx, staged, jobs, tables, srcs, n_signal=-1):
        status = cls.launch(ctx, staged, [j.row for j in jobs], tables, n_signal)      # the one decode call
        to_stage = [k for k, s in enumerate(srcs) if s.kind == 'stage']
        if not to_stage:
            return status
        payload = ctx.staged_payload(cls.coder)
        multi = [k for k in to_stage if srcs[k].s.ch > 1 and srcs[k].sched is None]
        fields = {}
        if multi:                                                     # (the survey synchronises: the status is valid after it)
            rows = [(k, srcs[k].s.n, srcs[k].s.ch, srcs[k].stage_format, srcs[k].full) for k in multi]
            whole, blocks = ctx.survey_blocks(None, rows, [srcs[k].blocks_of(srcs[k].s.n) for k in multi], coder=cls.coder)
            fields = dict(zip(multi, zip(whole, blocks)))
        ubeg = np.concatenate(([0], np.cumsum([s.units for s in srcs])))
        rows, scheds = [], []
        for k in to_stage:
            s = srcs[k]
            if multi and np.any(status[ubeg[k]:ubeg[k + 1]]):         # a malformed file decides nothing and writes nothing
                continue
            if k in fields:
                scheds.append(s.decide_blocks(*fields[k], s.s.sr))
            elif s.sched is not None:
                scheds.append(s.decide_blocks(None, None, s.s.sr))
            else:
                scheds.append(resample.Schedule([(0, None)]))         # one channel: nothing to decide
            rows.append((k, s.s.n, s.s.ch, s.stage_format, ctx.resample_filter(s.s.sr)[0], 0, jobs[k].dst, s.size))
        if rows:
            ctx.resample_staged_sched(cls.coder, payload, rows, scheds, -1)
        return status


def held(sig):
    """What a decoded signal holds, in 16-bit sample units: an array its samples, a source what it says."""
    return sig.held if isinstance(sig, Source) else sig.size


def batchable(sig):
    """May it go into a super-batch?  A float array may not (re-quantised is not exact), nor a source that says so."""
    return sig.batchable if isinstance(sig, Source) else sig.dtype == np.int16
