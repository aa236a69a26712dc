"""What the channels of a file hold: the result of a channel survey.

`Segmenter.survey_channels` (the device, csrc/survey.hip) and `io.survey_channels` (the host-only twin) both return a
`ChannelSurvey`: the measured fields of resample.SurveyFields (include/iss.h, "Channel survey", states them and the order of
the three sums) and what is derived from them here, in Python float64, from those fields only -- so two surveys whose
fields are equal are equal in everything.
"""
import math

import numpy as np

from . import resample as R

ACTIVE_FLOOR_DB = -60.0          # a definition, not a measurement: a channel whose RMS lies 60 dB below full scale counts as empty
INVERTED_CORR = -0.5             # likewise: a pair at or below this correlation counts as polarity-inverted


class ChannelSurvey:
    """The survey of stored frames [first, first + n) of a file of `channels` channels at `sr` Hz.

    Measured (numpy arrays, one entry per channel): peak, zeros, fullscale, nonfinite, s1, s2; s12 (one entry per pair c < d in
    the order of `pairs`; None above resample.SURVEY_PAIR_CHANNELS channels).
    Derived: dc = s1 / n, rms = sqrt(s2 / n), rms_db = 20 log10(rms) (-inf for 0), corr(c, d), downmix_loss_db, active(),
    inverted(), rows()."""
    __slots__ = ('fields', 'sr', 'first')

    def __init__(self, fields, sr, first=0):
        self.fields, self.sr, self.first = fields, int(sr), int(first)

    n = property(lambda self: self.fields.n)
    channels = property(lambda self: len(self.fields.peak))
    peak = property(lambda self: self.fields.peak)
    zeros = property(lambda self: self.fields.zeros)
    fullscale = property(lambda self: self.fields.fullscale)
    nonfinite = property(lambda self: self.fields.nonfinite)
    s1 = property(lambda self: self.fields.s1)
    s2 = property(lambda self: self.fields.s2)
    s12 = property(lambda self: self.fields.s12)
    pairs = property(lambda self: R.survey_pairs(self.channels))

    def __eq__(self, other):
        """Equal to the bit in every measured field (and the same frames of a file of the same rate)."""
        if not isinstance(other, ChannelSurvey):
            return NotImplemented
        a, b = self.fields, other.fields
        return (self.sr, self.first, a.n) == (other.sr, other.first, b.n) and (a.s12 is None) == (b.s12 is None) and all(
            np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64))
            for x, y in zip(a[1:7] + ((a.s12,) if a.s12 is not None else ()), b[1:7] + ((b.s12,) if b.s12 is not None else ())))

    __hash__ = None

    @property
    def dc(self):
        return [float(v) / self.n if self.n else 0.0 for v in self.s1]

    @property
    def rms(self):
        return [math.sqrt(float(v) / self.n) if self.n else 0.0 for v in self.s2]

    @property
    def rms_db(self):
        return [20.0 * math.log10(v) if v > 0 else -math.inf for v in self.rms]

    def pair(self, c, d):
        """s12 of channels c != d."""
        c, d = min(c, d), max(c, d)
        return float(self.s12[self.pairs.index((c, d))])

    def corr(self, c, d):
        """(s12 - s1c s1d / n) / sqrt((s2c - s1c^2 / n) (s2d - s1d^2 / n)); NaN when a factor is not positive (a silent or
        constant channel) or pairs were not computed."""
        if self.s12 is None or not self.n:
            return math.nan
        n, s1, s2 = self.n, self.s1, self.s2
        vc, vd = float(s2[c]) - float(s1[c]) ** 2 / n, float(s2[d]) - float(s1[d]) ** 2 / n
        if not (vc > 0 and vd > 0):
            return math.nan
        return (self.pair(c, d) - float(s1[c]) * float(s1[d]) / n) / math.sqrt(vc * vd)

    @property
    def downmix_loss_db(self):
        """10 log10(P_mix / P_avg): the power of the default downmix (the mean of all channels) against the mean power of the
        channels.  0 for identical channels, strongly negative when the downmix cancels them; None when pairs were not computed."""
        if self.s12 is None:
            return None
        ch, n = self.channels, self.n
        tot = math.fsum(float(v) for v in self.s2)
        if not n or not tot > 0:
            return 0.0
        p_mix = (tot + 2.0 * math.fsum(float(v) for v in self.s12)) / (ch * ch * n)
        p_avg = tot / (ch * n)
        return 10.0 * math.log10(p_mix / p_avg) if p_mix > 0 else -math.inf

    def active(self, floor_db=ACTIVE_FLOOR_DB):
        """The channels, ascending, with peak > 0 and rms_db >= floor_db: the list to pass as `channels=`.  The default floor
        is a definition, not a measurement."""
        db = self.rms_db
        return [c for c in range(self.channels) if self.peak[c] > 0 and db[c] >= floor_db]

    def inverted(self, threshold=INVERTED_CORR):
        """The pairs (c, d), c < d, with corr <= threshold.  The default threshold is a definition, not a measurement."""
        if self.s12 is None:
            return []
        return [(c, d) for c, d in self.pairs if self.corr(c, d) <= threshold]

    def safe_mix(self):
        """The downmix this survey suggests in place of the mean of all channels -> a resample.Mix, or None for "the plain
        downmix".  A definition, as active() and inverted() are, computed from the measured fields only, through active() and
        corr() with their default floor and threshold:
          1. A = active().  One channel, or A empty (a silent file has nothing to save): None.
          2. Signs.  Without pair sums (s12 None: more than resample.SURVEY_PAIR_CHANNELS channels) every sign is +1.  Else r = the
             channel of A with the largest s2 (ties: the lowest index), and for every other c of A the sign is -1 where
             corr(r, c) <= INVERTED_CORR, else +1 (NaN: +1).
          3. A = all channels and every sign +1: None.
          4. Else Mix(terms = (c, sign[c]) for c of A ascending, divisor = len(A)): the mean of the channels kept, the inverted
             ones turned back.  It divides by the number of terms, so no mix saturates.
        None rides as a job without mixes, whose output is the default call's to the bit: a healthy file is read as ever."""
        act = self.active()
        if self.channels == 1 or not act:
            return None
        sign = {c: 1.0 for c in act}
        if self.s12 is not None:
            r = max(act, key=lambda c: (float(self.s2[c]), -c))
            for c in act:
                if c != r and self.corr(r, c) <= INVERTED_CORR:      # (NaN compares False)
                    sign[c] = -1.0
        if len(act) == self.channels and all(v == 1.0 for v in sign.values()):
            return None
        return R.Mix(tuple((c, sign[c]) for c in act), float(len(act)))

    def rows(self, floor_db=ACTIVE_FLOOR_DB):
        """One tuple per channel for printing: (channel, frames, peak, rms_db, dc, zeros, fullscale, nonfinite, active)."""
        act, db, dc = set(self.active(floor_db)), self.rms_db, self.dc
        return [(c, self.n, float(self.peak[c]), db[c], dc[c], int(self.zeros[c]), int(self.fullscale[c]), int(self.nonfinite[c]),
                 c in act) for c in range(self.channels)]

    def __repr__(self):
        return f'ChannelSurvey({self.channels} channels, frames [{self.first}, {self.first + self.n}) at {self.sr} Hz)'


DEFAULT_BLOCK_SEC = 10.0         # a definition: the block length of a timeline where none is given
DEFAULT_FADE_SEC = 0.05          # likewise: the cross-fade at the run boundaries of a steady schedule
RULES = ('safe', 'steady')       # the decision rules of a timeline: safe_schedule(), steady_schedule()


def rule_fade(rule='safe', fade_sec=None):
    """The cross-fade a timeline's schedule gets, in seconds: fade_sec, or for None the rule's default -- 0 for 'safe' (hard
    cuts, as ever), DEFAULT_FADE_SEC for 'steady'.  ValueError for a rule that is none of RULES (hysteresis, a minimum run
    length and fade curves other than the linear one are not offered) and for a fade that is negative or not finite."""
    if rule not in RULES:
        raise ValueError(f"rule={rule!r}: 'safe' or 'steady' (no hysteresis, no minimum run length)")
    if fade_sec is None:
        return DEFAULT_FADE_SEC if rule == 'steady' else 0.0
    if isinstance(fade_sec, (bool, np.bool_)) or not isinstance(fade_sec, (int, float, np.integer, np.floating)) or \
            not math.isfinite(fade_sec) or fade_sec < 0:
        raise ValueError(f'fade_sec={fade_sec!r}: a finite number of seconds, 0 or above (the fade is linear)')
    return float(fade_sec)


def block_chunks(block_sec, sr):
    """K of include/iss.h's "Survey blocks": a block holds K = max(1, floor(block_sec * sr / 1024 + 0.5)) chunks of
    resample.SURVEY_CHUNK frames.  ValueError for a block_sec that is not a finite number above 0."""
    if isinstance(block_sec, (bool, np.bool_)) or not isinstance(block_sec, (int, float, np.integer, np.floating)) or \
            not math.isfinite(block_sec) or not block_sec > 0:
        raise ValueError(f'block_sec={block_sec!r}: a finite number of seconds above 0')
    return max(1, math.floor(float(block_sec) * sr / R.SURVEY_CHUNK + 0.5))


class SurveyTimeline:
    """A survey resolved in time (include/iss.h, "Survey blocks"): `whole`, the ChannelSurvey of the whole file; `blocks`, one
    ChannelSurvey per block of `block_frames` = K * resample.SURVEY_CHUNK stored frames counted from frame 0, the last block
    shorter.  Block b is the survey of frames [b * block_frames, min((b + 1) * block_frames, n)) to the bit.  Equal to another
    when `whole`, every block and block_frames are equal -- to the bit, as ChannelSurvey.__eq__ is."""
    __slots__ = ('whole', 'blocks', 'block_frames')

    def __init__(self, whole, blocks, block_frames):
        self.whole, self.blocks, self.block_frames = whole, list(blocks), int(block_frames)

    sr = property(lambda self: self.whole.sr)
    n = property(lambda self: self.whole.n)
    channels = property(lambda self: self.whole.channels)

    def __eq__(self, other):
        if not isinstance(other, SurveyTimeline):
            return NotImplemented
        return self.block_frames == other.block_frames and self.whole == other.whole and len(self.blocks) == len(other.blocks) \
            and all(a == b for a, b in zip(self.blocks, other.blocks))

    __hash__ = None

    def safe_schedule(self):
        """The schedule this timeline suggests -> a resample.Schedule.  A definition, as ChannelSurvey.safe_mix() is: block b
        decides blocks[b].safe_mix() alone, adjacent blocks with equal decisions merge into one run, and run begins are block
        begins.  Pure Python over measured fields, so timelines equal to the bit decide equally.  Known properties: the
        reference channel of safe_mix() may change from block to block, so an inverted pair may come out as (L - R)/2 in one
        run and (R - L)/2 in the next; a run that keeps one of two channels is 6 dB above its (L + R)/2 neighbours; either
        leaves a discontinuity of one filter length at the boundary.  No hysteresis, crossfade or minimum run length."""
        return R.Schedule((begin, mix) for begin, _, mix in self.runs())

    def runs(self):
        """[(begin frame, [block indices], mix or None)] per run of safe_schedule()."""
        out = []
        for b, blk in enumerate(self.blocks):
            mix = blk.safe_mix()
            if out and out[-1][2] == mix:
                out[-1][1].append(b)
            else:
                out.append((b * self.block_frames, [b], mix))
        return out or [(0, [], None)]

    def schedule(self, rule='safe', fade_sec=None):
        """The schedule `rule` decides, its run boundaries cross-faded over rule_fade(rule, fade_sec) seconds: 'safe' is
        safe_schedule() (with the defaults exactly that), 'steady' is steady_schedule()."""
        fade = rule_fade(rule, fade_sec)
        if rule == 'steady':
            return self.steady_schedule(fade)
        sched = self.safe_schedule()
        return R.Schedule(sched.runs, R.fade_halves([b for b, _ in sched.runs], fade, self.sr)) if fade else sched

    def steady_schedule(self, fade_sec=DEFAULT_FADE_SEC):
        """A schedule that is steady over time -> a resample.Schedule whose runs cross-fade over `fade_sec` seconds
        (resample.fade_halves; 0: hard cuts).  A definition, as INVERTED_CORR is; pure Python over measured fields, so timelines
        equal to the bit decide equally:
          1. One channel: [(0, None)].
          2. W = the channels that are active() in at least one block, ascending.  W empty: [(0, None)].
          3. Carried signs start at sign[c] = +1 for each c of W.
          4. Blocks in ascending order, A = the block's active().  Where len(A) >= 2 and the block has pair sums: r = the channel of
             A with the largest s2 (ties: the lowest index); raw[c] = -1 where c != r and corr(r, c) <= INVERTED_CORR, else +1
             (NaN: +1); g = the sum over A of raw[c] * sign[c]; all of raw is negated when g < 0, and when g == 0 and raw[min(A)]
             != sign[min(A)]; then sign[c] = raw[c] for c of A.  Any other block leaves the signs as they are.  The block decides
             None when W is every channel and all signs are +1, else Mix(((c, sign[c]) for c of W), divisor = len(W)).
          5. Adjacent equal decisions merge; run begins are block begins; fades come from resample.fade_halves.
        What follows: the divisor is constant over a file, so a leg that falls silent makes no boundary and no level jump; a
        channel dead throughout is dropped, as safe_mix() drops it; polarity is carried from block to block, so one inverted
        stretch never comes out as (L - R)/2 here and (R - L)/2 there.  Dual-mono material with one leg dead for a stretch comes
        out 6 dB low there: safe_schedule() gets that case right and the call-recording case wrong, and no rule that sums
        channels can have both.  No hysteresis on the correlation threshold, no change-point search inside a block."""
        runs = self.steady_runs()
        begins = [begin for begin, _, _ in runs]
        return R.Schedule(((begin, mix) for begin, _, mix in runs), R.fade_halves(begins, fade_sec, self.sr))

    def steady_runs(self):
        """[(begin frame, [block indices], mix or None)] per run of steady_schedule()."""
        if self.channels == 1:
            return [(0, list(range(len(self.blocks))), None)]
        active = [blk.active() for blk in self.blocks]
        keep = sorted(set(c for act in active for c in act))
        if not keep:
            return [(0, list(range(len(self.blocks))), None)]
        sign = {c: 1.0 for c in keep}
        out = []
        for b, (blk, act) in enumerate(zip(self.blocks, active)):
            if len(act) >= 2 and blk.s12 is not None:
                r = max(act, key=lambda c: (float(blk.s2[c]), -c))
                raw = {c: -1.0 if c != r and blk.corr(r, c) <= INVERTED_CORR else 1.0 for c in act}      # (NaN compares False)
                g = sum(raw[c] * sign[c] for c in act)
                if g < 0 or (g == 0 and raw[act[0]] != sign[act[0]]):
                    raw = {c: -v for c, v in raw.items()}
                sign.update(raw)
            plain = len(keep) == self.channels and all(v == 1.0 for v in sign.values())
            mix = None if plain else R.Mix(tuple((c, sign[c]) for c in keep), float(len(keep)))
            if out and out[-1][2] == mix:
                out[-1][1].append(b)
            else:
                out.append((b * self.block_frames, [b], mix))
        return out or [(0, [], None)]

    def __repr__(self):
        return f'SurveyTimeline({len(self.blocks)} blocks of {self.block_frames} frames, {self.whole!r})'


SCHEDULE_DECISION_COLUMNS = ('path', 'start', 'stop', 'blocks', 'plan', 'kept', 'flipped', 'downmix_loss_db')


def write_schedule_decisions_tsv(dst, names, decisions, failed=None):
    """The table `--channels auto --auto-block SEC --decisions` of scripts/ina_speech_segmenter_amd.py writes: one row per run of
    every file of `names`, in that order, under SCHEDULE_DECISION_COLUMNS.  decisions = [(path, timeline, schedule)] as
    batch_process(channels='auto', auto_block_sec=..., decisions=...) collects them.  start, stop: the run's first frame and
    the next run's (the file's end for the last) / sr, six decimals; blocks: how many blocks the run holds; plan, kept, flipped
    as write_decisions_tsv states them (`mono`: one row, no timeline); downmix_loss_db: the lowest of the run's blocks (empty
    where they have none).  A file in `failed` (path -> error text), or one without a decision, gets one row with plan `!` and
    the text in the last column.  A path listed more than once takes its decisions in their order."""
    _write_run_decisions(dst, names, decisions, failed, SurveyTimeline.runs)


def _write_run_decisions(dst, names, decisions, failed, runs_of):
    """The table of write_schedule_decisions_tsv, a timeline's runs being runs_of(timeline)."""
    by_name = {}
    for d in decisions:
        by_name.setdefault(d[0], []).append(d)
    failed = failed or {}
    with open(dst, 'w') as f:
        f.write('\t'.join(SCHEDULE_DECISION_COLUMNS) + '\n')
        for name in names:
            if name in failed or not by_name.get(name):
                text = str(failed.get(name, 'not processed')).replace('\t', ' ').replace('\n', ' ')
                f.write('\t'.join([name, '', '', '', '!', '', '', text]) + '\n')
                continue
            _, timeline, _ = by_name[name].pop(0)
            if timeline is None:
                f.write('\t'.join([name, '', '', '', 'mono', '0', '', '']) + '\n')
                continue
            runs, sr, n = runs_of(timeline), timeline.sr, timeline.n
            for k, (begin, blocks, mix) in enumerate(runs):
                stop = runs[k + 1][0] if k + 1 < len(runs) else n
                losses = [timeline.blocks[b].downmix_loss_db for b in blocks]
                losses = [v for v in losses if v is not None]
                terms = [(c, 1.0) for c in range(timeline.channels)] if mix is None else mix.terms
                f.write('\t'.join([name, f'{begin / sr:.6f}', f'{stop / sr:.6f}', str(len(blocks)), 'plain' if mix is None else 'mix',
                                   ','.join(str(c) for c, _ in terms), ','.join(str(c) for c, w in terms if w < 0),
                                   repr(min(losses)) if losses else '']) + '\n')


def write_steady_decisions_tsv(dst, names, decisions, failed=None):
    """write_schedule_decisions_tsv for `--auto-rule steady`: the same columns, one row per run of every file's
    steady_schedule(), downmix_loss_db the lowest of the run's blocks."""
    _write_run_decisions(dst, names, decisions, failed, SurveyTimeline.steady_runs)


TSV_COLUMNS = ('path', 'channel', 'frames', 'peak', 'rms_db', 'dc', 'zeros', 'fullscale', 'nonfinite', 'active')


def write_tsv(dst, names, surveys):
    """The table `--survey` of scripts/ina_speech_segmenter_amd.py writes: one row per file and channel under TSV_COLUMNS, then
    one row per file with channel `*` whose `rms_db` column carries downmix_loss_db and whose `active` column the inverted
    pairs ("0-1,2-3"; empty for none).  A file that could not be read (an entry of Segmenter.survey_files that is a text) gets
    one row: channel `!`, the text in the last column."""
    with open(dst, 'w') as f:
        f.write('\t'.join(TSV_COLUMNS) + '\n')
        for name, s in zip(names, surveys):
            if not isinstance(s, ChannelSurvey):
                f.write('\t'.join([name, '!'] + [''] * 7 + [str(s).replace('\t', ' ').replace('\n', ' ')]) + '\n')
                continue
            for c, n, peak, db, dc, zeros, full, nonf, act in s.rows():
                f.write('\t'.join([name, str(c), str(n), repr(peak), repr(db), repr(dc), str(zeros), str(full), str(nonf),
                                   '1' if act else '0']) + '\n')
            loss = s.downmix_loss_db
            f.write('\t'.join([name, '*', str(s.n), '', '' if loss is None else repr(loss), '', '', '', '',
                               ','.join(f'{c}-{d}' for c, d in s.inverted())]) + '\n')


DECISION_COLUMNS = ('path', 'plan', 'kept', 'flipped', 'downmix_loss_db')


def write_decisions_tsv(dst, names, decisions, failed=None):
    """The table `--channels auto --decisions` of scripts/ina_speech_segmenter_amd.py writes: one row per file of `names`, in
    that order, under DECISION_COLUMNS.  decisions = [(path, survey, mix)] as batch_process(channels='auto', decisions=...)
    collects them.  plan: `mono` (no survey: a one-channel file), `plain` (the mean of all channels, as ever) or `mix`; kept:
    the channels of the downmix, comma-joined (all of them for `plain`); flipped: those of them summed with weight -1;
    downmix_loss_db as the survey states it (empty where it has none).  A file in `failed` (path -> error text), or one without a
    decision, gets plan `!` and the text in the last column.  A path listed more than once takes its decisions in their order."""
    by_name = {}                                       # path -> its decisions in the order they came: a path may be listed twice
    for d in decisions:
        by_name.setdefault(d[0], []).append(d)
    failed = failed or {}
    with open(dst, 'w') as f:
        f.write('\t'.join(DECISION_COLUMNS) + '\n')
        for name in names:
            if name in failed or not by_name.get(name):
                text = str(failed.get(name, 'not processed')).replace('\t', ' ').replace('\n', ' ')
                f.write('\t'.join([name, '!', '', '', text]) + '\n')
                continue
            _, survey, mix = by_name[name].pop(0)
            if survey is None:
                f.write('\t'.join([name, 'mono', '0', '', '']) + '\n')
                continue
            loss = survey.downmix_loss_db
            terms = [(c, 1.0) for c in range(survey.channels)] if mix is None else mix.terms
            f.write('\t'.join([name, 'plain' if mix is None else 'mix', ','.join(str(c) for c, _ in terms),
                               ','.join(str(c) for c, w in terms if w < 0), '' if loss is None else repr(loss)]) + '\n')
