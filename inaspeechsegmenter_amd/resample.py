"""WAV input at any common rate without ffmpeg: filter design for the device resampler (csrc/resample.hip).

`Segmenter(ffmpeg=None, resample=True)` turns a WAV of rate `sr` and C channels into the 16 kHz mono PCM16 the front end
reads, in three steps that follow what `ffmpeg -ac 1 -ar 16000 -acodec pcm_s16le` is asked for (io.py:61-68):

  1. downmix     m = x.mean(axis=1) in float64, x converted with libsndfile's integer scaling (io._to_float)
  2. resample    y = scipy.signal.resample_poly(m, up, down) with its defaults: up/down = 16000/sr in lowest terms, a
                 Kaiser(5.0) windowed sinc of 2*hl+1 taps, hl = 10*max(up, down), cutoff 1/max(up, down), DC gain `up`;
                     y[i] = sum_j h[i*down + hl - j*up] * m[j]   over the taps in [0, 2*hl] and j in [0, n),
                 for i < ceil(n*up/down), summed in ascending j
  3. quantise    pcm = clip(rint(y * 32768), -32768, 32767).astype(int16)   (round half to even, then saturate)

Mixes (an extension: weighted sums of a file's channels, `Segmenter.load_pcm_mixes` and what follows it).  A MIX is K >= 1 terms
(c_k, w_k) and a divisor d: c_k a 0-based channel index (channels may repeat and come in any order), w_k a finite float64, d
finite and not zero.  It replaces step 1: for stored frame j, x[j, c] the stored sample scaled by io._to_float,

    m[j] = ( (w_0 * x[j, c_0]) + w_1 * x[j, c_1] + ... + w_{K-1} * x[j, c_{K-1}] ) / d

in float64, every product and every sum rounded on its own (no FMA), the terms taken in ascending k, the division always
performed, once, at the end (d = 1 is exact).  Steps 2 and 3 apply unchanged, at 16 kHz too (through the identity filter): a
mix whose sum leaves [-1, 1) saturates, as ffmpeg's pcm_s16le does, and the output is PCM16 whatever the stored format.
Two identities follow: K = 1, w = 1, d = 1 is the channel alone (1.0 * x and x / 1.0 are exact), and all C channels in order
with every w = 1 and d = C is the device's plain downmix, which sums the channels in order and divides by C.  numpy's
`mean(axis=1)` is NOT that sum for float64 rows of 8 or more channels (it adds pairwise); for samples of the integer formats
every partial sum is exact and the order cannot matter.  `mixdown` therefore states the loop and never calls `mean`.
`Mix` is the general form; `normalise_mixes` states the spellings a mix specification accepts, `parse_mixes` the command line's.

`plan(sr)` is the host part the device needs (one table per rate, cached).  `resample_ref` is the float64 statement of the
three steps that the tests and tools/bench_resample.py compare the device with; the product never calls it.
"""
import functools
import math
from typing import NamedTuple

import numpy as np

SR_OUT = 16000
MIN_RATE, MAX_RATE = 4000, 384000
KAISER_BETA = 5.0


def check_rate(sr):
    """The rates the device path takes: integers in [4 000, 384 000] Hz; ValueError (naming the rate) otherwise."""
    if isinstance(sr, (bool, np.bool_)) or not isinstance(sr, (int, np.integer)) or not MIN_RATE <= sr <= MAX_RATE:
        raise ValueError(f'sample rate {sr!r} Hz: the device resampler takes integer rates from {MIN_RATE} to {MAX_RATE} Hz')
    return int(sr)


@functools.lru_cache(maxsize=None)
def _plan(sr):
    g = math.gcd(sr, SR_OUT)
    up, down = SR_OUT // g, sr // g
    if up == down:                                   # 16 kHz, more than one channel: resample_poly returns its input (a copy)
        h = np.ones(1)
        h.setflags(write=False)
        return 1, 1, h
    mr = max(up, down)
    hl = 10 * mr
    ntaps = 2 * hl + 1
    cutoff = 1.0 / mr
    k = np.arange(ntaps) - hl                        # firwin: cutoff * sinc(cutoff * m), windowed, unit gain at DC
    h = cutoff * np.sinc(cutoff * k) * np.kaiser(ntaps, KAISER_BETA)
    h /= h.sum()
    h *= up
    h.setflags(write=False)
    return up, down, h


def plan(sr):
    """-> (up, down, h): h float64 of 2*10*max(up, down)+1 taps (read-only, cached per rate)."""
    return _plan(check_rate(sr))


def out_len(n, sr):
    """Output samples of an n-frame input: ceil(n * up / down)."""
    up, down, _ = plan(sr)
    return -(-int(n) * up // down)


def downmix(x):
    """Stored samples (n,) or (n, C) -> float64 mono: libsndfile's scaling, then the channel mean."""
    from .io import _to_float
    m = _to_float(np.asarray(x), np.float64)
    return m.mean(axis=1) if m.ndim == 2 else m


def input_span(sr, frames_total, out_begin, out_count):
    """-> (j_lo, j_hi): the first and last input frame that carry a tap of outputs [out_begin, out_begin + out_count) of a
    file of `frames_total` frames: j_lo = max(0, ceil((out_begin*down - hl)/up)), j_hi = min(frames_total - 1,
    floor(((out_begin + out_count - 1)*down + hl)/up)).  (floor at the low end, where a tile's staging starts, names one
    frame more whenever the division is not exact: that frame's tap would be 2*hl + something, outside the table.)"""
    up, down, h = plan(sr)
    hl = (h.size - 1) // 2
    return (max(0, -((hl - int(out_begin) * down) // up)),
            min(int(frames_total) - 1, ((int(out_begin) + int(out_count) - 1) * down + hl) // up))


def resample_float(m, sr, out_begin=0, out_count=None, in_begin=0, frames_total=None):
    """Step 2 on float64 mono samples, in the device's summation order (ascending input index).
    A window: outputs [out_begin, out_begin + out_count) of the file (default: all of them), from `m` = the file's frames
    [in_begin, in_begin + m.size) of `frames_total` (default: `m` ends the file).  A frame outside `m` counts as zero, as a
    frame outside the file does: the result is the whole-file result's slice when `m` holds input_span() of the window."""
    up, down, h = plan(sr)
    m = np.asarray(m, dtype=np.float64)
    n = int(in_begin) + m.size if frames_total is None else int(frames_total)
    nout = -(-n * up // down)
    if out_count is None:
        out_count = nout - int(out_begin)
    if out_begin < 0 or out_count < 0 or out_begin + out_count > nout:
        raise ValueError(f'outputs [{out_begin}, {out_begin + out_count}) outside the {nout} of {n} input frames')
    hl = (h.size - 1) // 2
    kmax = 2 * hl // up + 1                          # taps of the longest phase
    i = np.arange(int(out_begin), int(out_begin) + int(out_count), dtype=np.int64)
    j0 = -((hl - i * down) // up)                    # ceil((i*down - hl) / up): first input under the filter
    t0 = i * down + hl - j0 * up                     # its tap, in (2*hl - up, 2*hl]; the next input's is `up` lower
    mp = np.concatenate((np.zeros(1), m[:max(0, n - int(in_begin))]))     # mp[0] = 0 stands for the frames outside `m` / the file
    hp = np.concatenate((np.zeros(1), h))            # hp[0] = 0 stands for the taps below 0
    acc = np.zeros(i.size)
    for k in range(kmax):
        t = t0 - k * up
        j = j0 + k - int(in_begin)
        acc += hp[np.maximum(t, -1) + 1] * mp[np.where((j >= 0) & (j < mp.size - 1), j + 1, 0)]
    return acc


def quantise(y):
    return np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)


def resample_ref(x, sr, out_begin=0, out_count=None, in_begin=0, frames_total=None):
    """The three steps above on stored samples x ((n,) or (n, C), any io dtype) -> 16 kHz mono int16.  out_begin / out_count:
    only those outputs (the defaults give them all); in_begin / frames_total: x holds the file's frames from in_begin on
    (resample_float states the window)."""
    return quantise(resample_float(downmix(x), sr, out_begin, out_count, in_begin, frames_total))


# ---------------------------------------------------------------------------------------------- mixes: weighted sums of channels
class Mix(NamedTuple):
    """One mix: `terms` = ((channel, weight), ...) in the order they are summed, and the `divisor` of the sum."""
    terms: tuple
    divisor: float = 1.0


def _one_mix(k, m, channels, name):
    """Mix k of a specification -> a Mix with int channels and float weights, or ValueError naming it."""
    def bad(why):
        return ValueError(f'{name}: mix {k} ({m!r}): {why}')

    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))

    def is_num(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    if is_int(m):                                                       # a channel alone
        terms, divisor = [(m, 1.0)], 1.0
    elif isinstance(m, Mix):
        terms, divisor = m.terms, m.divisor
    elif isinstance(m, (str, bytes)):
        raise bad('a mix is a channel index, a sequence of them, (channel, weight) pairs, a mapping or a resample.Mix')
    elif hasattr(m, 'items'):                                           # channel -> weight: the weighted sum
        terms, divisor = list(m.items()), 1.0
    else:
        try:
            entries = list(m)
        except TypeError:
            raise bad('a mix is a channel index, a sequence of them, (channel, weight) pairs, a mapping or a resample.Mix') from None
        if entries and all(is_int(e) for e in entries):                 # channel indices: their mean, summed in the order given
            terms, divisor = [(e, 1.0) for e in entries], float(len(entries))
        else:                                                           # (channel, weight) pairs: the weighted sum
            terms, divisor = entries, 1.0
    out = []
    try:
        terms = [tuple(t) for t in terms]
    except TypeError:
        raise bad('its terms are (channel, weight) pairs') from None
    if not terms:
        raise bad('empty mix')
    for t in terms:
        if len(t) != 2 or not is_int(t[0]) or not is_num(t[1]):
            raise bad(f'term {t!r} is not a (channel, weight) pair')
        ch, w = int(t[0]), float(t[1])
        if ch < 0 or (channels is not None and ch >= channels):
            of = '' if channels is None else f" the file's {channels} channel{'s' if channels > 1 else ''} (0 .. {channels - 1})"
            raise bad(f'channel {ch} is outside{of}' if of else f'channel {ch} is negative')
        if not math.isfinite(w):
            raise bad(f'weight {w!r} of channel {ch} is not finite')
        out.append((ch, w))
    if not is_num(divisor) or not math.isfinite(divisor) or divisor == 0:
        raise bad(f'divisor {divisor!r} must be finite and not zero')
    return Mix(tuple(out), float(divisor))


def normalise_mixes(spec, channels=None, name='mixes'):
    """A mix specification -- a sequence of mixes -- as a list of `Mix`.  A mix is spelt
        an int c                                    that channel alone
        a sequence of ints                          their mean, summed in the order given (divisor = their count)
        a mapping channel -> weight, or a sequence of (channel, weight) pairs     the weighted sum (divisor 1)
        Mix(terms, divisor)                         the general form
    ValueError naming `name`, the mix and the reason: an empty specification or mix, a channel that is negative or (with
    `channels`, the file's channel count) outside the file, a weight that is not finite, a divisor that is zero or not finite."""
    if spec is None or isinstance(spec, (str, bytes, Mix)) or hasattr(spec, 'items'):
        raise ValueError(f'{name}: a mix specification is a sequence of mixes, not {spec!r}')
    try:
        spec = list(spec)
    except TypeError:
        raise ValueError(f'{name}: a mix specification is a sequence of mixes, not {spec!r}') from None
    if not spec:
        raise ValueError(f'{name}: empty mix specification')
    return [_one_mix(k, m, channels, name) for k, m in enumerate(spec)]


def parse_mixes(text):
    """The command line's spelling of a mix specification -> a list of `Mix`: mixes separated by commas, terms joined by `+`.
    A mix whose terms are all bare channel numbers ("0+1") is their mean; a mix with any `weight*channel` term
    ("0.7*4+0.7*5+2") is a weighted sum, in which a bare channel has weight 1 and nothing is divided."""
    spec = []
    for k, part in enumerate(str(text).split(',')):
        terms, weighted = [], False
        for t in part.split('+'):
            w, star, ch = t.partition('*')
            if not star:
                w, ch = '1', w
            weighted = weighted or bool(star)
            try:
                terms.append((int(ch.strip()), float(w.strip())))
            except ValueError:
                raise ValueError(f'--mixes: mix {k} ({part.strip()!r}): term {t.strip()!r} is not CHANNEL or WEIGHT*CHANNEL') from None
        spec.append(Mix(tuple(terms), 1.0 if weighted else float(len(terms))))
    return normalise_mixes(spec, None, '--mixes')


def mixdown(x, mix):
    """Stored samples (n,) or (n, C) -> float64 mono by the definition above: the explicit loop over the terms, vectorised over
    frames only (numpy rounds each elementwise product, sum and quotient on its own)."""
    from .io import _to_float
    m = _to_float(np.asarray(x), np.float64)
    if m.ndim == 1:
        m = m[:, None]
    (mix,) = normalise_mixes([mix], m.shape[1])
    (c0, w0), rest = mix.terms[0], mix.terms[1:]
    acc = w0 * m[:, c0]
    for ch, w in rest:
        acc = acc + w * m[:, ch]
    return acc / mix.divisor


def mix_ref(x, sr, mix, out_begin=0, out_count=None, in_begin=0, frames_total=None):
    """resample_ref with `mixdown(x, mix)` in place of the downmix -> 16 kHz mono int16 (windows as resample_ref states them)."""
    return quantise(resample_float(mixdown(x, mix), sr, out_begin, out_count, in_begin, frames_total))


# ---------------------------------------------------------------------------------------------- schedules: a mix per stretch of a file
class Schedule:
    """A downmix that changes over time (include/iss.h, "Schedules"): `runs` = ((begin, mix), ...), begin in stored frames at
    the file's own rate -- runs[0] begins at 0, the begins ascend strictly --, mix a `Mix` or None (the plain downmix of all
    channels).  Run r governs the frames [begin_r, begin_{r+1}), the last run to the end; a run at or past the end of the file
    governs nothing.  `fades` (include/iss.h, "Fades"): one half-width h_r >= 0 per run in stored frames, None for all 0; run
    r >= 1 fades in linearly over [begin_r - h_r, begin_r + h_r), h_0 = 0 and the zones disjoint and in order.  Equal to another
    when runs and fades are equal, to a list of (begin, mix) pairs when the runs are equal and every fade is 0."""
    __slots__ = ('runs', 'fades')

    def __init__(self, runs, fades=None):
        runs = tuple((int(b), m) for b, m in runs)
        if not runs or runs[0][0] != 0:
            raise ValueError(f'schedule: run 0 begins at frame {runs[0][0] if runs else None!r}, not 0')
        for r in range(1, len(runs)):
            if runs[r][0] <= runs[r - 1][0]:
                raise ValueError(f'schedule: run {r} begins at frame {runs[r][0]}, run {r - 1} at {runs[r - 1][0]}: begins ascend strictly')
        for r, (_, m) in enumerate(runs):
            if m is not None and not isinstance(m, Mix):
                raise ValueError(f'schedule: run {r}: its mix is a resample.Mix or None, not {m!r}')
        self.runs = runs
        self.fades = _check_fades(runs, fades)

    @property
    def faded(self):
        return any(self.fades)

    def __eq__(self, other):
        if isinstance(other, Schedule):
            return self.runs == other.runs and self.fades == other.fades
        if isinstance(other, (list, tuple)):
            return list(self.runs) == [tuple(r) for r in other] and not self.faded
        return NotImplemented

    __hash__ = None

    def __len__(self):
        return len(self.runs)

    def __iter__(self):
        return iter(self.runs)

    def __repr__(self):
        if self.faded:
            return f'Schedule({list(self.runs)!r}, fades={list(self.fades)!r})'
        return f'Schedule({list(self.runs)!r})'


def _check_fades(runs, fades):
    """The half-widths of a schedule's runs as a tuple of ints, validated as include/iss.h's "Fades" states."""
    if fades is None:
        return (0,) * len(runs)
    try:
        fades = tuple(fades)
    except TypeError:
        raise ValueError(f'schedule: fades are one half-width per run, not {fades!r}') from None
    if len(fades) != len(runs):
        raise ValueError(f'schedule: {len(fades)} fades for {len(runs)} runs: one half-width per run')
    for r, h in enumerate(fades):
        if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, np.integer)):
            raise ValueError(f'schedule: run {r}: its fade is a whole number of frames, not {h!r}')
        if h < 0:
            raise ValueError(f'schedule: run {r}: fade half-width {int(h)} is negative')
    fades = tuple(int(h) for h in fades)
    if fades[0] != 0:
        raise ValueError(f'schedule: run 0: fade half-width {fades[0]}: the first run has nothing to fade from')
    for r in range(1, len(runs)):
        if runs[r - 1][0] + fades[r - 1] > runs[r][0] - fades[r]:
            raise ValueError(f'schedule: run {r}: its fade zone [{runs[r][0] - fades[r]}, {runs[r][0] + fades[r]}) overlaps that of '
                             f'run {r - 1}, which ends at {runs[r - 1][0] + fades[r - 1]}')
    return fades


def fade_halves(begins, fade_sec, sr):
    """Half-widths for runs that begin at `begins` (stored frames) and cross-fade over `fade_sec` seconds at `sr` Hz: h =
    floor(fade_sec * sr / 2 + 0.5), and h_r = min(h, (begin_r - begin_{r-1}) // 2, (begin_{r+1} - begin_r) // 2) with no upper
    term for the last run, h_0 = 0: every run gives at most half its length to each side, so the zones are disjoint by
    construction.  ValueError: a fade that is negative or not finite."""
    if isinstance(fade_sec, (bool, np.bool_)) or not isinstance(fade_sec, (int, float, np.integer, np.floating)) or \
            not math.isfinite(fade_sec) or fade_sec < 0:
        raise ValueError(f'fade_sec: {fade_sec!r} s is negative, not finite or not a number')
    begins = [int(b) for b in begins]
    h = math.floor(float(fade_sec) * sr / 2 + 0.5)
    out = [0] * len(begins)
    for r in range(1, len(begins)):
        hr = min(h, (begins[r] - begins[r - 1]) // 2)
        if r + 1 < len(begins):
            hr = min(hr, (begins[r + 1] - begins[r]) // 2)
        out[r] = hr
    return out


def normalise_schedule(spec, sr, channels=None, name='schedule', fade_sec=0.0):
    """A schedule specification [(start_sec, mix), ...] for a file at `sr` Hz -> a `Schedule`: begin = floor(start_sec * sr +
    0.5), the rounding of segment_excerpts; a mix spelt as normalise_mixes states, or None.  A `Schedule` (begins in frames
    already) has its mixes checked against `channels` and is handed on.  fade_sec > 0: the result cross-fades at every run
    boundary over `fade_halves(begins, fade_sec, sr)`; a `Schedule` that carries fades of its own is then refused, one without
    gets them.  ValueError naming `name`, the run and the reason: an
    empty specification, a first start that is not 0, two starts that round to one frame, descending starts, a start that is
    negative or not finite, a channel outside the file's `channels`, and what normalise_mixes refuses of a mix."""
    def is_num(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    if isinstance(spec, Schedule):
        for r, (_, m) in enumerate(spec.runs):
            if m is not None:
                _one_mix(0, m, channels, f'{name}: run {r}')
        if fade_sec:
            if spec.faded:
                raise ValueError(f'{name}: fade_sec={fade_sec!r} passed with a Schedule that carries fades of its own')
            if sr is None:
                raise ValueError(f'{name}: fade_sec={fade_sec!r} needs the rate of the file')
            return Schedule(spec.runs, fade_halves([b for b, _ in spec.runs], fade_sec, sr))
        return spec
    if spec is None or isinstance(spec, (str, bytes, Mix)) or hasattr(spec, 'items'):
        raise ValueError(f'{name}: a schedule is a sequence of (start_sec, mix) runs, not {spec!r}')
    try:
        spec = [tuple(run) for run in spec]
    except TypeError:
        raise ValueError(f'{name}: a schedule is a sequence of (start_sec, mix) runs, not {spec!r}') from None
    if not spec:
        raise ValueError(f'{name}: empty schedule')
    runs = []
    for r, run in enumerate(spec):
        if len(run) != 2 or not is_num(run[0]):
            raise ValueError(f'{name}: run {r} ({run!r}) is not a (start_sec, mix) pair')
        start, m = float(run[0]), run[1]
        if not math.isfinite(start) or start < 0:
            raise ValueError(f'{name}: run {r}: start {start!r} s is negative or not finite')
        begin = math.floor(start * sr + 0.5)
        if r == 0 and begin != 0:
            raise ValueError(f'{name}: run 0 starts at {start!r} s (frame {begin}): the first run starts at 0')
        if r > 0 and begin == runs[-1][0]:
            raise ValueError(f'{name}: run {r}: starts {spec[r - 1][0]!r} s and {start!r} s round to one frame ({begin}) at {sr} Hz')
        if r > 0 and begin < runs[-1][0]:
            raise ValueError(f'{name}: run {r}: start {start!r} s lies before run {r - 1} ({spec[r - 1][0]!r} s): starts ascend')
        runs.append((begin, None if m is None else _one_mix(0, m, channels, f'{name}: run {r}')))
    return Schedule(runs, fade_halves([b for b, _ in runs], fade_sec, sr) if fade_sec else None)


def schedule_mixdown(x, schedule):
    """Stored samples (n,) or (n, C) -> the scheduled float64 mono signal: frame j mixed by `mixdown` with the mix of the run
    that governs it, None being the mix of all C channels in order with w = 1, d = C (the plain downmix, to the bit).  A
    schedule with fades (include/iss.h, "Fades"): frame j of run r's zone [begin_r - h_r, begin_r + h_r), k = j - (begin_r -
    h_r), is p + a * (q - p) with p and q the frame mixed by the runs r - 1 and r and a = (2k + 1) / (4 h_r) -- one division of
    two exact integers; the difference, the product and the sum rounded on their own, as numpy rounds them."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    schedule = normalise_schedule(schedule if isinstance(schedule, Schedule) else Schedule(schedule), None, ch)
    plain = Mix(tuple((c, 1.0) for c in range(ch)), float(ch))
    out = np.zeros(n)
    begins = [b for b, _ in schedule.runs] + [n]
    for r, (_, m) in enumerate(schedule.runs):
        a, b = min(begins[r], n), min(begins[r + 1], n)
        if b > a:
            out[a:b] = mixdown(x[a:b], plain if m is None else m)
    for r, h in enumerate(schedule.fades):
        a, b = max(schedule.runs[r][0] - h, 0), min(schedule.runs[r][0] + h, n)
        if h == 0 or b <= a:
            continue
        (_, m0), (_, m1) = schedule.runs[r - 1], schedule.runs[r]
        p = mixdown(x[a:b], plain if m0 is None else m0)
        q = mixdown(x[a:b], plain if m1 is None else m1)
        k = np.arange(a, b, dtype=np.int64) - (schedule.runs[r][0] - h)
        alpha = (2 * k + 1).astype(np.float64) / np.float64(4 * h)
        out[a:b] = p + alpha * (q - p)
    return out


def schedule_ref(x, sr, schedule):
    """The numpy statement of include/iss.h's "Schedules" and "Fades": resample_ref with `schedule_mixdown(x, schedule)` in
    place of the downmix -> 16 kHz mono int16.  The taps of outputs near a run boundary see samples of both runs: that is the
    definition."""
    return quantise(resample_float(schedule_mixdown(x, schedule), sr))


# ---------------------------------------------------------------------------------------------- channel survey: the reference
SURVEY_CHUNK, SURVEY_LANES, SURVEY_PAIR_CHANNELS = 1024, 256, 16      # include/iss.h: ISS_SURVEY_CHUNK, four waves of 64, ISS_SURVEY_PAIR_CHANNELS


class SurveyFields(NamedTuple):
    """What a survey measures of stored frames [a, b) (include/iss.h, "Channel survey"): per channel peak, s1, s2 (float64) and
    zeros, fullscale, nonfinite (int64), and s12 = the sums of products of the pairs (0,1), (0,2), ..., (1,2), ... in that order
    (float64; None for more than SURVEY_PAIR_CHANNELS channels)."""
    n: int
    peak: np.ndarray
    zeros: np.ndarray
    fullscale: np.ndarray
    nonfinite: np.ndarray
    s1: np.ndarray
    s2: np.ndarray
    s12: object


# the largest positive value each stored format holds, as the float64 the readers give it (`full` of a job row)
SURVEY_FULL = {'u8': 127 / 128, 'i8': 127 / 128, 'i16': 32767 / 32768, 'i24': (2 ** 31 - 256) / 2 ** 31, 'i32': (2 ** 31 - 1) / 2 ** 31,
               'ulaw': 32124 / 32768, 'alaw': 32256 / 32768, 'f32': 1.0, 'f64': 1.0, 'ima': 32767 / 32768, 'ms': 32767 / 32768}


def _survey_chunk_sums(terms):
    """The chunk sums of the rows of `terms` (n, Q), n a multiple of SURVEY_CHUNK but for the last chunk -> (chunks, Q)."""
    n, nq = terms.shape
    per = SURVEY_CHUNK // SURVEY_LANES
    m = -(-n // SURVEY_CHUNK)
    if n != m * SURVEY_CHUNK:
        pad = np.zeros((m * SURVEY_CHUNK, nq))
        pad[:n] = terms
        terms = pad
    rows = terms.reshape(m, per, SURVEY_LANES // 64, 64, nq)
    acc = np.zeros((m, SURVEY_LANES // 64, 64, nq))
    for r in range(per):
        acc = acc + rows[:, r]
    s = 32
    while s:
        acc = acc[:, :, :s] + acc[:, :, s:2 * s]
        s //= 2
    w = acc[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


_SURVEY_BLOCK = 256 * SURVEY_CHUNK                   # rows handled at a time: bounds the memory, not the order


def survey_sum(terms):
    """The sums of the columns of `terms` (n, Q) float64 in the SURVEY ORDER, the one order the device and the host twin share:
    the rows in chunks of SURVEY_CHUNK; within a chunk lane t of 256 starts from +0.0 and adds rows t, t + 256, t + 512, t + 768
    (a missing row adds nothing: +0.0 here, which changes no partial sum, as none is ever -0.0); each wave's 64 lanes by the
    tree `lane l += lane l + s`, s = 32 .. 1; the chunk's sum ((wave 0 + wave 1) + wave 2) + wave 3; the chunk sums added in
    ascending order from +0.0.  Every addition is numpy's float64 addition of two arrays: rounded on its own."""
    terms = np.asarray(terms, dtype=np.float64)
    total = np.zeros(terms.shape[1])
    for r0 in range(0, terms.shape[0], _SURVEY_BLOCK):
        for chunk in _survey_chunk_sums(terms[r0:r0 + _SURVEY_BLOCK]):
            total = total + chunk
    return total


def survey_pairs(ch):
    """The pairs c < d in the order s12 lists them."""
    return [(c, d) for c in range(ch) for d in range(c + 1, ch)]


def survey_ref(x, full, a=0, b=None):
    """The survey of frames [a, b) of stored samples x ((n,) or (n, C), any io dtype; b None: to the end) against the fullscale
    threshold `full` -> SurveyFields.  The numpy statement of include/iss.h's definition: samples scaled by io._to_float, a
    non-finite sample counted and taken as 0.0 everywhere else, peak and counts exact, the three sums by `survey_sum`."""
    from .io import _to_float
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    b = x.shape[0] if b is None else min(int(b), x.shape[0])
    a = int(a)
    if a < 0 or a > b:
        raise ValueError(f'frames [{a}, {b}) of {x.shape[0]}')
    n, ch = b - a, x.shape[1]
    pairs = survey_pairs(ch) if ch <= SURVEY_PAIR_CHANNELS else None
    pc, pd = ([c for c, _ in pairs], [d for _, d in pairs]) if pairs else ([], [])
    peak, sums = np.zeros(ch), np.zeros(2 * ch + len(pc))
    zeros, fullscale, nonfinite = (np.zeros(ch, dtype=np.int64) for _ in range(3))
    for r0 in range(a, b, _SURVEY_BLOCK):                        # blocks of whole chunks counted from a
        v = _to_float(x[r0:min(b, r0 + _SURVEY_BLOCK)], np.float64)
        bad = ~np.isfinite(v)
        if bad.any():
            v = np.where(bad, 0.0, v)
        mag = np.abs(v)
        peak = np.maximum(peak, mag.max(axis=0))
        zeros += (v == 0.0).sum(axis=0)
        fullscale += (mag >= float(full)).sum(axis=0)
        nonfinite += bad.sum(axis=0)
        for chunk in _survey_chunk_sums(np.concatenate([v, v * v] + ([v[:, pc] * v[:, pd]] if pc else []), axis=1)):
            sums = sums + chunk
    return SurveyFields(n, peak, zeros, fullscale, nonfinite, sums[:ch], sums[ch:2 * ch], None if pairs is None else sums[2 * ch:])
