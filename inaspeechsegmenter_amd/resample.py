"""WAV input at any common rate without ffmpeg: filter design for the device resampler (csrc/resample.hip).

`Segmenter(ffmpeg=None, resample=True)` turns a WAV of rate `sr` and C channels into the 16 kHz mono PCM16 the front end
reads, in three steps that follow what `ffmpeg -ac 1 -ar 16000 -acodec pcm_s16le` is asked for (io.py:61-68):

  1. downmix     m = x.mean(axis=1) in float64, x converted with libsndfile's integer scaling (io._to_float)
  2. resample    y = scipy.signal.resample_poly(m, up, down) with its defaults: up/down = 16000/sr in lowest terms, a
                 Kaiser(5.0) windowed sinc of 2*hl+1 taps, hl = 10*max(up, down), cutoff 1/max(up, down), DC gain `up`;
                     y[i] = sum_j h[i*down + hl - j*up] * m[j]   over the taps in [0, 2*hl] and j in [0, n),
                 for i < ceil(n*up/down), summed in ascending j
  3. quantise    pcm = clip(rint(y * 32768), -32768, 32767).astype(int16)   (round half to even, then saturate)

`plan(sr)` is the host part the device needs (one table per rate, cached).  `resample_ref` is the float64 statement of the
three steps that the tests and tools/bench_resample.py compare the device with; the product never calls it.
"""
import functools
import math

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
