"""The inputs of the channels='auto' tests (test_auto.py, test_gpu_auto.py): 2 s files of gated noise whose channels are what a
survey-guided downmix exists for.  L and N are independent noises behind the same gate, R = 0.7 L + 0.3 N (corr 0.92 with L):

    inverted    [L, -L]                       the plain downmix is digital silence
    healthy     [L, R]                        nothing to mend
    dead4       [L, 0, R, noise at -93 dB]    one track at digital zero, one under the floor of survey.ACTIVE_FLOOR_DB
    deadinv     [0, L, -R]                    a dead track and an inverted pair
    independent [L, N]
    silent      [0, 0]
    twins       [-L, L, L]                    a tie in s2: the reference is the lowest index (any other turns every sign over)
    wide17      17 channels, two of them dead, no pair sums

`stored(case, sr)` -> the (n, ch) int16 array every writer below starts from, so that a case holds the same samples whatever
the container (the lossy coders then code those)."""
import numpy as np

import flacgen
import msadpcmgen
import sndgen
import wavgen

SECONDS = 2.0
RATES = (8000, 16000, 44100, 48000)


def _noises(n, sr, seed):
    rng = np.random.default_rng(seed)
    gate = ((np.arange(n) // int(0.25 * sr)) % 2 == 0).astype(np.float64)      # 0.25 s on, 0.25 s off
    left, other = (rng.uniform(-0.5, 0.5, n) * gate for _ in range(2))
    return left, other, 0.7 * left + 0.3 * other


def stored(case, sr, seed=5, n=None):
    n = int(SECONDS * sr) if n is None else n
    left, other, right = _noises(n, sr, seed)
    zero = np.zeros(n)
    cols = {'inverted': [left, -left], 'healthy': [left, right], 'dead4': [left, zero, right, zero], 'deadinv': [zero, left, -right],
            'independent': [left, other], 'silent': [zero, zero], 'twins': [-left, left, left], 'mono': [left],
            'wide17': [left * (0.5 + 0.03 * c) if c not in (3, 11) else zero for c in range(17)]}[case]
    x = wavgen.encode(np.stack(cols, axis=1), 'i16')
    if case == 'inverted':
        x[:, 1] = -x[:, 0]                                       # (exactly: no sample of L is -32768)
    if case == 'twins':
        x[:, 1], x[:, 2] = -x[:, 0], -x[:, 0]
    if case == 'dead4':                                          # -93 dB: one step, on 53.8 % of the samples
        rng = np.random.default_rng(seed + 1)
        x[:, 3] = (rng.random(n) < (32768 * 10 ** (-93 / 20)) ** 2) * rng.choice(np.array([-1, 1], dtype=np.int16), n)
    return x[:, 0] if case == 'mono' else x


def write(path, case, sr, kind='i16', seed=5, n=None):
    """One case as a file of `kind`: i16 / f32 (WAV), flac (16-bit, left/side for two channels), ima, ms -> its path."""
    x = stored(case, sr, seed, n)
    if kind == 'i16':
        return wavgen.write_wav(path, x, sr, 'i16')
    if kind == 'f32':
        return wavgen.write_wav(path, (x.astype(np.float64) / 32768.0).astype('<f4'), sr, 'f32')
    if kind == 'flac':
        kw = {'channel_mode': 'left_side'} if x.ndim == 2 and x.shape[1] == 2 else {}
        # (noise: the encoder's own choice looks for a Rice parameter its 16-bit table does not hold)
        spec = lambda f, c: {'type': 'fixed', 'order': 1} if f % 2 else {'type': 'verbatim'}      # noqa: E731
        return flacgen.write(path, x.astype(np.int64), sr, 16, blocksize=1152, subframe=spec, **kw)
    if kind == 'ima':
        return sndgen.write(path, 'wav', 'ima', False, x.astype(np.float64) / 32768.0, sr)[0]
    assert kind == 'ms', kind
    ch = 1 if x.ndim == 1 else x.shape[1]
    align = 7 * ch + 121 * ch                                    # 244 samples per block, whatever the channel count
    return msadpcmgen.write_riff(path, msadpcmgen.fmt(sr, ch, align), msadpcmgen.encode(x, align), fact=len(x)) or str(path)
