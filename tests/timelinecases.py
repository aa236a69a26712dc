"""The fault fixture of the timeline tests (CPU and GPU): stereo PCM16 at 8 kHz, three and a half blocks of K = 8 chunks (8 192
frames, 1.024 s) of seeded noise at amplitude 0.1.  Block 0 has R = L, block 1 has R = -L, block 2 and the half block have R = 0:
over the whole file corr(L, R) is 0 and nothing is done; block by block the inverted second is turned back and the dead leg
dropped.  The plain downmix of block 1 is digital silence."""
import numpy as np

import flacgen
import sndgen
import wavgen
from inaspeechsegmenter_amd.resample import Mix

SR, BLOCK_SEC, K = 8000, 1.0, 8
B = K * 1024
N = 3 * B + B // 2
SCHEDULE = [(0, None), (B, Mix(((0, 1.0), (1, -1.0)), 2.0)), (2 * B, Mix(((0, 1.0),), 1.0))]


def stored(seed=11):
    """-> (N, 2) int16."""
    rng = np.random.default_rng(seed)
    left = wavgen.encode(rng.uniform(-0.1, 0.1, N), 'i16')
    right = left.copy()
    right[B:2 * B] = -left[B:2 * B]
    right[2 * B:] = 0
    return np.stack([left, right], axis=1)


def healthy(seed=12):
    """A file of the same shape with nothing wrong: R = 0.7 L + 0.3 noise."""
    rng = np.random.default_rng(seed)
    left, other = rng.uniform(-0.1, 0.1, N), rng.uniform(-0.1, 0.1, N)
    return wavgen.encode(np.stack([left, 0.7 * left + 0.3 * other], axis=1), 'i16')


def write(path, kind='i16', x=None):
    """The fixture (or `x`) as a file of `kind`: i16 (WAV), flac (16-bit, left/side), ima -> its path."""
    x = stored() if x is None else x
    if kind == 'i16':
        return wavgen.write_wav(path, x, SR, 'i16')
    if kind == 'flac':
        spec = lambda f, c: {'type': 'fixed', 'order': 1} if f % 2 else {'type': 'verbatim'}      # noqa: E731
        return flacgen.write(path, x.astype(np.int64), SR, 16, blocksize=1152, subframe=spec, channel_mode='left_side')
    assert kind == 'ima'
    return sndgen.write(path, 'wav', 'ima', False, x.astype(np.float64) / 32768.0, SR, block_align=256)[0]
