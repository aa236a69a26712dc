"""The x-vector path's ragged window widths on the CPU: every width the product runs (vbx.plan_windows), and the rule that
decides when a NaN x-vector is legitimate.

The reference pools the last ResNet stage as sqrt(mean(x^2) - mean(x)^2 + 1e-10) (resnet.py:123-125).  A last window of 10..16
frames leaves ceil(w / 8) = 2 stage-4 frames; where they agree to within float32 rounding, mean(x^2) - mean(x)^2 can come out
negative and the x-vector NaN, and vbx_segmenter.py:244 drops that window.  `ill_conditioned` is the rule the device tests
(test_gpu_vbx_widths.py) allow a NaN by: the float64 statistics hold an entry whose variance is at most 2^-20 of its mean square.
"""
import numpy as np
import pytest

from inaspeechsegmenter_amd import vbx as V, keras_model as KM
from oracle import vbx as ovbx
from conftest import synth_pcm

WIDTHS = range(10, V.WINLEN + 1)        # every last-window width: 10..120 (files of 34..144 frames), 121..144 (longer files)
VAR_RATIO = 2.0 ** -20                  # ill_conditioned: 16 x the largest ratio a float32 NaN was seen at (0.86 * 2^-24)


def ill_conditioned(pooled):
    """(B, 2n) float64 pooled statistics [mean | std] (oracle resnet101_forward(..., pooled=True)) -> (B,) bool: some entry has
    var = std^2 - 1e-10 <= 2^-20 * mean(x^2), where the reference formula loses all but ~20 bits of the variance."""
    pooled = np.asarray(pooled, np.float64)
    n = pooled.shape[1] // 2
    mean, std = pooled[:, :n], pooled[:, n:]
    var = std * std - 1e-10
    return (var <= VAR_RATIO * (var + mean * mean)).any(axis=1)


def oracle64(params, x_bft):
    """float64 oracle of a (B, 64, w) batch -> (x-vectors (B, 256), pooled statistics (B, 16384)), from one forward."""
    pooled = ovbx.resnet101_forward(params, x_bft, dtype=np.float64, pooled=True)
    emb = pooled @ np.asarray(params['embedding.weight'], np.float64).T + np.asarray(params['embedding.bias'], np.float64)
    return emb, pooled


def check_xvector(x, ref, pooled):
    """The acceptance rule for one x-vector `x` against its float64 oracle `ref` (and the oracle's pooled statistics) -> (ok, err):
    finite: max|x - ref| <= 1e-4 max|ref| (err = that ratio); NaN (and no inf): only where ill_conditioned (err = nan)."""
    x = np.asarray(x)
    if np.isfinite(x).all():
        err = float(np.abs(x.astype(np.float64) - ref).max() / np.abs(ref).max())
        return err <= 1e-4, err
    if np.isinf(x).any():
        return False, float('inf')
    return bool(ill_conditioned(np.asarray(pooled)[None])[0]), float('nan')


@pytest.mark.parametrize('w', list(WIDTHS))
def test_plan_windows_tail_widths(w):
    """A file of w + 24 frames has one last window, of width w at frame 24 (and from w = 121 on, a full window at 0 in front of
    it).  Files longer than 144 frames
    (w + 24 + 24 k) have full windows and a last window of 121..144 frames."""
    for k in (0, 1, 5, 37):
        T = w + 24 + 24 * k
        _, files, full, tails = V.plan_windows([T], [T / 100.0], ['f'])
        widths = [x for x, st in tails.items() for _ in st]
        assert len(widths) == 1 and [x for x, _ in ovbx.window_list(T)][-1] == T - widths[0], (T, tails)
        if k == 0:
            assert widths == [w] and list(tails[w]) == [24] and list(full) == ([0] if T > V.WINLEN else []), (T, tails, full)
            assert [key for key, _, _ in files[0]][-1] == f'f_{24:08}-{T:08}'

        elif T > V.WINLEN:
            assert 121 <= widths[0] <= 144 and full.size == len(ovbx.window_list(T)) - 1, (T, widths)
        else:
            assert widths == [T - 24] and full.size == 0, (T, widths)


def test_plan_windows_covers_every_width_once():
    frames = [w + 24 for w in WIDTHS] + [33, 20]
    _, files, full, tails = V.plan_windows(frames, [T / 100.0 for T in frames], [str(i) for i in range(len(frames))])
    assert full.size == 24 and sorted(tails) == list(WIDTHS) and all(len(st) == 1 for st in tails.values())
    assert files[-2:] == [[], []]                                   # under 34 frames: no window


def test_float32_nan_windows_are_ill_conditioned():
    """The NaN rule holds on the reference's own float32 arithmetic: at widths 10..16 (two stage-4 frames) the torch-f32 network
    pools some windows to NaN, and every one of them is ill_conditioned in float64.  A run without any NaN proves nothing."""
    import torch
    torch.set_num_threads(min(8, torch.get_num_threads()))
    params = KM.synthetic_resnet101(0)
    fea = ovbx.get_features(synth_pcm(11, 16000 * 30) / 32768.0)
    rng = np.random.default_rng(0)
    nan_total = flagged = n = 0
    for w in range(10, 17):
        starts = rng.choice(len(fea) - w, 15, replace=False)
        x = np.stack([fea[s:s + w].T for s in starts])
        e32 = ovbx.resnet101_forward(params, x)
        _, pooled = oracle64(params, x)
        nan = np.isnan(e32).any(axis=1)
        ill = ill_conditioned(pooled)
        assert np.isfinite(e32[~nan]).all(), w
        assert ill[nan].all(), (w, starts[nan & ~ill])
        nan_total += int(nan.sum())
        flagged += int(ill.sum())
        n += len(starts)
    print(f'{n} windows at widths 10..16: {nan_total} NaN in float32, {flagged} ill-conditioned in float64')
    assert n >= 100 and nan_total >= 1
