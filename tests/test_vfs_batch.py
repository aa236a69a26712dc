"""Batch voice-femininity scoring, host side: the window planner (vbx.plan_windows) against the reference's window loop, the
mid-speech pre-filter against apply_vad, and the command line."""
import os

import numpy as np
import pytest

from inaspeechsegmenter_amd import vbx as V, vfs
from oracle import vbx as ovbx


def _frame_counts():
    """40 seeded counts: 0-window files (< 34 frames), 1-window files (34..144 frames: one tail of width 10..120), every tail
    width 121..144 of the longer files, 24-window files (673..696 frames), and a few long ones."""
    rng = np.random.default_rng(40)
    counts = [0, 1, 20, 33, 34, 35, 100, 143, 144, 145, 168, 169, 673, 696]
    widths = set()
    while len(counts) < 40:
        T = int(rng.integers(145, 20000))
        w = T - ovbx.window_list(T)[-1][0]
        if w not in widths or len(counts) >= 38:
            widths.add(w)
            counts.append(T)
    return counts


class _CallOnly(V.VBxExtractor):
    """VBxExtractor.__call__ with a zero embedding per window: its keys, times and window order without a device."""

    def __init__(self):
        super().__init__(ctx=None, params=None)
        self.calls = []

    def get_embeddings(self, fea, starts, frames):
        self.calls.append((list(starts), frames))
        return np.zeros((len(starts), V.EMBED_DIM), np.float32)


def _plan_inputs():
    counts = _frame_counts()
    rng = np.random.default_rng(41)
    durations = [T / 100.0 + float(rng.uniform(0, 0.0159)) for T in counts]
    names = [f'f{i:02d}' for i in range(len(counts))]
    return counts, durations, names


def test_planner_matches_reference_window_loop():
    counts, durations, names = _plan_inputs()
    widths = {T - ovbx.window_list(T)[-1][0] for T in counts if ovbx.window_list(T)}
    assert set(range(121, 145)) <= widths and {10, 11, 76, 120} <= widths
    assert {len(ovbx.window_list(T)) for T in counts} >= {0, 1, 24}
    frame_off, files, full, tails = V.plan_windows(counts, durations, names)
    assert list(frame_off) == [0] + list(np.cumsum(counts))
    ref = _CallOnly()
    for f, (T, dur, name) in enumerate(zip(counts, durations, names)):
        base = frame_off[f]
        wins = []
        for key, times, slot in files[f]:
            if isinstance(slot, tuple):
                start, stop = tails[slot[0]][slot[1]] - base, tails[slot[0]][slot[1]] - base + slot[0]
            else:
                start, stop = full[slot] - base, full[slot] - base + V.WINLEN
            assert 0 <= start < stop <= T                                     # inside its own file
            wins.append((start, stop))
        assert wins == ovbx.window_list(T), f
        got = ref(name, np.zeros((T, 64), np.float32), dur)
        assert [(k, t) for k, t, _ in got] == [(k, t) for k, t, _ in files[f]], f


def test_tail_groups_cover_each_tail_once():
    counts, durations, names = _plan_inputs()
    frame_off, files, full, tails = V.plan_windows(counts, durations, names)
    used = [slot for wins in files for _, _, slot in wins if isinstance(slot, tuple)]
    assert len(used) == len(set(used)) == sum(len(st) for st in tails.values())
    assert set(used) == {(w, j) for w, st in tails.items() for j in range(len(st))}
    assert sorted(int(i) for wins in files for _, _, i in wins if not isinstance(i, tuple)) == list(range(len(full)))
    for f, T in enumerate(counts):                   # a file with windows has one tail (its last window, of its own width)
        mine = [slot for _, _, slot in files[f] if isinstance(slot, tuple)]
        if ovbx.window_list(T):
            a, b = ovbx.window_list(T)[-1]
            assert mine == [(b - a, mine[0][1])] and tails[b - a][mine[0][1]] == frame_off[f] + a and files[f][-1][2] == mine[0]
        else:
            assert mine == []
    assert full.dtype == np.int32 and all(st.dtype == np.int32 for st in tails.values())


def _random_speech(rng, duration):
    out, t = [], float(rng.uniform(0, 2))
    while t < duration:
        d = float(rng.choice([rng.uniform(0.05, 0.8), rng.uniform(0.8, 6.0)]))
        out.append((round(t, 2), round(min(duration, t + d), 2)))
        t += d + float(rng.choice([0.0, rng.uniform(0.02, 0.5), rng.uniform(0.5, 3)]))
    return vfs.speech_intervals([('speech', s, e) for s, e in out])


@pytest.mark.parametrize('thresh', [0.7, 0.62])
def test_mid_speech_filter_keeps_what_apply_vad_can_return(thresh):
    counts, durations, names = _plan_inputs()
    rng = np.random.default_rng(42)
    speeches = [_random_speech(rng, d) for d in durations]
    _, files, _, _ = V.plan_windows(counts, durations, names)
    _, kept, _, _ = V.plan_windows(counts, durations, names, keep=lambda f, t: vfs.is_mid_speech(t[0], t[1], speeches[f]))
    nonempty = 0
    for f in range(len(counts)):
        mid = [(k, t) for k, t, _ in files[f] if vfs.is_mid_speech(t[0], t[1], speeches[f])]
        assert [(k, t) for k, t, _ in kept[f]] == mid
        allx = [(k, t, np.full(4, i, np.float32)) for i, (k, t, _) in enumerate(files[f])]
        ids = {k: i for i, (k, _, _) in enumerate(files[f])}
        subx = [(k, t, np.full(4, ids[k], np.float32)) for k, t, _ in kept[f]]
        a = vfs.apply_vad(list(allx), speeches[f], thresh)
        b = vfs.apply_vad(list(subx), speeches[f], thresh)
        assert [(k, t, x[0]) for k, t, x in a] == [(k, t, x[0]) for k, t, x in b], f
        nonempty += bool(a)
    assert nonempty >= 10


def test_frame_count_and_pcm16_of():
    for n in (200, 201, 359, 360, 48037):
        assert V.frame_count(n) == len(ovbx.get_features(np.zeros(n)))
    pcm = np.array([-32768, -1, 0, 1, 32767], np.int16)
    assert V.pcm16_of(pcm) is pcm
    assert np.array_equal(V.pcm16_of(pcm / 32768.0), pcm)
    assert np.array_equal(V.pcm16_of((pcm / 32768.0).astype(np.float32)), pcm)
    assert V.pcm16_of(np.array([1.5])) is None


def test_cli_arguments(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location('ina_vfs_cli', os.path.join(os.path.dirname(__file__), '..', 'scripts',
                                                                             'ina_voice_femininity_amd.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    for name in ('b.wav', 'a.wav', 'c.mp3'):
        (tmp_path / name).write_bytes(b'')
    a = cli.build_parser().parse_args(['-i', str(tmp_path / '*.wav'), 'missing.wav', '-o', 'out.tsv', '-c', 'vfp', '-b', 'None',
                                       '--models', 'synthetic'])
    assert (a.output, a.criteria, a.ffmpeg_binary, a.models, a.batch_seconds) == ('out.tsv', 'vfp', 'None', 'synthetic', 3600)
    assert cli.expand_inputs(a.input) == [str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav'), 'missing.wav']
    d = cli.build_parser().parse_args(['-i', 'x.wav', '-o', 'o.tsv'])
    assert (d.criteria, d.ffmpeg_binary, d.models) == ('bgc', 'ffmpeg', None)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['-i', 'x.wav', '-o', 'o.tsv', '-c', 'xyz'])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['-o', 'o.tsv'])
