"""Batch voice-femininity scoring on the device: the ragged front end (iss_vbx_features_batch_pcm16) against the single-file
entry and the oracle, programs on shared parameters (iss_cnn_load_shared) against full loads, and
VoiceFemininityScoring.batch_process against __call__ file by file."""
import os
import wave

import numpy as np
import pytest

from inaspeechsegmenter_amd import _native, vbx as V, vfs, keras_model as KM
from oracle import vbx as ovbx
from conftest import GOLDEN, synth_pcm

pytestmark = pytest.mark.gpu
FEA_TOL = 2e-5                     # tests/test_gpu_vbx.py


def _fresh_context():
    from inaspeechsegmenter_amd import tables
    c = _native.Context(0)
    c.vbx_tables(tables.vbx_window(), tables.vbx_melbank())
    return c


# 200 samples (1 frame), < 300 frames (the global-mean CMN branch), 1 frame past the cumsum's 2 x 32-row and 4 x 32-row
# blocks, test_features_ragged_lengths_vs_oracle's lengths, a 5 000-frame file
BATCH_LENGTHS = [200, 40000, 160 * 64 + 80, 160 * 128 + 80, 1000, 16000, 48000 + 37, 160 * 301, 160 * 4999 + 80 + 37]


def test_batch_front_end_equals_single_file_entry(ctx):
    rng = np.random.default_rng(9)
    pcms = [np.clip(np.round(rng.normal(0, 0.1, n) * 32768), -32768, 32767).astype(np.int16) for n in BATCH_LENGTHS]
    fe = V.FeatureExtractor(ctx)
    fe._ensure_dither(max(BATCH_LENGTHS))
    singles = [ctx.vbx_features_pcm16(p) for p in pcms]
    foff, arena = ctx.vbx_features_batch_pcm16(pcms)
    assert list(np.diff(foff)) == [V.frame_count(n) for n in BATCH_LENGTHS] and foff[0] == 0
    assert arena.shape == (foff[-1], 64)
    for f, (p, one) in enumerate(zip(pcms, singles)):
        got = arena[foff[f]:foff[f + 1]]
        assert np.array_equal(got, one), (f, len(p), np.abs(got - one).max())
        ref = ovbx.get_features(p / 32768.0)
        assert np.abs(got - ref).max() <= FEA_TOL, f
    # resident: the arena is what iss_vbx_embed gathers from (c->vbx_T = sum T_f)
    foff2, none = ctx.vbx_features_batch_pcm16(pcms, to_host=False)
    assert none is None and np.array_equal(foff2, foff)


def test_batch_front_end_rejects_bad_input(ctx):
    fe = V.FeatureExtractor(ctx)
    fe._ensure_dither(1000)
    with pytest.raises(_native.NativeError, match='file 1 has 199 samples'):
        ctx.vbx_features_batch_pcm16([np.zeros(400, np.int16), np.zeros(199, np.int16)])
    with pytest.raises(_native.NativeError, match='dither'):
        ctx.vbx_features_batch_pcm16([np.zeros(400, np.int16), np.zeros(ctx._dither_n + 1, np.int16)])


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_shared_parameter_program_equals_full_load():
    c = _fresh_context()
    try:
        params = KM.synthetic_resnet101()
        fe = V.FeatureExtractor(c)
        pcm = synth_pcm(3, 16000 * 6)
        T = fe(pcm, to_host=False).nframes
        src = KM.compile_resnet101(params, 64, V.WINLEN, window_input=True)
        c.cnn_load(5, src)
        for w, (full_id, alias_id) in zip((131, 12), ((6, 2), (7, 3))):
            comp = KM.compile_resnet101(params, 64, w, window_input=True)
            assert np.array_equal(comp.blob, src.blob)
            starts = [0, 7, 130, T - w]
            f0 = _free_bytes()
            c.cnn_load(full_id, comp)
            full_bytes = f0 - _free_bytes()
            want = c.vbx_embed(full_id, starts)
            f0 = _free_bytes()
            c.cnn_load_shared(alias_id, 5, comp)
            shared_bytes = f0 - _free_bytes()
            got = c.vbx_embed(alias_id, starts)
            # (a 12-frame window can pool to NaN, as it does through the reference's network: the same rows must)
            assert np.array_equal(got, want, equal_nan=True), w
            assert np.isfinite(got[0]).all()
            print(f'width {w}: full load {full_bytes / 2**20:.1f} MiB, shared load {shared_bytes / 2**20:.2f} MiB')
            assert full_bytes > 0 and shared_bytes < 0.1 * full_bytes
        # unloading the source (a small program replaces it) leaves both aliases working on the parameters they share
        c.cnn_load(5, KM.compile_layers([dict(type='dense', W=np.ones((4, 2), np.float32), b=np.zeros(2, np.float32),
                                                   activation='linear')], (1, 1, 4), patch_input=False))
        assert np.array_equal(c.vbx_embed(2, [0, 7, 130, T - 131]), c.vbx_embed(6, [0, 7, 130, T - 131]), equal_nan=True)
        assert np.array_equal(c.vbx_embed(3, [0, 7, 130, T - 12]), c.vbx_embed(7, [0, 7, 130, T - 12]), equal_nan=True)
        with pytest.raises(_native.NativeError, match='not loaded'):
            c.cnn_load_shared(2, 4, comp)
    finally:
        c.close()


def _write_wav(path, pcm):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.ascontiguousarray(pcm, '<i2').tobytes())
    return str(path)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('vfs_batch')
    s15 = _write_wav(d / 'synth_1p5s.wav', synth_pcm(15, 24000))
    s20 = _write_wav(d / 'synth_20s.wav', synth_pcm(20, 16000 * 20))
    s180 = _write_wav(d / 'synth_3min.wav', synth_pcm(180, 16000 * 180))
    lam, mus, sil = (os.path.join(GOLDEN, f) for f in ('lamartine.wav', 'musanmix.wav', 'silence2sec.wav'))
    missing = str(d / 'missing.wav')
    return [lam, mus, s15, s20, s180, sil, missing, lam, s20, mus, s15, s180]


@pytest.fixture(scope='module')
def scorer():
    return vfs.VoiceFemininityScoring(ffmpeg=None, models='synthetic')


class _FixedVAD:
    """A VAD that finds speech in every file with signal (two segments, a gap between them) and none in a silent one: makes
    the x-vector half run on every file whatever the stand-in VAD decides.  Same answer through both entries."""

    def __init__(self, seg):
        self.seg = seg

    def segment_signal(self, sig, start_sec=0):
        d = len(sig) / 16000
        if np.abs(np.asarray(sig, np.float64)).max() < 1e-3 * (32768 if sig.dtype == np.int16 else 1):
            return [('noEnergy', 0.0, d)]
        return [('speech', round(0.1 * d, 2), round(0.45 * d, 2)), ('music', round(0.45 * d, 2), round(0.55 * d, 2)),
                ('speech', round(0.55 * d, 2), round(0.95 * d, 2))]

    def __call__(self, path):
        from inaspeechsegmenter_amd.io import decode_pcm
        return self.segment_signal(decode_pcm(path, ffmpeg=None))

    def __getattr__(self, name):
        return getattr(self.seg, name)


def _recording(v, monkeypatch):
    """Every x-vector matrix that reaches the gender MLP goes to the list in sink[0], in call order."""
    sink = [[]]
    orig = v.gender_predict

    def rec(x):
        sink[0].append(np.array(x, copy=True))
        return orig(x)
    monkeypatch.setattr(v, 'gender_predict', rec)
    return sink


def _singles(v, paths):
    res = []
    for p in paths:
        try:
            res.append(v(p))
        except FileNotFoundError as exc:
            res.append(exc)
    return res


@pytest.mark.parametrize('vad', ['standin', 'fixed'])
def test_batch_process_equals_call(scorer, files, vad, monkeypatch, tmp_path):
    v = scorer
    if vad == 'fixed':
        monkeypatch.setattr(v, 'vad', _FixedVAD(v.vad))
    sink = _recording(v, monkeypatch)
    want = _singles(v, files)
    want_x, sink[0] = sink[0], []
    got = v.batch_process(files, output_csv=str(tmp_path / 'out.tsv'))
    got_x = sink[0]
    assert len(got) == len(files)
    for p, g, w in zip(files, got, want):
        if isinstance(w, Exception):
            assert isinstance(g, str) and 'FileNotFoundError' in g, (p, g)
        else:
            assert g == w, (p, g, w)
    assert len(got_x) == len(want_x) and all(np.array_equal(a, b) for a, b in zip(got_x, want_x))
    sil = files.index(os.path.join(GOLDEN, 'silence2sec.wav'))
    assert got[sil] == (None, 0, 0)
    if vad == 'fixed':
        assert all(r[2] > 0 for i, r in enumerate(got) if isinstance(r, tuple) and i != sil)
    rows = open(tmp_path / 'out.tsv').read().splitlines()
    assert rows[0] == 'path\tscore\tspeech_duration\tnb_vectors' and len(rows) == len(files) + 1
    assert rows[1] == '\t'.join([files[0]] + [str(x) for x in got[0]]) and rows[7].startswith(files[6] + '\tFileNotFoundError')
    print(vad, got)


def test_batches_decodes_tail_loads_and_skipped_front_end(scorer, files, monkeypatch):
    v = scorer
    monkeypatch.setattr(v, 'vad', _FixedVAD(v.vad))
    paths = [files[3], files[2], files[3], files[5], files[3], files[2]]        # 20 s, 1.5 s, 20 s, silence, 20 s, 1.5 s
    want = _singles(v, paths)
    decodes, batches, loads = [], [], []
    dec = vfs.decode_pcm
    monkeypatch.setattr(vfs, 'decode_pcm', lambda p, **kw: (decodes.append(p), dec(p, **kw))[1])
    feat = v.ctx.vbx_features_batch_pcm16
    monkeypatch.setattr(v.ctx, 'vbx_features_batch_pcm16', lambda pcms, **kw: (batches.append([len(p) for p in pcms]), loads.append([]),
                                                                              feat(pcms, **kw))[2])
    shared, full = v.ctx.cnn_load_shared, v.ctx.cnn_load
    monkeypatch.setattr(v.ctx, 'cnn_load_shared', lambda nid, src, comp: (loads[-1].append(comp.in_shape[1]), shared(nid, src, comp))[1])
    monkeypatch.setattr(v.ctx, 'cnn_load', lambda nid, comp: (loads[-1].append(('full', comp.in_shape)), full(nid, comp))[1])
    got = v.batch_process(paths, batch_seconds=25)
    assert got == want
    assert sorted(decodes) == sorted(paths)                                     # one decode per file
    assert len(batches) == 3                                                     # 20 + 1.5 | 20 | 20 + 1.5 (silence: none)
    assert 32000 not in sum(batches, []) and sum(len(b) for b in batches) == 5   # the silent file never reached the front end
    for b in loads:                                                              # one shared load per tail width and batch at most
        assert len(b) == len(set(b)) and not any(isinstance(x, tuple) for x in b), loads
