"""Stale-workspace screen: a result must not depend on what the workspace held before the call.

Every activation buffer is grown on demand and reused, 8 MiB of slack sits behind each one, K and the channels are padded, row
tiles overhang M and footprints reach into the next window; the suite's other tests leave finite activations of the previous test
there, which hide a stale value multiplied by a zero weight or an overhang row read into a real output.  Here the scratch
buffers are overwritten (iss_scribble: capacity and slack, not the used size) with quiet NaN, -inf, 0 and FLT_MAX before the jobs
of tests/screen_jobs.py run, largest size first, so that each smaller run sits inside bytes the larger one did not rewrite; every
output must equal, bit for bit, what a fresh context gave straight after its set-up (and that baseline is held to the job's
reference).  The same again under the smallest workspace the library takes, where the passes index relative to themselves."""
import numpy as np
import pytest

import screen_jobs as SJ
from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, vbx as V, _native

pytestmark = pytest.mark.gpu


def _sweep(b, job, base, inst, what, ws_limit=None):
    job.settings(b, ws_limit)
    job.run(b, job.sizes[-1])                                   # every buffer at its final capacity
    for word in SJ.WORDS:
        b.scribble(word)
        for size in reversed(job.sizes):
            out = job.run(b, size)
            if not all(SJ.same_bits(g, w) for g, w in zip(out, base[size])) or len(out) != len(base[size]):
                pytest.fail(SJ.mismatch_report(job, size, out, base[size], inst[size], f'after scribble(0x{word:08X}), {what}'))


@pytest.mark.parametrize('job', SJ.jobs(), ids=lambda j: j.name)
def test_outputs_do_not_depend_on_stale_workspace(job):
    base, inst = SJ.serial_baseline(job)                        # context A: fresh, straight after prepare, held to the reference
    b = SJ.fresh_context()
    try:
        job.prepare(b)
        _sweep(b, job, base, inst, 'default workspace')
        if job.passes_at_floor is not None:
            # at least three passes on the largest size: pass-relative indexing meets scribbled bytes too.  The bits of a result may
            # depend on the workspace limit (pass boundaries move tile boundaries, and a tile's position decides which of a kernel's
            # paths a window takes: tests/test_gpu_cnn_defaults.py holds two limits to 2e-6 of each other, not to equality), so
            # this sweep is held to a baseline of its own, from a fresh context under the same limit; how many sizes differ from
            # the default-workspace baseline is printed.
            assert job.passes_at_floor >= 3, (job.name, job.passes_at_floor)
            small = SJ.fresh_context()
            try:
                job.prepare(small)
                job.settings(small, SJ.WS_FLOOR)
                base_small = {size: SJ.run_profiled(small, job, size)[0] for size in job.sizes}
            finally:
                small.close()
            moved = [size for size in job.sizes if not all(SJ.same_bits(g, w) for g, w in zip(base_small[size], base[size]))]
            print(f'{job.name}: {len(moved)} of {len(job.sizes)} sizes give other bits under the {SJ.WS_FLOOR >> 20} MiB limit {moved}')
            for size in job.sizes:
                job.check(size, base_small[size])
            _sweep(b, job, base_small, inst, f'{SJ.WS_FLOOR >> 20} MiB workspace ({job.passes_at_floor} passes)', SJ.WS_FLOOR)
    finally:
        b.close()


def test_every_kernel_family_is_screened():
    """The union of the kernel instances the serial baselines launched holds every family of the engine: a later dispatcher
    change cannot quietly drop one from the screens."""
    names = set()
    for job in SJ.jobs():
        mine = {k for v in SJ.serial_baseline(job)[1].values() for k in v}
        print(f'{job.name}: {sorted(mine)}')
        names |= mine
    assert not SJ.missing_families(names), SJ.missing_families(names)


def test_scribble_writes_the_word():
    """Positive control: the scribble really writes.  The decoders' staging buffers are scratch with a read-back
    (iss_flac_get_stage / iss_adpcm_get_stage): after a staged decode they hold the stored samples, after iss_scribble(w) every
    byte of what they return is w's (the staged job starts the buffer, so the words are aligned)."""
    from inaspeechsegmenter_amd import _native
    import test_gpu_sndfmt as tsnd
    x, fs, _ = SJ.FlacJob()._input()
    ad, twin, _ = SJ.AdpcmJob()._input()
    c = SJ.fresh_context()
    try:
        for word in (0x7FC00000, 0xDEADBEEF):
            st = c.flac_decode(fs.audio, fs.frames, [(0, 0, len(fs.frames), fs.n, fs.ch, fs.bps, _native.FLAC_TO_STAGE, -1, 0, 0)], n_signal=0)
            got = c.flac_get_stage(0, fs.n, fs.ch, fs.bps)
            assert not st.any() and np.array_equal(got, SJ.tflac._stored(x, fs.bps))
            assert np.array_equal(tsnd._decode_staged(c, ad), twin)
            c.scribble(word)
            for name, got in (('flac', c.flac_get_stage(0, fs.n, fs.ch, fs.bps)), ('adpcm', c.adpcm_get_stage(0, ad.n, ad.ch))):
                raw = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
                want = np.resize(np.frombuffer(np.uint32(word).tobytes(), np.uint8), raw.size)
                assert raw.size >= 4000 and np.array_equal(raw, want), (name, hex(word), raw[:8])
    finally:
        c.close()


def test_scribble_overwrites_scratch_not_state():
    """iss_scribble leaves the resident signal, log-mel, log-energy, x-vector features, tables and parameters alone: after it the
    read-backs and the probabilities of a loaded net are what they were, with no reload; a second word changes nothing either."""
    from conftest import synth_pcm
    from inaspeechsegmenter_amd import tables
    c = SJ.fresh_context()
    try:
        c.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank())
        c.vbx_tables(tables.vbx_window(), tables.vbx_melbank())
        pcm = synth_pcm(21, 48000)
        pcm[20000:21000] = 0                                     # -inf rows: dead windows, so the row flags matter
        c.set_signal(pcm)
        T = c.sidekit()
        layers, shp = KM.synthetic_ina_like(21, 3, seed=1)
        c.cnn_load(0, KM.compile_layers(layers, shp))
        c.cnn_load(5, SJ._xv_comp(V.WINLEN, True))
        c.vbx_set_dither(V.dither_stream(len(pcm)))
        c.vbx_features_pcm16(pcm, to_host=False)
        rows, starts = S._window_rows(T), [0, 24, 100]

        def state():
            p, fin = c.cnn_probs(0, rows)
            return c.get_mspec(), c.get_loge(), c.get_signal_pcm16(0, len(pcm)), c.vbx_embed(5, starts), p, fin

        want = state()
        assert np.array_equal(want[2], pcm) and not want[5].all() and want[5].any() and np.isfinite(want[3]).all()
        for word in (0x7FC00000, 0xDEADBEEF):
            c.scribble(word)
            got = state()
            for k, (g, w) in enumerate(zip(got, want)):
                assert SJ.same_bits(g, w), (hex(word), k)
    finally:
        c.close()
