#!/usr/bin/env python3
"""FLAC without ffmpeg: device decode (flac_decode_kernel) against host decode and against the WAV twins.

Seeded synthetic N x `--minutes` 16 kHz mono 16-bit recordings (bench.py's generator) are encoded by tests/flacgen.py's
realistic mode (best of FIXED 0-4 / LPC 1-8 per 4096-sample block) and written with their WAV twins to a temporary
directory.  Timed in one process, after one warm-up pass each:
  flac        batch_process on the FLAC files: compressed frames to the device, one decode launch per pass
  flac_host   batch_process on the same files with the frames decoded by iss_flac_decode_host in the decode threads
              (flac._HOST_DECODE, a benchmark switch)
  wav         batch_process on the WAV twins
  kernel      one iss_flac_decode call over all N files from page-locked memory, event-timed by the library's profiler:
              the H2D copy of the compressed bytes and the kernel, in ms per audio-hour
  index       the host frame index (FlacStream: metadata + iss_flac_index) per audio-hour
Writes one JSON (default profiles/flac_<n>.json) and prints it.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=8)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--kernel-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    import bench
    import flacgen
    from inaspeechsegmenter_amd import Segmenter, flac, _native
    n16 = int(args.minutes * 60 * 16000)
    tmp = tempfile.mkdtemp(prefix='bench_flac_')
    ff, fw, pcms = [], [], []
    t0 = time.time()
    for i in range(args.files):
        x = bench.synth_recording_numpy(i, n16)
        pcms.append(x)
        ff.append(flacgen.write(os.path.join(tmp, f'r{i}.flac'), x, 16000, 16))
        fw.append(flacgen.wav_twin(os.path.join(tmp, f'r{i}.wav'), x, 16000, 16))
    gen_s = time.time() - t0
    hours = args.files * args.minutes / 60.0
    flac_bytes = sum(os.path.getsize(f) for f in ff)
    pcm_bytes = sum(x.nbytes for x in pcms)

    seg = Segmenter(ffmpeg=None, models='synthetic')

    def run(files, tag):
        outs = [os.path.join(tmp, 'out', tag, os.path.basename(f) + '.csv') for f in files]
        t = time.perf_counter()
        _, nb, _, lmsg = seg.batch_process(files, outs)
        assert nb == len(files), lmsg
        return time.perf_counter() - t, outs

    def host_run(files, tag):
        flac._HOST_DECODE = True
        try:
            return run(files, tag)
        finally:
            flac._HOST_DECODE = False

    run(ff[:2], 'w1'); host_run(ff[:2], 'w2'); run(fw[:2], 'w3')          # warm-up: workers, code objects
    legs = {}
    for rep in range(2):                                                  # alternate the legs, keep the best of two
        for name, fn, files in (('flac', run, ff), ('flac_host', host_run, ff), ('wav', run, fw)):
            t, outs = fn(files, name)
            legs.setdefault(name, []).append(t)
            legs[name + '_outs'] = outs
    same = all(open(a).read() == open(b).read() == open(c).read()
               for a, b, c in zip(legs['flac_outs'], legs['flac_host_outs'], legs['wav_outs']))

    t = time.perf_counter()
    streams = []
    for f in ff:
        with open(f, 'rb') as fh:
            streams.append(flac.FlacStream(fh.read(), f))
    index_s = time.perf_counter() - t

    ctx = seg.ctx
    src = ctx.pinned_empty((sum(-(-s.audio.size // 16) * 16 for s in streams),), np.uint8)
    jobs, pos, fbeg, dpos = [], 0, 0, 0
    for s in streams:
        src[pos:pos + s.audio.size] = s.audio
        jobs.append((pos, fbeg, len(s.frames), s.n, 1, 16, _native.FLAC_TO_SIGNAL, -1, dpos, 0))
        pos += -(-s.audio.size // 16) * 16
        fbeg += len(s.frames)
        dpos += s.n
    frames = np.concatenate([s.frames for s in streams])
    ctx.flac_decode(src, frames, jobs, n_signal=dpos)
    ctx.synchronize()
    kern, h2d = [], []
    ctx.prof_enable(True)
    for _ in range(args.kernel_reps):
        ctx.prof_reset()
        st = ctx.flac_decode(src, frames, jobs, n_signal=dpos)
        ctx.synchronize()
        inst = {d['kernel'].split('(')[0]: d['ms'] for d in ctx.prof_instances()}
        kern.append(inst['flac_decode_kernel']); h2d.append(inst['flac_h2d'])
    ctx.prof_enable(False)
    ok = not st.any()
    dev = ctx.get_signal_pcm16(0, dpos)
    exact = ok and np.array_equal(dev, np.concatenate(pcms))
    ctx.pinned_free(src)

    best = {k: min(v) for k, v in legs.items() if not k.endswith('_outs')}
    out = {
        'files': args.files, 'minutes_per_file': args.minutes, 'source': '16 kHz mono 16-bit FLAC (flacgen realistic)',
        'audio_hours': hours, 'generate_s': round(gen_s, 2), 'frames': int(len(frames)),
        'compressed_over_pcm_bytes': flac_bytes / pcm_bytes,
        'flac_h_per_s': hours / best['flac'], 'flac_host_h_per_s': hours / best['flac_host'], 'wav_h_per_s': hours / best['wav'],
        'ratio_flac_vs_wav': best['wav'] / best['flac'], 'ratio_flac_vs_flac_host': best['flac_host'] / best['flac'],
        'leg_s_runs': {k: v for k, v in legs.items() if not k.endswith('_outs')},
        'kernel_ms_per_audio_hour': float(np.median(kern)) / hours, 'h2d_ms_per_audio_hour': float(np.median(h2d)) / hours,
        'index_ms_per_audio_hour': 1000.0 * index_s / hours, 'kernel_ms_runs': kern, 'h2d_ms_runs': h2d,
        'csv_identical_across_legs': same, 'device_bit_identical': bool(exact),
    }
    path = args.out or os.path.join(ROOT, 'profiles', f'flac_{args.files}.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    seg.close()
    return 0 if same and exact else 1


if __name__ == '__main__':
    sys.exit(main())
