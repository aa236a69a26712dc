#!/usr/bin/env python3
"""Device resampling (Segmenter(ffmpeg=None, resample=True)) against 16 kHz input and against resampling on the host.

Seeded synthetic N x `--minutes` 48 kHz stereo int16 WAVs (bench.py's recording generator at 16 kHz, upsampled by linear
interpolation, right channel 0.7 x left) are written to a temporary directory, with their 16 kHz mono PCM16
(resample.resample_ref, what the device must produce bit for bit) beside them.  Timed, after one warm-up pass each:
  resample    batch_process on the 48 kHz stereo files, resample=True
  mono16k     batch_process on the 16 kHz mono files (today's path, the same audio)
  host        per file: resample on the host (scipy.signal.resample_poly + quantise when scipy is there, else
              resample_ref), then segment_signal -- what a user without ffmpeg does today
  kernel      one iss_resample_pcm16 call over all N files from page-locked memory, event-timed by the library's
              profiler: the H2D copy of the stored samples and the kernel, in ms per audio-hour
Writes one JSON (default profiles/resample_<n>.json) and prints it.
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
    ap.add_argument('--host-files', type=int, default=2, help='files timed through the host path (it is slow)')
    ap.add_argument('--kernel-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    import bench
    from wavgen import write_wav
    from inaspeechsegmenter_amd import Segmenter, resample as R
    sr, n16 = 48000, int(args.minutes * 60 * 16000)
    tmp = tempfile.mkdtemp(prefix='bench_resample_')
    f48, f16, stored = [], [], []
    t0 = time.time()
    for i in range(args.files):
        base = bench.synth_recording_numpy(i, n16).astype(np.float64)
        up = np.interp(np.arange(n16 * 3) / 3.0, np.arange(n16), base)
        st = np.clip(np.round(np.stack([up, 0.7 * up], axis=1)), -32768, 32767).astype('<i2')
        stored.append(st)
        f48.append(write_wav(os.path.join(tmp, f'r{i}_48k.wav'), st, sr, 'i16'))
        f16.append(write_wav(os.path.join(tmp, f'r{i}_16k.wav'), R.resample_ref(st, sr), 16000, 'i16'))
    gen_s = time.time() - t0
    hours = args.files * args.minutes / 60.0

    rs = Segmenter(ffmpeg=None, models='synthetic', resample=True)
    plain = Segmenter(ffmpeg=None, models='synthetic')

    def run(seg, files):
        outs = [os.path.join(tmp, 'out', os.path.basename(f) + '.csv') for f in files]
        t = time.perf_counter()
        _, nb, _, _ = seg.batch_process(files, outs)
        assert nb == len(files)
        return time.perf_counter() - t, outs

    run(rs, f48[:2]); run(plain, f16[:2])                         # warm-up: contexts, workers, filters
    res, out_rs = run(rs, f48)
    mono, out_16 = run(plain, f16)
    same = all(open(a).read() == open(b).read() for a, b in zip(out_rs, out_16))

    try:
        import scipy.signal as ss
        host_how = 'scipy.signal.resample_poly'
        host_rs = lambda st: R.quantise(ss.resample_poly(R.downmix(st), 1, 3))
    except ImportError:
        host_how = 'resample_ref (numpy)'
        host_rs = lambda st: R.resample_ref(st, sr)
    nh = max(1, min(args.host_files, args.files))
    t = time.perf_counter()
    host_rs_s = 0.0
    for st in stored[:nh]:
        a = time.perf_counter()
        pcm = host_rs(st)
        host_rs_s += time.perf_counter() - a
        plain.segment_signal(pcm)
    host = time.perf_counter() - t
    host_hours = nh * args.minutes / 60.0

    # kernel alone: all files in one call from page-locked memory
    ctx = rs.ctx
    nbytes = sum(s.nbytes for s in stored)
    pin = ctx.pinned_empty((nbytes,), np.uint8)
    jobs, pos, opos = [], 0, 0
    for s in stored:
        pin[pos:pos + s.nbytes] = s.reshape(-1).view(np.uint8)
        jobs.append(ctx.resample_job(s, sr, pos, opos))
        pos += s.nbytes
        opos += jobs[-1][-1]
    ctx.resample(pin, jobs, n_signal=opos)
    ctx.synchronize()
    kern, h2d = [], []
    ctx.prof_enable(True)
    for _ in range(args.kernel_reps):
        ctx.prof_reset()
        ctx.resample(pin, jobs, n_signal=opos)
        ctx.synchronize()
        inst = {d['kernel'].split('(')[0]: d['ms'] for d in ctx.prof_instances()}
        kern.append(inst['resample_kernel']); h2d.append(inst['resample_h2d'])
    ctx.prof_enable(False)
    dev = ctx.get_signal_pcm16(0, opos)
    exact = all(np.array_equal(dev[j[6]:j[6] + j[7]], R.resample_ref(s, sr)) for s, j in list(zip(stored, jobs))[:2])
    ctx.pinned_free(pin)

    out = {
        'files': args.files, 'minutes_per_file': args.minutes, 'source': '48 kHz stereo int16 WAV', 'audio_hours': hours,
        'generate_s': round(gen_s, 2),
        'resample_h_per_s': hours / res, 'mono16k_h_per_s': hours / mono, 'ratio_resample_vs_mono16k': mono / res,
        'host_path': host_how, 'host_files': nh, 'host_h_per_s': host_hours / host,
        'host_resample_cpu_s_per_audio_hour': host_rs_s / host_hours,
        'kernel_ms_per_audio_hour': float(np.median(kern)) / hours, 'h2d_ms_per_audio_hour': float(np.median(h2d)) / hours,
        'h2d_bytes_per_audio_hour': nbytes / hours, 'kernel_ms_runs': kern, 'h2d_ms_runs': h2d,
        'csv_identical_to_mono16k': same, 'device_bit_identical_first_files': exact,
    }
    path = args.out or os.path.join(ROOT, 'profiles', f'resample_{args.files}.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    rs.close(); plain.close()
    return 0 if same and exact else 1


if __name__ == '__main__':
    sys.exit(main())
