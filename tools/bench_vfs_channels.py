#!/usr/bin/env python3
"""Voice femininity per channel of two-channel files: batch_process(channels='split') against mono twins written on the host.

`--files` x `--minutes` of two-channel audio per format (the generator of tools/bench_channels.py): 48 kHz PCM16 WAV, 16 kHz
FLAC (left/side) and 8 kHz IMA ADPCM.  One file per format is generated and copied.  Timed per format, `--reps` times, alternated,
after one warm-up of each leg:
  split   A: v.batch_process(files, channels='split') -- per file one decode pass, the channels scored from the resident signal
  twins   B: the only route before: v.vad.load_pcm_channels per file, one 16 kHz mono WAV per channel written to disk (inside the
          timed region), then v.batch_process on those
Audio-hours count channel-hours.  The results of A must equal those of B, channel for channel.  After the timed runs one more
pass of each leg runs with the library's profiler on (iss_prof): device milliseconds per kernel class against the wall time of
the pass say where the time goes.  Writes one JSON (default profiles/vfs_channels.json) and prints it.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PROF_KINDS = {'gemm': 0, 'front_ends': 1, 'other': 2}


def leg_split(v, files):
    t = time.perf_counter()
    res = v.batch_process(files, channels='split')
    return time.perf_counter() - t, [one for r in res for one in r]


def leg_twins(v, files, tdir):
    import wavgen
    os.makedirs(tdir, exist_ok=True)
    t = time.perf_counter()
    twins = []
    for f in files:
        for k, pcm in enumerate(v.vad.load_pcm_channels(f)):
            twins.append(wavgen.write_wav(os.path.join(tdir, os.path.splitext(os.path.basename(f))[0] + f'.ch{k}.wav'), pcm, 16000, 'i16'))
    res = v.batch_process(twins)
    return time.perf_counter() - t, res


def profiled(v, run):
    """One pass of `run` with the profiler on -> wall seconds and device ms per kernel class on the scorer's context."""
    v.ctx.prof_enable(True)
    try:
        v.ctx.prof_reset()
        dt = run()[0]
        v.ctx.synchronize()
        dev = {name: {'ms': round(v.ctx.prof_get(k)[0], 2), 'launches': v.ctx.prof_get(k)[1]} for name, k in PROF_KINDS.items()}
    finally:
        v.ctx.prof_enable(False)
    dev_ms = sum(d['ms'] for d in dev.values())
    return {'wall_s': round(dt, 3), 'device_ms': dev, 'device_share_of_wall': round(dev_ms / 1e3 / dt, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    import bench_channels
    from inaspeechsegmenter_amd.vfs import VoiceFemininityScoring
    tmp = tempfile.mkdtemp(prefix='bench_vfs_channels_')
    hours = 2 * args.files * args.minutes / 60.0                       # channel-hours per leg
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'channels': 2, 'channel_hours_per_leg': hours, 'reps': args.reps,
              'models': 'synthetic', 'formats': {}}
    v = VoiceFemininityScoring(ffmpeg=None, models='synthetic', resample=True)
    ok = True
    for fmt in bench_channels.FORMATS:
        t0 = time.time()
        files = bench_channels.generate(tmp, fmt, args.files, args.minutes)
        gen_s = time.time() - t0
        tdir = os.path.join(tmp, 'twins', fmt)
        legs = {'split': [], 'twins': []}
        _, a = leg_split(v, files)                                     # warm-up, and the results compared
        _, b = leg_twins(v, files, tdir)
        same = a == b and all(isinstance(r, tuple) for r in a)
        ok = ok and same
        for _ in range(args.reps):
            legs['split'].append(leg_split(v, files)[0])
            legs['twins'].append(leg_twins(v, files, tdir)[0])
        entry = {'generate_s': round(gen_s, 2), 'file_bytes': os.path.getsize(files[0]), 'results_equal': same,
                 'speech_share': sum(r[1] for r in a if isinstance(r, tuple)) / (hours * 3600),
                 'x_vectors': sum(r[2] for r in a if isinstance(r, tuple))}
        for leg, runs in legs.items():
            entry[leg] = {'s_runs': runs, 'channel_h_per_s_best': hours / min(runs),
                          'channel_h_per_s_spread': [hours / max(runs), hours / min(runs)]}
        entry['split_vs_twins_best'] = min(legs['twins']) / min(legs['split'])
        entry['split']['where'] = profiled(v, lambda: leg_split(v, files))
        entry['twins']['where'] = profiled(v, lambda: leg_twins(v, files, tdir))
        result['formats'][fmt] = entry
        print('%-20s split %.2f / twins %.2f channel-hours/s (best of %d), results equal: %s' % (
              fmt, entry['split']['channel_h_per_s_best'], entry['twins']['channel_h_per_s_best'], args.reps, same), flush=True)
        shutil.rmtree(tdir, ignore_errors=True)
        for f in files:
            os.remove(f)
    v.vad.close()
    path = args.out or os.path.join(ROOT, 'profiles', 'vfs_channels.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
