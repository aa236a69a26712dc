#!/usr/bin/env python3
"""Channel survey of multi-channel files: Segmenter.survey_files on the device against io.survey_channels on the host.

Three sets of `--files` x `--minutes`, the files of tools/bench_mixes.py (one file per set is generated and copied):
  wav_48k_8ch          48 kHz PCM16 WAV, 8 channels
  flac_16k_left_side   16 kHz FLAC, 2 channels
  ima_8k               8 kHz IMA ADPCM, 2 channels
Timed per set, `--reps` times a leg, alternated, after one warm-up of each leg:
  device  A: seg.survey_files(files)
  host    B: the route it replaces: io.survey_channels per file in four threads (the decode threads' count)
Every survey of A must equal its counterpart of B to the bit.  Audio-hours count file-hours.  survey_kernel's time per launch
comes from the library profiler over one further pass of leg A, with the stored bytes the launch reads as a fraction of the
HBM rate.  Writes one JSON (default profiles/survey.json) and prints it.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM_BYTES_PER_S = 8.0e12            # MI355X peak HBM3E rate
SETS = ('wav_48k_8ch', 'flac_16k_left_side', 'ima_8k')


def leg_device(seg, files):
    t = time.perf_counter()
    out = seg.survey_files(files)
    return time.perf_counter() - t, out


def leg_host(files):
    from inaspeechsegmenter_amd import io as iss_io
    t = time.perf_counter()
    with ThreadPoolExecutor(4) as pool:
        out = list(pool.map(iss_io.survey_channels, files))
    return time.perf_counter() - t, out


def profiled(seg, files, read_bytes):
    """-> survey_kernel and survey_reduce_kernel over one pass of the device leg, from the library profiler."""
    ctx = seg.ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    leg_device(seg, files)
    out = {}
    for inst in ctx.prof_instances():
        if inst['kernel'] in ('survey_kernel', 'survey_reduce_kernel'):
            out[inst['kernel']] = {'launches': inst['launches'], 'total_ms': inst['ms'], 'ms_per_launch': inst['ms'] / inst['launches']}
    ctx.prof_enable(False)
    k = out.get('survey_kernel')
    if k:
        k['stored_bytes_read'] = read_bytes
        k['bytes_per_s'] = read_bytes / (k['total_ms'] * 1e-3)
        k['fraction_of_hbm_rate'] = k['bytes_per_s'] / HBM_BYTES_PER_S
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sets', default=','.join(SETS), help='comma-separated subset of: ' + ', '.join(SETS))
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    import bench_mixes
    from inaspeechsegmenter_amd import Segmenter
    tmp = tempfile.mkdtemp(prefix='bench_survey_')
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'reps': args.reps, 'hbm_bytes_per_s': HBM_BYTES_PER_S, 'sets': {}}
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ok = True
    for name in args.sets.split(','):
        hours = args.files * args.minutes / 60.0
        files = bench_mixes.generate(tmp, name, args.files, args.minutes)
        legs = {'device': [], 'host': []}
        _, a = leg_device(seg, files)                                  # warm-up, and the surveys compared
        _, b = leg_host(files)
        same = len(a) == len(b) and all(x == y for x, y in zip(a, b))
        ok = ok and same
        for _ in range(args.reps):
            legs['device'].append(leg_device(seg, files)[0])
            legs['host'].append(leg_host(files)[0])
            print('%-20s device %.3f s, host %.3f s' % (name, legs['device'][-1], legs['host'][-1]), flush=True)
        s = b[0]
        width = {'wav_48k_8ch': 2, 'flac_16k_left_side': 2, 'ima_8k': 2}[name]      # bytes per sample the survey kernel reads
        entry = {'file_hours_per_leg': hours, 'file_bytes': os.path.getsize(files[0]), 'channels': s.channels, 'frames': s.n,
                 'rate': s.sr, 'bit_equal': same, 'downmix_loss_db': s.downmix_loss_db, 'active': s.active()}
        for leg, runs in legs.items():
            entry[leg] = {'s_runs': runs, 'file_h_per_s_median': hours / float(np.median(runs)),
                          'file_h_per_s_spread': [hours / max(runs), hours / min(runs)]}
        entry['device_vs_host'] = float(np.median(legs['host'])) / float(np.median(legs['device']))
        entry['device']['kernels'] = profiled(seg, files, args.files * s.n * s.channels * width)
        result['sets'][name] = entry
        print('%-20s device %.1f / host %.2f file-hours/s (medians of %d), bit-equal: %s, %s' % (
              name, entry['device']['file_h_per_s_median'], entry['host']['file_h_per_s_median'], args.reps, same,
              entry['device']['kernels']), flush=True)
        for f in files:
            os.remove(f)
    seg.close()
    path = args.out or os.path.join(ROOT, 'profiles', 'survey.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
