#!/usr/bin/env python3
"""Every channel of two-channel files segmented on its own: batch_process(channels='split') against mono twins written on the host.

`--files` x `--minutes` of two-channel audio per format (bench.py's generator; the right channel is the left one delayed by 1.5 s
and attenuated, so the two channels segment differently): 48 kHz PCM16 WAV, 16 kHz FLAC (left/side, tests/flacgen.py, FIXED order
2) and 8 kHz IMA ADPCM (tests/sndgen.py).  One file per format is generated and copied.  Timed per format, `--reps` times,
alternated, after one warm-up of each leg:
  split   A: seg.batch_process(files, outs, channels='split')
  twins   B: what a user had to do before: io.decode_source per file, one mono WAV per channel written at the stored rate (inside
          the timed region), then seg.batch_process on those
Audio-hours count channel-hours.  Every CSV of A must be byte-identical to its counterpart of B.  The resample kernel's time per
launch comes from a run of its own per format and leg under `rocprofv3 --kernel-trace --stats` (this script started again with
--kernel-child).  Writes one JSON (default profiles/channels.json) and prints it.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FORMATS = ('wav_48k', 'flac_16k_left_side', 'ima_8k')


def generate(tmp, fmt, nfiles, minutes):
    """-> the paths of `nfiles` copies of one two-channel file of `minutes` in format `fmt`."""
    import bench
    import flacgen
    import sndgen
    import wavgen
    n = int(minutes * 60 * 16000)
    left = bench.synth_recording_numpy(0, n).astype(np.int64)
    right = np.roll(left, 24000) * 7 // 10
    pair = np.stack([left, right], axis=1)
    first = os.path.join(tmp, f'{fmt}_0' + ('.flac' if fmt.startswith('flac') else '.wav'))
    if fmt == 'wav_48k':
        wavgen.write_wav(first, np.repeat(pair, 3, axis=0).astype('<i2'), 48000, 'i16')     # held samples: content is not the point
    elif fmt == 'flac_16k_left_side':
        flacgen.write(first, pair, 16000, 16, channel_mode='left_side', subframe={'type': 'fixed', 'order': 2})
    else:
        sndgen.write(first, 'wav', 'ima', False, pair[::2] / 32768.0, 8000, block_align=512)
    files = [first]
    for k in range(1, nfiles):
        files.append(first.replace(f'{fmt}_0', f'{fmt}_{k}'))
        shutil.copyfile(first, files[-1])
    return files


def leg_split(seg, files, odir):
    from inaspeechsegmenter_amd import io as iss_io
    outs = [os.path.join(odir, os.path.splitext(os.path.basename(f))[0] + '.csv') for f in files]
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='split')
    dt = time.perf_counter() - t
    assert nb == 2 * len(files), lmsg
    return dt, [iss_io.channel_name(o, k) for o in outs for k in (0, 1)]


def leg_twins(seg, files, odir, tdir):
    import wavgen
    from inaspeechsegmenter_amd import io as iss_io
    os.makedirs(tdir, exist_ok=True)
    t = time.perf_counter()
    twins = []
    for f in files:
        x, sr = iss_io.decode_source(f)
        for k in range(x.shape[1]):
            col = np.ascontiguousarray(x[:, k])
            fmt = {np.dtype('<i2'): 'i16', np.dtype('<i4'): 'i32'}[col.dtype]
            twins.append(wavgen.write_wav(os.path.join(tdir, os.path.splitext(os.path.basename(f))[0] + f'.ch{k}.wav'), col, sr, fmt))
    outs = [os.path.join(odir, os.path.splitext(os.path.basename(f))[0] + '.csv') for f in twins]
    _, nb, _, lmsg = seg.batch_process(twins, outs)
    dt = time.perf_counter() - t
    assert nb == len(twins), lmsg
    return dt, outs


def kernel_child(args):
    """One pass of one leg over one format, for the kernel trace."""
    from inaspeechsegmenter_amd import Segmenter
    tmp = args.kernel_child
    files = sorted(glob.glob(os.path.join(tmp, args.format + '_*')))
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    if args.leg == 'split':
        leg_split(seg, files, os.path.join(tmp, 'child_out'))
    else:
        leg_twins(seg, files, os.path.join(tmp, 'child_out'), os.path.join(tmp, 'child_twins'))
    seg.close()
    return 0


def kernel_times(tmp, fmt, leg):
    """-> {'launches', 'total_ms', 'ms_per_launch'} of resample_kernel in one pass of `leg` over `fmt`, or {'error': ...}."""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(prof):
        return {'error': 'rocprofv3 not found'}
    d = os.path.join(tmp, f'prof_{fmt}_{leg}')
    cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
           '--kernel-child', tmp, '--format', fmt, '--leg', leg]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    if r.returncode != 0:
        return {'error': 'rocprofv3 run failed (%d): %s' % (r.returncode, r.stdout.decode(errors='replace')[-400:])}
    calls, total = 0, 0.0
    for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                if 'resample_kernel' in (row.get('Name') or row.get('Kernel_Name') or ''):
                    calls += int(float(row.get('Calls') or 0))
                    total += float(row.get('TotalDurationNs') or row.get('Total_Duration_Ns') or 0) / 1e6
    if not calls:                                                     # (16 kHz mono twins are read as arrays: nothing to resample)
        return {'launches': 0, 'total_ms': 0.0, 'ms_per_launch': None}
    return {'launches': calls, 'total_ms': total, 'ms_per_launch': total / calls}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-kernel-trace', action='store_true')
    ap.add_argument('--kernel-child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--format', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.kernel_child:
        return kernel_child(args)

    from inaspeechsegmenter_amd import Segmenter
    tmp = tempfile.mkdtemp(prefix='bench_channels_')
    hours = 2 * args.files * args.minutes / 60.0                       # channel-hours per leg
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'channels': 2, 'channel_hours_per_leg': hours, 'reps': args.reps,
              'formats': {}}
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ok = True
    for fmt in FORMATS:
        t0 = time.time()
        files = generate(tmp, fmt, args.files, args.minutes)
        gen_s = time.time() - t0
        legs = {'split': [], 'twins': []}
        _, a_outs = leg_split(seg, files, os.path.join(tmp, 'out_a', fmt))                              # warm-up, and the CSVs compared
        _, b_outs = leg_twins(seg, files, os.path.join(tmp, 'out_b', fmt), os.path.join(tmp, 'twins', fmt))
        same = len(a_outs) == len(b_outs) and all(open(a, 'rb').read() == open(b, 'rb').read() for a, b in zip(a_outs, b_outs))
        ok = ok and same
        for _ in range(args.reps):
            legs['split'].append(leg_split(seg, files, os.path.join(tmp, 'out_a', fmt))[0])
            legs['twins'].append(leg_twins(seg, files, os.path.join(tmp, 'out_b', fmt), os.path.join(tmp, 'twins', fmt))[0])
        entry = {'generate_s': round(gen_s, 2), 'file_bytes': os.path.getsize(files[0]), 'csv_identical': same}
        for leg, runs in legs.items():
            entry[leg] = {'s_runs': runs, 'audio_h_per_s_median': hours / float(np.median(runs)),
                          'audio_h_per_s_spread': [hours / max(runs), hours / min(runs)]}
        entry['split_vs_twins'] = float(np.median(legs['twins'])) / float(np.median(legs['split']))
        result['formats'][fmt] = entry
        print('%-20s split %.2f / twins %.2f channel-hours/s (medians of %d), CSVs identical: %s' % (
              fmt, entry['split']['audio_h_per_s_median'], entry['twins']['audio_h_per_s_median'], args.reps, same), flush=True)
    seg.close()
    if not args.no_kernel_trace:                                      # (after close: one process on the device at a time)
        for fmt in FORMATS:
            for leg in ('split', 'twins'):
                result['formats'][fmt][leg]['resample_kernel'] = kernel_times(tmp, fmt, leg)
                print(fmt, leg, 'resample_kernel', result['formats'][fmt][leg]['resample_kernel'], flush=True)
    path = args.out or os.path.join(ROOT, 'profiles', 'channels.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
