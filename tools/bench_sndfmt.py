#!/usr/bin/env python3
"""Telephony audio without ffmpeg: G.711 mu-law and IMA ADPCM expanded on the device against the host and the PCM16 twins.

Seeded synthetic N x `--minutes` 8 kHz mono recordings (bench.py's generator at 16 kHz, every second sample) are written to a
temporary directory as mu-law WAV, IMA ADPCM WAV (256-byte blocks) and the PCM16 WAV twin of each.  All run through
Segmenter(ffmpeg=None, resample=True).batch_process in ONE process, legs alternated, `--reps` repeats each after a warm-up:
  ulaw, ima            the stored bytes go to the device (resample kernel reading ISS_RS_ULAW; adpcm_decode_kernel + resample)
  ulaw_twin, ima_twin  the PCM16 WAV twins
  ulaw_host, ima_host  the same files expanded on the host in the decode threads (sndfmt._HOST_DECODE, a benchmark switch:
                       numpy table / iss_adpcm_decode_host), then resampled on the device like the twins
Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats` (this script started again with
--kernel-child: one pass over the mu-law and one over the IMA files).  Writes one JSON (default profiles/sndfmt_<n>.json).
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


def make_files(tmp, nfiles, minutes):
    import bench
    import sndgen
    n8 = int(minutes * 60 * 8000)
    sets = {'ulaw': [], 'ima': [], 'ulaw_twin': [], 'ima_twin': []}
    for i in range(nfiles):
        x = bench.synth_recording_numpy(i, 2 * n8)[::2]
        x = np.asarray(x, dtype=np.float64) / (32768.0 if np.abs(x).max() > 2 else 1.0)
        for kind in ('ulaw', 'ima'):
            p, tfmt, twin = sndgen.write(os.path.join(tmp, f'r{i}_{kind}.wav'), 'wav', kind, False, x, 8000)
            sets[kind].append(p)
            sets[kind + '_twin'].append(sndgen.wav_twin(os.path.join(tmp, f'r{i}_{kind}_twin.wav'), twin, 8000, tfmt))
    return sets


def kernel_child(tmp, nfiles, minutes):
    """One pass over the mu-law files and one over the IMA files (after a warm-up), for the profiler."""
    from inaspeechsegmenter_amd import Segmenter
    sets = make_files(tmp, nfiles, minutes)
    seg = Segmenter(ffmpeg=None, models='synthetic', resample=True)
    for k in range(2):
        for kind in ('ulaw', 'ima'):
            files = sets[kind]
            _, nb, _, lmsg = seg.batch_process(files, [os.path.join(tmp, 'out', f'{k}_{os.path.basename(f)}.csv') for f in files])
            assert nb == len(files), lmsg
    seg.close()
    return 0


def kernel_times(args, tmp):
    """-> {kernel name: {'calls', 'total_ms', 'mean_us'}} of adpcm_decode_kernel and resample_kernel, or {'error': ...}."""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(prof):
        return {'error': 'rocprofv3 not found'}
    d = os.path.join(tmp, 'prof')
    cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
           '--kernel-child', os.path.join(tmp, 'child'), '--files', str(args.files), '--minutes', str(args.minutes)]
    os.makedirs(os.path.join(tmp, 'child'), exist_ok=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    if r.returncode != 0:
        return {'error': 'rocprofv3 run failed (%d): %s' % (r.returncode, r.stdout.decode(errors='replace')[-400:])}
    out = {}
    for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                name = row.get('Name') or row.get('Kernel_Name') or ''
                for want in ('adpcm_decode_kernel', 'resample_kernel'):
                    if want in name:
                        total = float(row.get('TotalDurationNs') or row.get('Total_Duration_Ns') or 0)
                        calls = int(float(row.get('Calls') or 0))
                        e = out.setdefault(want, {'calls': 0, 'total_ms': 0.0})
                        e['calls'] += calls
                        e['total_ms'] += total / 1e6
    for e in out.values():
        e['mean_us'] = 1000.0 * e['total_ms'] / max(e['calls'], 1)
    return out or {'error': 'no kernel_stats.csv rows for the two kernels'}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-kernel-trace', action='store_true')
    ap.add_argument('--kernel-child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if args.kernel_child:
        return kernel_child(args.kernel_child, args.files, args.minutes)

    from inaspeechsegmenter_amd import Segmenter, sndfmt
    tmp = tempfile.mkdtemp(prefix='bench_sndfmt_')
    t0 = time.time()
    sets = make_files(tmp, args.files, args.minutes)
    gen_s = time.time() - t0
    hours = args.files * args.minutes / 60.0
    seg = Segmenter(ffmpeg=None, models='synthetic', resample=True)

    def run(name, limit=None):
        host = name.endswith('_host')
        files = sets[name[:-5] if host else name][:limit]
        outs = [os.path.join(tmp, 'out', name, os.path.basename(f) + '.csv') for f in files]
        sndfmt._HOST_DECODE = host
        try:
            t = time.perf_counter()
            _, nb, _, lmsg = seg.batch_process(files, outs)
            dt = time.perf_counter() - t
        finally:
            sndfmt._HOST_DECODE = False
        assert nb == len(files), lmsg
        return dt, outs

    names = ('ulaw', 'ima', 'ulaw_twin', 'ima_twin', 'ulaw_host', 'ima_host')
    for name in names:                                                    # warm-up: workers, code objects, filters
        run(name, 2)
    legs, outs = {n: [] for n in names}, {}
    for rep in range(args.reps):                                          # alternate the legs
        for name in names:
            t, outs[name] = run(name)
            legs[name].append(t)
    same = all(open(a).read() == open(b).read() == open(c).read()
               for kind in ('ulaw', 'ima') for a, b, c in zip(outs[kind], outs[kind + '_twin'], outs[kind + '_host']))
    seg.close()

    res = {'files': args.files, 'minutes_per_file': args.minutes, 'source': '8 kHz mono: mu-law WAV, IMA ADPCM WAV (256-byte blocks), PCM16 twins',
           'audio_hours': hours, 'generate_s': round(gen_s, 2), 'reps': args.reps, 'leg_s_runs': legs,
           'h_per_s': {n: hours / float(np.median(v)) for n, v in legs.items()},
           'h_per_s_spread': {n: [hours / max(v), hours / min(v)] for n, v in legs.items()},
           'csv_identical_across_legs': same}
    for n, v in legs.items():
        print('%-10s %6.2f audio-hours/s (median of %d; %.2f .. %.2f)' % (n, hours / float(np.median(v)), len(v), hours / max(v), hours / min(v)))
    if not args.no_kernel_trace:
        res['kernel_trace'] = kernel_times(args, tmp)
    path = args.out or os.path.join(ROOT, 'profiles', f'sndfmt_{args.files}.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
