#!/usr/bin/env python3
"""Weighted channel mixes of multi-channel files: batch_process(mixes=...) against mono twins mixed and written on the host.

Three sets of `--files` x `--minutes` (bench.py's generator; channel c is channel 0 delayed by 1.5 s * c and attenuated, so the
mixes segment differently).  One file per set is generated and copied:
  wav_48k_8ch          48 kHz PCM16 WAV, 8 channels, mixes 0+1,2+3,4+5,6+7
  flac_16k_left_side   16 kHz FLAC, 2 channels (tests/flacgen.py, FIXED order 2), mixes 0,1,0+1
  ima_8k               8 kHz IMA ADPCM, 2 channels (tests/sndgen.py), mixes 0,1,0+1
Timed per set, `--reps` times, alternated, after one warm-up of each leg:
  mixes   A: seg.batch_process(files, outs, mixes=spec)
  twins   B: the route it replaces: io.decode_source per file, resample.mixdown per mix in numpy, one mono WAV per mix written
          (inside the timed region) -- float64 at the stored rate, which holds the mix exactly; at 16 kHz the quantised PCM16,
          since a 16 kHz mono float WAV takes the float path --, then seg.batch_process on those
Audio-hours count mix-hours.  Every CSV of A must be byte-identical to its counterpart of B.  resample_kernel's time per launch
comes from the library profiler (ctx.prof_instances of every worker context) over one further pass of each leg.  Writes one JSON
(default profiles/mixes.json) and prints it.
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

SETS = {'wav_48k_8ch': '0+1,2+3,4+5,6+7', 'flac_16k_left_side': '0,1,0+1', 'ima_8k': '0,1,0+1'}


def generate(tmp, name, nfiles, minutes):
    """-> the paths of `nfiles` copies of one file of `minutes` of set `name`."""
    import bench
    import flacgen
    import sndgen
    import wavgen
    n = int(minutes * 60 * 16000)
    left = bench.synth_recording_numpy(0, n).astype(np.int64)
    nch = 8 if name == 'wav_48k_8ch' else 2
    x = np.stack([np.roll(left, 24000 * c) * (10 - c) // 10 for c in range(nch)], axis=1)
    first = os.path.join(tmp, f'{name}_0' + ('.flac' if name.startswith('flac') else '.wav'))
    if name == 'wav_48k_8ch':
        wavgen.write_wav(first, np.repeat(x, 3, axis=0).astype('<i2'), 48000, 'i16')        # held samples: content is not the point
    elif name == 'flac_16k_left_side':
        flacgen.write(first, x, 16000, 16, channel_mode='left_side', subframe={'type': 'fixed', 'order': 2})
    else:
        sndgen.write(first, 'wav', 'ima', False, x[::2] / 32768.0, 8000, block_align=512)
    files = [first]
    for k in range(1, nfiles):
        files.append(first.replace(f'{name}_0', f'{name}_{k}'))
        shutil.copyfile(first, files[-1])
    return files


def leg_mixes(seg, files, odir, spec):
    from inaspeechsegmenter_amd import io as iss_io
    outs = [os.path.join(odir, os.path.splitext(os.path.basename(f))[0] + '.csv') for f in files]
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(files, outs, mixes=spec)
    dt = time.perf_counter() - t
    assert nb == len(spec) * len(files), lmsg
    return dt, [iss_io.mix_name(o, k) for o in outs for k in range(len(spec))]


def leg_twins(seg, files, odir, tdir, spec):
    import wavgen
    from inaspeechsegmenter_amd import io as iss_io
    from inaspeechsegmenter_amd import resample as R
    os.makedirs(tdir, exist_ok=True)
    t = time.perf_counter()
    twins = []
    for f in files:
        x, sr = iss_io.decode_source(f)
        for k, m in enumerate(spec):
            mono = R.mixdown(x, m)
            path = os.path.join(tdir, os.path.splitext(os.path.basename(f))[0] + f'.mix{k}.wav')
            if sr == R.SR_OUT:
                twins.append(wavgen.write_wav(path, R.quantise(mono).astype('<i2'), sr, 'i16'))
            else:
                twins.append(wavgen.write_wav(path, mono.astype('<f8'), sr, 'f64'))
    outs = [os.path.join(odir, os.path.splitext(os.path.basename(f))[0] + '.csv') for f in twins]
    _, nb, _, lmsg = seg.batch_process(twins, outs)
    dt = time.perf_counter() - t
    assert nb == len(twins), lmsg
    return dt, outs


def profiled(seg, leg):
    """-> {'launches', 'total_ms', 'ms_per_launch'} of resample_kernel over one pass of `leg()`, from the library profiler of
    every worker context."""
    ctxs = [w.ctx for w in seg.__dict__.get('_pipeline_workers', [])] or [seg.ctx]
    for c in ctxs:
        c.prof_enable(True)
        c.prof_reset()
    leg()
    calls, total = 0, 0.0
    for c in ctxs:
        for inst in c.prof_instances():
            if inst['kernel'] == 'resample_kernel':
                calls += inst['launches']
                total += inst['ms']
        c.prof_enable(False)
    if not calls:                                                     # (16 kHz mono twins are read as arrays: nothing to resample)
        return {'launches': 0, 'total_ms': 0.0, 'ms_per_launch': None}
    return {'launches': calls, 'total_ms': total, 'ms_per_launch': total / calls}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sets', default=','.join(SETS), help='comma-separated subset of: ' + ', '.join(SETS))
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    from inaspeechsegmenter_amd import Segmenter
    from inaspeechsegmenter_amd import resample as R
    tmp = tempfile.mkdtemp(prefix='bench_mixes_')
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'reps': args.reps, 'sets': {}}
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ok = True
    for name in args.sets.split(','):
        spec = R.parse_mixes(SETS[name])
        hours = len(spec) * args.files * args.minutes / 60.0           # mix-hours per leg
        t0 = time.time()
        files = generate(tmp, name, args.files, args.minutes)
        gen_s = time.time() - t0
        a_dir, b_dir, t_dir = (os.path.join(tmp, d, name) for d in ('out_a', 'out_b', 'twins'))
        legs = {'mixes': [], 'twins': []}
        _, a_outs = leg_mixes(seg, files, a_dir, spec)                                                 # warm-up, and the CSVs compared
        _, b_outs = leg_twins(seg, files, b_dir, t_dir, spec)
        same = len(a_outs) == len(b_outs) and all(open(a, 'rb').read() == open(b, 'rb').read() for a, b in zip(a_outs, b_outs))
        ok = ok and same
        for _ in range(args.reps):
            legs['mixes'].append(leg_mixes(seg, files, a_dir, spec)[0])
            legs['twins'].append(leg_twins(seg, files, b_dir, t_dir, spec)[0])
        entry = {'mixes_spec': SETS[name], 'mix_hours_per_leg': hours, 'generate_s': round(gen_s, 2),
                 'file_bytes': os.path.getsize(files[0]), 'csv_identical': same}
        for leg, runs in legs.items():
            entry[leg] = {'s_runs': runs, 'mix_h_per_s_median': hours / float(np.median(runs)),
                          'mix_h_per_s_spread': [hours / max(runs), hours / min(runs)]}
        entry['mixes_vs_twins'] = float(np.median(legs['twins'])) / float(np.median(legs['mixes']))
        entry['mixes']['resample_kernel'] = profiled(seg, lambda: leg_mixes(seg, files, a_dir, spec))
        entry['twins']['resample_kernel'] = profiled(seg, lambda: leg_twins(seg, files, b_dir, t_dir, spec))
        result['sets'][name] = entry
        print('%-20s mixes %.2f / twins %.2f mix-hours/s (medians of %d), CSVs identical: %s, resample_kernel %s / %s' % (
              name, entry['mixes']['mix_h_per_s_median'], entry['twins']['mix_h_per_s_median'], args.reps, same,
              entry['mixes']['resample_kernel'], entry['twins']['resample_kernel']), flush=True)
        for d in (a_dir, b_dir, t_dir):
            shutil.rmtree(d, ignore_errors=True)
        for f in files:
            os.remove(f)
    seg.close()
    path = args.out or os.path.join(ROOT, 'profiles', 'mixes.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
