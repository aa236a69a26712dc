#!/usr/bin/env python3
"""File sets (one mono file per channel) against the interleaved twins they stand for: batch_process on the sets, on twins
interleaved and written by the host first, and on twins that already exist.

Three cases of `--files` recordings x `--minutes` (bench.py's generator; channel c is channel 0 delayed by 1.5 s * c and
attenuated).  The members of one recording are generated and copied:
  pairs_8k_mixes     two 8 kHz mono PCM16 WAVs per recording (a call logger's -in / -out), mixes 0,1,0+1
  tracks_48k_mixes   eight 48 kHz mono PCM16 WAVs per recording (one per track), mixes 0+1,2+3,4+5,6+7
  tracks_48k_auto    the same recordings with channels='auto'
Timed per case, `--reps` times, alternated, after one warm-up of each leg:
  sets    a: seg.batch_process(sets, outs, ...): the members uploaded as stored, read by the SET kernels
  host    b: the route it replaces: io.decode_set per recording (host decode of every member, numpy interleave), the twin written
          as a WAV (inside the timed region), then seg.batch_process on the twins
  twins   c: seg.batch_process on twins that already exist (the files leg b wrote last): the floor -- the same arithmetic over
          interleaved reads, nothing to interleave
Audio-hours count output-hours (mix-hours; recording-hours for 'auto').  Every CSV of a, b and c must be byte-identical.
resample_kernel's and survey_kernel's time per launch come from the library profiler (ctx.prof_instances of every worker
context) over one further pass of legs a and c.  Writes one JSON (default profiles/sets.json) and prints it.
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

CASES = {'pairs_8k_mixes': (2, 8000, '0,1,0+1'), 'tracks_48k_mixes': (8, 48000, '0+1,2+3,4+5,6+7'), 'tracks_48k_auto': (8, 48000, None)}


def generate(tmp, name, nfiles, minutes):
    """-> one io.FileSet per recording: `nfiles` copies of the members of one recording of `minutes`."""
    import bench
    import wavgen
    from inaspeechsegmenter_amd.io import FileSet
    nch, sr, _ = CASES[name]
    n = int(minutes * 60 * 16000)
    left = bench.synth_recording_numpy(0, n).astype(np.int64)
    sets = []
    first = []
    for c in range(nch):
        x = (np.roll(left, 24000 * c) * (10 - c) // 10).astype('<i2')
        x = np.repeat(x, 3) if sr == 48000 else x[::2]               # held / dropped samples: content is not the point
        first.append(wavgen.write_wav(os.path.join(tmp, f'{name}_0.ch{c}.wav'), np.ascontiguousarray(x), sr, 'i16'))
    sets.append(FileSet(first, name=f'{name}_0'))
    for k in range(1, nfiles):
        members = [f.replace(f'{name}_0.', f'{name}_{k}.') for f in first]
        for a, b in zip(first, members):
            shutil.copyfile(a, b)
        sets.append(FileSet(members, name=f'{name}_{k}'))
    return sets


def run(seg, inputs, stems, odir, spec):
    """batch_process over `inputs` -> (seconds, the CSVs written, the decisions of 'auto')."""
    from inaspeechsegmenter_amd import io as iss_io
    os.makedirs(odir, exist_ok=True)
    outs = [os.path.join(odir, s + '.csv') for s in stems]
    decisions = []
    kw = {'channels': 'auto', 'decisions': decisions} if spec is None else {'mixes': spec}
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(inputs, outs, **kw)
    dt = time.perf_counter() - t
    per = 1 if spec is None else len(spec)
    assert nb == per * len(inputs), lmsg
    return dt, outs if spec is None else [iss_io.mix_name(o, k) for o in outs for k in range(per)], decisions


def write_twins(sets, tdir):
    import wavgen
    from inaspeechsegmenter_amd import io as iss_io
    os.makedirs(tdir, exist_ok=True)
    twins = []
    for s in sets:
        x, sr = iss_io.decode_set(s)
        twins.append(wavgen.write_wav(os.path.join(tdir, s.name + '.wav'), x, sr, 'i16'))
    return twins


def profiled(seg, leg):
    """-> per kernel {'launches', 'total_ms', 'ms_per_launch'} of resample_kernel and survey_kernel over one pass of `leg()`."""
    ctxs = [w.ctx for w in seg.__dict__.get('_pipeline_workers', [])] or [seg.ctx]
    for c in ctxs:
        c.prof_enable(True)
        c.prof_reset()
    leg()
    out = {}
    for kernel in ('resample_kernel', 'survey_kernel'):
        calls, total = 0, 0.0
        for c in ctxs:
            for inst in c.prof_instances():
                if inst['kernel'] == kernel:
                    calls += inst['launches']
                    total += inst['ms']
        out[kernel] = {'launches': calls, 'total_ms': total, 'ms_per_launch': total / calls if calls else None}
    for c in ctxs:
        c.prof_enable(False)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cases', default=','.join(CASES), help='comma-separated subset of: ' + ', '.join(CASES))
    ap.add_argument('--out', default=None)
    ap.add_argument('--tmp', default=None, help='directory for the generated audio (default: a fresh temporary one)')
    args = ap.parse_args(argv)

    from inaspeechsegmenter_amd import Segmenter
    from inaspeechsegmenter_amd import resample as R
    tmp = tempfile.mkdtemp(prefix='bench_sets_', dir=args.tmp)
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'reps': args.reps, 'staging': 'channel-major', 'cases': {}}
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ok = True
    for name in args.cases.split(','):
        nch, sr, text = CASES[name]
        spec = None if text is None else R.parse_mixes(text)
        hours = (1 if spec is None else len(spec)) * args.files * args.minutes / 60.0
        t0 = time.time()
        sets = generate(tmp, name, args.files, args.minutes)
        gen_s = time.time() - t0
        stems = [s.name for s in sets]
        a_dir, b_dir, c_dir, t_dir = (os.path.join(tmp, d, name) for d in ('out_a', 'out_b', 'out_c', 'twins'))

        def leg_a():
            return run(seg, sets, stems, a_dir, spec)

        def leg_b():
            t = time.perf_counter()
            twins = write_twins(sets, t_dir)
            dt, outs, dec = run(seg, twins, stems, b_dir, spec)
            return time.perf_counter() - t, outs, dec

        def leg_c():
            return run(seg, [os.path.join(t_dir, s + '.wav') for s in stems], stems, c_dir, spec)

        _, a_outs, a_dec = leg_a()                                   # warm-up of each leg, and the CSVs compared
        _, b_outs, _ = leg_b()
        _, c_outs, c_dec = leg_c()
        same = len(a_outs) == len(b_outs) == len(c_outs) and all(
            open(a, 'rb').read() == open(b, 'rb').read() == open(c, 'rb').read() for a, b, c in zip(a_outs, b_outs, c_outs))
        if spec is None:                                             # (and the same decisions: every recording holds the same samples)
            same = same and sorted(str(m) for _, _, m in a_dec) == sorted(str(m) for _, _, m in c_dec)
        ok = ok and same
        legs = {'sets': [], 'host': [], 'twins': []}
        for _ in range(args.reps):
            legs['sets'].append(leg_a()[0])
            legs['host'].append(leg_b()[0])
            legs['twins'].append(leg_c()[0])
        entry = {'members': nch, 'rate': sr, 'mixes_spec': text or "channels='auto'", 'output_hours_per_leg': hours,
                 'generate_s': round(gen_s, 2), 'member_bytes': os.path.getsize(sets[0].members[0]), 'csv_identical': same}
        if spec is None:
            entry['decisions'] = sorted({str(m) for _, _, m in a_dec})
        for leg, runs in legs.items():
            entry[leg] = {'s_runs': runs, 'h_per_s_median': hours / float(np.median(runs)),
                          'h_per_s_spread': [hours / max(runs), hours / min(runs)]}
        entry['sets_vs_host'] = float(np.median(legs['host'])) / float(np.median(legs['sets']))
        entry['sets_vs_twins'] = float(np.median(legs['twins'])) / float(np.median(legs['sets']))
        entry['sets']['kernels'] = profiled(seg, leg_a)
        entry['twins']['kernels'] = profiled(seg, leg_c)
        result['cases'][name] = entry
        print('%-18s sets %.2f / host %.2f / twins %.2f output-hours/s (medians of %d), CSVs identical: %s, kernels sets %s twins %s' % (
              name, entry['sets']['h_per_s_median'], entry['host']['h_per_s_median'], entry['twins']['h_per_s_median'], args.reps,
              same, entry['sets']['kernels'], entry['twins']['kernels']), flush=True)
        for d in (a_dir, b_dir, c_dir, t_dir):
            shutil.rmtree(d, ignore_errors=True)
        for s in sets:
            for m in s.members:
                os.remove(m)
    seg.close()
    path = args.out or os.path.join(ROOT, 'profiles', 'sets.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
