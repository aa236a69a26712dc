#!/usr/bin/env python3
"""Survey-guided downmix of multi-channel files: batch_process(channels='auto') against the route it replaces and its floor.

Three sets of `--files` x `--minutes`, the sets of tools/bench_survey.py; in each a third of the files are damaged:
  wav_48k_8ch          48 kHz PCM16 WAV, 8 channels; damaged: channel 3 at digital zero, channel 1 = channel 0 inverted
  flac_16k_left_side   16 kHz FLAC, 2 channels;      damaged: channel 1 = channel 0 inverted (two channels hold no dead one beside)
  ima_8k               8 kHz IMA ADPCM, 2 channels;  damaged: likewise
Timed per set, `--reps` times a leg, alternated, after one warm-up of each leg:
  auto    1: seg.batch_process(files, outs, channels='auto')
  route   2: what it replaces: seg.survey_files(files), then per file segment_mixes(f, [survey.safe_mix()]) or the plain call
  plain   3: seg.batch_process(files, outs): the floor -- the same work without a survey, and wrong for the damaged files
Every CSV of leg 1 must be byte-identical to leg 2's.  Per leg: the payload bytes uploaded (iss_upload_stats over every worker
context).  Kernel times come from the library profiler over one further pass of leg 1.  Writes one JSON (default
profiles/auto.json) and prints it.
"""
import argparse
import filecmp
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

SETS = ('wav_48k_8ch', 'flac_16k_left_side', 'ima_8k')
KERNELS = ('survey_kernel', 'survey_reduce_kernel', 'resample_kernel', 'flac_decode_kernel', 'adpcm_decode_kernel')


def generate(tmp, name, nfiles, minutes):
    """-> the paths of `nfiles` files of `minutes` of set `name`: copies of a healthy one, every third a copy of a damaged one."""
    import bench
    import flacgen
    import sndgen
    import wavgen
    n = int(minutes * 60 * 16000)
    left = bench.synth_recording_numpy(0, n).astype(np.int64)
    nch = 8 if name == 'wav_48k_8ch' else 2
    ext = '.flac' if name.startswith('flac') else '.wav'
    firsts = []
    for damaged in (False, True):
        x = np.stack([np.roll(left, 24000 * c) * (10 - c) // 10 for c in range(nch)], axis=1)
        if damaged:
            x[:, 1] = -(x[:, 0] * 9 // 10)
            if nch > 2:
                x[:, 3] = 0
        first = os.path.join(tmp, f'{name}_{"bad" if damaged else "ok"}{ext}')
        if name == 'wav_48k_8ch':
            wavgen.write_wav(first, np.repeat(x, 3, axis=0).astype('<i2'), 48000, 'i16')    # held samples: content is not the point
        elif name == 'flac_16k_left_side':
            flacgen.write(first, x, 16000, 16, channel_mode='left_side', subframe={'type': 'fixed', 'order': 2})
        else:
            sndgen.write(first, 'wav', 'ima', False, x[::2] / 32768.0, 8000, block_align=512)
        firsts.append(first)
    files = []
    for k in range(nfiles):
        files.append(os.path.join(tmp, f'{name}_{k}{ext}'))
        shutil.copyfile(firsts[1 if k % 3 == 2 else 0], files[-1])
    for f in firsts:
        os.remove(f)
    return files


def outputs(odir, files):
    os.makedirs(odir, exist_ok=True)
    return [os.path.join(odir, os.path.splitext(os.path.basename(f))[0] + '.csv') for f in files]


def leg_auto(seg, files, odir):
    outs, decisions = outputs(odir, files), []
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='auto', decisions=decisions)
    dt = time.perf_counter() - t
    assert nb == len(files), lmsg
    return dt, outs, decisions


def leg_route(seg, files, odir):
    from inaspeechsegmenter_amd.export_funcs import seg2csv
    outs = outputs(odir, files)
    t = time.perf_counter()
    for f, o, s in zip(files, outs, seg.survey_files(files)):
        mix = s.safe_mix()
        seg2csv(seg(f) if mix is None else seg.segment_mixes(f, [mix])[0], o)
    return time.perf_counter() - t, outs


def leg_plain(seg, files, odir):
    outs = outputs(odir, files)
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(files, outs)
    dt = time.perf_counter() - t
    assert nb == len(files), lmsg
    return dt, outs


def contexts(seg):
    from inaspeechsegmenter_amd import pipeline
    return [w.ctx for w in pipeline._workers(seg, pipeline.DEFAULT_WORKERS)]


def uploaded(seg):
    return sum(c.upload_stats()[1] for c in contexts(seg))


def profiled(seg, files, odir):
    """-> the front-end kernels over one pass of leg 1, summed over the worker contexts, from the library profiler."""
    for c in contexts(seg):
        c.prof_enable(True)
        c.prof_reset()
    leg_auto(seg, files, odir)
    out = {}
    for c in contexts(seg):
        for inst in c.prof_instances():
            if inst['kernel'] in KERNELS:
                k = out.setdefault(inst['kernel'], {'launches': 0, 'total_ms': 0.0})
                k['launches'] += inst['launches']
                k['total_ms'] += inst['ms']
        c.prof_enable(False)
    for k in out.values():
        k['ms_per_launch'] = k['total_ms'] / max(k['launches'], 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sets', default=','.join(SETS), help='comma-separated subset of: ' + ', '.join(SETS))
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    from inaspeechsegmenter_amd import Segmenter
    tmp = tempfile.mkdtemp(prefix='bench_auto_')
    path = args.out or os.path.join(ROOT, 'profiles', 'auto.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'reps': args.reps, 'sets': {}}
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ok = True
    for name in args.sets.split(','):
        hours = args.files * args.minutes / 60.0
        files = generate(tmp, name, args.files, args.minutes)
        dirs = {leg: os.path.join(tmp, f'{name}_{leg}') for leg in ('auto', 'route', 'plain')}
        legs = {'auto': lambda: leg_auto(seg, files, dirs['auto']), 'route': lambda: leg_route(seg, files, dirs['route']),
                'plain': lambda: leg_plain(seg, files, dirs['plain'])}
        runs, nbytes, outs, decisions = {leg: [] for leg in legs}, {}, {}, None
        for leg, run in legs.items():                                  # warm-up, the outputs compared, the bytes a leg uploads
            before = uploaded(seg)
            got = run()
            nbytes[leg], outs[leg] = uploaded(seg) - before, got[1]
            if leg == 'auto':
                decisions = got[2]
        same = all(filecmp.cmp(a, b, shallow=False) for a, b in zip(outs['auto'], outs['route']))
        differ = sum(not filecmp.cmp(a, b, shallow=False) for a, b in zip(outs['auto'], outs['plain']))
        ok = ok and same
        for _ in range(args.reps):
            for leg, run in legs.items():
                runs[leg].append(run()[0])
            print('%-20s %s' % (name, ', '.join('%s %.3f s' % (leg, runs[leg][-1]) for leg in legs)), flush=True)
        entry = {'file_hours_per_leg': hours, 'file_bytes': os.path.getsize(files[0]), 'csv_auto_equals_route': same,
                 'csv_auto_differs_from_plain': differ, 'files_with_a_mix': sum(d[2] is not None for d in decisions),
                 'mixes': sorted({repr(d[2]) for d in decisions if d[2] is not None})}
        for leg in legs:
            entry[leg] = {'s_runs': runs[leg], 's_median': float(np.median(runs[leg])), 'payload_bytes_uploaded': nbytes[leg],
                          'file_h_per_s_median': hours / float(np.median(runs[leg])),
                          'file_h_per_s_spread': [hours / max(runs[leg]), hours / min(runs[leg])]}
        entry['route_vs_auto'] = entry['route']['s_median'] / entry['auto']['s_median']
        entry['auto_vs_plain'] = entry['auto']['s_median'] / entry['plain']['s_median']
        entry['auto']['kernels'] = profiled(seg, files, dirs['auto'])
        result['sets'][name] = entry
        print('%-20s %s' % (name, json.dumps(entry)), flush=True)
        for f in files:
            os.remove(f)
        with open(path, 'w') as f:                                     # (after every set: a run cut short leaves what it measured)
            json.dump(result, f, indent=1)
    seg.close()
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
