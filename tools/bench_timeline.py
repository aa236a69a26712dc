#!/usr/bin/env python3
"""Downmixes that change over time: batch_process(channels='auto', auto_block_sec=10) against the route it replaces and its floor.

Three sets of `--files` x `--minutes` of 2-channel 48 kHz audio -- PCM16 WAV, and its FLAC and IMA ADPCM twins --, every third file
carrying a stretch whose right channel is inverted and a stretch whose right channel is dead (one minute each, a fifth of the file
where it is shorter than five minutes).  Timed per set, `--reps` times a leg, alternated, after one warm-up of each leg:
  timeline  1: seg.batch_process(files, outs, channels='auto', auto_block_sec=--block)
  route     2: what it replaces: io.decode_auto_timeline on the host, one mono WAV written per file, then batch_process on those
  auto      3: the floor: plain channels='auto', one decision per file, which segments the damaged stretches wrongly
  steady    4: leg 1 with auto_rule='steady' (one divisor per file, carried polarity, run boundaries cross-faded over 50 ms);
               its CSVs are compared once, untimed, with its own host route: io.decode_auto_timeline(rule='steady')
Every CSV of leg 1 must be byte-identical to leg 2's, every one of leg 4 to its host route's; how many differ from leg 3's is reported.  Kernel times come from the library
profiler over one further pass of leg 1 (survey_reduce_blocks_kernel next to survey_reduce_kernel among them).
Then, in the same process, the SCHED instantiation of resample_kernel against the MIX instantiation: one file's bytes, the same
single mix, as a one-run schedule, as a schedule of one run per `--block` seconds (all naming that mix), and as a mix call; 15
alternated runs a side, kernel time from the profiler; both medians and the MIX side's own spread.  Likewise the FADE instantiation
against SCHED: a six-run schedule as it is, and with 50 ms fades at its five boundaries.
Writes one JSON (default profiles/timeline.json) and prints it.
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

from bench_auto import contexts, outputs, uploaded      # noqa: E402  (the conventions of tools/bench_auto.py, written once)

SETS = ('wav_48k', 'flac_48k', 'ima_48k')
KERNELS = ('survey_kernel', 'survey_reduce_kernel', 'survey_reduce_blocks_kernel', 'resample_kernel', 'flac_decode_kernel',
           'adpcm_decode_kernel')
SR = 48000


def stored(minutes, damaged):
    """-> (n, 2) int16 at 48 kHz: bench.py's recording (held samples: content is not the point) and a quieter, delayed copy."""
    import bench
    n = int(minutes * 60 * 16000)
    left = bench.synth_recording_numpy(0, n).astype(np.int64)
    x = np.repeat(np.stack([left, np.roll(left, 160) * 9 // 10], axis=1), 3, axis=0)
    if damaged:
        stretch = min(60 * SR, x.shape[0] // 5)
        x[stretch:2 * stretch, 1] = -x[stretch:2 * stretch, 0]
        x[3 * stretch:4 * stretch, 1] = 0
    return x.astype('<i2')


def generate(tmp, name, nfiles, minutes):
    import flacgen
    import sndgen
    import wavgen
    ext = '.flac' if name.startswith('flac') else '.wav'
    firsts = []
    for damaged in (False, True):
        x = stored(minutes, damaged)
        first = os.path.join(tmp, f'{name}_{"bad" if damaged else "ok"}{ext}')
        if name == 'wav_48k':
            wavgen.write_wav(first, x, SR, 'i16')
        elif name == 'flac_48k':
            flacgen.write(first, x.astype(np.int64), SR, 16, channel_mode='left_side', subframe={'type': 'fixed', 'order': 2})
        else:
            sndgen.write(first, 'wav', 'ima', False, x / 32768.0, SR, block_align=512)
        firsts.append(first)
    files = []
    for k in range(nfiles):
        files.append(os.path.join(tmp, f'{name}_{k}{ext}'))
        shutil.copyfile(firsts[1 if k % 3 == 2 else 0], files[-1])
    for f in firsts:
        os.remove(f)
    return files


def leg_timeline(seg, files, odir, block, **rule):
    outs, decisions = outputs(odir, files), []
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='auto', auto_block_sec=block, decisions=decisions, **rule)
    dt = time.perf_counter() - t
    assert nb == len(files), lmsg
    return dt, outs, decisions


def leg_route(seg, files, odir, block, **rule):
    import wavgen
    from inaspeechsegmenter_amd import io as iss_io
    outs = outputs(odir, files)
    t = time.perf_counter()
    monos = []
    for f in files:
        monos.append(os.path.join(odir, os.path.basename(f) + '.mono.wav'))
        wavgen.write_wav(monos[-1], iss_io.decode_auto_timeline(f, block, **rule)[0], 16000, 'i16')
    _, nb, _, lmsg = seg.batch_process(monos, outs)
    dt = time.perf_counter() - t
    assert nb == len(files), lmsg
    return dt, outs


def leg_auto(seg, files, odir, block):
    outs = outputs(odir, files)
    t = time.perf_counter()
    _, nb, _, lmsg = seg.batch_process(files, outs, channels='auto')
    dt = time.perf_counter() - t
    assert nb == len(files), lmsg
    return dt, outs


def profiled(seg, run):
    for c in contexts(seg):
        c.prof_enable(True)
        c.prof_reset()
    run()
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


def kernel_ab(seg, minutes, block, runs=15):
    """The SCHED instantiation against the MIX instantiation on the same bytes with the same single mix, kernel ms per launch."""
    from inaspeechsegmenter_amd.resample import Mix
    ctx = seg.ctx
    x = stored(minutes, True)
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, SR, 0, 0)
    nout = job[-1]
    mix = Mix(((0, 1.0), (1, -1.0)), 2.0)
    step = int(block * SR)
    sides = {'mix': lambda: ctx.resample(src, [job], n_signal=nout, mixes=[(nout, [mix])]),
             'sched_one_run': lambda: ctx.resample_sched(src, [job], [[(0, mix)]], n_signal=nout),
             'sched_block_runs': lambda: ctx.resample_sched(src, [job], [[(b, mix) for b in range(0, x.shape[0], step)]], n_signal=nout)}
    got = {}
    for name, run in sides.items():                                    # warm-up, and the three write the same samples
        run()
        got[name] = ctx.get_signal_pcm16(0, nout)
    assert all(np.array_equal(got['mix'], g) for g in got.values())
    ms = {name: [] for name in sides}
    ctx.prof_enable(True)
    for _ in range(runs):
        for name, run in sides.items():
            ctx.prof_reset()
            run()
            ctx.synchronize()
            ms[name].append(sum(i['ms'] for i in ctx.prof_instances() if i['kernel'] == 'resample_kernel'))
    ctx.prof_enable(False)
    out = {'frames': int(x.shape[0]), 'runs_a_side': runs, 'block_runs': len(range(0, x.shape[0], step))}
    for name, v in ms.items():
        out[name] = {'ms_median': float(np.median(v)), 'ms_spread': [float(min(v)), float(max(v))]}
    for name in ('sched_one_run', 'sched_block_runs'):
        out[name]['vs_mix'] = out[name]['ms_median'] / out['mix']['ms_median']
    return out


def fade_ab(seg, minutes, runs=15):
    """The FADE instantiation against SCHED: six runs over one file, hard cuts against 50 ms fades, kernel ms per launch."""
    from inaspeechsegmenter_amd.resample import Mix, Schedule, fade_halves
    ctx = seg.ctx
    x = stored(minutes, True)
    src = x.reshape(-1).view(np.uint8)
    job = ctx.resample_job(x, SR, 0, 0)
    nout = job[-1]
    mixes = [None, Mix(((0, 1.0), (1, -1.0)), 2.0)]
    begins = [k * (x.shape[0] // 6) for k in range(6)]
    hard = Schedule([(b, mixes[k % 2]) for k, b in enumerate(begins)])
    faded = Schedule(hard.runs, fade_halves(begins, 0.05, SR))
    sides = {'sched': lambda: ctx.resample_sched(src, [job], [hard], n_signal=nout),
             'fade': lambda: ctx.resample_sched(src, [job], [faded], n_signal=nout)}
    for run in sides.values():
        run()
    ms = {name: [] for name in sides}
    ctx.prof_enable(True)
    for _ in range(runs):
        for name, run in sides.items():
            ctx.prof_reset()
            run()
            ctx.synchronize()
            ms[name].append(sum(i['ms'] for i in ctx.prof_instances() if i['kernel'] == 'resample_kernel'))
    ctx.prof_enable(False)
    out = {'frames': int(x.shape[0]), 'runs_a_side': runs, 'schedule_runs': 6, 'fade_half_widths': list(faded.fades)}
    for name, v in ms.items():
        out[name] = {'ms_median': float(np.median(v)), 'ms_spread': [float(min(v)), float(max(v))]}
    out['fade_vs_sched'] = out['fade']['ms_median'] / out['sched']['ms_median']
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--block', type=float, default=10.0)
    ap.add_argument('--sets', default=','.join(SETS), help='comma-separated subset of: ' + ', '.join(SETS))
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)

    from inaspeechsegmenter_amd import Segmenter
    tmp = tempfile.mkdtemp(prefix='bench_timeline_')
    path = args.out or os.path.join(ROOT, 'profiles', 'timeline.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    result = {'files': args.files, 'minutes_per_file': args.minutes, 'reps': args.reps, 'block_sec': args.block, 'sets': {}}
    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ok = True
    for name in [s for s in args.sets.split(',') if s]:
        hours = args.files * args.minutes / 60.0
        files = generate(tmp, name, args.files, args.minutes)
        dirs = {leg: os.path.join(tmp, f'{name}_{leg}') for leg in ('timeline', 'route', 'auto', 'steady', 'steady_route')}
        legs = {'timeline': lambda: leg_timeline(seg, files, dirs['timeline'], args.block),
                'route': lambda: leg_route(seg, files, dirs['route'], args.block), 'auto': lambda: leg_auto(seg, files, dirs['auto'], args.block),
                'steady': lambda: leg_timeline(seg, files, dirs['steady'], args.block, auto_rule='steady')}
        runs, nbytes, outs, decisions = {leg: [] for leg in legs}, {}, {}, None
        for leg, run in legs.items():                                  # warm-up, the outputs compared, the bytes a leg uploads
            before = uploaded(seg)
            got = run()
            nbytes[leg], outs[leg] = uploaded(seg) - before, got[1]
            if leg == 'timeline':
                decisions = got[2]
            if leg == 'steady':
                steady = got[2]
        twin = leg_route(seg, files, dirs['steady_route'], args.block, rule='steady')[1]      # once, untimed: the steady leg's own host route
        steady_same = all(filecmp.cmp(a, b, shallow=False) for a, b in zip(outs['steady'], twin))
        ok = ok and steady_same
        same = all(filecmp.cmp(a, b, shallow=False) for a, b in zip(outs['timeline'], outs['route']))
        differ = sum(not filecmp.cmp(a, b, shallow=False) for a, b in zip(outs['timeline'], outs['auto']))
        ok = ok and same
        for _ in range(args.reps):
            for leg, run in legs.items():
                runs[leg].append(run()[0])
            print('%-10s %s' % (name, ', '.join('%s %.3f s' % (leg, runs[leg][-1]) for leg in legs)), flush=True)
        entry = {'file_hours_per_leg': hours, 'file_bytes': os.path.getsize(files[0]), 'csv_timeline_equals_route': same,
                 'csv_timeline_differs_from_auto': differ, 'files_with_more_than_one_run': sum(len(d[2]) > 1 for d in decisions),
                 'schedules': sorted({repr(d[2]) for d in decisions if len(d[2]) > 1}),
                 'csv_steady_equals_its_host_route': steady_same,
                 'csv_steady_differs_from_timeline': sum(not filecmp.cmp(a, b, shallow=False) for a, b in zip(outs['steady'], outs['timeline'])),
                 'steady_schedules': sorted({repr(d[2]) for d in steady if len(d[2]) > 1})}
        for leg in legs:
            entry[leg] = {'s_runs': runs[leg], 's_median': float(np.median(runs[leg])), 'payload_bytes_uploaded': nbytes[leg],
                          'file_h_per_s_median': hours / float(np.median(runs[leg])),
                          'file_h_per_s_spread': [hours / max(runs[leg]), hours / min(runs[leg])]}
        entry['route_vs_timeline'] = entry['route']['s_median'] / entry['timeline']['s_median']
        entry['timeline_vs_auto'] = entry['timeline']['s_median'] / entry['auto']['s_median']
        entry['steady_vs_timeline'] = entry['steady']['s_median'] / entry['timeline']['s_median']
        entry['timeline']['kernels'] = profiled(seg, legs['timeline'])
        result['sets'][name] = entry
        print('%-10s %s' % (name, json.dumps(entry)), flush=True)
        for f in files:
            os.remove(f)
        with open(path, 'w') as f:                                     # (after every set: a run cut short leaves what it measured)
            json.dump(result, f, indent=1)
    result['sched_vs_mix_instantiation'] = kernel_ab(seg, args.minutes, args.block)
    result['fade_vs_sched_instantiation'] = fade_ab(seg, args.minutes)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    seg.close()
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
