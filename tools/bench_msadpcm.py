#!/usr/bin/env python3
"""Microsoft ADPCM without ffmpeg: decoded on the device against the host build and the PCM16 twins; and the IMA instantiation
of the shared kernel against another tree (A/B).

Default mode.  N x `--minutes` of 8 kHz mono (bench.py's generator at 16 kHz, every second sample; `--distinct` different
recordings, cycled) are written to a temporary directory as Microsoft ADPCM WAV (256-byte blocks, tests/msadpcmgen.py's
encoder) and as the PCM16 WAV twin of each (the host build's decode).  Segmenter(ffmpeg=None, resample=True).batch_process in
ONE process, legs alternated, `--reps` repeats each after a warm-up:
  ms        the stored blocks go to the device (adpcm_decode_kernel<MS> + resample)
  ms_twin   the PCM16 WAV twins
  ms_host   the same files expanded on the host in the decode threads (sndfmt._HOST_DECODE: iss_msadpcm_decode_host)
Kernel time per launch: the library profiler's event brackets (iss_prof) around `--kernel-reps` direct calls that decode and
resample all N files in one launch.  Writes one JSON (default profiles/msadpcm_<n>.json).

--ab TREE.  The IMA instantiation, this tree against TREE (a checkout of the parent commit with its library built), alternated:
3 invocations a side, `--kernel-reps` profiled runs each, every invocation a fresh process that imports the package of its own
tree.  One iss_adpcm_decode call: N x `--minutes` of 8 kHz mono IMA ADPCM in 256-byte blocks, staged and resampled.  Writes
profiles/msadpcm_ab.json.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _use_tree(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'tests'))


def recording(i, minutes):
    import bench
    n8 = int(minutes * 60 * 8000)
    x = np.asarray(bench.synth_recording_numpy(i, 2 * n8)[::2])
    return x.astype(np.int16) if np.abs(x).max() > 2 else np.round(x * 32767).astype(np.int16)


def make_files(tmp, nfiles, minutes, distinct):
    import msadpcmgen as M
    import wavgen
    from inaspeechsegmenter_amd import _native
    sets = {'ms': [], 'ms_twin': []}
    made = []
    for i in range(min(distinct, nfiles)):
        pcm = recording(i, minutes)
        blocks = M.encode(pcm, 256)
        twin, st = _native.msadpcm_decode_host(np.frombuffer(blocks, np.uint8), len(blocks) // 256, 1, 256, len(pcm))
        assert not st.any()
        made.append((blocks, twin, len(pcm)))
    for i in range(nfiles):
        blocks, twin, n = made[i % len(made)]
        sets['ms'].append(M.write_riff(os.path.join(tmp, f'r{i}_ms.wav'), M.fmt(8000, 1, 256), blocks, fact=n))
        sets['ms_twin'].append(wavgen.write_wav(os.path.join(tmp, f'r{i}_twin.wav'), twin, 8000, 'i16'))
    return sets


def one_launch(ctx, sounds, reps, kernel):
    """`reps` profiled calls (after a warm-up) that decode and resample every sound in one launch -> [kernel ms per call]."""
    from inaspeechsegmenter_amd import sources
    srcs = [s.source(resample=True) for s in sounds]
    placed, pos = [], 0
    for s in srcs:
        placed.append((s, pos))
        pos += s.stride
    runs = []
    for k in range(reps + 1):
        ctx.prof_enable(True)
        ctx.prof_reset()
        g = sources.Group(ctx, type(srcs[0]), placed).launch(pos)
        ctx.synchronize()
        g.check()
        ms = [d['ms'] for d in ctx.prof_instances() if d['kernel'].split('(')[0] == kernel]
        ctx.prof_enable(False)
        assert len(ms) == 1, ms
        if k:
            runs.append(ms[0])
    return runs


def ab_child(tree, nfiles, minutes, distinct, reps):
    """In a process of its own: the IMA call through the package of `tree` -> one JSON line."""
    _use_tree(tree)
    import sndgen
    from inaspeechsegmenter_amd import _native, sndfmt
    assert os.path.dirname(os.path.abspath(_native.__file__)) == os.path.join(os.path.abspath(tree), 'inaspeechsegmenter_amd')
    made = []
    for i in range(min(distinct, nfiles)):
        pcm = recording(i, minutes)
        made.append((np.frombuffer(sndgen.ima_encode(pcm, 256), np.uint8), len(pcm)))
    sounds = [sndfmt.Sound(f'r{i}.wav', 8000, 1, 'ima', False, made[i % len(made)][0], 0, frames=made[i % len(made)][1],
                           block_align=256, spb=505) for i in range(nfiles)]
    ctx = _native.Context(0)
    runs = one_launch(ctx, sounds, reps, 'adpcm_decode_kernel')
    ctx.close()
    print('AB ' + json.dumps({'tree': tree, 'lib': _native.LIB_PATH, 'ms_runs': runs}))
    return 0


def ab(args):
    parent = os.path.abspath(args.ab)
    runs = {parent: [], ROOT: []}
    for inv in range(3):
        for tree in (parent, ROOT):
            cmd = [sys.executable, os.path.abspath(__file__), '--ab-child', tree, '--files', str(args.files), '--minutes', str(args.minutes),
                   '--distinct', str(args.distinct), '--kernel-reps', str(args.kernel_reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=tree)
            if r.returncode != 0:
                print(r.stdout.decode(errors='replace')[-2000:])
                return r.returncode
            line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('AB ')][-1]
            runs[tree] += json.loads(line[3:])['ms_runs']
    p, n = runs[parent], runs[ROOT]
    spread = max(p) - min(p)
    res = {'method': 'parent tree (its own Python and library) and this tree alternated on one MI355X, 3 invocations each, '
                     f'{args.kernel_reps} profiled kernel runs per invocation ({3 * args.kernel_reps} runs a side), the library '
                     'profiler\'s event brackets; unwindowed calls only',
           'tool': f'tools/bench_msadpcm.py --ab <parent tree> --files {args.files} --minutes {args.minutes} --distinct {args.distinct}: one '
                   f'iss_adpcm_decode call, {args.files} x {args.minutes} min of 8 kHz mono IMA ADPCM in 256-byte blocks, staged and resampled',
           'margin': 'the spread of the parent\'s own runs (slowest - fastest); the kernel holds when the new median is not above the '
                     'parent median by more than it',
           'kernels': {'adpcm_decode_kernel': {
               'parent_ms_runs': p, 'new_ms_runs': n, 'parent_median_ms': float(np.median(p)), 'new_median_ms': float(np.median(n)),
               'parent_spread_ms': spread, 'new_spread_ms': max(n) - min(n),
               'new_minus_parent_median_ms': float(np.median(n) - np.median(p)),
               'holds': bool(np.median(n) - np.median(p) <= spread)}}}
    path = args.out or os.path.join(ROOT, 'profiles', 'msadpcm_ab.json')
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res['kernels']))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--minutes', type=float, default=5.0)
    ap.add_argument('--distinct', type=int, default=8, help='different recordings among the files (cycled)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-reps', type=int, default=5)
    ap.add_argument('--ab', default=None, metavar='TREE')
    ap.add_argument('--ab-child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if args.ab_child:
        return ab_child(args.ab_child, args.files, args.minutes, args.distinct, args.kernel_reps)
    if args.ab:
        return ab(args)

    _use_tree(ROOT)
    from inaspeechsegmenter_amd import Segmenter, sndfmt
    tmp = tempfile.mkdtemp(prefix='bench_msadpcm_')
    t0 = time.time()
    sets = make_files(tmp, args.files, args.minutes, args.distinct)
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

    names = ('ms', 'ms_twin', 'ms_host')
    for name in names:                                                    # warm-up: workers, code objects, filters
        run(name, 2)
    legs, outs = {n: [] for n in names}, {}
    for rep in range(args.reps):                                          # alternate the legs
        for name in names:
            t, outs[name] = run(name)
            legs[name].append(t)
    same = all(open(a).read() == open(b).read() == open(c).read() for a, b, c in zip(outs['ms'], outs['ms_twin'], outs['ms_host']))
    sounds = [sndfmt.parse(open(f, 'rb').read(), f) for f in sets['ms']]
    kruns = one_launch(seg.ctx, sounds, args.kernel_reps, 'msadpcm_decode_kernel')
    nblocks = sum(s.nblocks for s in sounds)
    seg.close()

    res = {'files': args.files, 'minutes_per_file': args.minutes,
           'source': f'8 kHz mono: Microsoft ADPCM WAV (256-byte blocks, 500 samples each), PCM16 twins; {min(args.distinct, args.files)} '
                     'different recordings, cycled',
           'audio_hours': hours, 'generate_s': round(gen_s, 2), 'reps': args.reps, 'leg_s_runs': legs,
           'h_per_s': {n: hours / float(np.median(v)) for n, v in legs.items()},
           'h_per_s_spread': {n: [hours / max(v), hours / min(v)] for n, v in legs.items()},
           'csv_identical_across_legs': same,
           'kernel': {'name': 'adpcm_decode_kernel<CODER_MS, false> (profiled as msadpcm_decode_kernel)', 'source': 'iss_prof event brackets',
                      'launch': f'one iss_msadpcm_decode call over all {args.files} files: {nblocks} blocks, staged and resampled',
                      'ms_runs': kruns, 'median_ms': float(np.median(kruns)), 'spread_ms': max(kruns) - min(kruns),
                      'blocks': nblocks, 'stored_bytes': nblocks * 256,
                      'stored_GB_per_s': nblocks * 256 / (float(np.median(kruns)) * 1e-3) / 1e9,
                      'samples_per_s': nblocks * 500 / (float(np.median(kruns)) * 1e-3)}}
    for n, v in legs.items():
        print('%-10s %6.2f audio-hours/s (median of %d; %.2f .. %.2f)' % (n, hours / float(np.median(v)), len(v), hours / max(v), hours / min(v)))
    path = args.out or os.path.join(ROOT, 'profiles', f'msadpcm_{args.files}.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
