#!/usr/bin/env python3
"""Voice femininity scoring of many files: a loop over VoiceFemininityScoring.__call__ against batch_process, same process,
same files, seeded stand-in weights (models='synthetic', the stand-in VAD included).

Input: N seeded synthetic WAVs of about `--seconds` each (the length jittered by up to +-1 s, so that the files' last windows
have different widths as an archive's do), made by bench.py's generator (silence, -30 dBFS noise, a harmonic voiced source,
chords): the stand-in VAD finds speech in them, so the x-vector half runs.  Both paths are warmed up, then timed --reps
times each, alternating.  One more pass of each runs with the library's profiling counters on (iss_prof_*): device time of
the x-vector front end, the ResNet (and gender MLP), and the VAD (the counters read around every VAD call).  Prints ONE
JSON line:
  audio_hours_per_s        per path, best of the timed passes
  resnet_loads             per path and timed pass: ResNet programs of another width loaded in full / on shared parameters
  param_h2d_bytes          per path and timed pass: parameter bytes those loads sent to the device (a full load sends the
                           f32 blob and its bf16 and fp16 hi / lo halves, 3 x the blob; a shared load none)
  prof_ms                  per path: {front_end, resnet, vad} device milliseconds of the profiled pass
  identical                every file's (score, speech_duration, nb_vectors) equal across the two paths

usage: python tools/bench_vfs_batch.py --files 64 [--seconds 180] [--reps 2] [--out profiles/x.json]
"""
import argparse
import json
import os
import platform
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_files(d, nfiles, seconds):
    import bench
    rng = np.random.default_rng(20261015)
    paths, total = [], 0
    for i in range(nfiles):
        n = int(round((seconds + rng.uniform(-1, 1)) * 16000))
        p = os.path.join(d, f'vfs_{i:04d}.wav')
        bench.write_wav(p, bench.synth_recording_numpy(i, n))
        paths.append(p)
        total += n
    return paths, total / 16000


class Counted:
    """Counts the ResNet program loads of the context (window programs other than the full width) and their parameter bytes;
    with `prof`, splits the library's profiling counters into VAD and the rest."""

    def __init__(self, v):
        self.v, self.ctx = v, v.ctx
        self.reset()
        full, shared = self.ctx.cnn_load, self.ctx.cnn_load_shared

        def load(nid, comp):
            if comp.in_shape[0] == 64 and comp.in_shape[1] != 144:
                self.loads['full'] += 1
                self.h2d += 3 * comp.blob.nbytes
            return full(nid, comp)

        def load_shared(nid, src, comp):
            self.loads['shared'] += 1
            return shared(nid, src, comp)
        self.ctx.cnn_load, self.ctx.cnn_load_shared = load, load_shared
        vad = v.vad
        outer = self

        class VadProbe:
            def __call__(self, *a, **k):
                return outer._vad(vad, *a, **k)

            def segment_signal(self, *a, **k):
                return outer._vad(vad.segment_signal, *a, **k)

            def __getattr__(self, name):
                return getattr(vad, name)
        v.vad = VadProbe()

    def reset(self):
        self.loads, self.h2d = {'full': 0, 'shared': 0}, 0
        self.vad_ms = np.zeros(3)

    def _prof(self):
        return np.array([self.ctx.prof_get(k)[0] for k in range(3)])

    def _vad(self, fn, *a, **k):
        if not self.prof:
            return fn(*a, **k)
        p0 = self._prof()
        try:
            return fn(*a, **k)
        finally:
            self.vad_ms += self._prof() - p0

    prof = False


def run(v, counted, paths, batch):
    counted.reset()
    t0 = time.perf_counter()
    res = v.batch_process(paths) if batch else [v(p) for p in paths]
    return res, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=180.0)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--warmup-files', type=int, default=16)
    ap.add_argument('--out', default=None, help='also write the JSON line here')
    args = ap.parse_args()

    import torch
    from inaspeechsegmenter_amd.vfs import VoiceFemininityScoring
    d = tempfile.mkdtemp(prefix='vfs_bench_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    try:
        paths, seconds = write_files(d, args.files, args.seconds)
        v = VoiceFemininityScoring(ffmpeg=None, models='synthetic')
        counted = Counted(v)
        for batch in (False, True):                              # warm-up: both paths, compiled programs and buffers
            run(v, counted, paths[:args.warmup_files], batch)
        out = {'call_loop': {'wall_s': [], 'resnet_loads': [], 'param_h2d_bytes': []},
               'batch_process': {'wall_s': [], 'resnet_loads': [], 'param_h2d_bytes': []}}
        results = {}
        for _ in range(args.reps):
            for name, batch in (('call_loop', False), ('batch_process', True)):
                res, wall = run(v, counted, paths, batch)
                results.setdefault(name, res)
                o = out[name]
                o['wall_s'].append(round(wall, 3))
                o['resnet_loads'].append(dict(counted.loads))
                o['param_h2d_bytes'].append(counted.h2d)
                if res != results[name]:
                    raise SystemExit(f'{name}: results differ between passes')
        counted.prof = True
        v.ctx.prof_enable(True)
        for name, batch in (('call_loop', False), ('batch_process', True)):
            v.ctx.prof_reset()
            run(v, counted, paths, batch)
            tot = counted._prof()
            rest = tot - counted.vad_ms
            out[name]['prof_ms'] = {'front_end': round(rest[1] + rest[2], 2), 'resnet': round(rest[0], 2),
                                    'vad': round(float(counted.vad_ms.sum()), 2)}
        v.ctx.prof_enable(False)
        for name in out:
            out[name]['audio_hours_per_s'] = round(seconds / 3600 / min(out[name]['wall_s']), 4)
        a, b = results['call_loop'], results['batch_process']
        props = torch.cuda.get_device_properties(0)
        box = {'host': platform.node(), 'gpu': torch.cuda.get_device_name(0), 'arch': getattr(props, 'gcnArchName', ''),
               'cus': props.multi_processor_count, 'hbm_gib': round(props.total_memory / 2 ** 30)}
        line = {'tool': 'tools/bench_vfs_batch.py', 'box': box,
                'files': args.files, 'seconds_per_file': args.seconds, 'audio_hours': round(seconds / 3600, 4),
                'files_scored': sum(r[2] > 0 for r in b), 'xvectors_scored': int(sum(r[2] for r in b)),
                **out, 'speedup': round(min(out['call_loop']['wall_s']) / min(out['batch_process']['wall_s']), 3),
                'identical': a == b}
        s = json.dumps(line)
        print(s)
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(s + '\n')
        return 0 if a == b else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
