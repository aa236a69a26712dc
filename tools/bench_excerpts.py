#!/usr/bin/env python3
"""Time ranges of one long file without ffmpeg: Segmenter.segment_excerpts against decoding the whole file.

One `--hours` recording (bench.py's generator, one minute of it repeated) is written as 48 kHz stereo PCM16 WAV, as 16 kHz
mono FLAC (tests/flacgen.py, FIXED order 2) and as 8 kHz mono IMA ADPCM (tests/sndgen.py).  `--excerpts` one-minute ranges are
spread evenly over it.  Timed per file, `--reps` times, alternated, after one warm-up of each route:
  excerpts    seg.segment_excerpts(file, ranges): only the bytes / frames / blocks of the ranges are read, staged and decoded
  whole       the route there was before: seg.load_pcm(file), then seg.segment_signal(slice, start_sec) per range
Both must give the same segments.  Also recorded: the bytes the excerpt route asks the disk for (io._read_range) against the
file's size, and, from one profiled call of each route, the bytes staged (the *_h2d brackets) and the decode / resample kernel
times of the library's profiler.
Writes one JSON (default profiles/excerpts.json) and prints it.

--channels is the channel leg: the same ranges of both channels of a two-channel recording, as 48 kHz PCM16 WAV, 16 kHz left/side
FLAC and 8 kHz IMA ADPCM (the second channel is the first one, delayed).  Timed the same way:
  excerpts    seg.segment_channel_excerpts(file, ranges): the ranges cut and the channels split on the device
  whole       the route there was before: seg.load_pcm_channels(file) once, host slices, seg.segment_signal per slice
Default output: profiles/channel_excerpts.json; each leg's spread ((max - min) / min of its runs) is recorded beside its times.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

KERNELS = ('resample_kernel', 'flac_decode_kernel', 'adpcm_decode_kernel')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--hours', type=float, default=2.0)
    ap.add_argument('--excerpts', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--channels', action='store_true', help='the channel leg: two-channel files, segment_channel_excerpts')
    args = ap.parse_args(argv)

    import bench
    import flacgen
    import sndgen
    import wavgen
    from inaspeechsegmenter_amd import Segmenter
    from inaspeechsegmenter_amd import io as iss_io
    minutes = int(round(args.hours * 60))
    tmp = tempfile.mkdtemp(prefix='bench_excerpts_')
    t0 = time.time()
    pcm = bench.synth_recording_numpy(0, 60 * 16000)                 # int16
    files = {}
    up = np.repeat(pcm, 3)                                         # 48 kHz (held samples: content is not the point), both channels
    files['wav_48k_stereo'] = wavgen.write_wav(os.path.join(tmp, 'r.wav'), np.tile(np.stack([up, up], axis=1), (minutes, 1)), 48000, 'i16')
    files['flac_16k_mono'] = flacgen.write(os.path.join(tmp, 'r.flac'), np.tile(pcm, minutes).astype(np.int64), 16000, 16,
                                           subframe={'type': 'fixed', 'order': 2})
    spb = sndgen.ima_samples_per_block(256, 1)
    blocks = sndgen.ima_encode(pcm[::2][:spb * (30 * 8000 // spb)], 256)        # whole blocks of ~30 s at 8 kHz, repeated
    nrep = int(args.hours * 3600 * 8000 / (spb * (30 * 8000 // spb)))
    files['ima_8k_mono'] = sndgen.write_riff(os.path.join(tmp, 'r_ima.wav'), sndgen.wav_fmt('ima', 8000, 1, 256), bytes(blocks) * nrep,
                                             fact=spb * (30 * 8000 // spb) * nrep)
    if args.channels:
        files = {}
        pcm2 = np.stack([pcm, np.roll(pcm, 16000 * 7)], axis=1)         # the second channel: the first, seven seconds later
        files['wav_48k_stereo'] = wavgen.write_wav(os.path.join(tmp, 'c.wav'), np.tile(np.repeat(pcm2, 3, axis=0), (minutes, 1)), 48000, 'i16')
        files['flac_16k_left_side'] = flacgen.write(os.path.join(tmp, 'c.flac'), np.tile(pcm2, (minutes, 1)).astype(np.int64), 16000, 16,
                                                    channel_mode='left_side', subframe={'type': 'fixed', 'order': 2})
        spb = sndgen.ima_samples_per_block(512, 2)
        per = spb * (30 * 8000 // spb)
        blocks = sndgen.ima_encode(pcm2[::2][:per], 512)
        nrep = int(args.hours * 3600 * 8000 / per)
        files['ima_8k_stereo'] = sndgen.write_riff(os.path.join(tmp, 'c_ima.wav'), sndgen.wav_fmt('ima', 8000, 2, 512), bytes(blocks) * nrep,
                                                   fact=per * nrep)
    gen_s = time.time() - t0
    step = args.hours * 3600.0 / args.excerpts
    ranges = [(round(k * step + 7.3, 3), round(k * step + 67.3, 3)) for k in range(args.excerpts)]

    seg = Segmenter(ffmpeg=None, resample=True, models='synthetic')
    ctx = seg.ctx

    def excerpts(path):
        return seg.segment_excerpts(path, ranges)

    def whole(path):
        twin = seg.load_pcm(path)
        return [seg.segment_signal(twin[slice(*iss_io.excerpt_bounds(path, twin.size, a, b))], start_sec=a) for a, b in ranges]

    if args.channels:
        def excerpts(path):                                             # noqa: F811
            return seg.segment_channel_excerpts(path, ranges)

        def whole(path):                                                # noqa: F811
            out = [[] for _ in ranges]
            for twin in seg.load_pcm_channels(path):
                for r, (a, b) in enumerate(ranges):
                    out[r].append(seg.segment_signal(twin[slice(*iss_io.excerpt_bounds(path, twin.size, a, b))], start_sec=a))
            return out

    def profiled(fn, path):
        ctx.prof_enable(True)
        ctx.prof_reset()
        fn(path)
        ctx.synchronize()
        inst = ctx.prof_instances()
        ctx.prof_enable(False)
        out = {'kernel_ms': {}, 'staged_bytes': 0}
        for d in inst:
            name = d['kernel'].split('(')[0]
            if name in KERNELS:
                out['kernel_ms'][name] = out['kernel_ms'].get(name, 0.0) + d['ms']
            elif name.endswith('_h2d'):
                out['staged_bytes'] += int(d['kernel'].split('(')[1].split(' ')[0])
        return out

    asked = []
    real = iss_io._read_range

    def counting(path, offset, size):
        asked.append(size)
        return real(path, offset, size)

    result = {'leg': 'channels' if args.channels else 'mono', 'hours': args.hours, 'excerpts': args.excerpts, 'excerpt_seconds': 60.0, 'reps': args.reps,
              'generate_s': round(gen_s, 2), 'files': {}}
    ok = True
    for name, path in files.items():
        a, b = excerpts(path), whole(path)                               # warm-up, and the two routes agree
        same = a == b
        ok = ok and same
        legs = {'excerpts': [], 'whole': []}
        for _ in range(args.reps):
            for leg, fn in (('excerpts', excerpts), ('whole', whole)):
                t = time.perf_counter()
                fn(path)
                legs[leg].append(time.perf_counter() - t)
        iss_io._read_range = counting
        try:
            del asked[:]
            excerpts(path)
        finally:
            iss_io._read_range = real
        te, tw = min(legs['excerpts']), min(legs['whole'])
        audio_h = args.excerpts * 60.0 / 3600.0 * (2 if args.channels else 1)
        result['files'][name] = {
            'file_bytes': os.path.getsize(path), 'bytes_read_excerpts': int(sum(asked)), 'segments_identical': same,
            'excerpts_s_runs': legs['excerpts'], 'whole_s_runs': legs['whole'],
            'excerpts_spread': max(legs['excerpts']) / te - 1.0, 'whole_spread': max(legs['whole']) / tw - 1.0,
            'excerpts_audio_h_per_s': audio_h / te, 'whole_audio_h_per_s': audio_h / tw, 'speedup': tw / te,
            'excerpts_profile': profiled(excerpts, path), 'whole_profile': profiled(whole, path),
        }
    path = args.out or os.path.join(ROOT, 'profiles', 'channel_excerpts.json' if args.channels else 'excerpts.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    seg.close()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
