#!/usr/bin/env python3
"""Command line front end of the MI355X-native voice femininity scoring (VoiceFemininityScoring.batch_process).

Scores every input file and writes one TSV: path, score, speech duration, number of x-vectors (a file that could not be
read gets its error message instead); with --channels split (-b None) one row per channel, the channel in a column of its
own.  Argument handling as scripts/ina_speech_segmenter_amd.py: -i takes paths or glob
patterns, -b None reads 16 kHz mono WAV or FLAC directly (with --resample: WAV / FLAC at any rate / channel count, resampled on
the GPU),
--models synthetic runs seeded stand-in weights.
"""
import argparse
import glob
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser(
        description='Voice femininity score of every input file: share of the speech x-vectors the gender model calls '
                    'female, with the speech duration and the number of x-vectors scored, written as one TSV.')
    ap.add_argument('-i', '--input', nargs='+', required=True, help='media paths or glob patterns')
    ap.add_argument('-o', '--output', required=True, help='TSV file receiving path, score, speech_duration, nb_vectors')
    ap.add_argument('-c', '--criteria', choices=['bgc', 'vfp'], default='bgc', help='gender detection model criteria')
    ap.add_argument('-b', '--ffmpeg_binary', default='ffmpeg', help="ffmpeg binary; 'None' reads 16 kHz mono WAV, FLAC, G.711 / IMA ADPCM / Microsoft ADPCM WAV, AIFF, AU, CAF, Wave64 and RF64 directly "
                                                                      "(FLAC, IMA and Microsoft ADPCM decoded on the GPU)")
    ap.add_argument('--batch_seconds', type=float, default=3600, help='audio held on the device per batch (seconds)')
    ap.add_argument('--models', default=None, help="'synthetic' = seeded stand-in weights")
    ap.add_argument('--resample', action='store_true',
                    help='with -b None: downmix and resample files of other rates / channel counts (8 kHz G.711 telephony, 44.1 kHz AIFF ...) to '
                         '16 kHz mono on the GPU')
    ap.add_argument('--channels', choices=['mix', 'split'], default='mix',
                    help="'split' (with -b None): score every channel of every file on its own, split on the GPU; the TSV then has a "
                         "channel column and one row per channel")
    return ap


def expand_inputs(patterns):
    inputs = []
    for pat in patterns:
        inputs += sorted(glob.glob(pat)) or [pat]         # a path that matches nothing is kept: it gets its error row
    return inputs


def main(argv=None):
    args = build_parser().parse_args(argv)
    ffmpeg = None if args.ffmpeg_binary.lower() in ('none', '') else args.ffmpeg_binary
    if args.resample and ffmpeg is not None:
        build_parser().error('--resample needs -b None (ffmpeg already resamples)')
    if args.channels == 'split' and ffmpeg is not None:
        build_parser().error('--channels split needs -b None (ffmpeg downmixes every file)')
    if ffmpeg is None:
        print('Disabling ffmpeg. WAV (PCM, float, G.711, IMA and Microsoft ADPCM), FLAC, AIFF, AU, CAF, Wave64 and RF64 files are read directly. '
              + ('Files at other rates or with several channels are resampled on the GPU.' if args.resample
                                      else 'Make sure your audio files are already sampled at 16kHz.'))
    inputs = expand_inputs(args.input)
    assert len(inputs) > 0, 'No media selected for analysis! Bad values provided to -i (%s)' % args.input
    odir = os.path.dirname(os.path.abspath(args.output))
    assert os.access(odir, os.W_OK), 'Directory %s is not writable!' % odir
    from inaspeechsegmenter_amd.vfs import VoiceFemininityScoring
    vfs = VoiceFemininityScoring(gd_model_criteria=args.criteria, ffmpeg=ffmpeg, models=args.models, resample=args.resample)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = vfs.batch_process(inputs, output_csv=args.output, batch_seconds=args.batch_seconds, verbose=True,
                                **({'channels': 'split'} if args.channels == 'split' else {}))
    print('%d files, %d scored, %d failed -> %s' % (len(res), sum(not isinstance(r, str) for r in res),
                                                  sum(isinstance(r, str) for r in res), args.output))
    return 0


if __name__ == '__main__':
    sys.exit(main())
