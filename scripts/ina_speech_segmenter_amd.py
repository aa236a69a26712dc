#!/usr/bin/env python3
"""Command line front end of the MI355X-native segmenter.

Same options as the reference's scripts/ina_speech_segmenter.py (-i -o -s -d -g -b -e -r, :45-53) and the
same output naming (<basename>.<format> inside the output directory, :80-84).  Extra: --models synthetic
(seeded stand-in weights, for machines without the Keras release assets), --resample (with -b None: WAV at any rate /
channel count, downmixed and resampled to 16 kHz on the GPU), --sets (with -b None: recordings stored as one file per channel,
read as one multichannel file) and multi-GPU operation: start it
under `python -m torch.distributed.run --nproc-per-node N` and the inputs are dealt to the N GPUs.
"""
import argparse
import glob
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _truthy(v):
    v = str(v).strip().lower()
    if v in ('y', 'yes', 't', 'true', 'on', '1'):
        return True
    if v in ('n', 'no', 'f', 'false', 'off', '0'):
        return False
    raise argparse.ArgumentTypeError(f'invalid truth value {v!r}')


def read_sets(path):
    """The list of --sets: one file set per line, `name<TAB>member<TAB>member...` (empty lines and lines starting with # are
    skipped) -> [io.FileSet].  The name becomes the output's: <output_directory>/<name>.<format>.  ValueError, naming the line:
    no member, an empty name, a name with a path separator, a name listed twice."""
    from inaspeechsegmenter_amd.io import FileSet
    sets, seen = [], set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip('\r\n')
            if not line.strip() or line.lstrip().startswith('#'):
                continue
            name, *members = [field.strip() for field in line.split('\t')]
            members = [m for m in members if m]
            where = f'{path}: line {no}'
            if not name:
                raise ValueError(f'{where}: empty name (a line reads name<TAB>member<TAB>member...)')
            if not members:
                raise ValueError(f'{where}: no member (a line reads name<TAB>member<TAB>member...)')
            if '/' in name or os.sep in name:
                raise ValueError(f'{where}: the name {name!r} holds a path separator; it names the output inside -o')
            if name in seen:
                raise ValueError(f'{where}: the name {name!r} is listed twice')
            seen.add(name)
            sets.append(FileSet(members, name=name))
    return sets


def output_stem(media):
    """What an input's outputs are called inside the output directory: a file's name without its extension, a set's name."""
    return os.path.splitext(os.path.basename(media))[0] if isinstance(media, str) else media.name


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.input and args.sets is None:
        ap.error('one of -i and --sets is required')
    return args


def build_parser():
    ap = argparse.ArgumentParser(
        description="Speech/Music(/Noise) and Male/Female segmentation into CSV or Praat TextGrid files. 'noEnergy' segments "
                    "are excluded from the music / noise / speech / gender analysis.")
    ap.add_argument('-i', '--input', nargs='+', default=[], help='media paths, glob patterns or http(s) URLs (optional with --sets)')
    ap.add_argument('-o', '--output_directory', required=True, help='directory receiving <basename>.<format>')
    ap.add_argument('-s', '--batch_size', type=int, default=32, help='accepted for compatibility (the engine sizes its own passes)')
    ap.add_argument('-d', '--vad_engine', choices=['sm', 'smn'], default='smn')
    ap.add_argument('-g', '--detect_gender', type=_truthy, default=True, metavar='{true,false}')
    ap.add_argument('-b', '--ffmpeg_binary', default='ffmpeg', help="ffmpeg binary; 'None' reads 16 kHz mono WAV, FLAC, G.711 / IMA ADPCM / Microsoft ADPCM WAV, AIFF, AU, CAF, Wave64 and RF64 directly "
                                                                      "(FLAC, IMA and Microsoft ADPCM decoded on the GPU)")
    ap.add_argument('-e', '--export_format', choices=['csv', 'textgrid'], default='csv')
    ap.add_argument('-r', '--energy_ratio', type=float, default=0.03)
    ap.add_argument('--models', default=None, help="'synthetic' = seeded stand-in weights")
    ap.add_argument('--resample', action='store_true',
                    help='with -b None: downmix and resample files of other rates / channel counts (8 kHz G.711 telephony, 44.1 kHz AIFF ...) to '
                         '16 kHz mono on the GPU')
    ap.add_argument('--channels', choices=['mix', 'split', 'auto'], default='mix',
                    help="with -b None: 'split' segments every channel of a file on its own (two-channel call recordings, multi-track "
                         "broadcast files) and writes <basename>.ch<k>.<format> per channel; 'auto' surveys every multichannel file "
                         "on the GPU and downmixes it without its dead channels, polarity-inverted channels turned back, from the "
                         "same upload (a healthy file as ever); 'mix' downmixes as ever")
    ap.add_argument('--auto-block', type=float, default=None, metavar='SEC',
                    help='with --channels auto: decide the downmix block by block instead of once per file -- every multichannel file '
                         'is surveyed in blocks of SEC seconds on the GPU and each stretch is downmixed as its own blocks suggest '
                         '(an item recorded out of phase, a leg that is dead for one call); --decisions then writes one row per '
                         'stretch: path, start, stop, blocks, plan, kept, flipped, downmix_loss_db')
    ap.add_argument('--auto-rule', choices=['safe', 'steady'], default=None,
                    help="with --auto-block: how the blocks decide.  'safe' (the default) decides every block on its own; 'steady' "
                         'keeps one divisor per file, so a leg that falls silent for a while changes no level, carries polarity from '
                         'block to block, and cross-fades where the downmix changes')
    ap.add_argument('--auto-fade', type=float, default=None, metavar='SEC',
                    help="with --auto-block: cross-fade over SEC seconds where the downmix changes (default: 0 for 'safe', 0.05 for "
                         "'steady'); 0 cuts")
    ap.add_argument('--decisions', default=None, metavar='OUT.tsv',
                    help="with --channels auto: write what was decided per file to OUT.tsv -- path, plan (mono, plain, mix; '!' for "
                         'a file that failed, with the error text), the channels kept, those of them turned back, and what the '
                         'default downmix would have lost in dB')
    ap.add_argument('--mixes', default=None, metavar='SPEC',
                    help='with -b None: segment weighted mixes of the channels of every file, each on its own, and write '
                         '<basename>.mix<k>.<format> per mix.  Mixes are separated by commas, terms joined by "+": "0+1,2+3" is the '
                         'mean of channels 0 and 1 and the mean of 2 and 3; a mix with any WEIGHT*CHANNEL term is a weighted sum, '
                         'in which a bare channel has weight 1 and nothing is divided: "0.7*4+0.7*5+1*2"')
    ap.add_argument('--survey', default=None, metavar='OUT.tsv',
                    help='with -b None: instead of segmenting, measure what the channels of every file hold (peak, RMS, DC, digital '
                         'zeros, clipped and non-finite samples, which channels carry signal) on the GPU and write one row per file '
                         "and channel to OUT.tsv; a row with channel '*' per file carries what the default downmix loses in dB and "
                         'the polarity-inverted channel pairs')
    ap.add_argument('--sets', default=None, metavar='LIST.tsv',
                    help='with -b None: recordings stored as one file per channel or group of channels (a call logger\'s X-in.wav / '
                         'X-out.wav, one mono WAV per track), one per line of LIST.tsv: name<TAB>member<TAB>member...  A set is read '
                         'as the one file holding its members\' channels side by side, shorter members continued with silence, on the '
                         'GPU and without writing that file; its output is <name>.<format>.  The sets follow the files of -i; '
                         '--channels, --mixes, --survey and --decisions treat them as files.  Members share rate and sample format; '
                         'FLAC and ADPCM members are not supported')
    return ap


def main(argv=None):
    args = parse_args(argv)
    ffmpeg = None if args.ffmpeg_binary.lower() in ('none', '') else args.ffmpeg_binary
    if args.resample and ffmpeg is not None:
        build_parser().error('--resample needs -b None (ffmpeg already resamples)')
    if args.channels == 'split' and ffmpeg is not None:
        build_parser().error('--channels split needs -b None (ffmpeg downmixes every file)')
    if args.channels == 'split' and int(os.environ.get('WORLD_SIZE', '1')) != 1:
        build_parser().error('--channels split runs on one GPU')
    if args.channels == 'auto' and ffmpeg is not None:
        build_parser().error('--channels auto needs -b None (ffmpeg downmixes every file)')
    if args.channels == 'auto' and int(os.environ.get('WORLD_SIZE', '1')) != 1:
        build_parser().error('--channels auto runs on one GPU')
    if args.channels == 'auto' and args.mixes is not None:
        build_parser().error('--mixes and --channels auto exclude each other')
    if args.auto_block is not None and args.channels != 'auto':
        build_parser().error('--auto-block goes with --channels auto')
    if args.auto_block is not None and not (args.auto_block > 0 and args.auto_block < float('inf')):
        build_parser().error('--auto-block takes a number of seconds above 0')
    if args.auto_block is None and (args.auto_rule is not None or args.auto_fade is not None):
        build_parser().error('--auto-rule and --auto-fade go with --auto-block')
    if args.auto_fade is not None and not (args.auto_fade >= 0 and args.auto_fade < float('inf')):
        build_parser().error('--auto-fade takes a number of seconds, 0 or above')
    if args.decisions is not None and args.channels != 'auto':
        build_parser().error('--decisions goes with --channels auto')
    mixes = None
    if args.mixes is not None:
        if ffmpeg is not None:
            build_parser().error('--mixes needs -b None (ffmpeg downmixes every file)')
        if args.channels == 'split':
            build_parser().error('--mixes and --channels split exclude each other')
        if int(os.environ.get('WORLD_SIZE', '1')) != 1:
            build_parser().error('--mixes runs on one GPU')
        from inaspeechsegmenter_amd.resample import parse_mixes
        try:
            mixes = parse_mixes(args.mixes)
        except ValueError as exc:
            build_parser().error(str(exc))
    if args.survey is not None and ffmpeg is not None:
        build_parser().error('--survey needs -b None (ffmpeg downmixes every file)')
    if args.survey is not None and int(os.environ.get('WORLD_SIZE', '1')) != 1:
        build_parser().error('--survey runs on one GPU')
    sets = []
    if args.sets is not None:
        if ffmpeg is not None:
            build_parser().error('--sets needs -b None (ffmpeg reads one file per run)')
        if int(os.environ.get('WORLD_SIZE', '1')) != 1:
            build_parser().error('--sets runs on one GPU')
        try:
            sets = read_sets(args.sets)
        except ValueError as exc:
            build_parser().error(str(exc))
    if ffmpeg is None:
        print('Disabling ffmpeg. WAV (PCM, float, G.711, IMA and Microsoft ADPCM), FLAC, AIFF, AU, CAF, Wave64 and RF64 files are read directly. '
              + ('Files at other rates or with several channels are resampled on the GPU.' if args.resample
                                      else 'Make sure your audio files are already sampled at 16kHz.'))
    inputs = []
    for pat in args.input:
        inputs += [pat] if pat.startswith('http') else sorted(glob.glob(pat))
    assert len(inputs) + len(sets) > 0, 'No existing media selected for analysis! Bad values provided to -i (%s)' % args.input
    inputs += sets
    names = [f if isinstance(f, str) else f.name for f in inputs]          # what the tables of --survey and --decisions carry
    odir = args.output_directory.strip(' \t\n\r').rstrip('/')
    assert os.access(odir, os.W_OK), 'Directory %s is not writable!' % odir
    outputs = [os.path.join(odir, output_stem(f) + '.' + args.export_format) for f in inputs]

    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    from inaspeechsegmenter_amd import Segmenter
    seg = Segmenter(vad_engine=args.vad_engine, detect_gender=args.detect_gender, ffmpeg=ffmpeg, batch_size=args.batch_size,
                    energy_ratio=args.energy_ratio, device=local_rank, models=args.models, resample=args.resample)
    if args.survey is not None:
        from inaspeechsegmenter_amd.survey import write_tsv
        write_tsv(args.survey, names, seg.survey_files(inputs))
        return 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if world == 1 and args.channels == 'auto':
            decisions = []
            lmsg = seg.batch_process(inputs, outputs, verbose=True, output_format=args.export_format, channels='auto',
                                     decisions=decisions, **({} if args.auto_block is None else {'auto_block_sec': args.auto_block}),
                                     **({} if args.auto_rule is None else {'auto_rule': args.auto_rule}),
                                     **({} if args.auto_fade is None else {'auto_fade_sec': args.auto_fade}))[3]
            if args.decisions is not None:
                from inaspeechsegmenter_amd.survey import write_decisions_tsv, write_schedule_decisions_tsv, write_steady_decisions_tsv
                if args.auto_block is not None:
                    write_decisions_tsv = write_steady_decisions_tsv if args.auto_rule == 'steady' else write_schedule_decisions_tsv
                failed = {dst: text for dst, code, text in lmsg if code == 2}
                write_decisions_tsv(args.decisions, names, decisions, {src: failed[dst] for src, dst in zip(names, outputs)
                                                                        if dst in failed})
            return 0
        if world == 1:
            seg.batch_process(inputs, outputs, verbose=True, output_format=args.export_format,
                              **({'channels': 'split'} if args.channels == 'split' else {}),
                              **({} if mixes is None else {'mixes': mixes}))
            return 0
        import torch
        import torch.distributed as dist
        from inaspeechsegmenter_amd.archive import segment_archive
        torch.cuda.set_device(local_rank)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
        table, lmsg = segment_archive(seg, inputs, outputs, output_format=args.export_format)
        if dist.get_rank() == 0:
            print('%d files, %d segments gathered from %d GPUs' % (len(table), sum(map(len, table.values())), world))
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
