"""Voice femininity scoring on top of the MI355X kernels: host mirror of vbx_segmenter.VoiceFemininityScoring
(vbx_segmenter.py:92-202) -- SURVEY.md 8(f) item 3.

Pipeline (same order as the reference's __call__, :147-202): decode -> smn VAD (Segmenter, no gender) ->
get_features (csrc/vbx.hip) -> ResNet-101 x-vectors on every 144-frame window (engine, batched) -> keep the
x-vectors whose midpoint lies in speech and that overlap speech by >= vad_thresh (:129-145, 28-52) -> gender MLP
(a Keras Dense stack, run on the same engine) -> share of windows with p >= 0.5 (:55-61).

The reference does the interval arithmetic with pyannote.core (Annotation / Timeline.crop / Timeline.duration).  The helpers
below follow that package's rules on plain tuples -- a segment of <= 1e-6 s is empty, a timeline is a SET of segments,
crop() and duration() work on the SUPPORT (touching / overlapping segments merged), `intersects` wants more than 1e-6 s of
overlap -- and tests/test_vfs.py compares them with a class-by-class restatement of the package (oracle/pyannote_core.py)
running the reference's own statements, on random timelines incl. equal boundaries, overlaps, duplicates and empty
segments.  PARITY UNPINNED against the package itself (absent here) and against the only reference test of this tail
(run_test.py:177-187, score 0.534884 on lamartine.wav), which needs the un-vendored weights (final.onnx / raw_81.pth,
interspeech2023_*.hdf5).
Known divergence: add_needed_vectors (:40-52) reads `s.stop` on a pyannote Segment, which has no such attribute --
the branch would raise in the reference; here it does what the code evidently intends (append (key, (start, end), x)).
"""
import os
import time

import numpy as np

from . import _native, keras_model
from .io import decode_pcm, media2sig16kmono, _to_float
from . import sndfmt
from . import io as iss_io
from .segmenter import Segmenter, locate_model, _parts_pcm
from .vbx import FeatureExtractor, VBxExtractor, SR, frame_count, pcm16_of, plan_windows

_MLP_NET = 3          # engine net id of the gender MLP (0/1: VAD / gender CNNs, 4..: ResNet programs)


PRECISION = 1e-6     # pyannote.core's SEGMENT_PRECISION: a segment with end - start <= 1e-6 s is EMPTY (dropped / ignored)


def _nonempty(s, e):
    return (e - s) > PRECISION


def _intersects(a0, a1, b0, b1):
    """pyannote.core Segment.intersects: more than PRECISION of overlap, or equal starts."""
    return (a0 < b0 and b0 < a1 - PRECISION) or (a0 > b0 and a0 < b1 - PRECISION) or (a0 == b0)


def _support(intervals):
    """pyannote.core Timeline.support(): the distinct non-empty segments in (start, end) order, neighbours merged unless a gap
    of more than PRECISION separates them."""
    segs = sorted({(s, e) for s, e in intervals if _nonempty(s, e)})
    out = []
    for s, e in segs:
        if out and not _nonempty(min(e, out[-1][1]), max(s, out[-1][0])):       # `segment ^ new_segment` is empty: no gap
            out[-1] = (min(s, out[-1][0]), max(e, out[-1][1]))
        else:
            out.append((s, e))
    return out


def speech_intervals(vad_tuples):
    """get_annot_VAD (vbx_segmenter.py:64-69): the 'speech' segments as an Annotation keeps them -- one entry per distinct
    non-empty Segment(start, end), in (start, end) order."""
    return sorted({(s, e) for lab, s, e in vad_tuples if lab == 'speech' and _nonempty(s, e)})


def speech_duration(speech):
    """annot_vad.label_duration("speech") (vbx_segmenter.py:163): the duration of the SUPPORT of the speech timeline."""
    return sum(e - s for s, e in _support(speech))


def is_mid_speech(start, stop, speech):
    """vbx_segmenter.py:28-37: midpoint strictly inside a speech segment."""
    m = (start + stop) / 2
    return any(s < m < e for s, e in speech)


def cropped_duration(start, stop, speech):
    """Timeline([Segment(start, stop)]).crop(vad.get_timeline()).duration()  (vbx_segmenter.py:138-142; crop mode
    'intersection'): the support of the speech timeline is taken first, every support segment that `intersects` the window
    contributes window & segment unless that piece is empty, and the pieces' own support is summed in time order."""
    if not _nonempty(start, stop):
        return 0
    pieces = set()
    for s, e in _support(speech):
        if (s, e) <= (stop, stop) and _intersects(start, stop, s, e):
            p = (max(start, s), min(stop, e))
            if _nonempty(*p):
                pieces.add(p)
    return sum(e - s for s, e in _support(pieces))


def overlap_ratio(start, stop, speech):
    return cropped_duration(start, stop, speech) / (stop - start)


def add_needed_vectors(xvectors, t_mid):
    """vbx_segmenter.py:40-52: keep at least round(50 %) of the mid-in-speech predictions, best overlap first."""
    min_pred = round(0.5 * len(t_mid))
    if len(xvectors) < min_pred:
        order = np.argsort(np.asarray([t[0] for t in t_mid], dtype=np.float64))[::-1]
        ranked = [t_mid[i] for i in order]
        diff = min_pred - len(xvectors)
        for _, k, (s, e), x in ranked[len(xvectors):len(xvectors) + diff]:
            xvectors.append((k, (s, e), x))
    return xvectors


def apply_vad(xvectors, speech, vad_thresh):
    """vbx_segmenter.py:129-145."""
    midpoint_seg, kept = [], []
    for key, (start, stop), x in xvectors:
        if is_mid_speech(start, stop, speech):
            r = overlap_ratio(start, stop, speech)
            if r >= vad_thresh:
                kept.append((key, (start, stop), x))
            midpoint_seg.append((r, key, (start, stop), x))
    return add_needed_vectors(kept, midpoint_seg)


def get_femininity_score(g_preds):
    """vbx_segmenter.py:55-61: an Annotation keyed by Segment(start, stop) keeps ONE entry per distinct non-empty segment
    (a later prediction on the same segment replaces the earlier one); score = #(p >= 0.5) / #segments."""
    seen = {}
    for start, stop, p in g_preds:
        if _nonempty(start, stop):
            seen[(float(start), float(stop))] = bool(p >= 0.5)
    return sum(seen.values()) / len(seen)


def _basename(fpath):
    """The name x-vector windows are keyed by: the file's name without its directory and extension.  File sets (io.FileSet, or
    a tuple or list of member paths) are the Segmenter's: scoring them is not supported."""
    if not isinstance(fpath, (str, bytes, os.PathLike)):
        raise ValueError(f'{iss_io.as_media(fpath)}: voice femininity scoring of a file set is not supported; score the '
                         f"members' files, or their interleaved twin")
    return os.path.splitext(os.path.basename(fpath))[0]


def _load_resnet_params(path):
    """final.onnx -- what the reference's live backend loads (OnnxBackendExtractor, vbx_segmenter.py:249-266) -- through the
    package's own protobuf walk (onnx_reader.py); or raw_81.pth, the torch checkpoint behind the reference's commented
    TorchBackendExtractor (:268-288)."""
    if path.lower().endswith('.onnx'):
        from .onnx_reader import load_resnet101_params
        return load_resnet101_params(path)
    if path.lower().endswith('.npz'):                     # locate_model also accepts a flat '<stem>.npz' export of either file
        with np.load(path) as z:
            return {k: np.asarray(z[k]) for k in z.files}
    import torch
    ck = torch.load(path, map_location='cpu')
    sd = ck.get('state_dict', ck)
    return {k: v.numpy() for k, v in sd.items() if hasattr(v, 'numpy')}


class VoiceFemininityScoring:
    def __init__(self, gd_model_criteria='bgc', backend='onnx', ffmpeg='ffmpeg', device=0, models=None, resample=False):
        """gd_model_criteria / backend: as vbx_segmenter.py:97-127.  models: None -> files from the
        remote_utils search path (final.onnx for the x-vector net, read by onnx_reader.py; raw_81.pth if only that exists);
        'synthetic' -> seeded stand-ins; or a dict {'resnet': state_dict-like, 'mlp': (layers, in_shape),
        'vad': the `models` argument of the inner Segmenter (optional; default = its Keras files)}.
        resample: passed on to the inner Segmenter (ffmpeg=None only): WAVs at other rates / channel counts are turned into
        16 kHz mono PCM16 on the device and scored as if ffmpeg had produced that PCM."""
        assert backend in ['onnx'], "Backend should be 'onnx' (or 'pytorch' if uncommented)."
        assert gd_model_criteria in ['bgc', 'vfp'], "Gender detection model Criteria must be 'bgc' (default) or 'vfp'"
        gd_model, self.vad_thresh = ('interspeech2023_all.hdf5', 0.7) if gd_model_criteria == 'bgc' else ('interspeech2023_cvfr.hdf5', 0.62)
        self.ffmpeg = ffmpeg
        if models == 'synthetic':
            vad_models = 'synthetic'
        elif isinstance(models, dict):
            vad_models = models.get('vad')                # {'keras_speech_music_noise_cnn.hdf5': (layers, in_shape)} or 'synthetic'
        else:
            vad_models = None
        self.vad = Segmenter(vad_engine='smn', detect_gender=False, ffmpeg=ffmpeg, device=device, models=vad_models,
                             resample=resample)
        self.resample = self.vad.resample
        self.ctx = self.vad.ctx
        if models == 'synthetic':
            rng = np.random.default_rng(23)
            resnet = keras_model.synthetic_resnet101()
            mlp = ([dict(type='dense', W=rng.normal(0, 0.1, (256, 64)).astype(np.float32), b=np.zeros(64, np.float32), activation='relu'),
                    dict(type='dense', W=rng.normal(0, 0.3, (64, 1)).astype(np.float32), b=np.zeros(1, np.float32), activation='sigmoid')],
                   (1, 1, 256))
        elif isinstance(models, dict):
            resnet, mlp = models['resnet'], models['mlp']
        else:
            try:                                          # the file `get_remote` fetches by default (remote_utils.py:13, backend='onnx')
                onnx_path = locate_model('final.onnx')
            except FileNotFoundError as exc:
                # no final.onnx: the torch checkpoint of the same network (remote_utils.py:14) if it is there, else that error
                try:
                    resnet = _load_resnet_params(locate_model('raw_81.pth'))
                except FileNotFoundError:
                    raise exc
            else:
                # a final.onnx the reader does not recognise as resnet.py's graph is an error of its own: no silent second try
                # (a torch ImportError from the .pth path would hide the real cause)
                try:
                    resnet = _load_resnet_params(onnx_path)
                except (ValueError, NotImplementedError) as exc:
                    raise type(exc)(f"{exc} -- {onnx_path} was found but could not be read as the ResNet-101 of resnet.py; remove it to "
                                    "fall back to raw_81.pth, or export it with `torch.onnx.export` from resnet.py") from exc
            mlp = keras_model.load_model_file(locate_model(gd_model))
        self.features = FeatureExtractor(self.ctx)
        self.xvector_model = VBxExtractor(self.ctx, resnet)
        layers, in_shape = mlp
        self.mlp_layers = layers                          # (kept for inspection / tests; the engine holds the compiled program)
        if len(in_shape) == 1:
            in_shape = (1, 1, in_shape[0])
        self.ctx.cnn_load(_MLP_NET, keras_model.compile_layers(layers, in_shape, patch_input=False))

    def gender_predict(self, x):
        x = np.asarray(x, dtype=np.float32)
        return self.ctx.cnn_forward(_MLP_NET, x.reshape(len(x), 1, 1, -1))

    def __call__(self, fpath):
        """-> (score, speech_duration, nb_vectors)  (vbx_segmenter.py:147-202)."""
        basename = _basename(fpath)
        if self.resample or self._decoded_on_device(fpath):     # one device decode: the VAD and the front end read the same PCM
            a = self.vad.load_pcm(fpath)
            signal = _to_float(a, np.float64) if a.dtype == np.int16 else a.astype(np.float64)   # = media2sig16kmono
            vad = self.vad.segment_signal(a)
        else:
            signal = media2sig16kmono(fpath, ffmpeg=self.ffmpeg, dtype='float64')
            vad = None
        duration = len(signal) / SR
        speech = speech_intervals(self.vad(fpath) if vad is None else vad)
        speech_dur = speech_duration(speech)
        if not speech_dur:
            return None, speech_dur, 0
        feats = self.features(signal)
        x_vectors = self.xvector_model(basename, feats, duration)
        x_vectors = apply_vad(x_vectors, speech, self.vad_thresh)
        if not x_vectors:                                 # (the reference fails inside the MLP predict on an empty batch)
            return None, speech_dur, 0
        pred = self.gender_predict(np.asarray([x for _, _, x in x_vectors])).reshape(len(x_vectors), -1)[:, 0]
        g = [(seg[0], seg[1], p) for (_, seg, _), p in zip(x_vectors, pred)]
        return get_femininity_score(g), speech_dur, len(g)

    def score_signal(self, sig, basename='<signal>'):
        """__call__ behind the decode, for an already decoded 16 kHz mono signal (int16 or float32 array) -> (score,
        speech_duration, nb_vectors): exactly what __call__ returns for the PCM16 (or float) WAV holding those samples read
        without ffmpeg.  The definition score_channels / score_excerpts / score_channel_excerpts refer to."""
        a = np.ascontiguousarray(sig)
        if a.dtype not in (np.int16, np.float32):
            raise TypeError(f'signal dtype {a.dtype}: need int16 or float32')
        signal = _to_float(a, np.float64) if a.dtype == np.int16 else a.astype(np.float64)
        speech = speech_intervals(self.vad.segment_signal(a))
        speech_dur = speech_duration(speech)
        if not speech_dur:
            return None, speech_dur, 0
        feats = self.features(signal)
        return self._score(self.xvector_model(basename, feats, len(signal) / SR), speech, speech_dur)

    # ---- channels and time ranges of one file, scored where the decode pass left them (an extension; ffmpeg=None only)
    def _alone(self, fpath, sig, basename):
        """A part that shares no pass (float media, under 68 frames), through score_signal as batch_process sends float media."""
        if sig.size < 400:
            raise ValueError(f"media {fpath}: {sig.size} samples, less than one 25 ms analysis window")
        return self.score_signal(self.vad._mono_pcm(sig), basename)

    def _score_passes(self, fpath, basename, sigs, passes):
        """The `passes` (pipeline.cut_passes) of the batchable signals `sigs`, one after the other on this scorer's context ->
        one (score, speech_duration, nb_vectors) per part of every signal of every pass, in that order.  Per pass: the
        worker's `run` stages, decodes and resamples every part into the resident signal and runs the VAD over all of them;
        the 64-band front end reads the parts with speech right there (iss_vbx_features_resident: no PCM comes back, none is
        uploaded again); then _score_batch's steps: windows with the mid-speech filter, one embed_batch, __call__'s tail per
        part.  The first malformed FLAC frame / IMA block of a pass raises its ValueError (the file and its byte offset)."""
        from . import pipeline
        worker = pipeline._workers(self.vad, 1)[0]                # drives self.ctx: the VAD, the tables and the ResNet share it
        out = []
        for idx in passes:
            batch = pipeline._Batch()
            batch.idx, batch.sigs, batch.names = list(idx), [sigs[k] for k in idx], [fpath] * len(idx)
            lsegs = worker.run(batch)
            if batch.errs:
                raise ValueError(str(batch.errs[min(batch.errs)]))
            speeches = [speech_intervals([(lab, a * .02, b * .02) for lab, a, b in lseg]) for lseg in lsegs]
            durs = [speech_duration(s) for s in speeches]
            res = [(None, d, 0) for d in durs]
            live = [p for p, d in enumerate(durs) if d]           # a part without speech never reaches the front end
            if live:
                counts = [batch.psize[p] for p in live]
                self.features._ensure_dither(max(counts))
                self.ctx.vbx_features_resident([batch.poffs[p] for p in live], counts)
                self.ctx._vbx_resident = None                     # the single-file arena is gone
                plan = plan_windows([frame_count(n) for n in counts], [n / SR for n in counts], [basename] * len(live),
                                    keep=lambda f, t: is_mid_speech(t[0], t[1], speeches[live[f]]))
                for p, x in zip(live, self.xvector_model.embed_batch(plan)):
                    res[p] = self._score(x, speeches[p], durs[p])
            out += res
        return out

    def score_channels(self, fpath, channels=None, batch_files=None, batch_seconds=None):
        """Score every selected channel of one file on its own -> [(score, speech_duration, nb_vectors) per selected channel],
        in the order of `channels`.  Entry k is exactly score_signal(self.vad.load_pcm_channels(fpath, [sel[k]])[0]), sel =
        `channels` as Segmenter.load_pcm_channels takes them (None: all, ascending; any order, repeats allowed).  Arguments,
        passes and errors as Segmenter.segment_channels (ValueError with ffmpeg set; a one-channel file gives its one result
        len(sel) times; a malformed FLAC frame or IMA block fails the call, naming its byte offset).  The channels of a
        pass are split on the device and scored from the resident signal (_score_passes); a file whose channels are under
        68 frames goes channel by channel through score_signal."""
        from . import pipeline
        basename = _basename(fpath)
        sel, sig = self.vad._channel_sig(fpath, channels)
        if getattr(sig, 'sel', None) is None:                     # a one-channel file
            return [self._alone(fpath, sig, basename)] * len(sel)
        return self._score_parts(fpath, basename, sel, sig, batch_files, batch_seconds)

    def _score_parts(self, fpath, basename, sel, sig, batch_files, batch_seconds):
        """score_channels and score_mixes: the signals `sel` (channels, or mixes) of the source `sig`, in passes."""
        from . import pipeline
        if sig.size < pipeline.MIN_SAMPLES:
            return [self._alone(fpath, one, basename) for one in _parts_pcm(self.ctx, sig)]
        passes = pipeline.cut_passes([sig.reselect([ch]) for ch in sel], batch_files, batch_seconds)
        sigs = [sig.reselect([sel[k] for k in idx]) for idx in passes]
        return self._score_passes(fpath, basename, sigs, [[k] for k in range(len(sigs))])

    def score_excerpts(self, fpath, ranges, batch_files=None, batch_seconds=None):
        """Score time ranges [(start_sec, stop_sec | None)] of one file -> [(score, speech_duration, nb_vectors) per range], in
        the order of `ranges` (they may overlap or repeat).  Entry r is exactly
        score_signal(self.vad.load_pcm_excerpts(fpath, [ranges[r]])[0]): window times count from the start of the range.
        Arguments, passes and errors as Segmenter.segment_excerpts; ranges under 68 frames and float media go alone through
        score_signal, the others are cut on the device and scored from the resident signal (_score_passes)."""
        from . import pipeline
        basename = _basename(fpath)
        ranges, sigs = self.vad._excerpt_sigs(fpath, ranges)
        out, todo = [None] * len(sigs), []
        for k, s in enumerate(sigs):
            if not pipeline.sources.batchable(s) or s.size < pipeline.MIN_SAMPLES:
                out[k] = self._alone(fpath, s, basename)
            else:
                todo.append(k)
        rest = [sigs[k] for k in todo]
        for k, r in zip(todo, self._score_passes(fpath, basename, rest, pipeline.cut_passes(rest, batch_files, batch_seconds))):
            out[k] = r
        return out

    def score_channel_excerpts(self, fpath, ranges, channels=None, batch_files=None, batch_seconds=None):
        """Score time ranges of single channels of one file -> out[r][k] = exactly
        score_signal(self.vad.load_pcm_channel_excerpts(fpath, [ranges[r]], [sel[k]])[0][0]) for every range r and selected
        channel k.  Arguments, passes and errors as Segmenter.segment_channel_excerpts (a one-channel file gives
        [score_excerpts(...)[r]] * len(sel) per range); window times count from the start of the range."""
        from . import pipeline
        basename = _basename(fpath)
        ranges, sel, sigs = self.vad._channel_excerpt_sigs(fpath, ranges, channels)
        if sigs is None:
            return [[one] * len(sel) for one in self.score_excerpts(fpath, ranges, batch_files, batch_seconds)]
        return self._score_pairs(fpath, basename, ranges, sel, sigs, batch_files, batch_seconds)

    def _score_pairs(self, fpath, basename, ranges, sel, sigs, batch_files, batch_seconds):
        """score_channel_excerpts and score_mix_excerpts: the signals `sel` (channels, or mixes) of every range's source."""
        from . import pipeline
        out, todo = [[None] * len(sel) for _ in ranges], []
        for r, s in enumerate(sigs):
            if s.size < pipeline.MIN_SAMPLES:
                out[r] = [self._alone(fpath, one, basename) for one in _parts_pcm(self.ctx, s)]
            else:
                todo.append(r)
        per_pass = self.vad._pair_passes(sigs, todo, sel, batch_files, batch_seconds)
        srcs, passes = [], []
        for per in per_pass:                                      # each range of a pass one source, that pass's channels selected
            passes.append(list(range(len(srcs), len(srcs) + len(per))))
            srcs += [sigs[r].reselect([sel[k] for k in ks]) for r, ks in per]
        res = iter(self._score_passes(fpath, basename, srcs, passes))
        for per in per_pass:
            for r, ks in per:
                for k in ks:
                    out[r][k] = next(res)
        return out

    def score_mixes(self, fpath, mixes, batch_files=None, batch_seconds=None):
        """Score every mix of one file on its own -> [(score, speech_duration, nb_vectors) per mix]: entry k is exactly
        score_signal(self.vad.load_pcm_mixes(fpath, [mixes[k]])[0]).  Arguments, passes and errors as Segmenter.segment_mixes."""
        self.vad._no_ffmpeg_mixes()
        basename = _basename(fpath)
        return self._score_parts(fpath, basename, *iss_io.mix_source(fpath, mixes, self.vad.resample), batch_files, batch_seconds)

    def score_mix_excerpts(self, fpath, ranges, mixes, batch_files=None, batch_seconds=None):
        """Score time ranges of mixes of one file -> out[r][k] = exactly
        score_signal(self.vad.load_pcm_mix_excerpts(fpath, [ranges[r]], [mixes[k]])[0][0]).  Arguments, passes and errors as
        Segmenter.segment_mix_excerpts; window times count from the start of the range."""
        self.vad._no_ffmpeg_mixes()
        basename = _basename(fpath)
        ranges = [tuple(r) for r in ranges]
        sel, sigs = iss_io.mix_excerpts(fpath, ranges, mixes, self.vad.resample)
        return self._score_pairs(fpath, basename, ranges, sel, sigs, batch_files, batch_seconds)

    def _decoded_on_device(self, fpath):
        """Is the file decoded on the device when read without ffmpeg (FLAC, or a file of sndfmt.py)?  Then it is decoded
        once (Segmenter.load_pcm), like a resampled WAV."""
        if self.ffmpeg is not None:
            return False
        try:
            return sndfmt.device_decoded(fpath) is not None
        except OSError:                                   # (missing file, URL: the decode raises as before)
            return False

    def _score(self, x_vectors, speech, speech_dur):
        """The tail of __call__ (vbx_segmenter.py:181-202) on one file's x-vectors."""
        x_vectors = apply_vad(x_vectors, speech, self.vad_thresh)
        if not x_vectors:
            return None, speech_dur, 0
        pred = self.gender_predict(np.asarray([x for _, _, x in x_vectors])).reshape(len(x_vectors), -1)[:, 0]
        g = [(seg[0], seg[1], p) for (_, seg, _), p in zip(x_vectors, pred)]
        return get_femininity_score(g), speech_dur, len(g)

    def _decode(self, fpath, nbtry, trydelay):
        for itry in range(nbtry):
            try:
                if self.resample or self._decoded_on_device(fpath):
                    return self.vad.load_pcm(fpath)
                return decode_pcm(fpath, ffmpeg=self.ffmpeg)
            except _native.NativeError:
                raise
            except Exception:
                if itry + 1 == nbtry:
                    raise
                time.sleep(trydelay)

    def _score_batch(self, batch):
        """batch: [(index, basename, pcm16, duration, speech, speech_dur)] -> {index: result}.  One front-end call for all
        files, the windows whose midpoint is not in speech left out before the ResNet (apply_vad and add_needed_vectors only
        read mid-speech windows, in list order: vbx_segmenter.py:28-52, 129-145), then __call__'s tail per file."""
        self.features._ensure_dither(max(len(b[2]) for b in batch))
        self.ctx.vbx_features_batch_pcm16([b[2] for b in batch], to_host=False)
        self.ctx._vbx_resident = None                     # the single-file arena is gone
        speeches = [b[4] for b in batch]
        plan = plan_windows([frame_count(len(b[2])) for b in batch], [b[3] for b in batch], [b[1] for b in batch],
                            keep=lambda f, t: is_mid_speech(t[0], t[1], speeches[f]))
        xv = self.xvector_model.embed_batch(plan)
        return {b[0]: self._score(x, b[4], b[5]) for b, x in zip(batch, xv)}

    def batch_process(self, linput, output_csv=None, batch_seconds=3600, nbtry=1, trydelay=2., verbose=False, channels=None):
        """__call__ on many files -> [(score, speech_duration, nb_vectors) or an error message] in `linput` order, the same
        results as __call__ on each file.  Every file is decoded once (to PCM16): the VAD and the x-vector front end read the
        same array.  Files with speech are gathered into batches of at most `batch_seconds` of audio (a longer file makes a
        batch of its own): per batch, one front-end call (iss_vbx_features_batch_pcm16), one ResNet call over all full
        windows, one per distinct last-window width on the parameters already on the device.  A file that cannot be decoded
        (`nbtry` attempts, `trydelay` s apart) or is too short for the VAD gets an error message and the batch goes on;
        device failures raise.  output_csv: also write a TSV `path score speech_duration nb_vectors` (header line first;
        a failed file's row carries its message).
        channels (an extension, ffmpeg=None only): None is the above; 'split' scores every channel of every file on its own
        (score_channels, file by file: passes are not shared across files; batch_seconds is its pass limit): results[i] is then
        a list with one (score, speech_duration, nb_vectors) per channel, or the file's error message, and the TSV reads
        `path channel score speech_duration nb_vectors`, one row per channel (a failed file: one row, its channel column empty)."""
        if channels not in (None, 'split'):
            raise ValueError(f"channels={channels!r}: None or 'split'")
        linput = list(linput)
        for fpath in linput:
            _basename(fpath)                              # (a file set: ValueError before anything is decoded)
        if channels is not None:
            return self._batch_channels(list(linput), output_csv, batch_seconds, nbtry, trydelay, verbose)
        linput = list(linput)
        results = [None] * len(linput)
        batch, held = [], 0.0

        def flush():
            if batch:
                for i, r in self._score_batch(batch).items():
                    results[i] = r
                if verbose:
                    print('%d/%d scored' % (sum(r is not None for r in results), len(linput)))
                batch.clear()

        for i, fpath in enumerate(linput):
            try:
                a = self._decode(fpath, nbtry, trydelay)
                vad = self.vad.segment_signal(a)
            except _native.NativeError:
                raise
            except Exception as exc:
                results[i] = f'{type(exc).__name__}: {exc}'
                if verbose:
                    print(fpath, results[i])
                continue
            speech = speech_intervals(vad)
            speech_dur = speech_duration(speech)
            if not speech_dur:
                results[i] = (None, speech_dur, 0)
                continue
            basename = _basename(fpath)
            duration = len(a) / SR
            pcm = pcm16_of(a)
            if pcm is None:                               # samples beyond int16 (float source): the single-file front end
                feats = self.features(np.asarray(a, dtype=np.float64))     # = media2sig16kmono(fpath) of __call__
                results[i] = self._score(self.xvector_model(basename, feats, duration), speech, speech_dur)
                continue
            if batch and held + duration > batch_seconds:
                flush()
                held = 0.0
            batch.append((i, basename, pcm, duration, speech, speech_dur))
            held += duration
        flush()
        if output_csv is not None:
            with open(output_csv, 'w') as fh:
                fh.write('path\tscore\tspeech_duration\tnb_vectors\n')
                for fpath, r in zip(linput, results):
                    fh.write('\t'.join([fpath] + ([str(v) for v in r] if isinstance(r, tuple) else [r])) + '\n')
        return results

    def _batch_channels(self, linput, output_csv, batch_seconds, nbtry, trydelay, verbose):
        """batch_process(channels='split')."""
        if self.ffmpeg is not None:
            raise ValueError(f"channels='split' reads files without ffmpeg (VoiceFemininityScoring(ffmpeg=None)); "
                             f"ffmpeg={self.ffmpeg!r} downmixes every file with -ac 1")
        results = []
        for fpath in linput:
            for itry in range(nbtry):
                try:
                    results.append(self.score_channels(fpath, batch_seconds=batch_seconds))
                    break
                except _native.NativeError:
                    raise
                except Exception as exc:
                    if itry + 1 == nbtry:
                        results.append(f'{type(exc).__name__}: {exc}')
                    else:
                        time.sleep(trydelay)
            if verbose:
                print('%d/%d' % (len(results), len(linput)), fpath, results[-1])
        if output_csv is not None:
            with open(output_csv, 'w') as fh:
                fh.write('path\tchannel\tscore\tspeech_duration\tnb_vectors\n')
                for fpath, r in zip(linput, results):
                    if isinstance(r, str):                    # a failed file: one row, no channel
                        fh.write('\t'.join([fpath, '', r]) + '\n')
                        continue
                    for k, one in enumerate(r):
                        fh.write('\t'.join([fpath, str(k)] + [str(v) for v in one]) + '\n')
        return results
