"""`Segmenter`: drop-in host mirror of the reference's public class, driving the gfx950 kernels.

Same constructor kwargs, methods, return values and error behaviour as
/root/reference/inaSpeechSegmenter/segmenter.py (Segmenter 207-335, DnnSegmenter 111-204,
medialist2feats 338-374); the body is re-organised around the native pipeline:

    decode (host) -> iss_signal_* -> iss_sidekit  (features stay in HBM)
                  -> log-energy to host -> energy Viterbi (compiled host code)
                  -> iss_cnn_probs(VAD net, 'energy' slots)   -> Viterbi per segment
                  -> iss_cnn_probs(gender net, 'speech' slots) -> Viterbi per segment
                  -> [(label, start_sec + i*.02, ...)]

The 68-frame patches of `_get_patches` (segmenter.py:76-88) are never materialised: the
host only builds the int32 list "first mel row of the window feeding slot i".

What `_load_source` reads is a numpy array (16 kHz mono samples) or a source of sources.py (stored bytes the device resamples
or decodes); `_place` is the one step that puts either on the device alone, shared by `_sig2feats` and `Segmenter.load_pcm`.
"""
import os
import time
import shutil
import warnings

import threading
import weakref
import numpy as np

from . import _native
from . import tables
from . import keras_model
from . import io as iss_io
from . import resample as resample_mod
from .io import decode_pcm, _to_float
from .sources import Source, RawSource               # noqa: F401  (RawSource is also imported from here, where it was)
from .export_funcs import seg2csv, seg2textgrid

_MODEL_DIRS = ('/root/.keras/inaSpeechSegmenter/', os.path.expanduser('~/.keras/inaSpeechSegmenter/'))


# ---------------------------------------------------------------- Viterbi helpers (host)
def pred2logemission(pred, eps=1e-10):
    """viterbi_utils.py:29-34."""
    pred = np.asarray(pred)
    ret = np.full((len(pred), 2), eps)
    ret[pred == 0, 0] = 1 - eps
    ret[pred == 1, 1] = 1 - eps
    return np.log(ret)


def log_trans_exp(exp, cost0=0, cost1=0):
    """viterbi_utils.py:36-42."""
    ret = np.full((2, 2), -exp * np.log(10))
    ret[0, 0] = cost0
    ret[1, 1] = cost1
    return ret


def diag_trans_exp(exp, dim):
    """viterbi_utils.py:44-49."""
    ret = np.full((dim, dim), -exp * np.log(10))
    ret[np.arange(dim), np.arange(dim)] = 0
    return ret


_ENERGY_TRANS = log_trans_exp(150, cost0=-5)


def viterbi_decoding(emission, transition):
    """pyannote_viterbi.py:118-224 (unconstrained path) via the compiled host routine."""
    return _native.viterbi(emission, transition)


_NEP50 = int(np.__version__.split('.')[0]) >= 2      # NumPy >= 2: python-scalar / 0-d promotion by dtype, not by value


def _energy_activity(loge, ratio):
    """segmenter.py:69-73."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                 # all-silent input: mean of an empty slice
        threshold = np.mean(loge[np.isfinite(loge)]) + np.log(ratio)
    if isinstance(loge, np.ndarray) and loge.dtype == np.float32 and isinstance(threshold, np.floating):
        # the comparison, pred2logemission and the two-state Viterbi in one compiled call: same arithmetic, no (T,2) float64
        # emission array per file.  `float32_array > float64_scalar` is a float64 comparison under NumPy >= 2 (NEP 50) and a
        # float32 one under NumPy 1.x (value-based casting demotes the scalar): the compiled call compares in float64, so for
        # 1.x the threshold is rounded to float32 first -- (double)x > (double)(float)t == x > (float)t -- and the labels are
        # whatever the installed NumPy (the one the fallback line below would use) decides
        thr = np.float64(threshold) if _NEP50 else np.float64(np.float32(threshold))
        return _native.energy_viterbi(loge, thr, _ENERGY_TRANS)
    raw_activity = (loge > threshold)
    return viterbi_decoding(pred2logemission(raw_activity), log_trans_exp(150, cost0=-5))


def _binidx2seglist(binidx):
    """Run-length encode a label sequence, segmenter.py:91-108 (vectorised)."""
    a = np.asarray(binidx)
    n = len(a)
    if n == 0:                                          # (the reference's loop dies with UnboundLocalError on [])
        raise ValueError('_binidx2seglist: empty label sequence')
    cut = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.concatenate(([0], cut))
    stops = np.concatenate((cut, [n]))
    return [(a[s].item() if hasattr(a[s], 'item') else a[s], int(s), int(e)) for s, e in zip(starts, stops)]


def _energy_segments(loge, ratio):
    """The energy detector's labelled segments in 20 ms slots (segmenter.py:261-267): [(label, start, stop)]."""
    return [('noEnergy' if lab == 0 else 'energy', start, stop)
            for lab, start, stop in _binidx2seglist(_energy_activity(loge, ratio)[::2])]


def _window_rows(nframes, difflen=0):
    """First mel row of the 68-frame window behind every 20 ms slot.

    Restates the index arithmetic of `_get_patches(mspec, 68, 2)` (segmenter.py:76-88):
    windows start every 2 frames; 17 copies of the first window are prepended and
    16 (+1 if the frame count is odd) copies of the last are appended (:83-84); for media
    shorter than 68 frames the last int(difflen/2) slots are dropped (:150-152)."""
    nwin = (nframes - 68) // 2 + 1
    nslots = nwin + 17 + 16 + (nframes % 2)
    if difflen > 0:
        nslots -= int(difflen / 2)
    w = np.clip(np.arange(nslots) - 17, 0, nwin - 1)
    return (2 * w).astype(np.int32)


# ---------------------------------------------------------------- model location
def locate_model(model_fname):
    """Same search order as remote_utils.py:18-27 (`/root/.keras/inaSpeechSegmenter/` first, then
    `~/.keras/inaSpeechSegmenter/`), plus the flat `.npz` export next to it.  There is no
    download step: the target machines have no network."""
    stem = os.path.splitext(model_fname)[0]
    for d in _MODEL_DIRS:
        for cand in (model_fname, stem + '.npz'):
            p = os.path.join(d, cand)
            if os.access(p, os.R_OK):
                return p
    raise FileNotFoundError(
        f"model file {model_fname} not found in {_MODEL_DIRS}. Download it from "
        f"https://github.com/ina-foss/inaSpeechSegmenter/releases/download/models/{model_fname} "
        "(or its tools/convert_keras_hdf5.py .npz export) into one of these directories, or "
        "construct Segmenter(..., models='synthetic') for seeded stand-in weights.")


def _guard_on(ctx):
    """Is the library's precision guard probing on this context?  (guard_threshold None: the library default, 5e-4, on.)"""
    thr = getattr(ctx, 'guard_threshold', None)
    return thr is None or thr > 0


class DnnSegmenter:
    """Mirror of segmenter.py:111-179.  Child classes define outlabels / model_fname / inlabel /
    nmel / viterbi_arg exactly as the reference does (:182-204)."""
    net_id = 0

    def __init__(self, batch_size, ctx=None, models=None):
        self.batch_size = batch_size                   # kept for API compatibility; the engine sizes
        self.ctx = ctx                                 # its own passes from the HBM workspace limit
        if models == 'synthetic':
            layers, in_shape = keras_model.synthetic_ina_like(self.nmel, len(self.outlabels), seed=self.net_id + 1)
        elif isinstance(models, dict) and self.model_fname in models:
            layers, in_shape = models[self.model_fname]
        else:
            layers, in_shape = keras_model.load_model_file(locate_model(self.model_fname))
        if tuple(in_shape) != (68, self.nmel, 1):
            raise ValueError(f"{self.model_fname}: input shape {in_shape}, expected (68, {self.nmel}, 1)")
        self.layers = layers
        self.compiled = keras_model.compile_layers(layers, in_shape, patch_input=True)
        if self.compiled.out_dim != len(self.outlabels):
            raise ValueError(f"{self.model_fname}: {self.compiled.out_dim} outputs for labels {self.outlabels}")
        if ctx is not None:
            ctx.cnn_load(self.net_id, self.compiled)

    def predict_slots(self, win_rows):
        """(n,C) float32 probabilities (+ finite mask) for the given slots of the resident mspec."""
        return self.probs(self.ctx, win_rows)

    _MODES = {'bf16x3': _native.PREC_BF16X3, 'f32': _native.PREC_F32, 'f16x3': _native.PREC_F16X3}

    def probs(self, ctx, win_rows, async_out=None):
        """iss_cnn_probs (or, with async_out = (probs, finite) page-locked arrays, iss_cnn_probs_async) of this network on `ctx`.
        The library's precision guard (include/iss.h) decides a network's arithmetic at its first call PER CONTEXT; the device
        contexts of one Segmenter (its own and the pipeline workers') must not decide differently, so the first call anywhere
        decides for all of them: it runs under a lock, and every other context is told the outcome before its first call.
        The decision is about the mode the Segmenter's own context was asked for (its `precision`): when that changes, the decision
        is dropped, every context that was told it follows its own mode again, and the next call anywhere decides anew.  Only a
        probe's outcome ('passed' / 'escalated') is passed on; a 'fixed' first call (exact f32, or a caller's per-network
        override) is nothing to agree on.  A change of the guard threshold alone does not reopen a decision."""
        def run():
            if async_out is None:
                return ctx.cnn_probs(self.net_id, win_rows)
            return ctx.cnn_probs_async(self.net_id, win_rows, *async_out)
        st = self.__dict__.setdefault('_mode_state', {'lock': threading.Lock(), 'mode': None, 'told': set(), 'asked': None,
                                                      'pinned': weakref.WeakValueDictionary()})
        if not hasattr(ctx, 'cnn_precision_info'):             # (a test double of the device context)
            return run()
        asked = getattr(self.__dict__.get('ctx') or ctx, 'precision', None)
        asked = _native.PREC_F16X3 if asked is None else asked      # (None: never set, the library default)
        if st['asked'] != asked:
            with st['lock']:
                if st['asked'] != asked:
                    for c in list(st['pinned'].values()):      # (a context this method pinned follows its own mode again)
                        if getattr(c, '_h', True) is not None:  # (a closed context: nothing to undo)
                            c.cnn_set_net_precision(self.net_id, -1)
                    st['pinned'].clear()
                    st['told'].clear()
                    st['mode'], st['asked'] = None, asked
        if st['mode'] is None:
            with st['lock']:
                if st['mode'] is None:
                    out = run()
                    info = ctx.cnn_precision_info(self.net_id)
                    if info['state'] in ('passed', 'escalated'):
                        st['mode'] = self._MODES[info['mode']]
                        st['told'].add(id(ctx))
                    elif info['state'] == 'fixed' or not _guard_on(ctx):
                        st['mode'] = -1                        # exact f32, the caller's own override, or the guard off: nothing to agree on
                    # (else the guard is on but compared no window -- e.g. all over -inf mel rows --: the decision stays open,
                    # the next call anywhere probes and decides for every context, this one included)
                    return out
        if st['mode'] >= 0 and id(ctx) not in st['told']:
            with st['lock']:
                if id(ctx) not in st['told']:
                    if ctx.cnn_precision_info(self.net_id)['state'] == 'pending':
                        ctx.cnn_set_net_precision(self.net_id, st['mode'])
                        st['pinned'][id(ctx)] = ctx
                    st['told'].add(id(ctx))
        return run()

    def __call__(self, mspec, lseg, difflen=0, dense=False, ctx=None, allpred=None):
        """mspec: the RESIDENT mel spectrogram's frame count holder (`_Resident`) or a (T,24)
        array (uploaded first).  lseg: [(label, start, stop)] in 20 ms slots.  Returns the
        refined list, like segmenter.py:135-179.
        dense=True evaluates the network on EVERY slot of the file and then keeps the rows of
        the `inlabel` segments (same result; input-independent device work, used by bench.py).
        ctx: another device context on which this network is loaded under the same id (pipeline workers).
        allpred: probabilities of EVERY slot, already computed (Segmenter.segment_slots submits both networks
        asynchronously in dense mode and smooths the first while the device evaluates the second)."""
        ctx = ctx or self.ctx
        nframes = _ensure_resident(ctx, mspec)
        todo = [(start, stop) for lab, start, stop in lseg if lab == self.inlabel]
        if todo:
            idx = np.concatenate([np.arange(s, e) for s, e in todo])
            if allpred is not None:                            # (whoever computed them built the window list)
                rawpred = allpred[idx]
            elif dense:
                allpred, _finite = self.probs(ctx, _window_rows(nframes, difflen))
                rawpred = allpred[idx]
            else:
                rawpred, _finite = self.probs(ctx, _window_rows(nframes, difflen)[idx])  # non-finite windows already at 0.5 (:175)
        ret = []
        trans = diag_trans_exp(self.viterbi_arg, len(self.outlabels))
        pos = 0
        for lab, start, stop in lseg:
            if lab != self.inlabel:
                ret.append((lab, start, stop))
                continue
            n = stop - start
            r = rawpred[pos:pos + n]
            pos += n
            with np.errstate(divide='ignore'):
                pred = viterbi_decoding(np.log(r), trans)
            for lab2, start2, stop2 in _binidx2seglist(pred):
                ret.append((self.outlabels[int(lab2)], start2 + start, stop2 + start))
        return ret

    def smooth_landed(self, ctx, ticket, allpred, lseg):
        """`__call__(..., allpred=allpred)` for probabilities that are still arriving: `allpred` is the page-locked result of
        cnn_probs_async `ticket`, whose slots land front to back, pass by pass (include/iss.h, iss_wait_slots).  The `inlabel`
        spans are walked in order: wait until the next one has landed, take every further span that has landed with it, and
        smooth them together -- one np.log over their rows, one iss_viterbi_segments_f32 call (each span on its own, the
        arithmetic of the per-span calls), one run-length encoding.  So only the spans of the last landing are left to do once
        the device is through.  A context without wait_slots (a test double) lands everything at wait(ticket)."""
        spans = [(start, stop) for lab, start, stop in lseg if lab == self.inlabel]
        if not spans:
            return list(lseg)
        trans = diag_trans_exp(self.viterbi_arg, len(self.outlabels))
        wait_slots = getattr(ctx, 'wait_slots', None)
        runs = [[] for _ in spans]                              # per span: its refined (label, start, stop)
        i = 0
        while i < len(spans):
            if wait_slots is None:
                ctx.wait(ticket)
                landed = len(allpred)
            else:
                landed = wait_slots(ticket, spans[i][1])
            j = i + 1
            while j < len(spans) and spans[j][1] <= landed:
                j += 1
            first = np.array([s for s, _ in spans[i:j]], dtype=np.int64)
            length = np.array([e - s for s, e in spans[i:j]], dtype=np.int64)
            with np.errstate(divide='ignore'):
                em = np.log(allpred[spans[i][0]:spans[i][1]] if j == i + 1 else
                            np.concatenate([allpred[s:e] for s, e in spans[i:j]]))
            pred = _native.viterbi_segments(em, length, trans)
            # run-length encode all spans at once: a run starts where the label changes, and where a span starts
            off = np.concatenate(([0], np.cumsum(length)))      # span k of the batch = rows [off[k], off[k + 1]) of pred
            a = np.union1d(np.flatnonzero(pred[1:] != pred[:-1]) + 1, off[:-1])
            b = np.append(a[1:], len(pred))
            k = np.searchsorted(off, a, side='right') - 1
            shift = first[k] - off[k]
            for lab, kk, s, e in zip(pred[a].tolist(), k.tolist(), (a + shift).tolist(), (b + shift).tolist()):
                runs[i + kk].append((self.outlabels[lab], s, e))
            i = j
        ret, k = [], 0
        for seg in lseg:
            if seg[0] != self.inlabel:
                ret.append(seg)
            else:
                ret.extend(runs[k])
                k += 1
        return ret


class SpeechMusic(DnnSegmenter):
    outlabels = ('speech', 'music')
    model_fname = 'keras_speech_music_cnn.hdf5'
    inlabel = 'energy'
    nmel = 21
    viterbi_arg = 150
    net_id = 0


class SpeechMusicNoise(DnnSegmenter):
    outlabels = ('speech', 'music', 'noise')
    model_fname = 'keras_speech_music_noise_cnn.hdf5'
    inlabel = 'energy'
    nmel = 21
    viterbi_arg = 80
    net_id = 0


class Gender(DnnSegmenter):
    outlabels = ('female', 'male')
    model_fname = 'keras_male_female_cnn.hdf5'
    inlabel = 'speech'
    nmel = 24
    viterbi_arg = 80
    net_id = 1


class _Resident:
    """Marker for "the mel spectrogram is already in HBM on this context"."""
    def __init__(self, ctx, nframes):
        self.ctx, self.nframes = ctx, nframes

    def __len__(self):
        return self.nframes

    def to_host(self):
        return self.ctx.get_mspec()


def _ensure_resident(ctx, mspec):
    if isinstance(mspec, _Resident):
        if mspec.ctx is not ctx:
            raise ValueError("mel spectrogram is resident on a different context")
        return mspec.nframes
    m = np.asarray(mspec)
    ctx.set_mspec(m.astype(np.float32))
    return m.shape[0]


def _load_source(medianame, start_sec, stop_sec, ffmpeg, resample=False, channels=None, auto_block_sec=None, auto_rule='safe',
                 auto_fade_sec=None):
    """decode_pcm's 16 kHz mono samples (a numpy array), or -- without ffmpeg -- a source of sources.py for the device to
    finish.  The file is read once and what io._classify makes of its bytes says what Segmenter reads: a FLAC stream
    becomes a flac.FlacSource (compressed frames, decoded on the device like its WAV twin reads), a file of sndfmt.py what
    sndfmt.source makes of it (a RawSource with its format, a sndfmt.AdpcmSource, or the twin's array), and a WAV at another
    rate or with several channels a RawSource with `resample` and decode_pcm's refusal without it (io.source_of).
    channels='split' (ffmpeg=None): every channel on its own -- io.split_source's source with all channels selected;
    channels = a list of resample.Mix: those mixes, each on its own -- io.mix_source's source.
    channels='auto' (ffmpeg=None): io.auto_source's source -- one signal, the downmix the file's own survey suggests; with
    auto_block_sec io.timeline_source's -- the downmix its survey suggests block by block (whole single files), decided by
    auto_rule and cross-faded over auto_fade_sec seconds.
    A file set (io.FileSet, or a tuple or list of member paths; ffmpeg=None) is read by the same calls: io.set_source's source
    without `channels`.  Whole sets only."""
    medianame = iss_io.as_media(medianame)
    if isinstance(medianame, iss_io.FileSet):
        if ffmpeg is not None:
            raise ValueError(f'{medianame}: file sets are read without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={ffmpeg!r} reads '
                             f'one file per run')
        if start_sec is not None or stop_sec is not None:
            iss_io._no_set_ranges(medianame)
        if channels is None:
            iss_io._check_no_ffmpeg(medianame, None, None)
            return iss_io.set_source(medianame, resample)
    if channels is not None:
        if channels == 'auto' and auto_block_sec is not None:
            return iss_io.timeline_source(medianame, auto_block_sec, resample, auto_rule, auto_fade_sec)
        if channels == 'auto':
            return iss_io.auto_source(medianame, resample)
        if channels != 'split':
            return iss_io.mix_source(medianame, channels, resample)[1]
        return iss_io.split_source(medianame, None, resample)[1]
    if ffmpeg is not None:
        return decode_pcm(medianame, start_sec, stop_sec, ffmpeg)
    iss_io._check_no_ffmpeg(medianame, start_sec, stop_sec)
    buf = iss_io._read_file(medianame)
    what = iss_io._classify(buf, medianame)
    if what is not None:
        return what.source(resample)
    return iss_io.source_of(*iss_io._parse_wav(buf, medianame), medianame, resample)


def _media2feats(medianame, start_sec, stop_sec, ffmpeg, ctx=None, resample=False):
    """segmenter.py:53-67 on the device: returns (mspec, loge, difflen) where mspec is a
    `_Resident` handle when a context is given (the (T,24) array stays in HBM)."""
    if ctx is None:
        raise _native.NativeError("feature extraction needs a device context (no CPU path)")
    sig = _load_source(medianame, start_sec, stop_sec, ffmpeg, resample)
    return _sig2feats(ctx, sig, medianame)


def _place(ctx, sig, resident=True):
    """One file on the device, alone: `sig` becomes the resident signal -> (its samples where the host holds them, else None;
    the status to hand to sig.check AFTER the context's next synchronising read-back, valid only then).  An array is uploaded
    (resident=False: left where it is); a source places itself, but one that cannot be batched -- 24-bit FLAC, the float path
    of its WAV twin -- comes back to the host as float32 and goes on as an array."""
    if isinstance(sig, Source):
        if sig.batchable:
            return None, sig.place(ctx)
        sig = _to_float(sig.samples(ctx), np.float32)
    if resident:
        ctx.set_signal(sig)
    return sig, None


def _parts_pcm(ctx, sig):
    """The signals of a source placed alone (one per selected channel, one otherwise), copied back to the host and checked."""
    status = sig.place(ctx)
    out = [ctx.get_signal_pcm16(k * sig.stride, sig.size) for k in range(sig.parts)]
    if status is not None:
        sig.check(status)
    return out


def _sig2feats(ctx, sig, medianame='<signal>'):
    """sig: 16 kHz mono samples, or a source of sources.py (resampled / decoded on the device into the resident signal)."""
    if sig.size < 400:
        raise ValueError(f"media {medianame}: {sig.size} samples, less than one 25 ms analysis window")
    host, status = _place(ctx, sig)
    nframes = ctx.sidekit()
    loge = ctx.get_loge()
    if host is None:                                            # read back with the log-energy
        sig.check(status)
    difflen = 0
    if nframes < 68:                                            # segmenter.py:61-65
        difflen = 68 - nframes
        warnings.warn("media %s duration is short. Robust results require length of at least 720 milliseconds" % medianame)
        mspec = ctx.get_mspec()
        mspec = np.concatenate((mspec, np.ones((difflen, 24)) * np.min(mspec)))
        ctx.set_mspec(mspec.astype(np.float32))
        nframes = 68
    return _Resident(ctx, nframes), loge, difflen


class Segmenter:
    def __init__(self, vad_engine='smn', detect_gender=True, ffmpeg='ffmpeg', batch_size=32, energy_ratio=0.03,
                 device=0, models=None, resample=False):
        """Load the networks onto one MI355X.

        vad_engine / detect_gender / ffmpeg / batch_size / energy_ratio: as segmenter.py:208-247
        (same assertions, same "ffmpeg program not found" exception).
        device: HIP device ordinal.  models: None -> Keras files from ~/.keras/inaSpeechSegmenter
        (remote_utils.py search path); 'synthetic' -> seeded stand-in weights; or a dict
        {model_fname: (layers, in_shape)}.
        resample (extension, ffmpeg=None only): files (WAV, FLAC, G.711 / IMA ADPCM / Microsoft ADPCM, AIFF, AU, CAF, Wave64) at other integer rates (4 000 - 384 000 Hz) or with several
        channels are downmixed, resampled to 16 kHz and quantised to PCM16 on the device (resample.py states the
        arithmetic) instead of failing; 16 kHz mono files are read as without it."""
        if resample and ffmpeg is not None:
            raise ValueError(f'resample=True reads WAV files without ffmpeg: pass ffmpeg=None (ffmpeg={ffmpeg!r} already '
                             f'resamples)')
        self.resample = bool(resample)
        if ffmpeg is not None:
            if shutil.which(ffmpeg) is None:
                raise (Exception("""ffmpeg program not found"""))
        self.ffmpeg = ffmpeg
        self.energy_ratio = energy_ratio
        self.dense_batches = False                     # extension: batch_process evaluates both networks on every slot (pipeline.py)

        self.ctx = _native.Context(device)
        self.ctx.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank())

        assert vad_engine in ['sm', 'smn']
        if vad_engine == 'sm':
            self.vad = SpeechMusic(batch_size, self.ctx, models)
        elif vad_engine == 'smn':
            self.vad = SpeechMusicNoise(batch_size, self.ctx, models)

        assert detect_gender in [True, False]
        self.detect_gender = detect_gender
        if detect_gender:
            self.gender = Gender(batch_size, self.ctx, models)

    def close(self):
        """Release the extra device contexts of the multi-file pipeline (the main context goes with the object)."""
        from . import pipeline
        pipeline.close_workers(self)

    def segment_slots(self, mspec, loge, difflen, dense=False):
        """The body of segmenter.py:250-275 in 20 ms slot units: [(label, start_slot, stop_slot)]."""
        pending = None
        if dense and self.detect_gender:
            # both networks on every slot, independent of each other and of the energy detector: enqueue them back to back
            # (iss_cnn_probs_async) BEFORE the host starts on the energy Viterbi, and smooth the VAD output while the device
            # evaluates the gender network (the reference overlaps host and device work across files, segmenter.py:377-387;
            # within one file its gender pass needs the VAD result)
            ctx = self.ctx
            rows = _window_rows(_ensure_resident(ctx, mspec), difflen)
            t1, p1, _ = self.vad.probs(ctx, rows, async_out=self._pinned_out(0, len(rows), len(self.vad.outlabels)))
            t2, p2, _ = self.gender.probs(ctx, rows, async_out=self._pinned_out(1, len(rows), len(self.gender.outlabels)))
            pending = (t1, p1, t2, p2)
        lseg = _energy_segments(loge, self.energy_ratio)
        if pending is not None:
            # both results land pass by pass: the energy spans are smoothed over the VAD ticket as they arrive, then the speech
            # spans over the gender ticket, so that after the device's last kernel only the spans of the last pass remain
            t1, p1, t2, p2 = pending
            lseg = self.vad.smooth_landed(self.ctx, t1, p1, lseg)
            lseg = self.gender.smooth_landed(self.ctx, t2, p2, lseg)
            self.ctx.wait(t2)                                   # (retires both tickets; all that was waited for has landed)
            return lseg
        lseg = self.vad(mspec, lseg, difflen, dense=dense)
        if self.detect_gender:
            lseg = self.gender(mspec, lseg, difflen, dense=dense)
        return lseg

    def _pinned_out(self, k, n, c):
        """Page-locked result arrays of the asynchronous dense path (grown on demand, one set per network)."""
        cache = self.__dict__.setdefault('_pin_out', {})
        cur = cache.get(k)
        if cur is None or cur[0].shape[0] < n or cur[0].shape[1] != c:
            if cur is not None:
                self.ctx.pinned_free(cur[0]); self.ctx.pinned_free(cur[1])
            cap = int(n * 1.1) + 64
            cur = (self.ctx.pinned_empty((cap, c), np.float32), self.ctx.pinned_empty((cap,), np.uint8))
            cache[k] = cur
        return cur[0][:n], cur[1][:n]

    def segment_feats(self, mspec, loge, difflen, start_sec):
        """segmenter.py:250-276.  `mspec` may be a (T,24) array or the resident handle."""
        lseg = self.segment_slots(mspec, loge, difflen)
        return [(lab, start_sec + start * .02, start_sec + stop * .02) for lab, start, stop in lseg]

    def segment_device_pcm(self, dev_ptr, n, dense=False):
        """Hot-path entry for PCM16 samples that are ALREADY in this GPU's HBM (`dev_ptr` = a
        hipMalloc'ed address, e.g. a torch int16 tensor's data_ptr(); it must stay alive during
        the call).  Returns slot-unit segments [(label, start_slot, stop_slot)]."""
        if n < 400 + 160 * 67:
            raise ValueError("segment_device_pcm needs at least 68 frames (use segment_signal for short media)")
        self.ctx.set_signal_device(dev_ptr, n)
        nframes = self.ctx.sidekit()
        loge = self.ctx.get_loge()
        return self.segment_slots(_Resident(self.ctx, nframes), loge, 0, dense=dense)

    def segment_signal(self, sig, start_sec=0):
        """Native-path entry for an already decoded 16 kHz mono signal (int16 or float32)."""
        mspec, loge, difflen = _sig2feats(self.ctx, np.ascontiguousarray(sig))
        return self.segment_feats(mspec, loge, difflen, start_sec)

    def _mono_pcm(self, sig):
        """The 16 kHz mono samples of what `_load_source` read, on the host: a source placed alone and copied back, checked."""
        host, status = _place(self.ctx, sig, resident=False)
        if host is None:
            host = self.ctx.get_signal_pcm16(0, sig.size)
            sig.check(status)
        return host

    def load_pcm(self, medianame):
        """The 16 kHz mono samples the front end reads for `medianame` (decode_pcm's int16 or float32 array); with
        resample=True a WAV at another rate or channel count is resampled on the device and its PCM16 copied back.  Without
        ffmpeg a FLAC file is decoded on the device and its samples copied back (what decode_pcm gives for its WAV twin),
        and so is an IMA or Microsoft ADPCM file; G.711 and big-endian files at other rates or channel counts go to the resampler as stored."""
        return self._mono_pcm(_load_source(medianame, None, None, self.ffmpeg, self.resample))

    # ---- the channels of one file, each on its own, without ffmpeg (an extension: the reference needs one ffmpeg run per channel)
    def _channel_sig(self, medianame, channels):
        if self.ffmpeg is not None:
            raise ValueError(f'channels are split without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} downmixes '
                             f'every file with -ac 1')
        return iss_io.split_source(medianame, channels, self.resample)

    def load_pcm_channels(self, medianame, channels=None):
        """One int16 array per selected channel of `medianame`: for a file of two or more channels exactly
        resample.resample_ref(stored[:, c], sr), stored and sr from io.decode_source -- channel c alone, scaled, resampled to
        16 kHz and quantised like load_pcm's downmix (at 16 kHz the stored PCM16 values themselves) --, all of them by ONE decode
        launch and ONE resample launch.  A one-channel file gives [load_pcm(medianame)] (the float path included).
        channels: None (all, ascending) or a sequence of 0-based indices, in the order given; repeats are allowed.
        ValueError, naming the file: an index outside the file's channels, an empty selection, an http source; naming the
        argument with ffmpeg set.  Without resample=True a rate other than 16 kHz is refused as load_pcm refuses it."""
        sel, sig = self._channel_sig(medianame, channels)
        if getattr(sig, 'sel', None) is None:                    # a one-channel file
            return [self._mono_pcm(sig)] * len(sel)
        return _parts_pcm(self.ctx, sig)

    def segment_channels(self, medianame, channels=None, batch_files=None, batch_seconds=None):
        """Segment every selected channel of one file on its own -> [[(label, start, stop), ...] per selected channel], in the
        order of `channels` (as load_pcm_channels takes them).  List k is exactly what
        segment_signal(load_pcm_channels(medianame, [channels[k]])[0]) gives.  All channels of the file that fit a pass (at most
        batch_files channels / batch_seconds of audio, the defaults of batch_process) go through one decode launch, one
        resample launch and one feature pass.  Channels shorter than 68 frames go alone as segment_signal takes them (padding
        and warning included).  Errors as load_pcm_channels; a malformed FLAC frame or IMA block fails the call (ValueError
        naming its byte offset)."""
        from . import pipeline
        sel, sig = self._channel_sig(medianame, channels)
        if getattr(sig, 'sel', None) is None:
            return [self.segment_signal(self._mono_pcm(sig))] * len(sel)
        return self._segment_parts(medianame, sel, sig, batch_files, batch_seconds)

    def _segment_parts(self, medianame, sel, sig, batch_files, batch_seconds):
        """segment_channels and segment_mixes: the signals `sel` (channels, or mixes) of the source `sig`, in passes."""
        from . import pipeline
        if sig.size < pipeline.MIN_SAMPLES:
            return pipeline.one_by_one(self, self.ctx, sig)
        # the channels cut into passes as files of their length would be (min(batch_files, ceil(limit / stride)) each), and
        # each pass one source again: the file with that pass's channels selected
        passes = pipeline.cut_passes([sig.reselect([ch]) for ch in sel], batch_files, batch_seconds)
        sigs = [sig.reselect([sel[k] for k in idx]) for idx in passes]
        lsegs = pipeline.run_passes(self, [medianame] * len(sigs), sigs, [[k] for k in range(len(sigs))])
        return [[(lab, a * .02, b * .02) for lab, a, b in lseg] for lseg in lsegs]

    # ---- time ranges of one file without ffmpeg (an extension: the reference cuts them with ffmpeg's -ss / -to)
    def _excerpt_sigs(self, medianame, ranges):
        """io.excerpts for this Segmenter -> (ranges as a list, per range an array or a windowed source).  What io.excerpts
        leaves to the whole-file read (None) is decoded once, as load_pcm does, and sliced."""
        if self.ffmpeg is not None:
            raise ValueError(f'excerpts are read without ffmpeg (Segmenter(ffmpeg=None)); with ffmpeg={self.ffmpeg!r} pass '
                             f'start_sec / stop_sec to Segmenter.__call__, one range per call')
        ranges = [tuple(r) for r in ranges]
        sigs = iss_io.excerpts(medianame, ranges, self.resample)
        whole = None
        for k, ((start, stop), s) in enumerate(zip(ranges, sigs)):
            if s is None:
                if whole is None:
                    whole = self.load_pcm(medianame)
                a, b = iss_io.excerpt_bounds(medianame, whole.size, start, stop)
                sigs[k] = whole[a:b]
        return ranges, sigs

    def load_pcm_excerpts(self, medianame, ranges, batch_files=None, batch_seconds=None):
        """load_pcm for time ranges [(start_sec, stop_sec | None)] of one file: [the samples [a, b) of what load_pcm(medianame)
        returns, per range], a = floor(start_sec * 16000 + 0.5), b = its length for stop_sec None, else min(length, floor(stop_sec
        * 16000 + 0.5)) -- a definition (io.excerpt_bounds): ffmpeg's rounding of -ss / -to was not at hand to pin it.  Only the
        bytes, IMA blocks and FLAC frames the ranges need are staged, and all ranges that fit a pass (batch_files /
        batch_seconds as for batch_process) take ONE launch per kernel.  Frames and blocks that are not decoded are not checked."""
        from . import pipeline
        from .sources import Group
        ranges, sigs = self._excerpt_sigs(medianame, ranges)
        out = [None if isinstance(s, Source) else s for s in sigs]
        todo = [k for k, s in enumerate(sigs) if isinstance(s, Source)]
        for idx in pipeline.cut_passes([sigs[k] for k in todo], batch_files, batch_seconds):
            placed, pos = [], 0                                  # end to end: the launch creates a signal of just these samples
            for i in idx:
                placed.append((sigs[todo[i]], pos))
                pos += placed[-1][0].size
            group = Group(self.ctx, type(placed[0][0]), placed).launch(pos)      # (one file: one class)
            for i, (s, o) in zip(idx, placed):
                out[todo[i]] = self.ctx.get_signal_pcm16(o, s.size)
            group.check()
        return out

    def segment_excerpts(self, medianame, ranges, batch_files=None, batch_seconds=None):
        """Segment time ranges [(start_sec, stop_sec | None)] of one file without ffmpeg -> [[(label, start, stop), ...] per range],
        in the order of `ranges` (they may overlap or repeat).  Range k gives exactly what
        segment_signal(load_pcm(medianame)[a:b], start_sec=start_sec) gives, a and b as load_pcm_excerpts states them (a
        definition: ffmpeg's rounding of -ss / -to was not at hand to pin it); times are offset by start_sec as given.
        The ranges are cut on the device: only the bytes, IMA blocks and FLAC frames they need are staged, and all ranges of a
        pass (at most batch_files ranges / batch_seconds of audio, the defaults of batch_process) share one launch per decode
        kernel, one resample launch and one feature pass.  Ranges shorter than 68 frames, and float media, go alone as
        segment_signal would take them (padding and warning included).  ValueError, naming the file: a bad range, one that
        starts at or past the end (the message states the duration), one of fewer than 400 samples, a malformed FLAC frame or IMA
        block among those decoded (by its byte offset in the file; what is not decoded is not checked).  With ffmpeg set, use
        __call__(medianame, start_sec, stop_sec)."""
        from . import pipeline
        ranges, sigs = self._excerpt_sigs(medianame, ranges)
        out = [None] * len(sigs)
        todo = []
        for k, s in enumerate(sigs):
            if not pipeline.sources.batchable(s) or s.size < pipeline.MIN_SAMPLES:
                mspec, loge, difflen = _sig2feats(self.ctx, s, medianame)
                out[k] = self.segment_feats(mspec, loge, difflen, ranges[k][0])
            else:
                todo.append(k)
        rest = [sigs[k] for k in todo]
        lsegs = pipeline.run_passes(self, [medianame] * len(rest), rest, pipeline.cut_passes(rest, batch_files, batch_seconds))
        for k, lseg in zip(todo, lsegs):
            start = ranges[k][0]
            out[k] = [(lab, start + a * .02, start + b * .02) for lab, a, b in lseg]
        return out

    # ---- time ranges of single channels without ffmpeg: the two extensions above in one launch per kernel
    def _channel_excerpt_sigs(self, medianame, ranges, channels):
        """io.channel_excerpts for this Segmenter -> (ranges as a list, the selection, per range a windowed source carrying it;
        None instead of the sources for a one-channel file, which the excerpt calls read)."""
        if self.ffmpeg is not None:
            raise ValueError(f'excerpts of channels are read without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} '
                             f'downmixes every file with -ac 1')
        ranges = [tuple(r) for r in ranges]
        sel, sigs = iss_io.channel_excerpts(medianame, ranges, channels, self.resample)
        if not all(isinstance(s, Source) and s.sel is not None for s in sigs):
            sigs = None
        return ranges, sel, sigs

    @staticmethod
    def _pair_passes(sigs, todo, sel, batch_files, batch_seconds):
        """The (range, channel) pairs of the ranges `todo`, range by range, cut into passes as signals of their length would be
        -> per pass [(range, [k of sel])]: each range of a pass is one source again, with that pass's channels selected."""
        from . import pipeline
        pairs = [(r, k) for r in todo for k in range(len(sel))]
        out = []
        for idx in pipeline.cut_passes([sigs[r].reselect([sel[k]]) for r, k in pairs], batch_files, batch_seconds):
            per = []
            for r, k in (pairs[i] for i in idx):
                if per and per[-1][0] == r:
                    per[-1][1].append(k)
                else:
                    per.append((r, [k]))
            out.append(per)
        return out

    def load_pcm_channel_excerpts(self, medianame, ranges, channels=None, batch_files=None, batch_seconds=None):
        """load_pcm_channels for time ranges [(start_sec, stop_sec | None)] of one file -> out[r][k] = the int16 samples [a, b)
        of load_pcm_channels(medianame, [sel[k]])[0], (a, b) = io.excerpt_bounds(medianame, n16, *ranges[r]) on the length n16
        of a channel's 16 kHz twin, sel = channels as load_pcm_channels takes them (None: all, ascending; repeats and any order
        allowed).  Only the bytes, IMA blocks and FLAC frames the ranges need are staged, and all (range, channel) pairs that
        fit a pass (batch_files / batch_seconds as for batch_process) take ONE launch per decode kernel and ONE resample launch.
        A one-channel file gives [load_pcm_excerpts(...)[r]] * len(sel) per range (the float path included).  Range errors as
        segment_excerpts, channel errors as load_pcm_channels; with ffmpeg set, ValueError naming the argument.  Frames and
        blocks that are not decoded are not checked."""
        ranges, sel, sigs = self._channel_excerpt_sigs(medianame, ranges, channels)
        if sigs is None:
            return [[one] * len(sel) for one in self.load_pcm_excerpts(medianame, ranges, batch_files, batch_seconds)]
        return self._load_pairs(ranges, sel, sigs, batch_files, batch_seconds)

    def _load_pairs(self, ranges, sel, sigs, batch_files, batch_seconds):
        """load_pcm_channel_excerpts and load_pcm_mix_excerpts: the signals `sel` (channels, or mixes) of every range's source."""
        from .sources import Group
        out = [[None] * len(sel) for _ in ranges]
        for per in self._pair_passes(sigs, range(len(ranges)), sel, batch_files, batch_seconds):
            placed, pos = [], 0                                  # end to end: the launch creates a signal of just these samples
            for r, ks in per:
                placed.append((sigs[r].reselect([sel[k] for k in ks]), pos))
                pos += len(ks) * placed[-1][0].stride
            group = Group(self.ctx, type(placed[0][0]), placed).launch(pos)      # (one file: one class)
            for (r, ks), (s, o) in zip(per, placed):
                for q, k in enumerate(ks):
                    out[r][k] = self.ctx.get_signal_pcm16(o + q * s.stride, s.size)
            group.check()
        return out

    def segment_channel_excerpts(self, medianame, ranges, channels=None, batch_files=None, batch_seconds=None):
        """Segment time ranges of single channels of one file without ffmpeg -> out[r][k] = exactly what
        segment_signal(load_pcm_channel_excerpts(...)[r][k], start_sec=ranges[r][0]) gives, for every range r and every selected
        channel k (arguments as load_pcm_channel_excerpts; times are offset by start_sec as given).  Ranges and channels are cut
        and split on the device: all (range, channel) pairs of a pass (at most batch_files pairs / batch_seconds of audio, the
        defaults of batch_process) share one launch per decode kernel, one resample launch and one feature pass.  Ranges
        shorter than 68 frames go alone as segment_signal would take them (padding and warning included).  A one-channel file
        gives [segment_excerpts(...)[r]] * len(sel) per range.  Errors as load_pcm_channel_excerpts; a malformed FLAC frame or IMA
        block among those decoded fails the call (ValueError naming its byte offset in the file)."""
        ranges, sel, sigs = self._channel_excerpt_sigs(medianame, ranges, channels)
        if sigs is None:
            return [[one] * len(sel) for one in self.segment_excerpts(medianame, ranges, batch_files, batch_seconds)]
        return self._segment_pairs(medianame, ranges, sel, sigs, batch_files, batch_seconds)

    def _segment_pairs(self, medianame, ranges, sel, sigs, batch_files, batch_seconds):
        """segment_channel_excerpts and segment_mix_excerpts: the signals `sel` (channels, or mixes) of every range's source."""
        from . import pipeline
        out = [[None] * len(sel) for _ in ranges]
        todo = []
        for r, s in enumerate(sigs):
            if s.size < pipeline.MIN_SAMPLES:
                for k, one in enumerate(_parts_pcm(self.ctx, s)):
                    mspec, loge, difflen = _sig2feats(self.ctx, one, medianame)
                    out[r][k] = self.segment_feats(mspec, loge, difflen, ranges[r][0])
            else:
                todo.append(r)
        per_pass = self._pair_passes(sigs, todo, sel, batch_files, batch_seconds)
        srcs, passes = [], []
        for per in per_pass:
            passes.append(list(range(len(srcs), len(srcs) + len(per))))
            srcs += [sigs[r].reselect([sel[k] for k in ks]) for r, ks in per]
        lsegs = iter(pipeline.run_passes(self, [medianame] * len(srcs), srcs, passes))
        for per in per_pass:
            for r, ks in per:
                start = ranges[r][0]
                for k in ks:
                    out[r][k] = [(lab, start + a * .02, start + b * .02) for lab, a, b in next(lsegs)]
        return out

    # ---- weighted sums of a file's channels without ffmpeg (an extension; resample.py states a mix): mixed on the device
    def _no_ffmpeg_mixes(self):
        if self.ffmpeg is not None:
            raise ValueError(f'mixes are read without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} downmixes every '
                             f'file with -ac 1')

    def load_pcm_mixes(self, medianame, mixes):
        """One int16 array per mix of the specification `mixes` (resample.normalise_mixes states its spellings): exactly
        resample.mix_ref(stored, sr, mix), stored and sr from io.decode_source -- the weighted sum of channels in float64,
        resampled to 16 kHz and quantised (saturating) like load_pcm's downmix --, all of them by ONE decode launch and ONE
        resample launch; PCM16 whatever the stored format.  ValueError, naming the file, the mix and the reason: a channel outside
        the file's, a weight that is not finite, a zero or non-finite divisor, an empty mix; an http source; naming the argument
        with ffmpeg set.  Without resample=True a rate other than 16 kHz is refused as load_pcm refuses it."""
        self._no_ffmpeg_mixes()
        return _parts_pcm(self.ctx, iss_io.mix_source(medianame, mixes, self.resample)[1])

    def segment_mixes(self, medianame, mixes, batch_files=None, batch_seconds=None):
        """Segment every mix of one file on its own -> [[(label, start, stop), ...] per mix].  List k is exactly what
        segment_signal(load_pcm_mixes(medianame, [mixes[k]])[0]) gives.  All mixes of the file that fit a pass (batch_files /
        batch_seconds as for segment_channels, a mix counting as a channel does) share one decode launch, one resample launch
        and one feature pass.  Errors as load_pcm_mixes; a malformed FLAC frame or ADPCM block fails the call."""
        self._no_ffmpeg_mixes()
        return self._segment_parts(medianame, *iss_io.mix_source(medianame, mixes, self.resample), batch_files, batch_seconds)

    def load_pcm_mix_excerpts(self, medianame, ranges, mixes, batch_files=None, batch_seconds=None):
        """load_pcm_mixes for time ranges [(start_sec, stop_sec | None)] of one file -> out[r][k] = the int16 samples [a, b) of
        load_pcm_mixes(medianame, [mixes[k]])[0], (a, b) as load_pcm_channel_excerpts states them.  Only the bytes, ADPCM blocks
        and FLAC frames the ranges need are staged, and all (range, mix) pairs that fit a pass take ONE launch per decode kernel
        and ONE resample launch.  Range errors as segment_excerpts, mix errors as load_pcm_mixes."""
        self._no_ffmpeg_mixes()
        ranges = [tuple(r) for r in ranges]
        sel, sigs = iss_io.mix_excerpts(medianame, ranges, mixes, self.resample)
        return self._load_pairs(ranges, sel, sigs, batch_files, batch_seconds)

    def segment_mix_excerpts(self, medianame, ranges, mixes, batch_files=None, batch_seconds=None):
        """Segment time ranges of mixes of one file without ffmpeg -> out[r][k] = exactly what
        segment_signal(load_pcm_mix_excerpts(...)[r][k], start_sec=ranges[r][0]) gives: segment_channel_excerpts with the mix in
        place of the channel (passes, short ranges and times as stated there).  Errors as load_pcm_mix_excerpts."""
        self._no_ffmpeg_mixes()
        ranges = [tuple(r) for r in ranges]
        sel, sigs = iss_io.mix_excerpts(medianame, ranges, mixes, self.resample)
        return self._segment_pairs(medianame, ranges, sel, sigs, batch_files, batch_seconds)

    # ---- survey-guided downmix (an extension): a file surveyed and downmixed from ONE upload, by the mix its survey suggests
    def _auto_sig(self, medianame):
        if self.ffmpeg is not None:
            raise ValueError(f"channels='auto' reads files without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} "
                             f"downmixes every file with -ac 1")
        return iss_io.auto_source(medianame, self.resample)

    def load_pcm_auto(self, medianame):
        """-> (pcm, survey, mix).  A file of two or more channels is uploaded once (a coded one decoded once), surveyed on the
        device and downmixed from the bytes that are there: survey == survey_channels(medianame) to the bit, mix =
        survey.safe_mix() (survey.py states the rule), pcm exactly load_pcm(medianame) where mix is None and
        load_pcm_mixes(medianame, [mix])[0] otherwise.  A one-channel file takes load_pcm's path untouched: survey and mix are
        None.  ValueError naming the argument with ffmpeg set; without resample=True a rate other than 16 kHz is refused as
        load_pcm_mixes refuses it; a malformed FLAC frame or ADPCM block is the ValueError load_pcm raises."""
        sig = self._auto_sig(medianame)
        pcm = self._mono_pcm(sig)
        return (pcm,) + (getattr(sig, 'decision', None) or (None, None))

    def segment_auto(self, medianame):
        """-> (segments, survey, mix): survey and mix as load_pcm_auto gives them, segments exactly segment_signal(pcm) of its pcm,
        from the same single upload.  Whole files only."""
        sig = self._auto_sig(medianame)
        mspec, loge, difflen = _sig2feats(self.ctx, sig, medianame)
        return (self.segment_feats(mspec, loge, difflen, 0),) + (getattr(sig, 'decision', None) or (None, None))

    # ---- downmixes that change over time (an extension): scheduled mixes, and schedules decided from a survey resolved in time
    def _no_ffmpeg_schedule(self, what):
        if self.ffmpeg is not None:
            raise ValueError(f'{what} are read without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} downmixes every '
                             f'file with -ac 1')

    def load_pcm_schedule(self, medianame, schedule, fade_sec=0.0):
        """The 16 kHz mono PCM16 of `medianame` downmixed by `schedule` = [(start_sec, mix), ...] (resample.normalise_schedule
        states the spelling; a resample.Schedule counts in stored frames): exactly resample.schedule_ref(stored, sr, schedule),
        stored and sr from io.decode_source -- frame j mixed by the mix of the run that governs it, None being the plain downmix,
        then resampled and quantised as ever, so outputs near a boundary see both runs.  One upload, one decode launch for a coded
        file, ONE resample launch (resample_kernel's SCHED instantiation).  [(0, None)] is load_pcm to the bit, [(0, mix)] is
        load_pcm_mixes(medianame, [mix])[0].  fade_sec > 0: every run but the first fades in linearly over fade_sec seconds centred
        on its begin, each run giving at most half its length to either side (resample.fade_halves; include/iss.h, "Fades"), in
        the same single launch (the FADE instantiation); a resample.Schedule may carry its own half-widths instead.  ValueError
        naming the file, the run and the reason for a bad schedule; for a fade that is negative or not finite; for a file set
        (whole single files only); naming the argument with ffmpeg set."""
        self._no_ffmpeg_schedule('schedules')
        return self._mono_pcm(iss_io.schedule_source(medianame, schedule, self.resample, fade_sec)[1])

    def segment_schedule(self, medianame, schedule, fade_sec=0.0):
        """-> exactly segment_signal(load_pcm_schedule(medianame, schedule, fade_sec)), the samples never leaving the device."""
        self._no_ffmpeg_schedule('schedules')
        mspec, loge, difflen = _sig2feats(self.ctx, iss_io.schedule_source(medianame, schedule, self.resample, fade_sec)[1], medianame)
        return self.segment_feats(mspec, loge, difflen, 0)

    def survey_timeline(self, medianame, block_sec=None):
        """survey_channels resolved in time -> a survey.SurveyTimeline: the whole file's survey and one per block of `block_sec`
        seconds (None: survey.DEFAULT_BLOCK_SEC; survey.block_chunks states the block length in frames), from ONE upload, one
        decode and one survey launch: the blocks are sums of the chunk rows the whole-file survey is made of.  Equal to the bit
        to io.survey_timeline, the host-only twin.  Whole single files; errors as survey_channels."""
        from .sources import Group, SchedSource
        self._no_ffmpeg_schedule('timelines')
        sig = iss_io.timeline_source(medianame, block_sec, True)
        if not isinstance(sig, SchedSource):
            raise ValueError(f'{medianame}: a timeline needs a file of two or more channels')
        group = Group(self.ctx, type(sig), [(sig, 0)], in_place=True).launch(sig.size)
        self.ctx.synchronize()
        group.check()
        return sig.decision[0]

    def load_pcm_auto_timeline(self, medianame, block_sec=None, rule='safe', fade_sec=None):
        """load_pcm_auto with decisions that vary over time -> (pcm, timeline, schedule).  A file of two or more channels is
        uploaded once (a coded one decoded once), surveyed in blocks on the device (ONE survey launch) and downmixed from the
        bytes that are there by ONE resample launch: timeline == survey_timeline(medianame, block_sec) to the bit, schedule =
        timeline.schedule(rule, fade_sec) (survey.py states the rules), pcm exactly load_pcm_schedule(medianame, schedule).  rule
        'safe' is safe_schedule(): every block on its own, hard cuts unless fade_sec is given.  rule 'steady' is
        steady_schedule(): one divisor per file, polarity carried from block to block, and the run boundaries cross-faded over
        fade_sec seconds (None: survey.DEFAULT_FADE_SEC), still in the one resample launch.  A one-channel file takes load_pcm's
        path untouched: timeline and schedule are None.  Errors as load_pcm_auto; ValueError for a rule that is neither."""
        self._no_ffmpeg_schedule('timelines')
        sig = iss_io.timeline_source(medianame, block_sec, self.resample, rule, fade_sec)
        pcm = self._mono_pcm(sig)
        return (pcm,) + (getattr(sig, 'decision', None) or (None, None))

    def segment_auto_timeline(self, medianame, block_sec=None, rule='safe', fade_sec=None):
        """-> (segments, timeline, schedule): timeline and schedule as load_pcm_auto_timeline gives them, segments exactly
        segment_signal(pcm) of its pcm, from the same single upload.  Whole files only."""
        self._no_ffmpeg_schedule('timelines')
        sig = iss_io.timeline_source(medianame, block_sec, self.resample, rule, fade_sec)
        mspec, loge, difflen = _sig2feats(self.ctx, sig, medianame)
        return (self.segment_feats(mspec, loge, difflen, 0),) + (getattr(sig, 'decision', None) or (None, None))

    # ---- channel survey: what the channels of a file hold, measured on the device (an extension)
    def _no_ffmpeg_survey(self):
        if self.ffmpeg is not None:
            raise ValueError(f'channels are surveyed without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} downmixes '
                             f'every file with -ac 1')

    def _survey_pass(self, items, out, on_error):
        """One pass of surveys: items = [(index into out, source, sr, first frame)].  All sources of a class share one launch
        (sources.Group.survey), the classes in pass order.  A malformed file: on_error(index, exception), or raised without it."""
        from .sources import Group
        from .survey import ChannelSurvey
        by_class = {}
        for it in items:
            by_class.setdefault(type(it[1]), []).append(it)
        for cls in sorted(by_class, key=lambda c: c.pass_order):
            mine = by_class[cls]
            group = Group(self.ctx, cls, [(src, 0) for _, src, _, _ in mine])
            fields = group.survey()
            bad = {}
            group.check(None if on_error is None else bad.__setitem__)
            for k, (i, _, sr, first) in enumerate(mine):
                if k in bad:
                    on_error(i, bad[k])
                else:
                    out[i] = ChannelSurvey(fields[k], sr, first)

    def survey_channels(self, medianame, ranges=None):
        """What the channels of `medianame` hold, measured on the device in one pass over the stored samples -> a
        survey.ChannelSurvey of the whole file, or with ranges = [(start_sec, stop_sec | None)] one per range (stored frames
        [a, b) by io.survey_bounds: the excerpt calls' rounding at the file's own rate).  Per channel: peak, digital zeros,
        fullscale and non-finite samples, DC and RMS; per pair of channels (files of up to 16) the correlation; and what the
        default downmix loses (`downmix_loss_db`), which channels carry signal (`active()`, the list to pass as `channels=`)
        and which pairs are polarity-inverted (`inverted()`).  Equal to the bit, in every field, to io.survey_channels, the
        host-only twin (include/iss.h states the figures and the order of the sums).  Only the bytes, FLAC frames and ADPCM
        blocks the ranges need are staged.  ValueError, naming the file: a range that holds no frame, a malformed FLAC frame
        or ADPCM block among those decoded, an http source; naming the argument with ffmpeg set."""
        from . import pipeline
        from .survey import ChannelSurvey
        self._no_ffmpeg_survey()
        sr, entries = iss_io.survey_sources(medianame, ranges)
        out = [None if isinstance(src, Source) else ChannelSurvey(src, sr, first) for src, first in entries]
        todo = [(k, src, sr, first) for k, (src, first) in enumerate(entries) if isinstance(src, Source)]
        for idx in pipeline.cut_passes([t[1] for t in todo], None, None):
            self._survey_pass([todo[k] for k in idx], out, None)
        return out[0] if ranges is None else out

    def survey_files(self, linput, batch_files=None, batch_seconds=None):
        """survey_channels for many files -> one entry per file of `linput`: its survey.ChannelSurvey, or for a file that
        cannot be read the text batch_process reports for it ('error: <class> <message>').  The files are read by four
        threads and packed into passes as batch_process packs them (at most batch_files files / batch_seconds of audio);
        all files of a pass that share a source class share ONE survey launch, so a pass costs one launch per class present
        (stored PCM / float / G.711, FLAC, IMA ADPCM, Microsoft ADPCM), the three decoders with their decode launch in front."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from . import pipeline
        from .survey import ChannelSurvey
        self._no_ffmpeg_survey()
        linput = list(linput)
        batch_files, batch_seconds = pipeline._limits(batch_files, batch_seconds)
        out = [None] * len(linput)

        def failed(i, exc):
            out[i] = 'error: %s %s' % (type(exc), exc)

        def read(name):
            try:
                return iss_io.survey_sources(name)
            except Exception as exc:                             # this file's error; the others go on
                return exc

        cur, items = pipeline._Batch(), []
        with ThreadPoolExecutor(4) as pool:
            ahead, names = deque(), iter(enumerate(linput))
            while True:
                while len(ahead) < 8:                            # a few files read ahead of the pass being packed, not all of them
                    nxt = next(names, None)
                    if nxt is None:
                        break
                    ahead.append((nxt[0], pool.submit(read, nxt[1])))
                if not ahead:
                    break
                i, fut = ahead.popleft()
                got = fut.result()
                if isinstance(got, Exception):
                    failed(i, got)
                    continue
                sr, ((src, first),) = got
                if not isinstance(src, Source):
                    out[i] = ChannelSurvey(src, sr, first)
                    continue
                cur.sigs.append(src)
                items.append((i, src, sr, first))
                if cur.full(batch_files, batch_seconds * 16000):
                    self._survey_pass(items, out, failed)
                    cur, items = pipeline._Batch(), []
        if items:
            self._survey_pass(items, out, failed)
        return out

    def __call__(self, medianame, start_sec=None, stop_sec=None):
        """segmenter.py:279-294."""
        mspec, loge, difflen = _media2feats(medianame, start_sec, stop_sec, self.ffmpeg, self.ctx, self.resample)
        if start_sec is None:
            start_sec = 0
        return self.segment_feats(mspec, loge, difflen, start_sec)

    def batch_process(self, linput, loutput, verbose=False, skipifexist=False, nbtry=1, trydelay=2., output_format='csv',
                      batch_files=None, workers=None, batch_seconds=None, channels=None, mixes=None, decisions=None,
                      auto_block_sec=None, auto_rule=None, auto_fade_sec=None):
        """segmenter.py:297-335: same arguments, same (t_batch_dur, nb_processed, avg, lmsg) with
        lmsg entries (dst, code, text), code 0 ok / 1 already exists / 2 error, in input order.
        The files run through pipeline.process_files: decode threads, super-batches of at most `batch_files` files /
        `batch_seconds` of audio per device pass (defaults 32 / 40 min), `workers` (default 4) device contexts in turn (the reference overlaps the feature extraction of file i+1 with the
        networks of file i, :377-387).  Undecodable or too-short media are per-file errors (code 2) as in the
        reference; device failures and unwritable outputs raise.
        channels (an extension, ffmpeg=None only): None is the above; 'split' segments every channel of every file on its own
        (segment_channels) and writes one output per channel, <dst stem>.ch<k><ext> (a.csv -> a.ch0.csv, a.ch1.csv; a mono file
        writes .ch0 only).  A file's outputs are written in descending channel order, so .ch0 existing means the file is complete:
        skipifexist tests that name.  lmsg then holds one entry per written output, files in input order and channels ascending;
        a file that fails to decode gives one code-2 entry carrying the unsplit dst.  Each channel counts as a file against
        batch_files, its samples against batch_seconds.
        mixes (an extension, ffmpeg=None only, not with channels='split'): a mix specification (resample.normalise_mixes), the same
        for every file: every mix of every file is segmented on its own (segment_mixes) and written to <dst stem>.mix<k><ext>,
        the last mix first, so .mix0 existing means the file is complete: skipifexist tests that name.  lmsg as for
        channels='split'; a file with too few channels for the specification is a code-2 entry like any file that fails to decode.
        channels='auto' (an extension, ffmpeg=None only, not with mixes): every file of two or more channels is surveyed on the
        device and downmixed by the mix its own survey suggests (segment_auto; survey.ChannelSurvey.safe_mix states the rule),
        from one upload and one decode, all files of a pass and a class in one survey launch and one resample launch.  Outputs,
        names, skipifexist, lmsg and the return value are the default call's: one output per file, at dst; a healthy or
        one-channel file writes what the default call writes.  decisions: a list that receives (src, survey, mix) per processed
        file, in completion order (survey and mix None for a one-channel file).
        auto_block_sec (with channels='auto' only; else ValueError): every file of two or more channels takes the timeline route
        instead (segment_auto_timeline with block_sec = auto_block_sec): surveyed in blocks of that many seconds and downmixed by
        the schedule its timeline suggests, the files of a pass and a class in one survey launch and one resample launch as for
        'auto'.  decisions then receives (src, timeline, schedule).  A healthy file writes what plain 'auto' writes.  File sets
        are code-2 entries on this route (whole single files only).
        auto_rule, auto_fade_sec (with auto_block_sec only; else ValueError): the rule that decides the schedule, 'safe' (the
        default) or 'steady', and the cross-fade at its run boundaries in seconds (None: 0 for 'safe', survey.DEFAULT_FADE_SEC
        for 'steady'), as segment_auto_timeline takes them.
        File sets (an extension, ffmpeg=None only): an entry of linput may be an io.FileSet, or a tuple or list of member paths
        -- a recording stored as one file per channel or group of channels.  It is read as its interleaved twin would be, by
        every mode above, the sets of a pass in one launch of their own; its messages and `decisions` carry the set's name, and
        a set that cannot be read (a coded member, members of different rates or formats) is a code-2 entry naming the member."""
        from . import pipeline
        if channels not in (None, 'split', 'auto'):
            raise ValueError(f"channels={channels!r}: None, 'split' or 'auto'")
        part_name = iss_io.channel_name
        auto = channels == 'auto'
        if auto_block_sec is not None:
            if not auto:
                raise ValueError(f"auto_block_sec={auto_block_sec!r} needs channels='auto': it sets the block length of its decisions")
            from .survey import block_chunks, rule_fade
            block_chunks(auto_block_sec, 16000)                # (ValueError for a block length that is none)
            rule_fade(auto_rule or 'safe', auto_fade_sec)      # (... for a rule or a fade that is none)
        elif auto_rule is not None or auto_fade_sec is not None:
            what = f'auto_rule={auto_rule!r}' if auto_rule is not None else f'auto_fade_sec={auto_fade_sec!r}'
            raise ValueError(f"{what} needs auto_block_sec: it shapes the schedule of a timeline")
        if auto:
            if mixes is not None:
                raise ValueError("mixes and channels='auto' exclude each other: 'auto' derives every file's mix from its survey")
            if self.ffmpeg is not None:
                raise ValueError(f"channels='auto' reads files without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} "
                                 f"downmixes every file with -ac 1")
            channels = None                                    # outputs and messages are the default call's
        if mixes is not None:
            if channels is not None:
                raise ValueError("mixes and channels='split' exclude each other")
            self._no_ffmpeg_mixes()
            channels, part_name = resample_mod.normalise_mixes(mixes), iss_io.mix_name
        if channels is not None and self.ffmpeg is not None:
            raise ValueError(f"channels='split' reads files without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={self.ffmpeg!r} "
                             f"downmixes every file with -ac 1")
        first = (lambda dst: dst) if channels is None else (lambda dst: part_name(dst, 0))
        if verbose:
            print('batch_processing %d files' % len(linput))
        if output_format == 'csv':
            fexport = seg2csv
        elif output_format == 'textgrid':
            fexport = seg2textgrid
        else:
            raise NotImplementedError()

        t_batch_start = time.time()
        linput, loutput = list(linput), list(loutput)
        msgs, skip, done = {}, set(), [0]
        for i, dst in enumerate(loutput):
            if skipifexist and os.path.exists(first(dst)):
                msgs[i] = (first(dst), 1, 'already exists')
                skip.add(i)
            else:
                dname = os.path.dirname(dst)
                if dname and not os.path.isdir(dname):
                    os.makedirs(dname, exist_ok=True)

        def on_result(i, src, lseg, err, secs=0.0):
            dst = loutput[i]
            if lseg is None:
                msgs[i] = (dst, 2, err)
            elif channels is not None:                         # one segment list per channel: the last channel's output first
                b = time.time()
                for k in reversed(range(len(lseg))):
                    fexport(lseg[k], part_name(dst, k))
                text = 'ok ' + str(secs + (time.time() - b) / len(lseg))
                msgs[i] = [(part_name(dst, k), 0, text) for k in range(len(lseg))]
            else:
                b = time.time()
                fexport(lseg, dst)
                # per-file processing time as in segmenter.py:322-327 (networks + smoothing + export, features excluded
                # there; here: this file's share of its device pass + its export)
                msgs[i] = (dst, 0, 'ok ' + str(secs + time.time() - b))
            done[0] += 1
            if verbose:
                print('%d/%d' % (done[0] + len(skip), len(linput)), [msgs[i]])

        pipeline.process_files(self, linput, on_result, skip=skip, nbtry=nbtry, trydelay=trydelay,
                               batch_files=batch_files, workers=workers, batch_seconds=batch_seconds,
                               **({'channels': 'auto', 'decided': None if decisions is None else decisions.append,
                                   **({} if auto_block_sec is None else {'auto_block_sec': auto_block_sec}),
                                   **({} if auto_rule is None and auto_fade_sec is None else
                                      {'auto_rule': auto_rule or 'safe', 'auto_fade_sec': auto_fade_sec})} if auto
                                  else {'channels': channels}))
        lmsg = [m for i in range(len(linput)) for m in (msgs[i] if isinstance(msgs[i], list) else [msgs[i]])]
        t_batch_dur = time.time() - t_batch_start
        nb_processed = len([e for e in lmsg if e[1] == 0])
        avg = t_batch_dur / nb_processed if nb_processed > 0 else -1
        return t_batch_dur, nb_processed, avg, lmsg
