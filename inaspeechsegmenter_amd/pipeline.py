"""Multi-file engine behind `Segmenter.batch_process` and the archive driver.

The reference processes a file list one file at a time: features of file i+1 are extracted on a helper thread while the
main thread runs the two Keras `predict` calls, the Viterbi smoothing and the export of file i
(segmenter.py:297-335, medialist2feats :338-374).  On an MI355X a 5-minute file is ~14 ms of device work, so per-file
launches, copies and Python bookkeeping become the limit.  Here files are processed in SUPER-BATCHES:

  decode threads   N files  ->  int16 PCM as a numpy array (RIFF parse, or the ffmpeg pipe), or -- without ffmpeg -- a source of
                   sources.py, handed on as stored for the device to finish: a WAV at another rate / channel count with
                   Segmenter(resample=True), G.711 and big-endian files (RawSource), FLAC frames (flac.FlacSource), IMA ADPCM
                   and Microsoft ADPCM blocks (sndfmt.AdpcmSource, sndfmt.MsAdpcmSource)
  packer           the PCM of a super-batch (default <= 32 files / ~40 min of audio) is laid end to end in ONE page-locked
                   buffer, every file starting on a multiple of 160 samples: frame t of file f is then frame
                   off_f / 160 + t of the concatenation, and the frames that straddle two files are simply never used
                   (room is left for the sources; the payloads of each class go end to end into a page-locked buffer of its own)
  device worker    ONE H2D copy; per source class ONE more H2D copy of its payloads and ONE launch for all its files of the pass
                   (resample; FLAC decode; IMA ADPCM decode -- the decoders add at most one resample launch each); ONE sidekit
                   launch, one log-energy read-back (with the decoders' status); per-file energy Viterbi (compiled);
                   ONE iss_cnn_probs call for the VAD windows of all files, per-segment Viterbi; ONE call for the
                   gender windows, Viterbi; hand the segment lists to the exporter
  exporter         CSV / TextGrid writers

Four device workers with a context each (own stream, own workspace) take super-batches in turn, so while some are in their
host phases (packing, Viterbi, bookkeeping) the others' kernels run.  Results are identical to per-file processing: every frame and
every 20 ms slot is computed from the same samples by the same kernels (tests/test_gpu_segmenter.py).

"Array or source" is the only distinction made here, and what a source is asked is what sources.py lists: a new format needs
no line in this file.
"""
import queue
import sys
import threading
import time
import warnings

import numpy as np

from . import _native
from . import segmenter as S
from . import sources

FRAME_HOP = sources.FRAME_HOP
MIN_SAMPLES = 400 + FRAME_HOP * 67                  # 68 frames: shorter media take the single-file path (mspec padding)


class _Batch:
    __slots__ = ('idx', 'sigs', 'names', 'errs', 'poffs', 'psize')

    def __init__(self):
        self.idx, self.sigs, self.names, self.errs = [], [], [], {}
        # set by _Worker.run, per part of the pass: where it starts in the resident signal and how many samples it has -- the signal
        # stays resident after the pass, so a caller can read the parts there (vfs.py: iss_vbx_features_resident)
        self.poffs, self.psize = None, None

    def samples(self):                               # 16 kHz samples (a RawSource's size is its resampled length), of every part
        return sum(_parts(s) * (-(-s.size // FRAME_HOP) * FRAME_HOP) for s in self.sigs)

    def parts(self):                                 # signals of the pass: a file split by channel counts one per channel
        return sum(_parts(s) for s in self.sigs)

    def full(self, batch_files, limit_samples):      # the one rule that closes a pass
        return self.parts() >= batch_files or self.samples() >= limit_samples


def _parts(sig):
    """Signals a decoded file writes: an array one, a source what it says (one per selected channel)."""
    return sig.parts if isinstance(sig, sources.Source) else 1


def _name(src):
    """What `decided` carries for an input: a path as given, a file set (io.FileSet, a tuple or list of paths) by its name."""
    from . import io
    return src if isinstance(src, str) else str(io.as_media(src))


_held = sources.held                                # what a decoded signal holds while it waits, for the audio budget


class _AudioBudget:
    """Bounds the decoded-but-not-yet-packed audio by DURATION (the item count of the queue says nothing about memory:
    a 2 h file is 230 MB of PCM16).  A decode thread that holds a decoded signal waits until the signals queued in front
    of it fit the budget again; a single signal larger than the budget passes when nothing else is queued."""

    def __init__(self, max_samples):
        self.max, self.held, self.cv = int(max_samples), 0, threading.Condition()

    def acquire(self, n):
        with self.cv:
            while self.held > 0 and self.held + n > self.max:
                self.cv.wait(0.5)
            self.held += n

    def release(self, n):
        with self.cv:
            self.held -= n
            self.cv.notify_all()


def _decode_stage(items, ffmpeg, nbtry, trydelay, out_q, nthreads, budget=None, resample=False, channels=None, **how):
    """items: [(index, src)].  Puts (index, src, sig | None, errtext | None) on out_q in completion order, then None."""
    import random
    in_q = queue.Queue()
    for it in items:
        in_q.put(it)

    def work():
        while True:
            try:
                i, src = in_q.get_nowait()
            except queue.Empty:
                return
            sig, err, itry = None, None, 0
            while sig is None and itry < nbtry:
                try:
                    sig = S._load_source(src, None, None, ffmpeg, resample, channels, **how)
                except:                                            # noqa: E722  (reference semantics, segmenter.py:364-370)
                    itry += 1
                    err = 'error: ' + str(sys.exc_info()[0])
                    if not isinstance(src, str):                   # a file set (io.FileSet, a tuple or list): which member, and why
                        err += ' ' + str(sys.exc_info()[1])
                    if itry != nbtry:
                        time.sleep(random.random() * trydelay)
            if budget is not None and sig is not None:
                budget.acquire(_held(sig))
            out_q.put((i, src, sig, err))

    ths = [threading.Thread(target=work, daemon=True) for _ in range(max(1, nthreads))]
    for t in ths:
        t.start()

    def closer():
        for t in ths:
            t.join()
        out_q.put(None)
    threading.Thread(target=closer, daemon=True).start()


class _Worker:
    """One device context + the networks of `seg` loaded on it."""

    def __init__(self, seg, ctx=None):
        from . import tables
        self.seg = seg
        if ctx is None:
            ctx = _native.Context(seg.ctx.device)
            ctx.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank())
            ctx.cnn_load(seg.vad.net_id, seg.vad.compiled)
            if seg.detect_gender:
                ctx.cnn_load(seg.gender.net_id, seg.gender.compiled)
            self.owned = True
        else:
            self.owned = False
        self.ctx = ctx
        self.pins = {}                               # page-locked buffers by what they hold: 'signal', or a source class's staged bytes
        # wall seconds this worker spent per phase since the last reset (bench.py reports them: where a step's host time goes)
        self.stats = {k: 0.0 for k in ('pack', 'features', 'energy_host', 'cnn_device', 'smooth_host', 'batches', 'files')}

    def close(self):
        if self.owned:
            self.ctx.close()

    def pinned(self, key, n, dtype):
        """This worker's page-locked buffer `key`, grown on demand to hold n items."""
        cur = self.pins.get(key)
        if cur is None or cur.size < n:
            if cur is not None:
                self.ctx.pinned_free(cur)
            cur = self.pins[key] = self.ctx.pinned_empty((int(n * 1.25) + 4096,), dtype)
        return cur

    def sync_settings(self):
        """Arithmetic mode and workspace cap follow the Segmenter's own context (they may have changed since this
        worker was created: the workers are cached between calls)."""
        if self.owned:
            self.ctx.mirror_settings(self.seg.ctx)

    def run(self, batch):
        """-> [ [(label, start_slot, stop_slot)] per part of the batch ] -- per file, but one per selected channel, in order, for
        a file split by channel --; None for (every part of) a FLAC / IMA ADPCM file whose frames / blocks the device found
        malformed (the ValueError in batch.errs, by file)"""
        seg, ctx = self.seg, self.ctx
        st = self.stats
        t_ = time.perf_counter()
        offs, pos = [], 0                            # per file: where its first part starts
        owner, poffs, psize = [], [], []             # per part: its file, its offset, its samples
        for f, s in enumerate(batch.sigs):
            offs.append(pos)
            stride = -(-s.size // FRAME_HOP) * FRAME_HOP
            for _ in range(_parts(s)):
                owner.append(f); poffs.append(pos); psize.append(s.size)
                pos += stride
        batch.poffs, batch.psize = list(poffs), list(psize)
        buf = self.pinned('signal', pos, np.int16)
        placed, files = {}, {}                       # source class -> [(source, offset in the signal)]; -> [its file]
        for f, (s, o) in enumerate(zip(batch.sigs, offs)):
            if isinstance(s, sources.Source):        # written by its class's kernel (and the resample kernel)
                buf[o:o + s.parts * s.stride] = 0
                placed.setdefault(type(s), []).append((s, o))
                files.setdefault(type(s), []).append(f)
            elif s.dtype == np.int16:
                buf[o:o + s.size] = s
            else:                                    # float sources: what libsndfile's float32 read holds, re-quantised is NOT exact
                raise TypeError('float media take the single-file path')
            buf[o + s.size:o + -(-s.size // FRAME_HOP) * FRAME_HOP] = 0
        # the payloads of each class staged in a page-locked buffer of its own
        groups = [sources.Group(ctx, cls, placed[cls], lambda n, cls=cls: self.pinned(cls, n, np.uint8))
                  for cls in sorted(placed, key=lambda c: c.pass_order)]
        st['pack'] += time.perf_counter() - t_; t_ = time.perf_counter()
        ctx.set_signal(buf[:pos])
        for g in groups:                             # ONE launch per class for all its files of the pass, into the signal above
            g.launch()
        ctx.sidekit()
        loge = ctx.get_loge()
        for g in groups:                             # the frame / block status came back with the log-energy
            g.check(lambda k, exc, g=g: batch.errs.__setitem__(files[g.cls][k], exc))
        st['features'] += time.perf_counter() - t_; t_ = time.perf_counter()
        g0 = [o // FRAME_HOP for o in poffs]
        nfr = [(n - 400) // FRAME_HOP + 1 for n in psize]
        # energy segmentation per part (segmenter.py:261-267)
        lsegs = []
        for f in range(len(owner)):
            if owner[f] in batch.errs:               # a malformed FLAC / ADPCM file: no segments, no network rows, for any part
                lsegs.append([])
                continue
            lsegs.append(S._energy_segments(loge[g0[f]:g0[f] + nfr[f]], seg.energy_ratio))
        st['energy_host'] += time.perf_counter() - t_
        wrs = [S._window_rows(nfr[f]) + np.int32(g0[f]) for f in range(len(lsegs))]
        # Segmenter.dense_batches (an extension, default False): every network on EVERY slot of every file -- the most work
        # the reference semantics can require, independent of what the networks decide (bench.py's "dense" figures); the rows
        # of the `inlabel` segments are then picked from the full result, so the segments are the same
        dense = bool(getattr(seg, 'dense_batches', False))
        if dense:
            wbase = np.concatenate(([0], np.cumsum([len(w) for w in wrs])))
            allw = np.concatenate(wrs)
        for net in ([seg.vad, seg.gender] if seg.detect_gender else [seg.vad]):
            t_ = time.perf_counter()
            # slots of every `inlabel` segment of every file, in order (segmenter.py:156-159), in ONE device call; the
            # per-segment smoothing (:168-178) in ONE host call on np.log of the whole probability array (elementwise: the
            # same values as per-segment np.log calls); run-length encoding vectorised over the pass
            rows, seglen, sel = [], [], []
            for f, lseg in enumerate(lsegs):
                wr = wrs[f]
                for lab, start, stop in lseg:
                    if lab == net.inlabel:
                        rows.append(wr[start:stop])
                        seglen.append(stop - start)
                        if dense:
                            sel.append(np.arange(wbase[f] + start, wbase[f] + stop))
            if not rows:
                st['smooth_host'] += time.perf_counter() - t_; t_ = time.perf_counter()
                if dense and len(allw):              # no `inlabel` segment in the whole pass: dense work does not depend on that
                    net.probs(ctx, allw)
                    st['cnn_device'] += time.perf_counter() - t_
                continue
            allrows = np.concatenate(rows)
            st['smooth_host'] += time.perf_counter() - t_; t_ = time.perf_counter()
            if dense:
                probs, _fin = net.probs(ctx, allw)
                probs = probs[np.concatenate(sel)]
            else:
                probs, _fin = net.probs(ctx, allrows)
            st['cnn_device'] += time.perf_counter() - t_; t_ = time.perf_counter()
            with np.errstate(divide='ignore'):
                logp = np.log(probs)
            states = _native.viterbi_segments(logp, seglen, S.diag_trans_exp(net.viterbi_arg, len(net.outlabels)))
            seg_off = np.concatenate(([0], np.cumsum(seglen)))
            change = np.empty(len(states), dtype=bool)
            change[0] = True
            np.not_equal(states[1:], states[:-1], out=change[1:])
            change[seg_off[:-1]] = True
            run_start = np.flatnonzero(change)
            run_stop = np.concatenate((run_start[1:], [len(states)]))
            run_seg = np.searchsorted(seg_off, run_start, side='right') - 1
            run_lab = states[run_start].tolist()
            rs = (run_start - seg_off[run_seg]).tolist()
            re_ = (run_stop - seg_off[run_seg]).tolist()
            run_seg = run_seg.tolist()
            out, k, sidx = [], 0, 0
            for lseg in lsegs:
                ret = []
                for lab, start, stop in lseg:
                    if lab != net.inlabel:
                        ret.append((lab, start, stop))
                        continue
                    while k < len(run_seg) and run_seg[k] == sidx:
                        ret.append((net.outlabels[run_lab[k]], start + rs[k], start + re_[k]))
                        k += 1
                    sidx += 1
                out.append(ret)
            lsegs = out
            st['smooth_host'] += time.perf_counter() - t_
        st['batches'] += 1
        st['files'] += len(batch.sigs)
        return [None if owner[f] in batch.errs else l for f, l in enumerate(lsegs)]


DEFAULT_BATCH_FILES = 32          # files per device pass at most ...
DEFAULT_BATCH_SECONDS = 40 * 60   # ... and ~40 minutes of audio (120 k slots: four full-size passes of each network).  Smaller
RAMP_SECONDS = 300                # first pass of a call; doubles per pass up to batch_seconds
DEFAULT_WORKERS = 4               # passes with more contexts in flight overlap the host phases better than 32-file passes on
                                  # two contexts did (same box, 128 x 5 min files: 7.2 -> 8.2 audio-hours/s)


def process_files(seg, linput, on_result, skip=None, nbtry=1, trydelay=2., batch_files=None, batch_seconds=None,
                  workers=None, decode_threads=4, channels=None, decided=None, auto_block_sec=None, auto_rule='safe',
                  auto_fade_sec=None):
    """Segment `linput` with the networks of `seg`; on_result(index, src, lseg | None, errtext | None, secs) is called from
    the worker threads (serialised by a lock) as results become available, lseg = [(label, start_sec, stop_sec)], secs =
    this file's share of the processing time of its device pass (the pass's wall time / its files: what the reference's
    per-file 'ok <secs>' message reports, segmenter.py:322-327, when files are processed one by one).
    skip: set of indices not to process.  Device failures (NativeError) and exceptions raised by on_result (unwritable
    outputs) propagate to the caller: the first one is re-raised here once every stage has drained.
    channels='split': every channel of every file on its own; lseg is then a LIST of segment lists, one per channel of the file.
    channels = a list of resample.Mix: those mixes of every file, likewise (segmenter._load_source reads either).
    channels='auto': every file downmixed as its own survey suggests (io.auto_source); lseg is one segment list, as without
    `channels`, and decided((src, survey, mix)) is called before on_result for every file that was processed.
    auto_block_sec (with channels='auto'): every file of two or more channels by the schedule its own timeline suggests
    (io.timeline_source, blocks of that many seconds, decided by auto_rule and cross-faded over auto_fade_sec seconds); decided
    then gets (src, timeline, schedule)."""
    multi = channels is not None and channels != 'auto'        # on_result gets a list of segment lists
    batch_files, batch_seconds = _limits(batch_files, batch_seconds)
    workers = workers or DEFAULT_WORKERS
    items = [(i, src) for i, src in enumerate(linput) if not (skip and i in skip)]
    dec_q = queue.Queue(maxsize=4 * batch_files)
    budget = _AudioBudget(2 * batch_seconds * 16000)        # decoded audio waiting for the packer: <= 2 super-batches
    _decode_stage(items, seg.ffmpeg, nbtry, trydelay, dec_q, decode_threads, budget, getattr(seg, 'resample', False),
                  **({} if channels is None else {'channels': channels}),
                  **({} if auto_block_sec is None else {'auto_block_sec': auto_block_sec, 'auto_rule': auto_rule,
                                                         'auto_fade_sec': auto_fade_sec}))
    batch_q = queue.Queue(maxsize=max(2, workers))
    lock = threading.Lock()
    failure = []

    def packer():
        cur = _Batch()
        nbatch = 0
        ended = False                                              # the decoders' end marker has been read
        try:
            while True:
                it = dec_q.get()
                if it is None:
                    ended = True
                    break
                i, src, sig, err = it
                if sig is not None:
                    budget.release(_held(sig))
                if failure:                                        # a worker failed: drain the decoders, pack nothing more
                    continue
                if sig is None:
                    try:
                        with lock:
                            on_result(i, src, None, err, 0.0)
                    except BaseException as exc:                   # noqa: B902
                        failure.append(exc)
                    continue
                if not sources.batchable(sig) or sig.size < MIN_SAMPLES:
                    batch_q.put(('single', i, src, sig))
                    continue
                cur.idx.append(i); cur.sigs.append(sig); cur.names.append(src)
                # the first passes of a call are short (5, 10, 20 ... minutes of audio) so that the device starts as soon as
                # a few files are decoded instead of after a whole 40-minute pass per worker
                lim_s = min(batch_seconds, RAMP_SECONDS * (1 << min(nbatch, 20)))
                if cur.full(batch_files, lim_s * 16000):
                    batch_q.put(('batch', cur))
                    cur = _Batch()
                    nbatch += 1
            if cur.idx and not failure:
                batch_q.put(('batch', cur))
        except BaseException as exc:                               # noqa: B902  (MemoryError while batching, a bad array, ...)
            # record it and keep draining the decoders -- they block on the bounded queue / the audio budget while holding
            # their PCM -- until their end marker, exactly like the `if failure: continue` path above
            failure.append(exc)
            while not ended:                                       # (an exception AFTER the marker was read: nothing left to drain --
                it = dec_q.get()                                   #  a second get() would block forever)
                if it is None:
                    break
                if it[2] is not None:
                    budget.release(_held(it[2]))
        finally:
            for _ in range(workers):
                batch_q.put(None)

    def work(w):
        # A failure (device error, or an exception out of on_result) is recorded and the loop KEEPS consuming batch_q until
        # the packer's end marker: a worker that simply returned would leave the packer blocked on the bounded queue (and
        # the decode threads behind it) with nobody left to drain it, and process_files would hang instead of raising.
        while True:
            job = batch_q.get()
            if job is None:
                return
            if failure:
                continue
            try:
                t0 = time.time()
                if job[0] == 'single':
                    _, i, src, sig = job
                    try:
                        with warnings.catch_warnings():
                            warnings.simplefilter('ignore')
                            lseg = one_by_one(seg, w.ctx, sig, src)
                        res = (lseg if multi else lseg[0], None)
                    except ValueError as exc:                      # too short to analyse: a per-file error
                        res = (None, 'error: %s %s' % (type(exc), exc))
                    with lock:
                        if decided is not None and res[0] is not None:
                            decided((_name(src),) + (getattr(sig, 'decision', None) or (None, None)))
                        on_result(i, src, res[0], res[1], time.time() - t0)
                    continue
                b = job[1]
                lsegs = w.run(b)
                share = (time.time() - t0) / max(len(lsegs), 1)
                with lock:
                    q = 0
                    for f, (i, src, sig) in enumerate(zip(b.idx, b.names, b.sigs)):
                        mine = lsegs[q:q + _parts(sig)]
                        q += len(mine)
                        if f in b.errs:
                            on_result(i, src, None, 'error: %s %s' % (type(b.errs[f]), b.errs[f]), share)
                            continue
                        mine = [[(lab, a * .02, c * .02) for lab, a, c in lseg] for lseg in mine]
                        if decided is not None:
                            decided((_name(src),) + (getattr(sig, 'decision', None) or (None, None)))
                        on_result(i, src, mine if multi else mine[0], None, share)
            except BaseException as exc:                           # noqa: B902  propagate to the caller's thread
                failure.append(exc)

    ws = _workers(seg, workers)
    for w in ws:
        w.sync_settings()
    threads = [threading.Thread(target=work, args=(w,), daemon=True) for w in ws]
    pk = threading.Thread(target=packer, daemon=True)
    pk.start()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    pk.join()
    if failure:
        raise failure[0]


def _limits(batch_files, batch_seconds):
    """(files, seconds of audio) a device pass holds at most: the defaults where none is given."""
    return batch_files or DEFAULT_BATCH_FILES, batch_seconds or DEFAULT_BATCH_SECONDS


def _workers(seg, n):
    """The first n device workers of `seg` (at least one; the first drives seg's own context).  They are kept with the
    Segmenter between calls: context creation, network upload and the first workspace allocation cost more than a 5-minute file."""
    cache = seg.__dict__.setdefault('_pipeline_workers', [])
    while len(cache) < max(1, n):
        cache.append(_Worker(seg, seg.ctx if not cache else None))
    return cache[:max(1, n)]


def close_workers(seg):
    for w in seg.__dict__.pop('_pipeline_workers', []):
        w.close()


def cut_passes(sigs, batch_files=None, batch_seconds=None):
    """`sigs` in order, cut into device passes under the limits of process_files -> [[index into sigs]]."""
    batch_files, batch_seconds = _limits(batch_files, batch_seconds)
    passes, cur = [], _Batch()
    for k, s in enumerate(sigs):
        cur.idx.append(k); cur.sigs.append(s)
        if cur.full(batch_files, batch_seconds * 16000):
            passes.append(cur.idx)
            cur = _Batch()
    return passes + [cur.idx] if cur.idx else passes


def run_passes(seg, names, sigs, passes):
    """The `passes` (cut_passes) of `sigs`, one after the other on seg's own context -> [(label, start_slot, stop_slot)]
    lists, one per part of every signal of every pass, in that order.  The first malformed file of a pass raises its ValueError."""
    out = []
    for idx in passes:
        batch = _Batch()
        batch.idx, batch.sigs, batch.names = list(idx), [sigs[k] for k in idx], [names[k] for k in idx]
        out += _workers(seg, 1)[0].run(batch)
        if batch.errs:
            raise ValueError(str(batch.errs[min(batch.errs)]))
    return out


def one_by_one(seg, ctx, sig, name='<signal>'):
    """A signal that shares no pass (float, or under 68 frames), on `ctx` -> [[(label, start_sec, stop_sec)] per part]: the
    channels of a file split by channel come back to the host and go one after the other, as any signal alone does."""
    alone = S._parts_pcm(ctx, sig) if getattr(sig, 'sel', None) is not None else [sig]
    out = []
    for one in alone:
        mspec, loge, difflen = S._sig2feats(ctx, one, name)
        out.append([(lab, a * .02, b * .02) for lab, a, b in _slots(seg, ctx, mspec, loge, difflen)])
    return out


def _slots(seg, ctx, mspec, loge, difflen):
    """segment_slots of `seg` on another context (the networks are loaded there under the same ids)."""
    lseg = S._energy_segments(loge, seg.energy_ratio)
    for net in ([seg.vad, seg.gender] if seg.detect_gender else [seg.vad]):
        lseg = net(mspec, lseg, difflen, ctx=ctx)
    return lseg
