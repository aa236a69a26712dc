"""Media decode boundary: anything -> 16 kHz mono samples on the host.

Mirrors io.py:32-79 `media2sig16kmono(medianame, start_sec, stop_sec, ffmpeg, dtype)`:
  * ffmpeg given  -> `ffmpeg -i <media> -f wav -acodec pcm_s16le -ar 16000 -ac 1 [-ss] [-to] pipe:1`
    (same command line, io.py:61-68); non-zero exit raises Exception(stderr) (io.py:72-75).
    The PCM is taken straight from the pipe instead of a TemporaryFile + soundfile.
  * ffmpeg=None   -> direct read; start/stop and http(s) sources raise NotImplementedError
    with the reference's wording (io.py:37-50); the file must already be 16 kHz (io.py:53-55).
Decode stays on the host (north star); soundfile/libsndfile is not available in the target
image, so RIFF/WAVE is parsed here with libsndfile's conversion rules (PCM16 -> x/32768,
unknown chunks skipped).  FLAC (flac.py) reads exactly like its WAV twin, decoded here by the host build of the
device's frame decoder; so do G.711, IMA ADPCM and Microsoft ADPCM in WAV, RF64 / BW64, Wave64, AIFF / AIFF-C, AU and CAF (sndfmt.py: numpy
tables, byte swaps and the host builds of the device's two ADPCM decoders).  A file is read once (`_read_file`) and `_classify` says
from its bytes which parser takes it: a new format is one line there.  `decode_pcm` is the entry the native pipeline uses: it keeps
PCM16 as int16 so the device does the x/32768 scaling (2 B/sample over PCIe, not 4).
`split_source` reads the channels of a file each on its own (an extension: the reference needs one ffmpeg -map_channel run per
channel): a source with a channel selection for the device; `decode_channels` is its host-only twin.
`excerpts` reads time ranges of one file without ffmpeg (an extension: start/stop through decode_pcm keep raising): per range the
samples of the 16 kHz mono twin or a windowed source holding only the bytes it needs; `decode_excerpts` finishes them on the host.
`channel_excerpts` is both at once: time ranges of single channels, windowed sources with a channel selection;
`decode_channel_excerpts` is its host-only twin.
`mix_source` and `mix_excerpts` read weighted sums of a file's channels (resample.py states a mix) where the two above read single
channels: the same sources, an entry of whose selection is a resample.Mix; `decode_mixes` and `decode_mix_excerpts` are the
host-only twins.
`survey_sources` reads what a channel survey needs of a file -- per-channel levels and the cross-products between channels of the
stored frames, measured on the device (Segmenter.survey_channels) --, `survey_channels` is its host-only twin.
`auto_source` reads a file for channels='auto': a source that is staged once, surveyed and then downmixed by the mix its survey
suggests (survey.ChannelSurvey.safe_mix); `decode_auto` is the host-only twin.
`FileSet` is a recording stored as one file per channel or group of channels, read as the interleaved file it stands for: every
whole-file read above takes one (or a tuple or list of member paths) where it takes `medianame`, `set_source` is what the plain
read gives, `decode_set` the host-only twin -- the interleaved, zero-padded stored samples, which no other call ever builds.
"""
import os
import struct
import subprocess

import numpy as np

from . import resample as R
from .sources import RawSource


def _parse_wav(buf, name='<buffer>'):
    """-> (samples ndarray shaped (n,) or (n,ch), sr).  dtype int16 / uint8 / int32 / float32 / float64
    exactly as stored (24-bit widened to int32 << 8)."""
    if len(buf) < 12 or buf[:4] not in (b'RIFF', b'RF64') or buf[8:12] != b'WAVE':
        raise ValueError(f'{name}: not a RIFF/WAVE file')
    pos, fmt, data = 12, None, None
    n = len(buf)
    while pos + 8 <= n:
        cid, size = buf[pos:pos + 4], struct.unpack_from('<I', buf, pos + 4)[0]
        body = pos + 8
        if cid == b'fmt ':
            tag, ch, sr, _, _, bits = struct.unpack_from('<HHIIHH', buf, body)
            if tag == 0xFFFE and size >= 26:                      # WAVE_FORMAT_EXTENSIBLE
                tag = struct.unpack_from('<H', buf, body + 24)[0]
            fmt = (tag, ch, sr, bits)
        elif cid == b'data':
            end = n if (size == 0xFFFFFFFF or body + size > n) else body + size   # piped WAVs carry no length
            data = buf[body:end]
            break
        pos = body + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f'{name}: missing fmt or data chunk')
    tag, ch, sr, bits = fmt
    if tag == 1:
        if bits == 16:
            a = np.frombuffer(data, dtype='<i2', count=len(data) // 2)
        elif bits == 8:
            a = np.frombuffer(data, dtype=np.uint8)
        elif bits == 32:
            a = np.frombuffer(data, dtype='<i4', count=len(data) // 4)
        elif bits == 24:
            raw = np.frombuffer(data, dtype=np.uint8, count=(len(data) // 3) * 3).reshape(-1, 3)
            a = ((raw[:, 0].astype(np.int32) << 8) | (raw[:, 1].astype(np.int32) << 16) | (raw[:, 2].astype(np.int32) << 24))
        else:
            raise ValueError(f'{name}: unsupported PCM width {bits}')
    elif tag == 3:
        a = np.frombuffer(data, dtype='<f4' if bits == 32 else '<f8', count=len(data) // (bits // 8))
    else:
        raise ValueError(f'{name}: unsupported WAVE format tag {tag}')
    if ch > 1:
        a = a[:(len(a) // ch) * ch].reshape(-1, ch)
    return a, sr


def _read_file(medianame):
    with open(medianame, 'rb') as f:
        return f.read()


# ---------------------------------------------------------------------------------------------- file sets
MAX_SET_CHANNELS = 1024


class FileSet:
    """An ordered list of member files that reads as ONE multichannel source (an extension, ffmpeg=None only): a call logger's
    one mono file per direction, a production system's one mono WAV per track.  It reads exactly like its interleaved twin --
    the one file holding the members' channels side by side (member 0's first), as many frames as the longest member, a shorter
    member continued with samples of value 0.0 --, which is never written: the device reads the members where they lie.
    Members share the sample rate and the stored sample format; they may differ in container and in channel count.  Wherever a
    call takes `medianame`, a tuple or list of paths means FileSet(paths).  `name` is what error texts and `decisions` carry."""
    __slots__ = ('members', 'name')

    def __init__(self, members, name=None):
        if isinstance(members, (str, bytes)) or isinstance(members, FileSet):
            raise ValueError(f'FileSet({members!r}): members must be a sequence of paths')
        self.members = tuple(os.fspath(m) for m in members)
        if name is None:
            name = f'set({self.members[0]}, +{len(self.members) - 1})' if self.members else 'set()'
        self.name = str(name)

    def __len__(self):
        return len(self.members)

    def __iter__(self):
        return iter(self.members)

    def __str__(self):
        return self.name

    def __repr__(self):
        return f'FileSet({list(self.members)!r}, name={self.name!r})'

    def __eq__(self, other):
        return isinstance(other, FileSet) and (self.members, self.name) == (other.members, other.name)

    def __hash__(self):
        return hash((self.members, self.name))


def as_media(medianame):
    """`medianame` as the reads below take it: a path as given; a FileSet, tuple or list of one member that member's path (a
    one-member set is that file); any other tuple or list FileSet(medianame)."""
    if isinstance(medianame, (tuple, list)):
        medianame = FileSet(medianame)
    if isinstance(medianame, FileSet) and len(medianame) == 1:
        return medianame.members[0]
    return medianame


def _no_set_ranges(medianame, what='time ranges'):
    if isinstance(as_media(medianame), FileSet):
        raise ValueError(f'{as_media(medianame)}: {what} of a set are not supported; read the whole set, or cut the members '
                         f'beforehand')


class _SetSound:
    """A parsed file set, answering what a sndfmt.Sound answers to the reads below: `sr`, `ch` (all members'), `n` (the longest
    member's frames), `kind`, `stored()` (the interleaved twin's samples, io.decode_set), and the sources the device reads."""
    __slots__ = ('name', 'sr', 'ch', 'n', 'kind', 'parts', 'fmt', 'full')

    def __init__(self, fs):
        from . import flac, sndfmt
        name = self.name = fs.name
        if len(fs) == 0:
            raise ValueError(f'{name}: the set is empty')
        self.parts = []
        for m in fs.members:
            _check_local(m)
            h, full = _survey_parsed(m, False)
            label = 'FLAC' if isinstance(h, flac.FlacStream) else sndfmt._BLOCK[h.kind].label if h.kind in sndfmt._BLOCK else None
            if label is not None:
                raise ValueError(f'{name}: member {m}: {label} is not supported in a file set')
            if h.n < 1:
                raise ValueError(f'{name}: member {m} has no frames')
            self.parts.append((m, h, full) + h.raw()[::-1])      # (..., its ISS_RS_* format, its samples as stored)
        m0, h0, self.full, self.fmt, _ = self.parts[0]
        for m, h, full, fmt, _ in self.parts[1:]:
            if h.sr != h0.sr:
                raise ValueError(f'{name}: the members differ in sample rate: {m0} is sampled at {h0.sr} Hz, {m} at {h.sr} Hz')
            if (fmt, full) != (self.fmt, self.full):
                raise ValueError(f'{name}: the members differ in stored sample format: {m0} holds {_kind_text(h0, self.full)} samples, '
                                 f'{m} holds {_kind_text(h, full)}')
        self.sr, self.kind = h0.sr, h0.kind
        self.ch = sum(p[1].ch for p in self.parts)
        self.n = max(p[1].n for p in self.parts)
        if self.ch > MAX_SET_CHANNELS:
            raise ValueError(f'{name}: {self.ch} channels in all, a set holds at most {MAX_SET_CHANNELS}')

    def _xs(self):
        return [p[4] for p in self.parts]

    def stored(self):
        """The samples io._parse_wav would return for the interleaved twin: (n, ch), a shorter member continued with the stored
        value of 0.0 (128 for unsigned bytes, else 0)."""
        cols = [p[1].stored() for p in self.parts]
        out = np.full((self.n, self.ch), 128 if cols[0].dtype == np.uint8 else 0, dtype=cols[0].dtype)
        c = 0
        for a in cols:
            a = a.reshape(a.shape[0], -1)
            out[:a.shape[0], c:c + a.shape[1]] = a
            c += a.shape[1]
        return out

    def source(self, resample=False):
        from .sources import SetSource
        if not resample:
            need_16k_mono(self.name, self.sr, self.ch)
        R.check_rate(self.sr)
        return SetSource(self._xs(), self.sr, self.fmt, None, self.name)

    def split_source(self, sel):
        from .sources import SetSource
        return SetSource(self._xs(), self.sr, self.fmt, sel, self.name)

    def auto_source(self, full):
        from .sources import SetAuto
        return SetAuto(self._xs(), self.sr, self.fmt, full, self.name)

    def survey_source(self, full):
        from .sources import SetSurvey
        return SetSurvey(self._xs(), self.sr, self.fmt, full, self.name)


def _kind_text(h, full):
    """A member's stored sample format for a refusal (24-bit PCM of a plain WAV file is parsed as the int32 it is widened to)."""
    kind = 'i24' if h.kind == 'i32' and full == R.SURVEY_FULL['i24'] else h.kind
    return f'{"big-endian " if h.big and kind not in ("u8", "i8", "ulaw", "alaw") else ""}{kind}'


def decode_set(members):
    """Host-only twin of a file set -> (the interleaved, zero-padded stored samples (n, C), sr): what decode_source would return
    for the set's interleaved twin.  They go straight into resample.resample_ref, mix_ref and survey_ref.  ValueError as the
    device read raises it: an empty set, members that differ in rate or stored format, a coded or empty member, more than 1024
    channels."""
    fs = members if isinstance(members, FileSet) else FileSet(members)
    if len(fs) == 1:
        x, sr = decode_source(fs.members[0])
        return x.reshape(x.shape[0], -1), sr
    h = _SetSound(fs)
    return h.stored(), h.sr


def set_source(members, resample=False):
    """What Segmenter reads for a file set: a sources.SetSource (the members' bytes as stored; the device downmixes the set as
    its interleaved twin would be), or for a one-member set what the file's own read gives.  Without `resample` a set is refused
    as its twin would be (need_16k_mono: the rate first, then the channel count)."""
    fs = as_media(members if isinstance(members, FileSet) else FileSet(members))
    if not isinstance(fs, FileSet):
        buf = _read_file(fs)
        what = _classify(buf, fs)
        return what.source(resample) if what is not None else source_of(*_parse_wav(buf, fs), fs, resample)
    return _SetSound(fs).source(resample)


def _read_range(path, offset, size):
    """`size` bytes of the file at `path` from byte `offset` (fewer at its end).  Every read of the excerpt path (`excerpts`)
    goes through here, so what an excerpt costs in disk reads can be counted."""
    with open(path, 'rb') as f:
        f.seek(offset)
        return f.read(size)


def _classify(buf, name):
    """What the bytes of a file are to the ffmpeg-free read: a flac.FlacStream, a sndfmt.Sound (G.711 / IMA / Microsoft ADPCM WAV, RF64,
    Wave64, AIFF, AU, CAF), or None for what _parse_wav reads or refuses.  One line per format; what comes back has `sr`,
    `stored()` (the host decode) and `source(resample)` (what Segmenter reads).  (flac and sndfmt import this
    module for need_16k_mono and _to_float, so they are imported here and not at the top.)"""
    from . import flac, sndfmt
    if flac.is_flac(buf):
        return flac.FlacStream(buf, name)
    if flac.is_ogg_flac(buf):
        raise ValueError(f'{name}: Ogg-FLAC (FLAC in an Ogg container) is not supported without ffmpeg')
    return sndfmt.parse(buf, name)


def _stored(what, buf, name):
    """what = _classify(buf, name) -> (samples as stored, sr) as _parse_wav returns them (for the WAV twin), decoded on the host."""
    return _parse_wav(buf, name) if what is None else (what.stored(), what.sr)


def _to_float(a, dtype):
    """libsndfile's integer -> float scaling."""
    if a.dtype == np.int16:
        return (a.astype(np.float64) / 32768.0).astype(dtype)
    if a.dtype == np.uint8:
        return ((a.astype(np.float64) - 128.0) / 128.0).astype(dtype)
    if a.dtype == np.int32:
        return (a.astype(np.float64) / 2147483648.0).astype(dtype)
    return a.astype(dtype)


def _run_ffmpeg(medianame, start_sec, stop_sec, ffmpeg):
    cmd = [ffmpeg, '-i', medianame, '-f', 'wav', '-acodec', 'pcm_s16le', '-ar', '16000', '-ac', '1']
    if start_sec is not None:
        cmd += ['-ss', '%f' % start_sec]
    if stop_sec is not None:
        cmd += ['-to', '%f' % stop_sec]
    cmd += ['pipe:1']
    ret = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if ret.returncode != 0:
        raise Exception(ret.stderr)
    a, fs = _parse_wav(ret.stdout, medianame)
    assert fs == 16000
    return a


def _check_no_ffmpeg(medianame, start_sec, stop_sec):
    if start_sec is not None or stop_sec is not None:
        raise NotImplementedError(
            f'start_sec={start_sec} and stop_sec={stop_sec} cannot be set '
            f' when running inaSpeechSegmenter without ffmpeg. Please cut '
            f'down your audio files beforehand or use ffmpeg.')
    if isinstance(medianame, FileSet):
        for m in medianame.members:
            _check_no_ffmpeg(m, None, None)
        return
    if medianame.startswith('http://') or medianame.startswith('https://'):
        raise NotImplementedError(
            f'Without ffmpeg you cannot process media content on http '
            f'servers. You need to download your audio files beforehand '
            f'or use ffmpeg. You gave medianame={medianame}.')


def need_16k(name, sr):
    """The rate half of need_16k_mono, for reads that take the channels apart."""
    assert sr == 16_000, \
        f'Without ffmpeg, inaSpeechSegmenter can only take files sampled ' \
        f'at 16000 Hz. The file {name} is sampled at {sr} Hz.'


def need_16k_mono(name, sr, channels):
    """The refusal of the ffmpeg-free read without `resample` (io.py:53-55), the same for every format: rate first."""
    need_16k(name, sr)
    if channels != 1:
        raise ValueError(f'{name}: {channels} channels; without ffmpeg only mono files are supported')


def source_of(x, sr, name, resample=False):
    """What Segmenter reads for samples as stored on the host: the 16 kHz mono array (int16, or float32 for the float path);
    anything else is refused without `resample` and handed to the device resampler as a RawSource with it."""
    if sr == R.SR_OUT and x.ndim == 1:
        return np.ascontiguousarray(x) if x.dtype == np.int16 else np.ascontiguousarray(_to_float(x, np.float32))
    if not resample:
        need_16k_mono(name, sr, 1 if x.ndim == 1 else x.shape[1])
    R.check_rate(sr)
    return RawSource(x, sr)


def decode_pcm(medianame, start_sec=None, stop_sec=None, ffmpeg='ffmpeg'):
    """16 kHz mono samples for the device: int16 when the source is PCM16 (always, through
    ffmpeg), else float32 holding exactly what soundfile's float32 read would return."""
    medianame = as_media(medianame)
    if isinstance(medianame, FileSet) and ffmpeg is not None:
        raise ValueError(f'{medianame}: file sets are read without ffmpeg (Segmenter(ffmpeg=None)); ffmpeg={ffmpeg!r} reads one '
                         f'file per run')
    if ffmpeg is None:
        _check_no_ffmpeg(medianame, start_sec, stop_sec)
        a, sr = decode_source(medianame)
        need_16k_mono(medianame, sr, 1 if a.ndim == 1 else a.shape[1])
    else:
        a = _run_ffmpeg(medianame, start_sec, stop_sec, ffmpeg)
    if a.dtype == np.int16:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(_to_float(a, np.float32))


def decode_source(medianame):
    """ffmpeg-free read of a WAV, FLAC or sndfmt.py file: -> (samples as stored, (n,) or (n, C), sr).  Nothing is converted:
    the device downmixes, resamples and quantises (inaspeechsegmenter_amd/resample.py).  A file set: decode_set."""
    medianame = as_media(medianame)
    if isinstance(medianame, FileSet):
        return decode_set(medianame)
    buf = _read_file(medianame)
    return _stored(_classify(buf, medianame), buf, medianame)


def media2sig16kmono(medianame, start_sec=None, stop_sec=None, ffmpeg='ffmpeg', dtype='float64'):
    """Reference-compatible signature and result (float array of `dtype`)."""
    a = decode_pcm(medianame, start_sec, stop_sec, ffmpeg)
    return _to_float(a, np.dtype(dtype)) if a.dtype == np.int16 else a.astype(dtype)


# ---------------------------------------------------------------------------------------------- channels of a file, each on its own
def channel_selection(name, channels, nch):
    """The selection `channels` of a file of `nch` channels as a list: None = all, ascending; else 0-based indices in the order
    given (repeats allowed).  ValueError, naming the file: an empty selection, an index outside the file's channels."""
    if channels is None:
        return list(range(nch))
    if isinstance(channels, (str, bytes)):
        raise ValueError(f'{name}: channels={channels!r} must be None or a sequence of channel indices')
    sel = [int(ch) for ch in channels]
    if not sel:
        raise ValueError(f'{name}: empty channel selection')
    for ch in sel:
        if not 0 <= ch < nch:
            raise ValueError(f'{name}: channel {ch} is outside the file\'s {nch} channel{"s" if nch > 1 else ""} (0 .. {nch - 1})')
    return sel


def channel_name(dst, k):
    """The output of channel k of a file whose unsplit output is `dst`: a.csv -> a.ch<k>.csv."""
    stem, ext = os.path.splitext(dst)
    return f'{stem}.ch{k}{ext}'


def _check_local(medianame):
    if isinstance(medianame, FileSet):
        for m in medianame.members:
            _check_local(m)
        return
    if medianame.startswith('http://') or medianame.startswith('https://'):
        raise ValueError(f'{medianame}: the channels of media on http servers cannot be read; download the file beforehand')


def split_source(medianame, channels=None, resample=False):
    """-> (sel, sig): the selection as a list, and what Segmenter reads for it.  A file of two or more channels gives a source
    of sources.py carrying the selection (RawSource, flac.FlacSource, sndfmt.AdpcmSource: one signal per selected channel, the
    16 kHz twin of that channel alone); a one-channel file gives what the whole-file read gives (sel is then all zeros).
    Without `resample` a rate other than 16 kHz is refused as the whole-file read refuses it; the channel count is not.
    A file set gives a sources.SetSource carrying the selection, channels counted across its members."""
    medianame = as_media(medianame)
    _check_local(medianame)
    if isinstance(medianame, FileSet):
        what = _SetSound(medianame)
        sel = channel_selection(what.name, channels, what.ch)
        if not resample:
            need_16k(what.name, what.sr)
        R.check_rate(what.sr)
        return sel, what.split_source(sel)
    buf = _read_file(medianame)
    what = _classify(buf, medianame)
    if what is None:
        x, sr = _parse_wav(buf, medianame)
        nch = 1 if x.ndim == 1 else x.shape[1]
    else:
        nch, sr = what.ch, what.sr
    sel = channel_selection(medianame, channels, nch)
    if nch == 1:
        return sel, what.source(resample) if what is not None else source_of(x, sr, medianame, resample)
    if not resample:
        need_16k(medianame, sr)
    R.check_rate(sr)
    return sel, RawSource(x, sr, sel=sel) if what is None else what.split_source(sel)


def decode_channels(medianame, channels=None, resample=True):
    """Host-only twin of Segmenter.load_pcm_channels: [resample.resample_ref(stored[:, c], sr) for c in channels] for a file of
    two or more channels (stored, sr = decode_source(medianame)), [decode_pcm(medianame, ffmpeg=None)] per selected entry for a
    one-channel file.  channels: None (all, ascending) or 0-based indices in the order given.  resample=False refuses a rate
    other than 16 kHz as Segmenter(resample=False) does."""
    medianame = as_media(medianame)
    _check_local(medianame)
    x, sr = decode_source(medianame)
    nch = 1 if x.ndim == 1 else x.shape[1]
    sel = channel_selection(medianame, channels, nch)
    if nch == 1:
        if sr != R.SR_OUT and resample:
            return [R.resample_ref(x, sr)] * len(sel)
        return [decode_pcm(medianame, ffmpeg=None)] * len(sel)
    if not resample:
        need_16k(medianame, sr)
    R.check_rate(sr)
    return [R.resample_ref(x[:, ch], sr) for ch in sel]


# ---------------------------------------------------------------------------------------------- mixes: weighted sums of channels
def mix_name(dst, k):
    """The output of mix k of a file whose unmixed output is `dst`: a.csv -> a.mix<k>.csv."""
    stem, ext = os.path.splitext(dst)
    return f'{stem}.mix{k}{ext}'


def mix_source(medianame, mixes, resample=False):
    """-> (mixes, sig): the mix specification as a list of resample.Mix (resample.normalise_mixes against the file's channel
    count: ValueError naming the file, the mix and the reason), and what Segmenter reads for it: a source of sources.py whose
    selection is that list (RawSource, flac.FlacSource, sndfmt.AdpcmSource and its Microsoft twin), one signal per mix,
    resample.mix_ref(stored, sr, mix) of the file's host decode.  A one-channel file is no exception (its mixes name channel 0),
    and the output is PCM16 also where the whole-file read takes the float path.  Without `resample` a rate other than 16 kHz
    is refused as the whole-file read refuses it.  A file set gives a sources.SetSource whose selection is the list."""
    medianame = as_media(medianame)
    _check_local(medianame)
    R.normalise_mixes(mixes, None, medianame)                    # (what can be refused before the file is read)
    if isinstance(medianame, FileSet):
        what, x = _SetSound(medianame), None
    else:
        buf = _read_file(medianame)
        what = _classify(buf, medianame)
    if what is None:
        x, sr = _parse_wav(buf, medianame)
        nch = 1 if x.ndim == 1 else x.shape[1]
    else:
        nch, sr = what.ch, what.sr
    mixes = R.normalise_mixes(mixes, nch, medianame)
    if not resample:
        need_16k(medianame, sr)
    R.check_rate(sr)
    return mixes, RawSource(x, sr, sel=mixes) if what is None else what.split_source(mixes)


def decode_mixes(medianame, mixes, resample=True):
    """Host-only twin of Segmenter.load_pcm_mixes: [resample.mix_ref(stored, sr, mix) for mix in mixes], stored and sr from
    decode_source(medianame).  resample=False refuses a rate other than 16 kHz as Segmenter(resample=False) does."""
    medianame = as_media(medianame)
    _check_local(medianame)
    R.normalise_mixes(mixes, None, medianame)
    x, sr = decode_source(medianame)
    mixes = R.normalise_mixes(mixes, 1 if x.ndim == 1 else x.shape[1], medianame)
    if not resample:
        need_16k(medianame, sr)
    R.check_rate(sr)
    return [R.mix_ref(x, sr, m) for m in mixes]


# ---------------------------------------------------------------------------------------------- excerpts (time ranges of a file)
def _check_range(name, start_sec, stop_sec):
    """What can be refused of a range before the file is opened."""
    import math
    if isinstance(start_sec, bool) or not isinstance(start_sec, (int, float, np.integer, np.floating)) or \
            not math.isfinite(start_sec) or start_sec < 0:
        raise ValueError(f'{name}: start_sec={start_sec!r} must be a finite number of seconds, 0 or more')
    if stop_sec is not None:
        if isinstance(stop_sec, bool) or not isinstance(stop_sec, (int, float, np.integer, np.floating)) or math.isnan(stop_sec):
            raise ValueError(f'{name}: stop_sec={stop_sec!r} must be a number of seconds or None')
        if stop_sec <= start_sec:
            raise ValueError(f'{name}: stop_sec={stop_sec!r} is not after start_sec={start_sec!r}')


def excerpt_bounds(name, n16, start_sec, stop_sec):
    """-> (a, b): the samples of the file's 16 kHz mono twin (n16 of them) that the range (start_sec, stop_sec) means:
    a = floor(start_sec * 16000 + 0.5), b = n16 for stop_sec None, else min(n16, floor(stop_sec * 16000 + 0.5)).
    This rounding is a definition: ffmpeg's own for -ss / -to was not at hand to pin it.  ValueError (naming the file) for a
    start at or past the end, and for fewer than 400 samples."""
    import math
    _check_range(name, start_sec, stop_sec)
    a = math.floor(start_sec * R.SR_OUT + 0.5)
    b = n16 if stop_sec is None or math.isinf(stop_sec) else min(n16, math.floor(stop_sec * R.SR_OUT + 0.5))
    if a >= n16:
        raise ValueError(f'{name}: start_sec={start_sec!r} is at or past the end of the file, which lasts '
                         f'{n16 / R.SR_OUT:.3f} s ({n16} samples at 16 kHz)')
    if b - a < 400:
        raise ValueError(f"media {name}: {b - a} samples, less than one 25 ms analysis window")
    return a, b


def _twin_length(h, resample):
    """-> (is the parsed file `h` 16 kHz mono?, the length of its 16 kHz mono twin).  A file that is not is refused as the
    whole-file read refuses it: without `resample` altogether (need_16k_mono), with it for a rate the resampler does not take."""
    mono16k = h.sr == R.SR_OUT and h.ch == 1
    if not mono16k:
        if not resample:
            need_16k_mono(h.name, h.sr, h.ch)
        R.check_rate(h.sr)
    return mono16k, h.n if mono16k else R.out_len(h.n, h.sr)


def _sound_excerpts(h, ranges, resample):
    """The excerpts of a sndfmt.Sound or SoundHeader `h`: arrays where the whole-file read hands on an array (16 kHz mono:
    the bytes of [a, b) alone, expanded as sndfmt.source expands the file), windowed sources for the device otherwise."""
    from . import sndfmt
    from .sources import RawExcerpt
    mono16k, n16 = _twin_length(h, resample)
    out = []
    for start, stop in ranges:
        a, b = excerpt_bounds(h.name, n16, start, stop)
        blocks = sndfmt.block_excerpt(h, 'pcm' if mono16k else 'resample', a, b)
        if blocks is not None:
            out.append(blocks)
        elif mono16k:
            x = sndfmt.sub_sound(h, a, b)[0].stored()
            out.append(np.ascontiguousarray(x) if x.dtype == np.int16 else np.ascontiguousarray(_to_float(x, np.float32)))
        else:
            j_lo, j_hi = R.input_span(h.sr, h.n, a, b - a)
            sub, _ = sndfmt.sub_sound(h, j_lo, j_hi + 1)
            out.append(RawExcerpt(sub, *sub.raw(), a, b, j_lo, h.n))
    return out


def excerpts(medianame, ranges, resample=False):
    """The time ranges [(start_sec, stop_sec | None)] of one file, read without ffmpeg: per range the samples [a, b) of the
    file's 16 kHz mono twin (excerpt_bounds) as a numpy array, or a windowed source of sources.py that the device -- or its
    `host()` -- turns into exactly those samples, holding only the bytes it needs.  None stands for "as the whole-file read
    does, sliced" (the float path of 24-bit FLAC; a WAV whose chunk sizes need the whole file): the caller decodes the file once.
    A plain RIFF/WAVE file is read by byte ranges (its chunk headers, then per range the frames or IMA blocks needed); every
    other container, and FLAC -- whose frame index needs the scan --, is read whole once, and the ranges are cut from its bytes.
    Ranges are validated before any sample is read where the header allows it; without `resample` a file that is not 16 kHz
    mono is refused as the whole-file read refuses it (need_16k_mono: the rate first)."""
    from . import flac, sndfmt
    _no_set_ranges(medianame)
    medianame = as_media(medianame)
    ranges = [tuple(r) for r in ranges]
    for start, stop in ranges:
        _check_range(medianame, start, stop)
    _check_no_ffmpeg(medianame, None, None)
    h = sndfmt.read_header(medianame)
    if h is None:
        buf = _read_range(medianame, 0, os.path.getsize(medianame))
        h = _classify(buf, medianame)
        if h is None:                                             # a WAV only the whole-file read can judge (or refuse)
            return [None] * len(ranges)
    if not isinstance(h, flac.FlacStream):
        return _sound_excerpts(h, ranges, resample)
    mono16k, n16 = _twin_length(h, resample)
    out = []
    for start, stop in ranges:
        a, b = excerpt_bounds(h.name, n16, start, stop)
        out.append(None if mono16k and h.bps > 16 else flac.FlacExcerpt(h, 'pcm' if mono16k else 'resample', a, b))
    return out


def decode_excerpts(medianame, ranges, resample=False):
    """Host-only twin of Segmenter.load_pcm_excerpts: [the samples [a, b) of the file's 16 kHz mono twin, per range], by the
    host builds of the decoders (compiled FLAC / IMA, numpy G.711) on the frames, blocks and bytes of each excerpt alone, and
    a windowed resample.resample_ref for sources at another rate or channel count."""
    from .sources import Source
    ranges = [tuple(r) for r in ranges]
    sigs = excerpts(medianame, ranges, resample)
    whole = None
    out = []
    for (start, stop), s in zip(ranges, sigs):
        if s is None:
            if whole is None:
                x, sr = decode_source(medianame)
                whole = source_of(x, sr, medianame, resample)
                if isinstance(whole, Source):
                    whole = R.resample_ref(x, sr)
            a, b = excerpt_bounds(medianame, whole.size, start, stop)
            s = whole[a:b]
        out.append(s.host() if isinstance(s, Source) else s)
    return out


# ---------------------------------------------------------------------------------------------- excerpts of single channels
def channel_excerpts(medianame, ranges, channels=None, resample=False):
    """-> (sel, [source | None per range]): the time ranges of `excerpts`, of the channels `split_source` selects.  For a file
    of two or more channels every range is a windowed source carrying the selection (sources.RawExcerpt, flac.FlacExcerpt,
    sndfmt.AdpcmExcerpt: one signal per selected channel, the samples [a, b) of that channel's 16 kHz twin, a and b from
    excerpt_bounds on the twin's length), holding only the bytes, frames or blocks the range needs.  A one-channel file gives
    what `excerpts` gives (sel is then all zeros).  Ranges are validated as `excerpts` validates them, the selection by
    channel_selection; without `resample` a rate other than 16 kHz is refused, the channel count is not.  A plain RIFF/WAVE
    file is read by byte ranges; every other container, and FLAC, is read whole once."""
    return _selected_excerpts(medianame, ranges, lambda nch: channel_selection(medianame, channels, nch), resample, True)


def _selected_excerpts(medianame, ranges, select, resample, mono_plain):
    """channel_excerpts and mix_excerpts: `select(channel count)` -> the selection (channel indices, or mixes); mono_plain: a
    one-channel file gives what `excerpts` gives."""
    from . import flac, sndfmt
    from .sources import RawExcerpt
    _no_set_ranges(medianame)
    medianame = as_media(medianame)
    ranges = [tuple(r) for r in ranges]
    for start, stop in ranges:
        _check_range(medianame, start, stop)
    _check_local(medianame)
    h = sndfmt.read_header(medianame)
    if h is None:
        buf = _read_range(medianame, 0, os.path.getsize(medianame))
        h = _classify(buf, medianame)
        if h is None:                                             # a WAV only the whole-file read can judge (or refuse)
            x, sr = _parse_wav(buf, medianame)
            kind = {'uint8': 'u8', 'int16': 'i16', 'int32': 'i32', 'float32': 'f32', 'float64': 'f64'}[x.dtype.name]
            x = np.ascontiguousarray(x)                           # (24-bit: widened, as the whole-file read stages it)
            h = sndfmt.Sound(medianame, sr, 1 if x.ndim == 1 else x.shape[1], kind, False, x.reshape(-1).view(np.uint8), 0)
    sel = select(h.ch)
    if h.ch == 1 and mono_plain:
        return sel, excerpts(medianame, ranges, resample)
    if not resample:
        need_16k(medianame, h.sr)
    R.check_rate(h.sr)
    n16 = R.out_len(h.n, h.sr)
    out = []
    for start, stop in ranges:
        a, b = excerpt_bounds(medianame, n16, start, stop)
        if isinstance(h, flac.FlacStream):
            out.append(flac.FlacExcerpt(h, 'resample', a, b, sel))
            continue
        blocks = sndfmt.block_excerpt(h, 'resample', a, b, sel)
        if blocks is not None:
            out.append(blocks)
        else:
            j_lo, j_hi = R.input_span(h.sr, h.n, a, b - a)
            sub, _ = sndfmt.sub_sound(h, j_lo, j_hi + 1)
            out.append(RawExcerpt(sub, *sub.raw(), a, b, j_lo, h.n, sel))
    return sel, out


def decode_channel_excerpts(medianame, ranges, channels=None, resample=True):
    """Host-only twin of Segmenter.load_pcm_channel_excerpts: out[r][k] = the samples [a, b) of decode_channels(medianame,
    [sel[k]])[0] for range r, by the host builds of the decoders on the frames, blocks and bytes of each excerpt alone and a
    windowed resample.resample_ref per selected channel; [decode_excerpts(...)[r]] * len(sel) for a one-channel file."""
    from .sources import Source
    ranges = [tuple(r) for r in ranges]
    sel, sigs = channel_excerpts(medianame, ranges, channels, resample)
    if not all(isinstance(s, Source) and s.sel is not None for s in sigs):          # a one-channel file
        return [[one] * len(sel) for one in decode_excerpts(medianame, ranges, resample)]
    return [s.host() for s in sigs]


# ---------------------------------------------------------------------------------------------- excerpts of mixes
def mix_excerpts(medianame, ranges, mixes, resample=False):
    """-> (mixes, [source per range]): the time ranges of `excerpts`, of the mixes `mix_source` normalises: every range a
    windowed source whose selection is the list of resample.Mix (sources.RawExcerpt, flac.FlacExcerpt, sndfmt.AdpcmExcerpt: one
    signal per mix, the samples [a, b) of that mix's 16 kHz twin), holding only the bytes, frames or blocks the range needs.
    Ranges, rate and reads as for channel_excerpts; a one-channel file is no exception."""
    R.normalise_mixes(mixes, None, medianame)
    return _selected_excerpts(medianame, ranges, lambda nch: R.normalise_mixes(mixes, nch, medianame), resample, False)


def decode_mix_excerpts(medianame, ranges, mixes, resample=True):
    """Host-only twin of Segmenter.load_pcm_mix_excerpts: out[r][k] = the samples [a, b) of decode_mixes(medianame, [mixes[k]])[0]
    for range r, by the host builds of the decoders on the frames, blocks and bytes of each excerpt alone and a windowed
    resample.mix_ref per mix."""
    return [s.host() for s in mix_excerpts(medianame, ranges, mixes, resample)[1]]


# ---------------------------------------------------------------------------------------------- channel survey
def survey_bounds(name, frames, sr, start_sec, stop_sec):
    """-> (a, b): the stored frames of a file of `frames` frames at `sr` Hz that the range (start_sec, stop_sec) means:
    a = floor(start_sec * sr + 0.5), b = frames for stop_sec None, else min(frames, floor(stop_sec * sr + 0.5)) -- excerpt_bounds'
    rounding at the file's own rate.  ValueError (naming the file) for a range that holds no frame of the file."""
    import math
    _check_range(name, start_sec, stop_sec)
    a = math.floor(start_sec * sr + 0.5)
    b = frames if stop_sec is None or math.isinf(stop_sec) else min(frames, math.floor(stop_sec * sr + 0.5))
    if b - a < 1:
        raise ValueError(f'{name}: the range ({start_sec!r}, {stop_sec!r}) holds no frame of the file, which lasts '
                         f'{frames / sr:.3f} s ({frames} frames at {sr} Hz)')
    return a, b


def _wav_bits(buf):
    """Bits per sample of the `fmt ` chunk of a RIFF/WAVE buffer _parse_wav has read."""
    pos = 12
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack_from('<I', buf, pos + 4)[0]
        if cid == b'fmt ':
            return struct.unpack_from('<H', buf, pos + 22)[0]
        pos += 8 + size + (size & 1)
    return 0


def _survey_parsed(medianame, header_ok):
    """-> (h, full): the file parsed for a survey -- a flac.FlacStream, a sndfmt.Sound, or with header_ok the
    sndfmt.SoundHeader of a plain RIFF/WAVE file, whose samples are then read by byte ranges -- and the fullscale threshold of
    its stored format (resample.SURVEY_FULL).  A file set: its _SetSound, and the threshold its members share."""
    from . import flac, sndfmt
    medianame = as_media(medianame)
    _check_local(medianame)
    if isinstance(medianame, FileSet):
        h = _SetSound(medianame)
        return h, h.full
    h = sndfmt.read_header(medianame) if header_ok else None
    if h is None:
        buf = _read_file(medianame)
        h = _classify(buf, medianame)
        if h is None:                                             # what _parse_wav reads (or refuses)
            x, sr = _parse_wav(buf, medianame)
            kind = {'uint8': 'u8', 'int16': 'i16', 'int32': 'i32', 'float32': 'f32', 'float64': 'f64'}[x.dtype.name]
            full = R.SURVEY_FULL['i24' if kind == 'i32' and _wav_bits(buf) == 24 else kind]
            x = np.ascontiguousarray(x)                           # (24-bit: widened, as the whole-file read stages it)
            return sndfmt.Sound(medianame, sr, 1 if x.ndim == 1 else x.shape[1], kind, False, x.reshape(-1).view(np.uint8), 0), full
    if isinstance(h, flac.FlacStream):
        return h, R.SURVEY_FULL[{8: 'i8', 16: 'i16', 24: 'i24'}[h.bps]]
    return h, R.SURVEY_FULL[h.kind]


def _survey_spans(h, ranges):
    return [(0, h.n)] if ranges is None else [survey_bounds(h.name, h.n, h.sr, start, stop) for start, stop in ranges]


def survey_channels(medianame, ranges=None):
    """Host-only twin of Segmenter.survey_channels: the file decoded as decode_source decodes it, then resample.survey_ref on
    its frames -> a survey.ChannelSurvey of the whole file (ranges None), or one per time range (start_sec, stop_sec | None),
    frames [a, b) by survey_bounds.  ValueError for a range that holds no frame."""
    from .survey import ChannelSurvey
    if ranges is not None:
        _no_set_ranges(medianame, 'ranges')
        ranges = [tuple(r) for r in ranges]
        for start, stop in ranges:
            _check_range(medianame, start, stop)
    h, full = _survey_parsed(medianame, False)
    spans = _survey_spans(h, ranges)
    x = h.stored()
    out = [ChannelSurvey(R.survey_ref(x, full, a, b), h.sr, a) for a, b in spans]
    return out[0] if ranges is None else out


# ---------------------------------------------------------------------------------------------- survey-guided downmix (channels='auto')
def _auto_parsed(medianame):
    """-> (the file parsed as a survey parses it, its fullscale threshold, is it one of two or more channels with frames?)."""
    medianame = as_media(medianame)
    _check_no_ffmpeg(medianame, None, None)
    h, full = _survey_parsed(medianame, False)
    return h, full, h.ch > 1 and h.n > 0


def auto_source(medianame, resample=False):
    """What Segmenter reads for channels='auto'.  A one-channel file gives the samples the whole-file read gives, from what
    that read hands on (its array, a RawSource, the float path) -- but a FLAC or ADPCM file that shares passes comes as its
    coder's two-step class too ('pcm' into the signal as ever, or staged and resampled as it is, with no survey and no
    decision), so that a pass makes one decode call per coder whatever it holds.  A file of two or more channels gives a source of its class that is staged once,
    surveyed on the device, told its mix -- survey.ChannelSurvey.safe_mix() of that survey, None being the plain downmix --
    and resampled from the staged bytes (sources.RawAuto, flac.FlacAuto, sndfmt.AdpcmAuto and its Microsoft twin): `parts` 1,
    `size` the downmix's length, `decision` = (survey, mix) once launched.  Without `resample` a rate other than 16 kHz is
    refused as load_pcm_mixes refuses it.  A file set gives a sources.SetAuto, the same two steps over its members' bytes."""
    medianame = as_media(medianame)
    h, full, multi = _auto_parsed(medianame)
    if h.n == 0:
        return h.source(resample)
    if h.ch > 1 or h.sr != R.SR_OUT:
        if not resample:
            need_16k_mono(medianame, h.sr, 1) if h.ch == 1 else need_16k(medianame, h.sr)
        R.check_rate(h.sr)
    return h.auto_source(full)


def decode_auto(medianame, resample=True):
    """Host-only twin of Segmenter.load_pcm_auto -> (pcm, survey, mix): survey = survey_channels(medianame) and mix =
    survey.safe_mix() for a file of two or more channels (None, None for one channel); pcm = decode_mixes(medianame, [mix])[0],
    or for mix None the plain decode: resample.resample_ref of the stored samples (decode_pcm's array for a 16 kHz mono file)."""
    medianame = as_media(medianame)
    h, full, multi = _auto_parsed(medianame)
    x = h.stored()
    if not multi:
        if h.sr != R.SR_OUT and resample:
            return R.resample_ref(x, h.sr), None, None
        return decode_pcm(medianame, ffmpeg=None), None, None
    from .survey import ChannelSurvey
    if not resample:
        need_16k(medianame, h.sr)
    R.check_rate(h.sr)
    survey = ChannelSurvey(R.survey_ref(x, full, 0, h.n), h.sr, 0)
    mix = survey.safe_mix()
    return (R.resample_ref(x, h.sr) if mix is None else R.mix_ref(x, h.sr, mix)), survey, mix


# ---------------------------------------------------------------------------------------------- schedules and timelines
def _sched_parsed(medianame, what, resample):
    """-> (the file parsed as a survey parses it, its fullscale threshold), for a schedule or a timeline: whole single files
    without ffmpeg, a rate other than 16 kHz only with `resample`."""
    medianame = as_media(medianame)
    _no_set_ranges(medianame, what)
    h, full, multi = _auto_parsed(medianame)
    if multi or (h.n > 0 and h.sr != R.SR_OUT):
        if not resample:
            need_16k_mono(medianame, h.sr, 1) if h.ch == 1 else need_16k(medianame, h.sr)
        R.check_rate(h.sr)
    return h, full


def _fade_arg(fade_sec):
    """fade_sec of the schedule calls -> seconds; ValueError unless it is a finite number, 0 or above (survey.rule_fade's text)."""
    from .survey import rule_fade
    return rule_fade('safe', 0.0 if fade_sec is None else fade_sec)


def schedule_source(medianame, schedule, resample=False, fade_sec=0.0):
    """What Segmenter reads for load_pcm_schedule -> (the resample.Schedule, the source).  The schedule is normalised against the
    file's rate and channels (resample.normalise_schedule, the errors naming the file; fade_sec: its cross-fades).  The source is io.auto_source's as a
    scheduled source of its class (sources.scheduled); a one-channel file whose every run is the plain downmix is read as ever."""
    from . import sources
    h, full = _sched_parsed(medianame, 'schedules', resample)
    sched = R.normalise_schedule(schedule, h.sr, h.ch, f'{as_media(medianame)}: schedule', _fade_arg(fade_sec))
    if h.n == 0:
        return sched, h.source(resample)
    src = h.auto_source(full)
    if type(src) not in sources.SCHED_OF or getattr(src, 'kind', 'stage') != 'stage':      # one channel, read as it always was
        if any(m is not None for _, m in sched.runs):
            x = h.stored()
            src = sources.RawAuto(x[:, None] if x.ndim == 1 else x, h.sr, full=full)       # the mixes of one channel: on the device too
        else:
            return sched, src
    return sched, sources.scheduled(src, sched, None)


def timeline_source(medianame, block_sec=None, resample=False, rule='safe', fade_sec=None):
    """What Segmenter reads for the timeline calls: io.auto_source's source, and for a file of two or more channels that source
    as a scheduled source that is to decide its schedule from blocks of `block_sec` seconds (survey.block_chunks) by `rule`, its
    run boundaries cross-faded over `fade_sec` seconds (survey.rule_fade states the defaults and the refusals)."""
    from . import sources
    from .survey import DEFAULT_BLOCK_SEC, block_chunks, rule_fade
    fade_sec = rule_fade(rule, fade_sec)
    h, full = _sched_parsed(medianame, 'timelines', resample)
    k = block_chunks(DEFAULT_BLOCK_SEC if block_sec is None else block_sec, h.sr)
    if h.n == 0:
        return h.source(resample)
    src = h.auto_source(full)
    if type(src) not in sources.SCHED_OF:
        return src
    return sources.scheduled(src, None, k, rule, fade_sec)


def decode_schedule(medianame, schedule, resample=True, fade_sec=0.0):
    """Host-only twin of Segmenter.load_pcm_schedule: resample.schedule_ref of the stored samples as decode_source decodes them,
    the schedule normalised against the file's rate and channels, its run boundaries cross-faded over `fade_sec` seconds."""
    h, _ = _sched_parsed(medianame, 'schedules', resample)
    sched = R.normalise_schedule(schedule, h.sr, h.ch, f'{as_media(medianame)}: schedule', _fade_arg(fade_sec))
    x = h.stored()
    if h.ch == 1 and all(m is None for _, m in sched.runs):
        return R.resample_ref(x, h.sr) if h.sr != R.SR_OUT else decode_pcm(medianame, ffmpeg=None)
    return R.schedule_ref(x, h.sr, sched)


def survey_timeline(medianame, block_sec=None):
    """Host-only twin of Segmenter.survey_timeline -> a survey.SurveyTimeline: `whole` = survey_channels(medianame), block b =
    resample.survey_ref of stored frames [b * B, min((b + 1) * B, n)), B = survey.block_chunks(block_sec, sr) * 1024 (block_sec
    None: survey.DEFAULT_BLOCK_SEC)."""
    from .survey import DEFAULT_BLOCK_SEC, ChannelSurvey, SurveyTimeline, block_chunks
    _no_set_ranges(medianame, 'timelines')
    h, full = _survey_parsed(medianame, False)
    per = block_chunks(DEFAULT_BLOCK_SEC if block_sec is None else block_sec, h.sr) * R.SURVEY_CHUNK
    x = h.stored()
    blocks = [ChannelSurvey(R.survey_ref(x, full, a, min(a + per, h.n)), h.sr, a) for a in range(0, h.n, per)]
    return SurveyTimeline(ChannelSurvey(R.survey_ref(x, full, 0, h.n), h.sr, 0), blocks, per)


def decode_auto_timeline(medianame, block_sec=None, resample=True, rule='safe', fade_sec=None):
    """Host-only twin of Segmenter.load_pcm_auto_timeline -> (pcm, timeline, schedule): timeline = survey_timeline(medianame,
    block_sec), schedule = timeline.schedule(rule, fade_sec) -- safe_schedule() by default --, pcm = decode_schedule(medianame,
    schedule); a one-channel file gives decode_auto's pcm and (None, None)."""
    from .survey import rule_fade
    rule_fade(rule, fade_sec)                              # (the refusals, for a one-channel file too)
    h, _ = _sched_parsed(medianame, 'timelines', resample)
    if not (h.ch > 1 and h.n > 0):
        return decode_auto(medianame, resample)[0], None, None
    timeline = survey_timeline(medianame, block_sec)
    schedule = timeline.schedule(rule, fade_sec)
    return R.schedule_ref(h.stored(), h.sr, schedule), timeline, schedule


def survey_sources(medianame, ranges=None):
    """What the device surveys for `medianame` -> (sr, [(source or resample.SurveyFields, first frame) per range]; one entry, the
    whole file, for ranges None).  A source stages only what its frames [a, b) need: the bytes of a plain RIFF/WAVE file, read by
    byte ranges (sources.RawSurvey); the covering frames of a FLAC stream or blocks of an ADPCM file, for a decode to the staging
    buffer without a filter (kind 'stage' of flac.FlacExcerpt, sndfmt.AdpcmExcerpt and its Microsoft twin).  A file without
    frames is surveyed here (SurveyFields of no samples)."""
    from . import flac, sndfmt
    from .sources import RawSurvey
    if ranges is not None:
        _no_set_ranges(medianame, 'ranges')
        ranges = [tuple(r) for r in ranges]
        for start, stop in ranges:
            _check_range(medianame, start, stop)
    h, full = _survey_parsed(medianame, True)
    out = []
    for a, b in _survey_spans(h, ranges):
        if b == a:
            out.append((R.survey_ref(np.zeros((0, h.ch)), full), a))
            continue
        if isinstance(h, _SetSound):
            src = h.survey_source(full)
        elif isinstance(h, flac.FlacStream):
            src = flac.FlacExcerpt(h, 'stage', a, b)
        elif h.kind in sndfmt._BLOCK:
            src = sndfmt.block_excerpt(h, 'stage', a, b)
        else:
            sub, _ = sndfmt.sub_sound(h, a, b)
            x, fmt = sub.raw()
            src = RawSurvey(x, h.sr, fmt, full, a, b, first=a, total=h.n)
        src.size = -(-(b - a) * R.SR_OUT // h.sr)                 # what packs it into a pass: its length at 16 kHz
        out.append((src, a))
    return h.sr, out
