"""Time ranges of single channels without ffmpeg (CPU): io.decode_channel_excerpts -- the host builds of the decoders on the
frames, blocks and bytes of each excerpt alone, and a windowed resample_ref per selected channel -- against slices of
io.decode_channels; the one-channel fallback; the refusals; the byte ranges read; and what a pass of such excerpts hands to the
device (on the recording fake of test_host.py).  No device: the kernels are tested in test_gpu_channel_excerpts.py.

Everything is bit-exact: out[r][k] is decode_channels(path, [sel[k]])[0][a:b], (a, b) = excerpt_bounds on the length of a channel's
16 kHz twin.  Ranges are given as sample / 16000, which that rounding maps back to the sample."""
import os

import numpy as np
import pytest

import flacgen
import sndgen
import wavgen
from test_channels import flac_int
from test_excerpts import sec, unit_ranges
from inaspeechsegmenter_amd import flac, sndfmt, sources
from inaspeechsegmenter_amd import io as iss_io
from inaspeechsegmenter_amd import resample as R
from inaspeechsegmenter_amd.segmenter import Segmenter

CASES = {                                                        # name -> (selection, stored frames between unit starts)
    'wav44k2': ([1, 0], 2000), 'wav16k2': ([0, 1], 1152), 'wav22k11': ([10, 0, 7, 7, 3], 1000), 'ulaw8k2': ([1, 1, 0], 700),
    'flac16k_ls': (None, 1152), 'ima8k2': ([1, 0], 498),                   # (IMA: every second block start, 996 outputs apart)
}


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('channel_excerpts')
    return {
        'wav44k2': wavgen.write_wav(d / 'w44.wav', wavgen.encode(wavgen.make_signal(30000, 2, 1), 'i16'), 44100, 'i16'),
        'wav16k2': wavgen.write_wav(d / 'w16.wav', wavgen.encode(wavgen.make_signal(1152 * 10 + 500, 2, 2), 'i16'), 16000, 'i16'),
        'wav22k11': wavgen.write_wav(d / 'w22.wav', wavgen.encode(wavgen.make_signal(9000, 11, 3), 'i16'), 22050, 'i16'),
        'ulaw8k2': sndgen.write(d / 'u.wav', 'wav', 'ulaw', False, wavgen.make_signal(6000, 2, 4), 8000)[0],
        'flac16k_ls': flacgen.write(d / 'f.flac', flac_int(1152 * 10 + 500, 2, 16, 5), 16000, 16, blocksize=1152,
                                    channel_mode='left_side', subframe={'type': 'fixed', 'order': 2}),
        'ima8k2': sndgen.write(d / 'i.wav', 'wav', 'ima', False, wavgen.make_signal(249 * 24 + 100, 2, 6), 8000, block_align=256)[0],
        'mono16k': wavgen.write_wav(d / 'mono.wav', wavgen.encode(wavgen.make_signal(6000, 1, 7), 'i16'), 16000, 'i16'),
        'monof32': wavgen.write_wav(d / 'monof.wav', wavgen.encode(wavgen.make_signal(6000, 1, 8), 'f32'), 16000, 'f32'),
        'mono44k': wavgen.write_wav(d / 'mono44.wav', wavgen.encode(wavgen.make_signal(20000, 1, 9), 'i16'), 44100, 'i16'),
    }


# ------------------------------------------------------------------------------------------------ slices
@pytest.mark.parametrize('name', sorted(CASES))
def test_decode_channel_excerpts_equal_channel_slices(files, name):
    path = files[name]
    sel, unit = CASES[name]
    x, sr = iss_io.decode_source(path)
    nch = x.shape[1]
    if name == 'ima8k2':
        assert sndfmt.parse(open(path, 'rb').read(), path).spb * 2 == unit
    want_sel = list(range(nch)) if sel is None else sel
    twins = [iss_io.decode_channels(path, [c])[0] for c in range(nch)]
    n16 = twins[0].size
    assert n16 == R.out_len(x.shape[0], sr)
    # the starts of the frames / blocks / thousands of stored frames, in 16 kHz samples
    bounds = sorted({int(j) * 16000 // sr for j in range(0, x.shape[0], unit)})
    ranges, ab = unit_ranges(bounds, n16)
    got = iss_io.decode_channel_excerpts(path, ranges, sel)
    assert len(got) == len(ab)
    for g, (a, b), r in zip(got, ab, ranges):
        assert len(g) == len(want_sel)
        for k, c in enumerate(want_sel):
            assert g[k].dtype == np.int16
            np.testing.assert_array_equal(g[k], twins[c][a:b], err_msg=f'{name} {r} = [{a}, {b}) channel {c}')
    assert not np.array_equal(got[0][0], got[0][-1]) or want_sel[0] == want_sel[-1]
    if name == 'wav16k2':                                            # the identity filter: the stored column itself
        a, b = ab[2]
        np.testing.assert_array_equal(got[2][1], x[a:b, 1])


def test_sources_carry_window_and_selection(files):
    for name, cls in (('wav44k2', sources.RawExcerpt), ('ulaw8k2', sources.RawExcerpt), ('flac16k_ls', flac.FlacExcerpt),
                      ('ima8k2', sndfmt.AdpcmExcerpt)):
        sel, sigs = iss_io.channel_excerpts(files[name], [(sec(500), sec(1500)), (sec(100), None)], [1, 0, 1], resample=True)
        assert sel == [1, 0, 1]
        for s in sigs:
            assert type(s) is cls and s.sel == [1, 0, 1] and s.parts == 3 and s.win is not None, name
            assert s.stride == -(-s.size // 160) * 160
            assert s.held >= 3 * s.size if cls is sources.RawExcerpt else s.held == max(1, s.nbytes // 2)   # as whole files
            one = s.reselect([0])
            assert one.parts == 1 and one.sel == [0] and s.parts == 3 and one.win == s.win
            if cls is not sources.RawExcerpt:
                assert s.kind == 'resample'                          # also at 16 kHz: through the identity filter
        assert sigs[0].size == 1000 and sigs[0].win[3:] == (500, 1000)
    # without a selection argument: all channels, ascending
    sel, sigs = iss_io.channel_excerpts(files['wav22k11'], [(0, None)], None, resample=True)
    assert sel == list(range(11)) == sigs[0].sel


# ------------------------------------------------------------------------------------------------ one-channel files
@pytest.mark.parametrize('name,resample', [('mono16k', False), ('monof32', False), ('mono44k', True)])
def test_one_channel_file_falls_back_to_excerpts(files, name, resample):
    path = files[name]
    ranges = [(sec(700), sec(3000)), (sec(4000), None)]
    want = iss_io.decode_excerpts(path, ranges, resample)
    got = iss_io.decode_channel_excerpts(path, ranges, [0, 0], resample=resample)
    assert len(got) == 2
    for g, w in zip(got, want):
        assert len(g) == 2 and g[0].dtype == w.dtype
        np.testing.assert_array_equal(g[0], w)
        np.testing.assert_array_equal(g[1], w)
    sel, sigs = iss_io.channel_excerpts(path, ranges, None, resample)
    assert sel == [0] and len(sigs) == 2
    assert all(getattr(s, 'sel', None) is None for s in sigs)
    with pytest.raises(ValueError, match=r'%s: channel 1 is outside' % os.path.basename(path).replace('.', r'\.')):
        iss_io.channel_excerpts(path, ranges, [1], resample)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('reader', ['decode_channel_excerpts', 'channel_excerpts'])
def test_refusals_name_the_file(files, reader, tmp_path):
    read = getattr(iss_io, reader)
    path = files['wav16k2']
    n16 = 1152 * 10 + 500
    for bad in (-0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r'w16\.wav.*start_sec'):
            read(path, [(bad, None)])
    with pytest.raises(ValueError, match=r'w16\.wav.*stop_sec.*not after start_sec'):
        read(path, [(0.5, 0.25)])
    with pytest.raises(ValueError, match=r'w16\.wav.*past the end of the file.*%.3f s' % sec(n16)):
        read(path, [(sec(n16), None)])
    with pytest.raises(ValueError, match=r'media .*w16\.wav: 399 samples, less than one 25 ms analysis window'):
        read(path, [(sec(100), sec(499))])
    with pytest.raises(ValueError):                                      # a good range in front of a bad one: nothing comes back
        read(path, [(0, None), (0.5, 0.25)])
    with pytest.raises(ValueError, match='start_sec'):                   # before the file is opened
        read(str(tmp_path / 'no_such_file.wav'), [(-1.0, None)])
    with pytest.raises(ValueError, match=r'w16\.wav: channel 2 is outside'):
        read(path, [(0, None)], [0, 2])
    with pytest.raises(ValueError, match=r'w16\.wav: channel -1 is outside'):
        read(path, [(0, None)], [-1])
    with pytest.raises(ValueError, match=r'w16\.wav: empty channel selection'):
        read(path, [(0, None)], [])
    with pytest.raises(ValueError, match=r'http://host/a\.wav'):
        read('http://host/a.wav', [(0, None)])
    with pytest.raises(AssertionError, match=r'can only take files sampled at 16000 Hz\. The file .*w44\.wav is sampled at 44100 Hz'):
        read(files['wav44k2'], [(0, None)], None, resample=False)
    read(path, [(0, None)], None, resample=False)                        # two channels at 16 kHz are not refused


def test_segmenter_refuses_ffmpeg(files):
    seg = Segmenter.__new__(Segmenter)                                   # (a double: no device, no networks)
    seg.ffmpeg, seg.resample = 'ffmpeg', False
    for method in (seg.load_pcm_channel_excerpts, seg.segment_channel_excerpts):
        with pytest.raises(ValueError, match=r"ffmpeg=None.*ffmpeg='ffmpeg'"):
            method(files['wav16k2'], [(0, None)])


# ------------------------------------------------------------------------------------------------ bytes read
def test_plain_wav_is_read_by_byte_ranges(tmp_path, monkeypatch):
    """A 1 s range of both channels in the middle of a 5-minute 48 kHz stereo WAV: chunk headers plus span, under 1 % of the file,
    and never the whole-file read."""
    sec1 = wavgen.encode(wavgen.make_signal(48000, 2, 10), 'i16')
    x = np.tile(sec1, (300, 1))
    path = wavgen.write_wav(tmp_path / 'long.wav', x, 48000, 'i16')
    a, count = 150 * 16000, 16000                                        # (the reference from the window's own span: test_excerpts.py
    j_lo, j_hi = R.input_span(48000, x.shape[0], a, count)               # shows that it is the whole-file result's slice)
    want = [R.resample_ref(x[j_lo:j_hi + 1, c], 48000, a, count, j_lo, x.shape[0]) for c in (1, 0)]
    calls, real = [], iss_io._read_range

    def counting(p, offset, size):
        calls.append((offset, size))
        return real(p, offset, size)

    def refuse(p):
        raise AssertionError('the whole file was read')
    monkeypatch.setattr(iss_io, '_read_range', counting)
    monkeypatch.setattr(iss_io, '_read_file', refuse)
    got = iss_io.decode_channel_excerpts(path, [(150.0, 151.0)], [1, 0])[0]
    size = os.path.getsize(path)
    assert sum(s for _, s in calls) < 0.01 * size and all(o + s <= size for o, s in calls)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------------------------------------------ malformed input
def test_flac_bad_frame_inside_and_outside(tmp_path):
    x = flac_int(1152 * 8, 2, 16, 11)
    data, offs = flacgen.encode(x, 16000, 16, blocksize=1152, channel_mode='left_side', subframe={'type': 'fixed', 'order': 2},
                                return_offsets=True)
    bad = bytearray(data)
    bad[offs[6] - 4] ^= 0x10                                                      # inside frame 5, in front of its CRC-16
    path = tmp_path / 'bad.flac'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.flac: frame at byte %d: ' % offs[5]):
        iss_io.decode_channel_excerpts(str(path), [(sec(1152 * 4 + 100), sec(1152 * 5 + 600))])
    a, b = 1152 * 2 + 100, 1152 * 5                                               # frames 2 to 4; ends where frame 5 starts
    got = iss_io.decode_channel_excerpts(str(path), [(sec(a), sec(b)), (sec(1152 * 6), None)], [1])
    np.testing.assert_array_equal(got[0][0], x[a:b, 1])
    np.testing.assert_array_equal(got[1][0], x[1152 * 6:, 1])


def test_ima_bad_block_inside_and_outside(tmp_path):
    clean = sndgen.write(tmp_path / 'clean.wav', 'wav', 'ima', False, wavgen.make_signal(249 * 24, 2, 12), 8000, block_align=256)[0]
    snd = sndfmt.parse(open(clean, 'rb').read(), clean)
    assert snd.spb == 249
    twin = iss_io.decode_channels(clean, [1])[0]
    bad = bytearray(open(clean, 'rb').read())
    bad[snd.base + 14 * 256 + 2] = 89                                             # block 14, channel 0: step index above 88
    path = tmp_path / 'bad.wav'
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r'bad\.wav: block at byte %d: step index above 88' % (snd.base + 14 * 256)):
        iss_io.decode_channel_excerpts(str(path), [(sec(2 * (249 * 13 + 10)), sec(2 * (249 * 14 + 200)))], [1])
    # far enough from block 14 that the filter's reach (10 input frames at 8 kHz) stays outside it
    a, b = 2 * (249 * 8 + 10), 2 * (249 * 14 - 20)
    got = iss_io.decode_channel_excerpts(str(path), [(sec(a), sec(b)), (sec(2 * (249 * 15 + 20)), None)], [1])
    np.testing.assert_array_equal(got[0][0], twin[a:b])
    np.testing.assert_array_equal(got[1][0], twin[2 * (249 * 15 + 20):])


# ------------------------------------------------------------------------------------------------ launch plumbing
def test_a_pass_of_excerpts_makes_one_launch_per_class(files):
    """Excerpts with and without a selection, of stored samples, FLAC and IMA ADPCM, in one pass on the recording fake: one
    launch per class, `windows` beside every job, `splits` with None for the downmixed ones."""
    from test_host import _RecordingDevice
    from inaspeechsegmenter_amd.sources import Group
    fake = _RecordingDevice({}, {})
    ranges = [(sec(500), sec(1500)), (sec(1000), sec(2400))]
    for name, call in (('wav44k2', 'resample'), ('flac16k_ls', 'flac_decode'), ('ima8k2', 'adpcm_decode')):
        sel, split = iss_io.channel_excerpts(files[name], ranges, [1, 0], resample=True)
        # the downmixed excerpt of the same file (FLAC and IMA at 16 kHz mono would be 'pcm'; these files are stereo)
        mixed = iss_io.excerpts(files[name], ranges[:1], resample=True)
        assert type(mixed[0]) is type(split[0]) and mixed[0].sel is None
        placed, pos = [], 0
        for s in (split[0], mixed[0], split[1].reselect([0])):
            placed.append((s, pos))
            pos += s.parts * s.stride
        del fake.calls[:]
        group = Group(fake, type(split[0]), placed).launch(pos)
        launches = [c for c in fake.calls if c[0] != 'resample_filter']
        assert len(launches) == 1 and launches[0][0] == call, name
        extras = dict(e for e in launches[0] if isinstance(e, list) and e and e[0] in ('windows', 'splits'))
        assert extras['windows'] == [list(s.win) for s, _ in placed]
        assert extras['splits'] == [[split[0].stride, [1, 0]], None, [split[1].stride, [0]]]
        rows = next(e for e in launches[0] if isinstance(e, list) and e and isinstance(e[0], list))
        assert len(rows) == 3
        group.check()


def test_native_wrapper_routes_both_to_the_joint_entry_point():
    """_native.Context._decode_call: base, base_windows, base_split, base_windows_split -- by what is given, argument order as
    include/iss.h declares them."""
    from inaspeechsegmenter_amd import _native
    seen = []

    class Lib:
        def __getattr__(self, name):
            return lambda h, *args: seen.append((name, len(args))) or 0
    ctx = object.__new__(_native.Context)
    ctx._L, ctx._h = Lib(), None
    ctx._ck = lambda rc, name: None
    lead, trail = (1, 2, 3), (1, -1)
    win, sp = [(0, 10, 10, 0, 4)], [(160, [0, 1])]
    ctx._decode_call('iss_resample_pcm16', lead, trail, None, None)
    ctx._decode_call('iss_resample_pcm16', lead, trail, win, None)
    ctx._decode_call('iss_resample_pcm16', lead, trail, None, sp)
    ctx._decode_call('iss_resample_pcm16', lead, trail, win, sp)
    assert seen == [('iss_resample_pcm16', 5), ('iss_resample_pcm16_windows', 6), ('iss_resample_pcm16_split', 8),
                    ('iss_resample_pcm16_windows_split', 9)]


def test_wav_that_needs_the_whole_file_read(tmp_path):
    """A piped WAV (no length in its data chunk) has no header to read ranges by: the file is read whole once, and the ranges
    are cut from its bytes -- the same samples."""
    x = wavgen.encode(wavgen.make_signal(9000, 2, 13), 'i16')
    path = wavgen.write_wav(tmp_path / 'piped.wav', x, 22050, 'i16')
    buf = bytearray(open(path, 'rb').read())
    at = buf.index(b'data') + 4
    buf[at:at + 4] = b'\xff\xff\xff\xff'
    open(path, 'wb').write(bytes(buf))
    assert sndfmt.read_header(path) is None
    got = iss_io.decode_channel_excerpts(path, [(sec(1234), sec(3734))], [1, 0])[0]
    for g, c in zip(got, (1, 0)):
        np.testing.assert_array_equal(g, R.resample_ref(x[:, c], 22050)[1234:3734])
