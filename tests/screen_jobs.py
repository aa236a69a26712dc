"""One corpus of small jobs for the two screens that hold "same input -> same bits, whatever the workspace held before the call
(tests/test_gpu_stale_workspace.py) and whatever runs beside it (tests/test_gpu_co_scheduling.py)".

A job has
  prepare(ctx)        tables, networks, filters, resident inputs: off the clock, once per context;
  run(ctx, size)      the only part that launches -> a tuple of ndarrays (settings go through set_precision / set_diag /
                      set_workspace_limit, never through the environment);
  sizes               what `run` is parametrised over, smallest workspace footprint first;
  families            kernel-instance prefixes, or (prefix, suffix) pairs, the job must launch (prof_instances);
  check(size, out)    the serial baseline against the reference the suite already holds that kernel to, with the bounds of the
                      test the helper comes from (nothing new is fixed here): two runs that agree are then also right;
  launched            {size: kernel instances of the last profiled run} (run_profiled), for a bound that goes by the kernels run.
The shapes are the ones the edge tests already found (their helpers are imported, not copied).  Every context runs with the
precision guard off and an explicit arithmetic mode, so no probe launch is mixed in."""
import functools

import numpy as np

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, vbx as V, flac, sndfmt, tables, _native
from inaspeechsegmenter_amd import resample as R
from oracle import sidekit as osk, vbx as ovbx
import topologies as TP
import wavgen
import test_gpu_cnn as tcnn
import test_gpu_cnn_defaults as tdef
import test_gpu_flac as tflac
import test_gpu_resample as trs
import test_gpu_sidekit as tsk
import test_gpu_sndfmt as tsnd
import test_gpu_topologies as ttop
import test_gpu_vfs_batch as tvb

MODES = tdef.MODES
GROUPS = ('front_ends', 'decoders', 'segmenter_nets', 'segmenter_switches', 'topology_families', 'xvector', 'pointwise')
WS_FLOOR = 64 << 20                       # the smallest workspace iss_set_workspace_limit takes
WS_DEFAULT = 24 << 30
WORDS = (0x7FC00000, 0xFF800000, 0x00000000, 0x7F7FFFFF)      # quiet NaN, -inf, 0, FLT_MAX

# every kernel family the screens must reach (the union over the serial baselines, see missing_families)
FAMILY_PREFIXES = ('conv_x3_wq_kernel<', 'conv_x3_wq3_kernel<', 'conv_x3_wq3h_kernel<', 'conv_dhl_kernel<', 'conv_x3_ws_kernel<',
                   'conv_x3_fp_kernel<', 'conv_x3_kernel<0', 'conv_x3_pw_kernel<', 'conv_x3_pws_kernel<', 'conv_x3_pws2_kernel<',
                   'conv_x3_pwc_kernel<', 'conv1_patch_x3_kernel<', 'conv_igemm_kernel<')
WS_FORMS = ('ring>', 'fs>', 'ncb1>', 'plain>', 'f32>')


def missing_families(names):
    """What of the family list the instance names `names` leave out (empty: every family is screened)."""
    names = set(names)
    miss = [p for p in FAMILY_PREFIXES if not any(k.startswith(p) for k in names)]
    miss += [f'conv_x3_ws_kernel<...{e}' for e in WS_FORMS if not any(k.startswith('conv_x3_ws_kernel<') and k.endswith(e) for k in names)]
    if not any(k.startswith(('conv_x3_kernel<3', 'conv_x3_kernel<4')) for k in names):
        miss.append('conv_x3_kernel<3|4')
    if not any(k.startswith('conv_x3_pws2_kernel<') and 'dual' in k for k in names):
        miss.append('conv_x3_pws2_kernel<...dual>')
    return miss


def fresh_context():
    c = _native.Context(0)
    c.set_precision_guard(0)
    c.set_precision(_native.PREC_BF16X3)
    c._screen = {}                        # what the jobs' prepare() left on this context
    return c


class Job:
    group = None
    families = ()
    passes_at_floor = None                # CNN jobs: passes of the largest size under WS_FLOOR (None: no pass structure)

    def __init__(self, name, sizes):
        self.name, self.sizes, self.launched = name, list(sizes), {}

    def prepare(self, ctx):
        pass

    def settings(self, ctx, ws_limit=None):
        """Mode, switches and workspace of this job on `ctx` (no launch)."""

    def run(self, ctx, size):
        raise NotImplementedError

    def check(self, size, out):
        raise NotImplementedError

    def __repr__(self):
        return self.name


def _once(ctx, key, fn):
    if key not in ctx._screen:
        ctx._screen[key] = fn()
    return ctx._screen[key]


# ------------------------------------------------------------------------------------------------------------ front ends
class Sidekit(Job):
    group = 'front_ends'

    def __init__(self, kind):
        super().__init__(f'sidekit_{kind}', [16000, 160 * 2048 * 4 + 400 + 3])      # the second: 8193 frames, two grid-stride passes
        self.kind = kind

    @functools.lru_cache(None)
    def _input(self, n):
        pcm = np.clip(np.random.default_rng(n).normal(0, 3000, n), -32768, 32767).astype(np.int16)   # test_ragged_lengths_vs_oracle
        pcm[n // 2:n // 2 + 800] = 0                                                                  # digital silence: -inf rows
        return pcm if self.kind == 'i16' else (pcm / 32768.0).astype(np.float32)

    def prepare(self, ctx):
        _once(ctx, 'sidekit_tables', lambda: ctx.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank()))

    def run(self, ctx, size):
        ctx.set_signal(self._input(size))
        ctx.sidekit()
        return ctx.get_loge(), ctx.get_mspec()

    def check(self, size, out):
        x = self._input(size)
        ref_loge, ref_mspec = osk.mfcc_mspec(x if self.kind == 'f32' else (x / 32768.0).astype(np.float32))
        assert not np.isfinite(ref_loge).all()
        tsk._check(out[0], out[1], ref_loge, ref_mspec, (self.name, size))


@functools.lru_cache(None)
def _vbx_pcm(n):
    return np.clip(np.round(np.random.default_rng(9 + n).normal(0, 0.1, n) * 32768), -32768, 32767).astype(np.int16)


def _vbx_prepare(ctx, n):
    _once(ctx, 'vbx_tables', lambda: ctx.vbx_tables(tables.vbx_window(), tables.vbx_melbank()))
    if ctx._dither_n < n:
        ctx.vbx_set_dither(V.dither_stream(n))


class VbxFeatures(Job):
    group = 'front_ends'

    def __init__(self):
        super().__init__('vbx_features_pcm16', [48037, 160 * 301])

    def prepare(self, ctx):
        _vbx_prepare(ctx, 160 * 4999)

    def run(self, ctx, size):
        return (ctx.vbx_features_pcm16(_vbx_pcm(size)),)

    def check(self, size, out):
        assert np.abs(out[0] - ovbx.get_features(_vbx_pcm(size) / 32768.0)).max() <= tvb.FEA_TOL, (self.name, size)


class VbxBatch(Job):
    group = 'front_ends'
    lengths = [n for n in tvb.BATCH_LENGTHS if n < 160 * 4999]          # without its 5000-frame file

    def __init__(self):
        super().__init__('vbx_features_batch_pcm16', ['batch'])

    def prepare(self, ctx):
        _vbx_prepare(ctx, 160 * 4999)

    def run(self, ctx, size):
        return ctx.vbx_features_batch_pcm16([_vbx_pcm(n) for n in self.lengths])

    def check(self, size, out):
        foff, arena = out
        assert list(np.diff(foff)) == [V.frame_count(n) for n in self.lengths] and foff[0] == 0
        for f, n in enumerate(self.lengths):
            assert np.abs(arena[foff[f]:foff[f + 1]] - ovbx.get_features(_vbx_pcm(n) / 32768.0)).max() <= tvb.FEA_TOL, (self.name, n)


# ------------------------------------------------------------------------------------------------- decoders and resampler
class Resample(Job):
    group = 'decoders'

    def __init__(self, sr, ch, n):
        super().__init__(f'resample_{sr}_{ch}ch', [n])
        self.sr, self.ch = sr, ch

    @functools.lru_cache(None)
    def _input(self, n):
        return wavgen.encode(wavgen.make_signal(n, self.ch, self.sr % 97), 'i16')

    def prepare(self, ctx):
        ctx.resample_filter(self.sr)

    def run(self, ctx, size):
        n = ctx.resample_signal(self._input(size), self.sr)
        return (ctx.get_signal_pcm16(0, n),)

    def check(self, size, out):
        assert np.array_equal(out[0], R.resample_ref(self._input(size), self.sr)), self.name


class ResampleMixed(Job):
    """One launch over stored formats that the five little-endian WAV formats do not cover: resample_kernel<true>."""
    group = 'decoders'

    def __init__(self):
        super().__init__('resample_mixed_batch', ['batch'])

    @functools.lru_cache(None)
    def _input(self):
        srcs, want = [], []
        for k, (kind, big, sr, ch, n) in enumerate((('i16', False, 44100, 2, 9001), ('ulaw', False, 8000, 1, 4003),
                                                    ('i16', True, 48000, 2, 7777), ('f32', False, 22050, 6, 3001), ('alaw', False, 11025, 2, 2600))):
            s, twin = tsnd._sound(wavgen.make_signal(n, ch, 31 + k), kind, big, sr)
            raw, fmt = s.raw()
            srcs.append((raw, sr, fmt))
            want.append(R.resample_ref(twin, sr))
        return srcs, want

    def prepare(self, ctx):
        for _, sr, _ in self._input()[0]:
            ctx.resample_filter(sr)

    def run(self, ctx, size):
        srcs, want = self._input()
        raw, jobs, rpos, dpos = [], [], 0, 0
        for (x, sr, fmt), w in zip(srcs, want):
            b = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
            raw += [b, np.zeros(-b.size % 16, np.uint8)]
            jobs.append(ctx.resample_job(x, sr, rpos, dpos, fmt))
            rpos += b.size + -b.size % 16
            dpos += -(-w.size // 160) * 160
        ctx.set_signal(np.full(dpos, 12345, np.int16))
        ctx.resample(np.concatenate(raw), jobs)
        return (ctx.get_signal_pcm16(0, dpos),)

    def check(self, size, out):
        pos = 0
        for w in self._input()[1]:
            assert np.array_equal(out[0][pos:pos + w.size], w), self.name
            pad = -w.size % 160
            assert np.all(out[0][pos + w.size:pos + w.size + pad] == 12345)
            pos += w.size + pad


class FlacJob(Job):
    group = 'decoders'
    K = 9                                  # (44100, 2, 16, left_side): decoded, staged, downmixed and resampled in one call

    def __init__(self):
        super().__init__('flac_44100_left_side', ['stream'])

    @functools.lru_cache(None)
    def _input(self):
        sr, ch, bps, kw = tflac.MATRIX[self.K]
        x, s = tflac._stream(sr, ch, bps, kw, self.K)
        return x, s, flac.source(s, resample=True)

    def prepare(self, ctx):
        ctx.resample_filter(self._input()[1].sr)

    def run(self, ctx, size):
        _, _, src = self._input()
        st = flac.decode_on(ctx, src)
        sig = ctx.get_signal_pcm16(0, src.size)
        return sig, np.array(st)

    def check(self, size, out):
        x, s, _ = self._input()
        want = tflac._stored(x, s.bps)
        assert np.array_equal(s.decode_host(), want) and not out[1].any()
        assert np.array_equal(out[0], R.resample_ref(want, s.sr)), self.name


class AdpcmJob(Job):
    group = 'decoders'

    def __init__(self):
        super().__init__('ima_adpcm_1024_2ch', ['file'])

    @functools.lru_cache(None)
    def _input(self):
        s, twin = tsnd._sound(wavgen.make_signal(7000 + 501 * 2, 2, 1024 + 2 + 44100 % 7), 'ima', False, 44100, 1024)
        return s, twin, sndfmt.source(s, resample=True)

    def prepare(self, ctx):
        ctx.resample_filter(44100)

    def run(self, ctx, size):
        _, _, src = self._input()
        st = sndfmt.decode_on(ctx, src)
        sig = ctx.get_signal_pcm16(0, src.size)
        return sig, np.array(st)

    def check(self, size, out):
        s, twin, _ = self._input()
        assert np.array_equal(s.stored(), twin) and not out[1].any()
        assert np.array_equal(out[0], R.resample_ref(twin, 44100)), self.name


# ---------------------------------------------------------------------------------------------------------- segmenter CNNs
SEG_T = 6000


@functools.lru_cache(None)
def seg_mspec():
    """Log-mel rows of a minute of the bench generator's audio (its silence gives 772 -inf rows from row 5099 on) with three more
    non-finite rows near the start, so every row list below has dead windows."""
    import bench
    pcm = bench.synth_recording_numpy(0, 160 * (400 + SEG_T - 1) + 400)
    _, mspec = osk.mfcc_mspec((pcm / 32768.0).astype(np.float32))
    mspec = np.ascontiguousarray(mspec[400:], dtype=np.float32)      # (the first 291 frames are silence)
    assert np.isfinite(mspec[:3100]).all() and not np.isfinite(mspec[5000:]).all()
    assert mspec.shape == (SEG_T, 24)
    mspec[40:43, 5] = -np.inf
    return mspec


@functools.lru_cache(None)
def seg_rows(size):
    """'T141' / 'T1000' / 'T3001': the segmenter's overlapping list (one tile; an odd tile count; a few-row last tile with
    persistent workgroups that loop); 'scat333': 333 scattered rows over the 6000 frames (per-window first layer)."""
    if size == 'scat333':
        return np.sort(np.random.default_rng(333).integers(0, SEG_T - 68, 333)).astype(np.int32)
    return S._window_rows(int(size[1:]))


SEG_SIZES = ['T141', 'scat333', 'T1000', 'T3001']       # by window count


@functools.lru_cache(None)
def _seg_net(nmel, ncls, seed):
    layers, shp = KM.synthetic_ina_like(nmel, ncls, seed=seed)
    return layers, KM.compile_layers(layers, shp)


@functools.lru_cache(None)
def _seg_sample():
    """64 log-mel row indices whose windows are compared with float64: 24 that every overlapping list holds, the rest from the
    longer lists and the scattered one; the rows around the non-finite ones are among them."""
    rng = np.random.default_rng(64)
    a = np.unique(seg_rows('T141'))
    pick = set(rng.choice(a, 20, replace=False).tolist()) | {0, 38, 40, 42}
    for size, k in (('T1000', 18), ('T3001', 12), ('scat333', 10)):
        pool = np.setdiff1d(np.unique(seg_rows(size)), list(pick))
        pick |= set(rng.choice(pool, k, replace=False).tolist())
    return np.array(sorted(pick), dtype=np.int32)


@functools.lru_cache(None)
def _seg_oracle(nmel, ncls, seed):
    layers, _ = _seg_net(nmel, ncls, seed)
    return tdef._oracle64(layers, seg_mspec(), nmel, _seg_sample())


class SegNet(Job):
    NETS = {'smn': (21, 3, 1), 'gender': (24, 2, 2)}

    def __init__(self, net, mode, diag='', sizes=SEG_SIZES, group='segmenter_nets'):
        super().__init__(f'{net}_{mode}' + (f'_{diag.replace(",", "+")}' if diag else ''), sizes)
        self.net, self.mode, self.diag, self.group = net, mode, diag, group
        self.families = SEG_FAMILIES[mode] if not diag else () if mode == 'f32' else SWITCH_FAMILIES[diag] + \
            ({('no_pws', 'bf16x3'): ('conv_x3_pw_kernel<',), ('no_pws2', 'bf16x3'): ('conv_x3_pws_kernel<',),
              ('no_pws', 'f16x3'): SEG_FAMILIES['f16x3'], ('no_pws2', 'f16x3'): SEG_FAMILIES['f16x3']}.get((diag, mode), ()))
        self.net_id = list(self.NETS).index(net)
        comp = _seg_net(*self.NETS[net])[1]
        self.passes_at_floor = -(-len(seg_rows(self.sizes[-1])) // tdef._plan_chunk(comp, 1 << 30, WS_FLOOR)[0])

    def prepare(self, ctx):
        _once(ctx, 'mspec', lambda: ctx.set_mspec(seg_mspec()))
        _once(ctx, ('net', self.net_id, self.net), lambda: ctx.cnn_load(self.net_id, _seg_net(*self.NETS[self.net])[1]))

    def settings(self, ctx, ws_limit=None):
        ctx.set_precision(MODES[self.mode])
        ctx.set_diag(self.diag or 0)
        ctx.set_workspace_limit(ws_limit or WS_DEFAULT)

    def run(self, ctx, size):
        p, fin = ctx.cnn_probs(self.net_id, seg_rows(size))
        return p, fin

    def bound_mode(self, size):
        """The arithmetic the run is held to.  Without a switch: the mode asked for.  A switch sends rows to an older family, and
        those have split-bf16 instantiations only (ConvArgs::f16: "only the kernels with an F16 instantiation are launched with
        it"), so an f16x3 run under a switch is held to the f16x3 bound where it launches every fp16 instantiation that
        test_gpu_cnn_defaults requires before it applies that bound (F16_KERNELS), and to the split-bf16 bound otherwise.
        Which (switch, size) that is, is pinned in F16_UNDER_SWITCH, and check() holds the launched instances to it: a change of
        routing fails there by name and has to be acknowledged in the table, it cannot relax a bound by itself."""
        if self.diag and self.mode == 'f16x3' and size not in F16_UNDER_SWITCH.get(self.diag, ()):
            return 'bf16x3'
        return self.mode

    def check(self, size, out):
        p, fin = out
        rows, sample = seg_rows(size), _seg_sample()
        lp64, rfin = _seg_oracle(*self.NETS[self.net])
        names = set(self.launched[size])
        if self.mode == 'f16x3':
            all_f16 = tdef.F16_KERNELS <= names
            assert all_f16 == (self.bound_mode(size) == 'f16x3') or not self.diag, (self.name, size, sorted(names))
            if self.diag == 'no_shared_first' or size == 'scat333':      # the per-window first layer: its fp16 form, by name
                patch = {k for k in names if k.startswith('conv1_patch_x3_kernel<')}
                assert patch and all(k.endswith(',true>') for k in patch), (self.name, size, sorted(names))
        pos = np.flatnonzero(np.isin(rows, sample))
        at = np.searchsorted(sample, rows[pos])
        assert len(pos) >= 10 and not fin.all(), (self.name, size, len(pos))
        assert np.array_equal(fin[pos], rfin[at]), (self.name, size)
        err = tdef._dlogp(p[pos], lp64[at], rfin[at])
        print(f'{self.name} {size}: max |d log p| {err:.2e} on {len(pos)} windows, held to {self.bound_mode(size)}')
        assert err < tdef.BOUND[self.bound_mode(size)], (self.name, size, err)


SWITCHES = ('no_wq', 'no_wq,no_hl', 'no_ws', 'no_shared_first', 'no_pws', 'no_pws2')
# f16x3 under a switch: the sizes at which every fp16 instantiation (F16_KERNELS) still runs, so the f16x3 bound holds; every other
# (switch, size) has conv2 or more in a split-bf16 family (conv_x3_ws_kernel / conv_x3_fp_kernel) and is held to the bf16x3 bound
F16_UNDER_SWITCH = {'no_pws': ('T141', 'T1000', 'T3001'), 'no_pws2': ('T141', 'T1000', 'T3001')}
# what a switch job must launch, by switch and mode ('' = both): the family the switch routes to
SWITCH_FAMILIES = {'no_wq': ('conv_x3_ws_kernel<5,3', 'conv_x3_ws_kernel<3,3'), 'no_wq,no_hl': ('conv_x3_ws_kernel<5,3', 'conv_x3_ws_kernel<3,3'),
                   'no_ws': ('conv_x3_fp_kernel<3,3', 'conv_x3_fp_kernel<5,3'), 'no_shared_first': ('conv1_patch_x3_kernel<',),
                   'no_pws': (), 'no_pws2': ()}
SEG_FAMILIES = {'f16x3': tuple(sorted(tdef.F16_KERNELS)) + (('conv1_patch_x3_kernel<', ',true>'),),
                'bf16x3': ('conv_x3_wq_kernel<', 'conv_x3_wq3h_kernel<', 'conv_dhl_kernel<', ('conv1_patch_x3_kernel<', ',false>')),
                'f32': (('conv_x3_ws_kernel<', 'f32>'), 'conv_igemm_kernel<')}


# ---------------------------------------------------------------------------------------------------- topology families
TOPO = ('conv2_7x7', 'conv1_same', 'ch32_64', 'ch48_96', 'conv2_stride2', 'conv1_pool')      # ring, fs, ncb1, plain, gather <3|4>
TOPO_T = 3001                              # resident rows; the issue's T = 700 and, for three passes under WS_FLOOR, 3001


@functools.lru_cache(None)
def topo_mspec():
    m = ttop._mspec(np.random.default_rng(700), TOPO_T)
    m[300:303, 5] = -np.inf
    return m


@functools.lru_cache(None)
def _topo_net(name, which):
    layers, shp = TP.nets(name)[which]
    return layers, shp, KM.compile_layers(layers, shp)


@functools.lru_cache(None)
def _topo_oracle(name, which):
    """float32 Keras-semantics oracle of test_topology_parity on 48 windows every list holds (the non-finite rows among them)."""
    layers, shp, _ = _topo_net(name, which)
    rows = np.unique(S._window_rows(700))
    rng = np.random.default_rng(48)
    sample = np.array(sorted(set(rng.choice(rows, 40, replace=False).tolist()) | set(range(296, 304, 2))), dtype=np.int32)
    return (sample,) + ttop._oracle_probs(layers, topo_mspec(), shp[1], sample)


# the kernel form each topology is in the corpus for
TOPO_FAMILIES = {'conv2_7x7': (('conv_x3_ws_kernel<7,7', 'ring>'),), 'conv1_same': (('conv_x3_ws_kernel<', 'fs>'),),
                 'ch32_64': (('conv_x3_ws_kernel<', 'ncb1>'), ('conv_x3_ws_kernel<', 'plain>')), 'ch48_96': (('conv_x3_ws_kernel<', 'plain>'),),
                 'conv2_stride2': ('conv_x3_kernel<3', 'conv_x3_wq3_kernel<'), 'conv1_pool': ('conv_x3_kernel<3', 'conv_x3_wq3_kernel<')}


class Topology(Job):
    group = 'topology_families'

    def __init__(self, name, which, mode, net_id):
        super().__init__(f'{name}_{which}_{mode}', [700, 3001])
        self.topo, self.which, self.mode, self.net_id = name, which, mode, net_id
        self.families = TOPO_FAMILIES[name]
        comp = _topo_net(name, which)[2]
        self.passes_at_floor = -(-len(S._window_rows(3001)) // tdef._plan_chunk(comp, 1 << 30, WS_FLOOR)[0])

    def prepare(self, ctx):
        _once(ctx, 'mspec', lambda: ctx.set_mspec(topo_mspec()))
        _once(ctx, ('net', self.net_id, self.topo), lambda: ctx.cnn_load(self.net_id, _topo_net(self.topo, self.which)[2]))

    def settings(self, ctx, ws_limit=None):
        ctx.set_precision(MODES[self.mode])
        ctx.set_diag(0)
        ctx.set_workspace_limit(ws_limit or WS_DEFAULT)

    def run(self, ctx, size):
        return ctx.cnn_probs(self.net_id, S._window_rows(size))

    def check(self, size, out):
        p, fin = out
        rows = S._window_rows(size)
        sample, ref, rfin = _topo_oracle(self.topo, self.which)
        pos = np.flatnonzero(np.isin(rows, sample))
        at = np.searchsorted(sample, rows[pos])
        assert len(pos) >= 40 and not fin.all()
        assert np.array_equal(fin[pos], rfin[at]), (self.name, size)
        err = np.abs(p[pos] - ref[at]).max()
        assert err < 1e-4, (self.name, size, err)


# -------------------------------------------------------------------------------------------------------------- x-vector
@functools.lru_cache(None)
def _xv_params():
    return KM.synthetic_resnet101(0)


@functools.lru_cache(None)
def _xv_comp(frames, window):
    return KM.compile_resnet101(_xv_params(), V.FEAT_DIM, frames, window_input=window)


_XV = {}                                   # the resident features of the first context that made them, and oracle x-vectors


def _xv_pcm():
    from conftest import synth_pcm
    return synth_pcm(3, 16000 * 6)         # 598 frames


def _xv_features(ctx):
    """The features are made on the device (there is no entry that uploads them): every context must make the same bits."""
    def make():
        _vbx_prepare(ctx, 16000 * 6)
        fea = ctx.vbx_features_pcm16(_xv_pcm())
        ref = _XV.setdefault('fea', fea)
        assert np.array_equal(fea, ref), 'the x-vector front end gave other features on another context'
        return True
    _once(ctx, 'xv_fea', make)


XV_CHECKED = {144: (0, 8, 10, 16), 65: (0, 2)}      # windows held to float64: both ends, and both sides of the pass boundary at 8


def _xv_oracle(frames, windows):
    """float64 x-vectors of the given windows (one forward per width, made once)."""
    if frames not in _XV:
        x = np.stack([_XV['fea'][w * V.STEP:w * V.STEP + frames].T for w in XV_CHECKED[frames]])
        _XV[frames] = ovbx.resnet101_forward(_xv_params(), x, dtype=np.float64)
    return _XV[frames][[XV_CHECKED[frames].index(w) for w in windows]]


class XVector(Job):
    """iss_vbx_embed over (frames, windows): 11 and 17 windows of 144 frames, 3 of 65, in passes of 8 (a partial last pass; 17
    windows make three passes, and three under WS_FLOOR too): pwc chains, dual launches, pws2, pws and the statistics pooling."""
    group = 'xvector'
    SIZES = [(65, 3), (144, 11), (144, 17)]
    NET = {144: 5, 65: 6}

    def __init__(self, mode, diag=''):
        super().__init__(f'xvector_{mode}' + (f'_{diag.replace(",", "+")}' if diag else ''), self.SIZES)
        self.mode, self.diag = mode, diag
        self.families = ('conv_igemm_kernel<',) if mode == 'f32' else ('conv_x3_pws_kernel<', 'conv_x3_pws2_kernel<') + \
            (() if diag else ('conv_x3_pwc_kernel<', ('conv_x3_pws2_kernel<', 'dual>')))
        self.per = sum(int(v) for v in _xv_comp(144, True).buf_elems) * 4
        self.passes_at_floor = -(-17 // (WS_FLOOR // self.per))

    def prepare(self, ctx):
        _xv_features(ctx)
        _once(ctx, ('net', 5), lambda: ctx.cnn_load(5, _xv_comp(144, True)))
        _once(ctx, ('net', 6), lambda: ctx.cnn_load_shared(6, 5, _xv_comp(65, True)))

    def settings(self, ctx, ws_limit=None):
        ctx.set_precision(MODES[self.mode])
        ctx.set_diag(self.diag or 0)
        ctx.set_workspace_limit(ws_limit or 8 * self.per)

    def run(self, ctx, size):
        frames, n = size
        return (ctx.vbx_embed(self.NET[frames], np.arange(n, dtype=np.int32) * V.STEP),)

    def check(self, size, out):
        frames, n = size
        wins = [w for w in XV_CHECKED[frames] if w < n]
        ref, got = _xv_oracle(frames, wins), out[0][wins]
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (self.name, size, np.abs(got - ref).max())


class XVectorHost(Job):
    """The host entry iss_cnn_forward on 3 stacked windows."""
    group = 'xvector'

    def __init__(self):
        super().__init__('xvector_host_forward', [3])
        self.families = ('conv_x3_pwc_kernel<', ('conv_x3_pws2_kernel<', 'dual>'), 'conv_x3_pws_kernel<')

    def prepare(self, ctx):
        _xv_features(ctx)
        _once(ctx, ('net', 4), lambda: ctx.cnn_load(4, _xv_comp(144, False)))

    def settings(self, ctx, ws_limit=None):
        ctx.set_precision(_native.PREC_BF16X3)
        ctx.set_diag(0)
        ctx.set_workspace_limit(ws_limit or WS_DEFAULT)

    def run(self, ctx, size):
        x = np.stack([_XV['fea'][w * V.STEP:w * V.STEP + 144].T for w in (0, 8, 10)])[..., None].astype(np.float32)
        return (ctx.cnn_forward(4, x),)

    def check(self, size, out):
        ref = _xv_oracle(144, (0, 8, 10))
        assert np.abs(out[0] - ref).max() <= 1e-4 * np.abs(ref).max(), self.name


# ------------------------------------------------------------------------------------------------------------- pointwise
PW_CASES = ('bottleneck_odd_channels', 'dense_192')      # of test_gpu_cnn.PW_CASES: M = 385 (three row tiles + a single row); the dense head


@functools.lru_cache(None)
def _pw(case):
    """The program, input and float64 reference test_pointwise_streaming_kernels draws for `case`."""
    return tcnn._pw_case(case)


class Pointwise(Job):
    group = 'pointwise'

    def __init__(self, case, mode, net_id):
        super().__init__(f'{case}_{mode}', [case])
        self.case, self.mode, self.net_id = case, mode, net_id
        self.families = ('conv_igemm_kernel<',) if mode == 'f32' else ('conv_x3_pws_kernel<',)

    def prepare(self, ctx):
        _once(ctx, ('net', self.net_id, self.case), lambda: ctx.cnn_load(self.net_id, _pw(self.case)[0]))

    def settings(self, ctx, ws_limit=None):
        ctx.set_precision(MODES[self.mode])
        ctx.set_diag(0)

    def run(self, ctx, size):
        return (ctx.cnn_forward(self.net_id, _pw(self.case)[1]),)

    def check(self, size, out):
        ref = _pw(self.case)[2]
        err = np.abs(out[0] - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 1e-4, (self.name, err)


# ---------------------------------------------------------------------------------------------------------------- corpus
@functools.lru_cache(None)
def jobs():
    J = [Sidekit('i16'), Sidekit('f32'), VbxFeatures(), VbxBatch(),
         Resample(44100, 2, 20011), Resample(44056, 1, 20011), ResampleMixed(), FlacJob(), AdpcmJob()]
    for net in SegNet.NETS:
        J += [SegNet(net, mode) for mode in ('f16x3', 'bf16x3', 'f32')]
    for net in SegNet.NETS:
        for sw in SWITCHES:
            J += [SegNet(net, mode, sw, group='segmenter_switches') for mode in ('f16x3', 'bf16x3', 'f32')]
    for k, name in enumerate(TOPO):
        J += [Topology(name, 'vad', mode, k) for mode in ('bf16x3', 'f16x3')]
    J += [XVector('bf16x3'), XVector('bf16x3', 'no_chain,no_dual'), XVector('f32'), XVectorHost()]
    for k, case in enumerate(PW_CASES):
        J += [Pointwise(case, mode, k) for mode in ('bf16x3', 'f16x3', 'f32')]
    assert len({j.name for j in J}) == len(J) and {j.group for j in J} == set(GROUPS)
    return tuple(J)


def group_jobs(group):
    return [j for j in jobs() if j.group == group]


def run_profiled(ctx, job, size):
    """(outputs, sorted kernel instance names) of one run."""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = job.run(ctx, size)
        ctx.synchronize()
        job.launched[size] = sorted(e['kernel'] for e in ctx.prof_instances())
        return out, job.launched[size]
    finally:
        ctx.prof_enable(False)


_BASE = {}


def serial_baseline(job):
    """{size: outputs} and {size: kernel instances} of `job` on a fresh context of its own, straight after prepare, every size
    held to its reference (check) and the job's families to what was launched.  Computed once per process."""
    if job.name not in _BASE:
        ctx = fresh_context()
        try:
            job.prepare(ctx)
            job.settings(ctx)
            base, inst = {}, {}
            for size in job.sizes:
                base[size], inst[size] = run_profiled(ctx, job, size)
                job.check(size, base[size])
        finally:
            ctx.close()
        names = {k for v in inst.values() for k in v}
        for fam in job.families:
            pre, suf = (fam, '') if isinstance(fam, str) else fam
            assert any(k.startswith(pre) and k.endswith(suf) for k in names), (job.name, fam, sorted(names))
        _BASE[job.name] = (base, inst)
    return _BASE[job.name]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def mismatch_report(job, size, got, want, inst, extra=''):
    """What differs between two output tuples: per array the number of differing elements and their row / column indices
    modulo the tile sizes (the pattern usually names the kernel)."""
    lines = [f'{job.name} size {size} {extra}', f'  kernel instances: {inst}']
    for k, (g, w) in enumerate(zip(got, want)):
        if same_bits(g, w):
            continue
        if g.shape != w.shape or g.dtype != w.dtype:
            lines.append(f'  output {k}: {g.dtype}{g.shape} against {w.dtype}{w.shape}')
            continue
        g2 = g.reshape(g.shape[0], -1) if g.ndim > 1 else g.reshape(-1, 1)
        w2 = w.reshape(g2.shape)
        bad = g2.view(np.uint8).reshape(g2.shape[0], g2.shape[1], -1) != w2.view(np.uint8).reshape(g2.shape[0], g2.shape[1], -1)
        r, c = np.nonzero(bad.any(axis=2))
        lines.append(f'  output {k} {g.dtype}{g.shape}: {len(r)} elements differ; first (row, col, got, want): '
                     f'{[(int(i), int(j), g2[i, j], w2[i, j]) for i, j in list(zip(r, c))[:6]]}')
        for m in (64, 128, 192, 256, 512):
            lines.append(f'    rows mod {m}: {sorted(set((r % m).tolist()))[:24]}  cols mod {m}: {sorted(set((c % m).tolist()))[:24]}')
    return '\n'.join(lines)
