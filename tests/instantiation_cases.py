"""One small deterministic case per conv kernel instantiation the library holds (tests/golden/conv_instantiations.json,
tools/list_conv_instantiations.py), and the one runner every case goes through (tests/test_gpu_conv_instantiations.py).

A case names a net, the arithmetic mode the instantiation belongs to and the iss_set_diag bits that route a layer to it; the
runner returns which instantiations the call launched (ctx.prof_instances()) and the distance of the result from a float64
evaluation of the same layers.  Nothing here takes a reference from the device.

Case names:

    fp/<kh>x<kw>/<valid|same>/<tr|rm>[/nh2]     host-fed single conv on conv_x3_fp_kernel (tr: bias + relu, transposed epilogue; rm: + 2x2
                                               max-pool, row-major epilogue; nh2: 128 output channels, two column halves)
    fpf/<kh>x<kw>/<tr|rm>                       patch net: first layer fused into conv_x3_fp_kernel (no_ws / no_ring where another form owns the shape)
    ws/<kh>x<kw>/<valid|same>/<tr|rm>/<epi>     patch net: first layer fused into conv_x3_ws_kernel (8..16 taps); epi 1 = relu (+ average pool),
                                               epi 0 = sigmoid (+ max-pool): the generic epilogue
    ring/<kh>x<kw>/<valid|same>/<epi>           ... the ring form (more than 16 taps): epi 1 = relu + 2x2 max-pool, epi 0 = relu, no pool
    fs/<kh>x<kw>/<valid|same>/0                 ... behind a zero-padded first layer, sigmoid + max-pool (EPI = 0)
    wsplain/epi0, wsnh2/tr/epi0                 host-fed 3x3 layers on the plain / two-column-half forms with a sigmoid epilogue
    wq3h/kind1/f32out/<mode>                    the stand-in's conv stack cut behind conv4's (2, 1) pool: CHL in, f32 out
    x3/patch_7x7, x3/gather_<valid|same>_pooled conv_x3_kernel<2, ..> (a first layer of more than 32 taps), <3 | 4, false, ..> (gather form, pooled)
    topo/<name>/<net>/<mode>/<overlapping|scattered>[/<diag>]      tests/topologies.py SPECS, whole net
    layers/<name>/<mode>                        tests/test_gpu_cnn.py TOPOLOGIES at 21 mel, whole net, scattered windows
    graph/<name>/<nmel>/<mode>                  tests/graph_nets.py NETS, host-fed
    pw/<name>                                   tests/test_gpu_cnn.py PW_CASES (hand-lowered 1x1 chains, their own float64 reference)
    xvec/<mode>/<host|resident>[/<diag>]        the seeded ResNet-101 of tests/test_gpu_vbx.py on three windows

Bounds (the project's own, no new figure): element-wise max |out - ref| < 1e-4 max(1, max |ref|) where the net ends at the layer
under test (test_generic_forward_nhwc, test_pointwise_streaming_kernels); max |log p - log p64| < BOUND[mode] of
tests/test_gpu_cnn_defaults.py where the case is a whole net with a softmax head; check_xvector's rule (tests/test_vbx_widths.py)
for x-vectors; a case that sets diag bits is also compared with the same call without them, < 5e-5 (test_topology_parity) on
the same scale.  Patch cases run T = 200 log-mel frames (100 overlapping windows of the segmenter's own list, one -inf row:
21 dead windows) at 21 AND 24 mel columns: a conv2 output of 61 x 15 rows per window spans several 512-row tiles and a partial one."""
import numpy as np

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, _native
from oracle import keras_cnn as ocnn
import topologies as TP

MODES = {'bf16x3': _native.PREC_BF16X3, 'f16x3': _native.PREC_F16X3, 'f32': _native.PREC_F32}
ELEM_BOUND = 1e-4                     # x max(1, max |ref|)
PARITY_BOUND = 5e-5                   # a diag switch against the default routing, same scale
LOGP_BOUND = {'f32': 5e-5, 'f16x3': 1e-4, 'bf16x3': 1e-3}       # tests/test_gpu_cnn_defaults.py BOUND
T_PATCH = 200
NET = 5                               # engine slot the cases load into

SIGMOID = dict(type='activation', fn='sigmoid')


def chain(spec, in_shape, seed):
    """Layer list of a topologies.py-style spec on any input shape, WITHOUT a classifier behind it: ('conv', kh, kw, cout[, padding[,
    stride]]) | ('bn_relu',) | ('relu',) | ('sigmoid',) | ('maxpool' | 'avgpool', ph, pw) | ('flatten',) | ('dense', n[, act]).  A net that
    ends on a map gets a Flatten behind it (no program row: the output is the (H, W, C) tensor as stored, and the oracle's in the same order)."""
    rng = np.random.default_rng(seed)
    h, w, c = in_shape
    L = []
    for item in spec:
        t = item[0]
        if t == 'conv':
            kh, kw, cout = item[1:4]
            padding = item[4] if len(item) > 4 else 'valid'
            s = item[5] if len(item) > 5 else 1
            L.append(TP._conv(rng, kh, kw, c, cout, padding, (s, s)))
            h, w, c = TP._out(h, kh, s, padding), TP._out(w, kw, s, padding), cout
        elif t == 'bn_relu':
            L += [TP._bn(rng, c), dict(TP.RELU)]
        elif t == 'relu':
            L.append(dict(TP.RELU))
        elif t == 'sigmoid':
            L.append(dict(SIGMOID))
        elif t in ('maxpool', 'avgpool'):
            L.append(dict(type=t, pool=(item[1], item[2]), strides=(item[1], item[2]), padding='valid'))
            h, w = h // item[1], w // item[2]
        elif t == 'flatten':
            L.append(dict(type='flatten'))
            h, w, c = 1, 1, h * w * c
        elif t == 'dense':
            L.append(TP._dense(rng, c, item[1], item[2] if len(item) > 2 else 'relu'))
            c = item[1]
        else:
            raise ValueError(t)
    if h * w != 1:
        L.append(dict(type='flatten'))
    return L


class Case:
    """kind 'patch': make(nmel) -> layers on (68, nmel, 1), read through cnn_probs at both mel widths (rows: 'overlapping' |
    'scattered').  kind 'host': make() -> (layers, in_shape, n images) through compile_layers(patch_input=False) and cnn_forward.
    kind 'lowered': make() -> (CompiledNet, x, float64 reference).  kind 'xvec': the seeded ResNet-101."""

    def __init__(self, kind, make, mode='bf16x3', diag='', rows='overlapping', nmels=(21, 24)):
        self.kind, self.make, self.mode, self.diag, self.rows, self.nmels = kind, make, mode, diag, rows, nmels


CASES = {}

# ---------------------------------------------------------------------------------------------------------------------------
# conv_x3_fp_kernel, host-fed: 3 images of 13 x 14 x 32.  A 'same' conv has 182 outputs per image (546 rows: four 128-row tiles and a
# partial one; every edge of every image is read), a 'valid' one 100..156; the pooled ones run the pool-window-major row order.
_FP_SHAPES = ((1, 3), (3, 1), (2, 2), (3, 3), (3, 5), (4, 4), (5, 3), (5, 5))


def _fp_case(kh, kw, padding, pooled, cout):
    spec = [('conv', kh, kw, cout, padding), ('relu',)] + ([('maxpool', 2, 2)] if pooled else [])
    return lambda: (chain(spec, (13, 14, 32), 100 * kh + 10 * kw + pooled), (13, 14, 32), 3)


for _kh, _kw in _FP_SHAPES:
    for _pad in ('valid', 'same'):
        for _pooled in (False, True):
            if (_kh, _kw, _pad, _pooled) == (5, 5, 'valid', True):      # (a 128-row tile of the pooled 9 x 10 output spans more than the
                continue                                                 #  360-pixel footprint: the gather kernel; topo/conv2_5x5 has the form)
            # 3x3: the weight-stationary forms own these layers by default (no_ws3: NH = 2, no_wsu3: the unpadded plain launch)
            CASES[f'fp/{_kh}x{_kw}/{_pad}/{"rm" if _pooled else "tr"}'] = Case(
                'host', _fp_case(_kh, _kw, _pad, _pooled, 72), diag='no_wsu3' if (_kh, _kw, _pad) == (3, 3, 'valid') else '')
for _pad in ('valid', 'same'):
    for _pooled in (False, True):
        CASES[f'fp/3x3/{_pad}/{"rm" if _pooled else "tr"}/nh2'] = Case('host', _fp_case(3, 3, _pad, _pooled, 128), diag='no_ws3,no_wsu3')

# ---------------------------------------------------------------------------------------------------------------------------
# first-layer-fused families: conv1 (4x5, 64, BatchNorm + relu) -> the conv under test -> end of the net
def _fused_case(kh, kw, padding, tail, conv1_padding='valid', cout=64, stride=1):
    spec = [('conv', 4, 5, 64, conv1_padding), ('bn_relu',), ('conv', kh, kw, cout, padding, stride)] + list(tail)
    return lambda nmel: chain(spec, (68, nmel, 1), 1000 + 100 * kh + 10 * kw + len(tail) + nmel)


_RELU, _RELU_MAX, _RELU_AVG, _SIG, _SIG_MAX = ([('relu',)], [('relu',), ('maxpool', 2, 2)], [('relu',), ('avgpool', 2, 2)],
                                               [('sigmoid',)], [('sigmoid',), ('maxpool', 2, 2)])
for (_kh, _kw), _diag in (((3, 5), ''), ((4, 4), ''), ((5, 3), 'no_ws'), ((5, 5), 'no_ring')):
    CASES[f'fpf/{_kh}x{_kw}/tr'] = Case('patch', _fused_case(_kh, _kw, 'valid', _RELU), diag=_diag)
    CASES[f'fpf/{_kh}x{_kw}/rm'] = Case('patch', _fused_case(_kh, _kw, 'valid', _RELU_MAX), diag=_diag)
for _kh, _kw in ((5, 3), (3, 3)):
    for _pad in ('valid', 'same'):
        CASES[f'ws/{_kh}x{_kw}/{_pad}/tr/1'] = Case('patch', _fused_case(_kh, _kw, _pad, _RELU))
        CASES[f'ws/{_kh}x{_kw}/{_pad}/tr/0'] = Case('patch', _fused_case(_kh, _kw, _pad, _SIG))
        CASES[f'ws/{_kh}x{_kw}/{_pad}/rm/1'] = Case('patch', _fused_case(_kh, _kw, _pad, _RELU_AVG))
        CASES[f'ws/{_kh}x{_kw}/{_pad}/rm/0'] = Case('patch', _fused_case(_kh, _kw, _pad, _SIG_MAX))
        CASES[f'fs/{_kh}x{_kw}/{_pad}/0'] = Case('patch', _fused_case(_kh, _kw, _pad, _SIG_MAX, conv1_padding='same'))
for _kh, _kw in ((7, 7), (5, 5), (4, 5)):
    for _pad in ('valid', 'same'):
        CASES[f'ring/{_kh}x{_kw}/{_pad}/1'] = Case('patch', _fused_case(_kh, _kw, _pad, _RELU_MAX))
        CASES[f'ring/{_kh}x{_kw}/{_pad}/0'] = Case('patch', _fused_case(_kh, _kw, _pad, _RELU))
# conv_x3_kernel<4, false, ..>: zero-padded first layer read by the gather kernel (a stride-2 second conv), pooled -> row-major
CASES['x3/gather_same_pooled'] = Case('patch', _fused_case(5, 3, 'valid', [('relu',), ('maxpool', 2, 1)], conv1_padding='same', stride=2))
# conv_x3_kernel<3, false, ..>: the same behind a 'valid' first layer
CASES['x3/gather_valid_pooled'] = Case('patch', _fused_case(5, 3, 'valid', [('relu',), ('maxpool', 2, 1)], stride=2))
# conv_x3_kernel<2, false, ..>: a patch first layer of more than 32 taps, nothing behind it to defer it for
CASES['x3/patch_7x7'] = Case('patch', lambda nmel: chain([('conv', 7, 7, 8), ('relu',)], (68, nmel, 1), 77 + nmel))
# conv_x3_wq3h_kernel<1, false, *>: conv4 reads conv3's CHL output and writes f32 (no dense layer behind its pool)
_STANDIN_CONVS = TP.SPECS['standin'][:10]
for _mode in ('bf16x3', 'f16x3'):
    CASES[f'wq3h/kind1/f32out/{_mode}'] = Case('patch', lambda nmel: chain(_STANDIN_CONVS, (68, nmel, 1), 31 + nmel), mode=_mode)

# ---------------------------------------------------------------------------------------------------------------------------
# host-fed weight-stationary 3x3 forms with the generic (sigmoid) epilogue
# WsPlain: a zero-padded layer too WIDE for the 360-pixel footprint kernel (8 x 144: 1152 rows, two 512-row tiles and a quarter)
CASES['wsplain/epi0'] = Case('host', lambda: (chain([('conv', 3, 3, 32, 'same'), ('sigmoid',)], (8, 144, 32), 41), (8, 144, 32), 1))
# WsNh2: unpadded, 128 channels, transposed (3 images of 22 x 20 -> 20 x 18: 1080 rows)
CASES['wsnh2/tr/epi0'] = Case('host', lambda: (chain([('conv', 3, 3, 128), ('sigmoid',)], (22, 20, 32), 42), (22, 20, 32), 3))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases the suite already has, through the same runner
def _topo(name, net):
    return lambda nmel: TP.nets(name)[net][0]


def _layers_case(name):
    import test_gpu_cnn as TC
    return lambda nmel: TC.TOPOLOGIES[name](np.random.default_rng(sum(map(ord, name)) + nmel), nmel)


def _graph_case(name, nmel):
    import graph_nets as GN

    def make():
        layers, shp = GN.NETS[name](nmel, 3 if nmel == 21 else 2, 5)
        return layers, tuple(shp), 5
    return make


def _pw_case(name):
    def make():
        import test_gpu_cnn as TC
        return TC._pw_case(name)
    return make


# (every name of the suite's own case tables parses; the ones the ledger points at are registered)
SUITE_CASES = (
    'topo/standin/gender/bf16x3/overlapping',
    'topo/standin/gender/f32/overlapping',
    'topo/standin/gender/f16x3/overlapping/no_shared_first',
    'topo/standin/gender/f16x3/overlapping/no_hl',
    'topo/standin/gender/f16x3/overlapping/no_wq',
    'topo/ch32_64/vad/bf16x3/overlapping',
    'topo/ch48_96/gender/bf16x3/overlapping',
    'topo/conv1_pool/gender/bf16x3/overlapping',
    'topo/conv1_pool/gender/bf16x3/scattered',
    'topo/conv1_same/gender/bf16x3/overlapping',
    'topo/conv1_same3x3_avg/gender/bf16x3/overlapping',
    'topo/conv1_same_conv2_same/gender/bf16x3/overlapping',
    'topo/conv1_same_conv2_stride2/gender/bf16x3/overlapping',
    'topo/conv1_same_nopool/gender/bf16x3/overlapping',
    'topo/conv2_5x5/vad/bf16x3/overlapping',
    'topo/conv2_5x5/gender/bf16x3/scattered',
    'topo/dense512x4/gender/f16x3/overlapping',
    'topo/overlap_pool_avg/gender/bf16x3/overlapping',
    'topo/vgg_same_3x3/gender/bf16x3/overlapping',
    'layers/bn_after_act_avgpool_global/f32',
    'layers/cin_not_multiple_of_4/f16x3',
    'graph/dense_skip/21/bf16x3',
    'graph/residual/21/bf16x3',
    'pw/bottleneck_odd_channels',
    'pw/dense_192',
    'pw/k1024_n256',
    'pw/post_affine_and_sigmoid',
    'pw/strided_projection',
    'xvec/bf16x3/host',
    'xvec/bf16x3/resident',
)


def suite_case(name):
    """The Case of a name in the suite's own vocabulary (see the module docstring)."""
    p = name.split('/')
    if p[0] == 'topo':
        net, mode, rows = p[2:5]
        return Case('patch', _topo(p[1], net), mode=mode, diag=p[5] if len(p) > 5 else '', rows=rows, nmels=(21 if net == 'vad' else 24,))
    if p[0] == 'layers':
        return Case('patch', _layers_case(p[1]), mode=p[2], rows='scattered', nmels=(21,))
    if p[0] == 'graph':
        return Case('host', _graph_case(p[1], int(p[2])), mode=p[3])
    if p[0] == 'pw':
        return Case('lowered', _pw_case(p[1]))
    if p[0] == 'xvec':
        return Case('xvec', p[2], mode=p[1], diag=p[3] if len(p) > 3 else '')
    raise KeyError(name)


for _name in SUITE_CASES:
    CASES[_name] = suite_case(_name)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references (computed once per case and kept)
def patch_input(kind, nmel):
    """(mspec, rows): log-mel-like rows (test_gpu_topologies._mspec) with one -inf bin, so that the windows over it are dead, and the
    window list.  'overlapping': T_PATCH frames under the segmenter's own list (100 windows, edge replicas included: the first
    layer is shared).  'scattered': 64 windows drawn over 1500 frames (under the 4-fold overlap rule: per-window first layer)."""
    T = T_PATCH if kind == 'overlapping' else 1500
    rng = np.random.default_rng(nmel + T)
    t = np.arange(T)[:, None]
    m = (-3 + 1.5 * np.sin(t / 37.0 + np.arange(24)[None, :] / 5.0) + rng.normal(0, 1.2, (T, 24))).astype(np.float32)
    if kind == 'overlapping':
        rows = S._window_rows(T)
        m[190, 5] = -np.inf
    else:
        rows = np.sort(rng.integers(0, T - 68, 64)).astype(np.int32)
        m[int(rows[5]) + 10, 5] = -np.inf
    return m, rows


def oracle64_patch(layers, mspec, nmel, rows):
    """float64 evaluation of `layers` on the windows, z-normalised in float64 (test_gpu_cnn_defaults._oracle64); -> (values
    (windows, out_dim), finite mask, is_logp).  A net that ends in a softmax yields log-probabilities."""
    patches = np.stack([mspec[r:r + 68, :nmel] for r in rows]).astype(np.float64)
    flat = patches.reshape(len(rows), -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        z = (flat - flat.mean(axis=1, keepdims=True)) / flat.std(axis=1, keepdims=True)
    fin = np.all(np.isfinite(z), axis=1)
    z = np.where(fin[:, None], z, 0).reshape(len(rows), 68, nmel, 1)
    logp = ends_in_softmax(layers)
    ref = ocnn.forward(layers, z, dtype=np.float64, log=logp)
    return np.asarray(ref, np.float64).reshape(len(rows), -1), fin, logp


def ends_in_softmax(layers):
    last = layers[-1]
    return last.get('activation') == 'softmax' or (last['type'] == 'activation' and last.get('fn') == 'softmax')


def elem_err(out, ref):
    """max |out - ref| / max(1, max |ref|)"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(out, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def logp_err(p, lp64, fin):
    ok = fin[:, None] & (lp64 > np.log(1e-30))
    with np.errstate(divide='ignore'):
        return float(np.abs(np.log(np.asarray(p, np.float64)) - lp64)[ok].max())


_XVEC = {}


def _xvec_bed(ctx):
    """Features of 3 s of the suite's synthetic signal (resident on the context), the seeded ResNet-101, three windows and their
    float64 x-vectors."""
    if not _XVEC:
        from conftest import synth_pcm
        from inaspeechsegmenter_amd import vbx as V
        from oracle import vbx as ovbx
        from test_vbx_widths import oracle64
        params = ovbx.resnet101_random_params(0)
        _XVEC['params'] = params
        _XVEC['sig'] = synth_pcm(11, 16000 * 3) / 32768.0
        _XVEC['V'] = V
        _XVEC['ex'] = {}
        _XVEC['starts'] = [0, 24, 48]
        fea = np.array(V.FeatureExtractor(ctx)(_XVEC['sig']))
        _XVEC['fea'] = fea
        _XVEC['ref'], _XVEC['pooled'] = oracle64(params, np.stack([fea[s:s + 144].T for s in _XVEC['starts']]))
    if id(ctx) not in _XVEC['ex']:
        _XVEC['ex'][id(ctx)] = _XVEC['V'].VBxExtractor(ctx, _XVEC['params'], batch_windows=8)
    return _XVEC


_RESULTS = {}


def run_case(ctx, name):
    """Run case `name` on `ctx` (precision, diag and profiling state restored) -> {'insts': {profiler name: launches}, 'err': float,
    'bound': float, 'metric': 'elem' | 'logp' | 'xvec', 'mode': str, 'ok': bool, 'parity': float | None, 'dead': int}.
    Results are kept per (context, case)."""
    key = (id(ctx), name)
    if key not in _RESULTS:
        _RESULTS[key] = _run(ctx, CASES[name])
    return _RESULTS[key]


def _profiled(ctx, fn):
    ctx.prof_reset()
    out = fn()
    return out, {i['kernel']: int(i['launches']) for i in ctx.prof_instances()}


def _run(ctx, case):
    prev_prec, prev_diag = getattr(ctx, 'precision', _native.PREC_BF16X3), getattr(ctx, 'diag', 0)
    res = dict(insts={}, err=0.0, metric='elem', mode=case.mode, parity=None, dead=0, ok=True)

    def add(insts):
        for k, v in insts.items():
            res['insts'][k] = res['insts'].get(k, 0) + v

    def both(fn):
        """fn() under the case's diag bits (profiled) and, where it sets any, without them."""
        ctx.set_diag(case.diag)
        out, insts = _profiled(ctx, fn)
        add(insts)
        plain = None
        if case.diag:
            ctx.set_diag(0)
            plain = fn()
        return out, plain

    ctx.prof_enable(True)
    try:
        ctx.set_precision(MODES[case.mode])
        if case.kind == 'patch':
            for nmel in case.nmels:
                layers = case.make(nmel)
                mspec, rows = patch_input(case.rows, nmel)
                ref, rfin, logp = oracle64_patch(layers, mspec, nmel, rows)
                ctx.set_mspec(mspec)
                ctx.cnn_load(NET, KM.compile_layers(layers, (68, nmel, 1)))
                (out, fin), plain = both(lambda: ctx.cnn_probs(NET, rows))
                res['ok'] &= bool(np.array_equal(fin, rfin))
                res['dead'] += int((~rfin).sum())
                res['metric'] = 'logp' if logp else 'elem'
                err = logp_err(out, ref, rfin) if logp else elem_err(out[rfin], ref[rfin])
                res['err'] = max(res['err'], err)
                if plain is not None:
                    res['ok'] &= bool(np.array_equal(plain[1], rfin))
                    scale = 1.0 if logp else max(1.0, np.abs(ref[rfin]).max())
                    res['parity'] = max(res['parity'] or 0.0, float(np.abs(out[rfin] - plain[0][rfin]).max() / scale))
        elif case.kind in ('host', 'lowered'):
            if case.kind == 'host':
                layers, shp, n = case.make()
                x = np.random.default_rng(n * 1000 + shp[0]).normal(0, 1, (n,) + tuple(shp)).astype(np.float32)
                comp = KM.compile_layers(layers, shp, patch_input=False)
                ref = np.asarray(ocnn.forward(layers, x.astype(np.float64), dtype=np.float64), np.float64).reshape(n, -1)
            else:
                comp, x, ref = case.make()
            ctx.cnn_load(NET, comp)
            out, plain = both(lambda: ctx.cnn_forward(NET, x))
            res['err'] = elem_err(out, ref)
            if plain is not None:
                res['parity'] = float(np.abs(out - plain).max() / max(1.0, np.abs(ref).max()))
        elif case.kind == 'xvec':
            from test_vbx_widths import check_xvector
            bed = _xvec_bed(ctx)
            ex = bed['ex'][id(ctx)]
            if case.make == 'resident':
                fea = bed['V'].FeatureExtractor(ctx)(bed['sig'])         # resident on the context: the windows are gathered on the device
            else:
                fea = bed['fea']
            out, plain = both(lambda: ex.get_embeddings(fea, bed['starts'], 144))
            res['metric'] = 'xvec'
            for x, r, p in zip(out, bed['ref'], bed['pooled']):
                ok, err = check_xvector(x, r, p)
                res['ok'] &= bool(ok) and bool(np.isfinite(err))
                res['err'] = max(res['err'], err)
            if plain is not None:
                res['parity'] = float(np.abs(out - plain).max() / max(1.0, np.abs(bed['ref']).max()))
        else:
            raise ValueError(case.kind)
    finally:
        ctx.prof_enable(False)
        ctx.set_diag(prev_diag)
        ctx.set_precision(prev_prec)
    res['bound'] = LOGP_BOUND[case.mode] if res['metric'] == 'logp' else ELEM_BOUND
    return res
