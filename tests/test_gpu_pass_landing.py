"""Results of iss_cnn_probs_async land pass by pass (include/iss.h, iss_wait_slots): with page-locked outputs every pass stores
its slot range straight into the caller's arrays and the host may read it while later passes run.  What has landed is byte-equal to the
synchronous call's result, `landed` only grows, and pageable outputs keep the single landing.  No tolerance anywhere: the same
kernels run on the same data."""
import numpy as np
import pytest

from inaspeechsegmenter_amd import keras_model as KM, segmenter as S, _native
from test_gpu_cnn_defaults import _fresh

pytestmark = pytest.mark.gpu

NETS = ((21, 3, 1), (24, 2, 2))                      # (mel columns, classes, seed) of the two stand-ins
LIMIT = 64 << 20                                     # the smallest workspace the library takes: passes of a few dozen windows
N = 1203                                             # consecutive windows; no multiple of a pass size (asserted below)


def _pass_size(comp):
    """plan_chunk (csrc/cnn.hip) for a list longer than one pass: what fits the workspace, rounded down to a multiple of 8."""
    bc = LIMIT // (4 * int(np.sum(comp.buf_elems)))
    return bc - bc % 8 if bc > 8 else bc


@pytest.fixture(scope='module')
def dev():
    """A context of this file's own (shipped defaults, small workspace) with both stand-ins loaded -> (context, [(nmel, pass size)])."""
    c = _fresh()
    c.set_workspace_limit(LIMIT)
    info = []
    for k, (nmel, ncls, seed) in enumerate(NETS):
        layers, shp = KM.synthetic_ina_like(nmel, ncls, seed=seed)
        comp = KM.compile_layers(layers, shp)
        c.cnn_load(k, comp)
        bc = _pass_size(comp)
        assert bc >= 8 and N % bc and -(-N // bc) >= 4, (bc, N)
        info.append((nmel, bc))
    yield c, info
    c.close()


def _mspec(T, seed=5):
    return np.random.default_rng(seed).normal(-3.0, 1.5, (T, 24)).astype(np.float32)


def _dead(m, nmel, rows):
    bad = np.concatenate([[0], np.cumsum(~np.isfinite(m[:, :nmel]).all(axis=1))])
    return bad[rows + 68] != bad[rows]


def _boundaries(rows, dead, bc):
    """Slot ends of the passes' landings: a pass of bc live windows lands up to the slot of the next live window."""
    live = np.flatnonzero(~dead)
    if len(live) == len(rows):
        return list(range(bc, len(rows), bc)) + [len(rows)]
    return [int(live[i]) for i in range(bc, len(live), bc)] + [len(rows)]


def _sentinel_outputs(c, n, ncls, pinned=True):
    if pinned:
        p, f = c.pinned_empty((n, ncls), np.float32), c.pinned_empty((n,), np.uint8)
    else:
        p, f = np.empty((n, ncls), np.float32), np.empty((n,), np.uint8)
    p[:] = np.nan
    f[:] = 0xFF
    return p, f


def _release(c, *arrays):
    for a in arrays:
        c.pinned_free(a)


def _check_prefix(p, f, want_p, want_f, landed):
    assert not np.isnan(p[:landed]).any() and not (f[:landed] == 0xFF).any()
    assert p[:landed].tobytes() == want_p[:landed].tobytes()
    assert np.array_equal(f[:landed], want_f[:landed].astype(np.uint8))


def _walk(c, ticket, p, f, want, bounds, n):
    """wait_slots at every pass boundary and one slot either side of it; -> the answers."""
    seen, last = [], 0
    for b in bounds:
        for upto in (b - 1, b, b + 1):
            landed = c.wait_slots(ticket, upto)
            assert landed >= min(upto, n) and landed >= last and landed <= n, (upto, landed, last)
            _check_prefix(p, f, want[0], want[1], landed)
            seen.append(landed)
            last = landed
    assert last == n
    assert c.wait_slots(ticket, 0) == n                  # a poll after the end
    return seen


def _case(c, net_id, nmel, ncls, bc, m, rows, pinned=True):
    c.set_mspec(m)
    want = c.cnn_probs(net_id, rows)                     # (the network's first call also settles the precision guard)
    n = len(rows)
    dead = _dead(m, nmel, rows)
    bounds = _boundaries(rows, dead, bc) if pinned and not dead.all() else [n]
    p, f = _sentinel_outputs(c, n, ncls, pinned)
    t, p, f = c.cnn_probs_async(net_id, rows, p, f)
    polled = c.wait_slots(t, 0)                          # never blocks
    assert 0 <= polled <= n
    seen = _walk(c, t, p, f, want, bounds, n)
    print(f'net {net_id}: {n} slots, {int(dead.sum())} dead, passes of {bc}: {len(bounds)} landings expected; polled {polled} at once, '
          f'then {sorted(set(seen))}')
    c.wait(t)
    c.wait(-1)
    assert c.wait_slots(t, n) >= n                       # retired: everything has landed
    if pinned:
        _release(c, p, f)
    return dead, bounds, seen


@pytest.mark.parametrize('k', [0, 1])
def test_plain_path_lands_pass_by_pass(dev, k):
    """(a) no dead window: pass k lands slots [k * bc, (k + 1) * bc)."""
    c, info = dev
    nmel, bc = info[k]
    rows = np.arange(N, dtype=np.int32)
    dead, bounds, seen = _case(c, k, nmel, NETS[k][1], bc, _mspec(N + 67), rows)
    assert not dead.any() and len(bounds) >= 4
    assert set(seen) <= set(bounds) | {0}                # only whole passes land


@pytest.mark.parametrize('k', [0, 1])
def test_compact_path_lands_with_its_dead_slots(dev, k):
    """(b) -inf rows: dead windows at the very start, at the very end, across a pass boundary and inside a pass."""
    c, info = dev
    nmel, bc = info[k]
    m = _mspec(N + 67)
    m[0:2] = -np.inf                                     # windows 0 and 1
    m[N + 66] = -np.inf                                  # the last window
    m[67 + 2 + 3 * bc] = -np.inf                         # 68 windows from live index 3 * bc on: the fourth pass starts behind them
    m[67 + 2 + 3 * bc + 68 + bc + bc // 2] = -np.inf     # ... and 68 in the middle of a later pass
    rows = np.arange(N, dtype=np.int32)
    dead, bounds, seen = _case(c, k, nmel, NETS[k][1], bc, m, rows)
    live = np.flatnonzero(~dead)
    assert dead[0] and dead[1] and not dead[2] and dead[-1] and not dead[-2]
    assert live[3 * bc - 1] + 69 == live[3 * bc]        # a pass boundary with 68 dead slots in it: they land with the pass in front
    assert len(bounds) >= 4 and set(seen) <= set(bounds) | {0}


def test_every_window_dead_is_one_landing(dev):
    """(c)"""
    c, info = dev
    m = _mspec(N + 67)
    m[::50] = -np.inf
    dead, bounds, seen = _case(c, 0, info[0][0], NETS[0][1], info[0][1], m, np.arange(N, dtype=np.int32))
    assert dead.all() and bounds == [N]


def test_five_windows_are_one_pass(dev):
    """(d)"""
    c, info = dev
    dead, bounds, seen = _case(c, 1, info[1][0], NETS[1][1], info[1][1], _mspec(400), np.arange(100, 110, 2, dtype=np.int32))
    assert bounds == [5]


@pytest.mark.parametrize('with_dead', [False, True])
def test_pageable_outputs_keep_the_single_landing(dev, with_dead):
    """(e) a copy into pageable memory would hold the submitting thread: such a call lands once, after its last pass."""
    c, info = dev
    m = _mspec(N + 67)
    if with_dead:
        m[300] = -np.inf
    dead, bounds, seen = _case(c, 0, info[0][0], NETS[0][1], info[0][1], m, np.arange(N, dtype=np.int32), pinned=False)
    assert dead.any() == with_dead and set(seen) == {N}


def test_two_tickets_in_flight_waited_on_in_turns(dev):
    """VAD then gender queued back to back, their landings waited for alternately; wait(-1) retires both."""
    c, info = dev
    m = _mspec(N + 67, seed=9)
    m[500] = -np.inf
    c.set_mspec(m)
    rows = np.arange(N, dtype=np.int32)
    want = [c.cnn_probs(k, rows) for k in (0, 1)]
    outs = [_sentinel_outputs(c, N, NETS[k][1]) for k in (0, 1)]
    tick = [c.cnn_probs_async(k, rows, *outs[k])[0] for k in (0, 1)]
    assert tick[1] == tick[0] + 1
    bounds = [_boundaries(rows, _dead(m, info[k][0], rows), info[k][1]) for k in (0, 1)]
    last = [0, 0]
    for i in range(max(len(b) for b in bounds)):
        for k in (1, 0):                                 # the later ticket first: it waits for the earlier one's work too
            upto = bounds[k][min(i, len(bounds[k]) - 1)]
            landed = c.wait_slots(tick[k], upto)
            assert upto <= landed <= N and landed >= last[k]
            last[k] = landed
            _check_prefix(*outs[k], want[k][0], want[k][1], landed)
            if k == 1:                                   # one stream: the gender call's first landing is behind the whole VAD call
                assert c.wait_slots(tick[0], 0) == N
    assert last == [N, N]
    c.wait(-1)
    for k in (0, 1):
        assert c.wait_slots(tick[k], N) >= N and c.wait_slots(tick[k], 0) >= N
        assert outs[k][0].tobytes() == want[k][0].tobytes() and np.array_equal(outs[k][1].astype(bool), want[k][1])
        _release(c, *outs[k])
    assert c.wait_slots(tick[1] + 5, 1) >= 1             # a ticket never given out


def test_dense_segmentation_does_not_depend_on_the_pass_count():
    """Segmenter.segment_device_pcm(dense=True) smooths what has landed: with passes of a few dozen windows (dozens of landings
    per network) == the default workspace (one pass) == the reference-semantics call."""
    import torch
    import bench
    seg = S.Segmenter(vad_engine='smn', detect_gender=True, ffmpeg=None, models='synthetic')
    try:
        pcm = bench.synth_recording(0, 40 * 16000, 'cuda')
        torch.cuda.synchronize()
        n = pcm.numel()
        one_pass = seg.segment_device_pcm(pcm.data_ptr(), n, dense=True)
        seg.ctx.set_workspace_limit(LIMIT)
        nslots = len(S._window_rows((n - 400) // 160 + 1))
        for net in (seg.vad, seg.gender):
            assert -(-nslots // _pass_size(net.compiled)) >= 4
        many = seg.segment_device_pcm(pcm.data_ptr(), n, dense=True)
        ref = seg.segment_device_pcm(pcm.data_ptr(), n, dense=False)
        assert many == one_pass and many == ref
        assert len({lab for lab, _, _ in many}) >= 3, many
    finally:
        seg.close()
