"""The dense path smooths results as they land (DnnSegmenter.smooth_landed, Segmenter.segment_slots): against a device double
that lands a fixed probability table in chunks, the segment list is the one DnnSegmenter.__call__(allpred=...) gives for the
whole table -- whatever the chunks are -- and no slot is read before it has landed (the double's array holds NaN until then)."""
import numpy as np
import pytest

from inaspeechsegmenter_amd import segmenter as S


class _Lander:
    """wait_slots over a table that arrives chunk by chunk: chunk k = slots [ends[k - 1], ends[k]).  A blocking wait lands no
    more chunks than it must; a poll lands nothing."""

    def __init__(self, table, ends):
        self.table, self.ends = table, list(ends)
        assert self.ends and self.ends[-1] == len(table) and all(a < b for a, b in zip(self.ends, self.ends[1:]))
        self.out = np.full_like(table, np.nan)
        self.landed, self.calls = 0, []

    def _land_upto(self, upto):
        while self.landed < min(upto, len(self.table)):
            end = next(e for e in self.ends if e > self.landed)
            self.out[self.landed:end] = self.table[self.landed:end]
            self.landed = end

    def wait_slots(self, ticket, upto):
        assert ticket == 7
        self.calls.append(upto)
        self._land_upto(upto)
        return self.landed

    def wait(self, ticket=-1):
        self._land_upto(len(self.table))


class _WaitOnly:
    """A double of the context as it was: wait(ticket) and nothing else."""

    def __init__(self, lander):
        self._l = lander

    def wait(self, ticket=-1):
        self._l.wait(ticket)


def _table(n, k, seed, run=7, peak=1.0):
    rng = np.random.default_rng(seed)
    # sticky classes with noise, so that the Viterbi has something to smooth; a few exact 0.5 rows (non-finite windows) and
    # exact zeros (log -> -inf)
    cls = np.repeat(rng.integers(0, k, n // run + 1), run)[:n]
    p = rng.random((n, k)).astype(np.float32) * 0.6
    p[np.arange(n), cls] += peak
    p /= p.sum(axis=1, keepdims=True)
    p[rng.integers(0, n, 9)] = 0.5
    p[rng.integers(0, n, 5), 0] = 0.0
    return np.ascontiguousarray(p, dtype=np.float32)


def _net(cls):
    return object.__new__(cls)


N = 400
# 'energy' / 'speech' spans: one of length 1, two that touch, the last one ending at N
SPANS = [(3, 40), (41, 42), (60, 130), (130, 131), (200, 290), (333, N)]


def _lseg(inlabel, spans, n):
    out, pos = [], 0
    for a, b in spans:
        if a > pos:
            out.append(('noEnergy', pos, a))
        out.append((inlabel, a, b))
        pos = b
    if pos < n:
        out.append(('noEnergy', pos, n))
    return out


def _chunkings(n, spans):
    ends_at_spans = sorted({b for _, b in spans} | {n})
    mid = sorted({(a + b) // 2 for a, b in spans if b - a > 1} | {n})
    return {'one slot at a time': list(range(1, n + 1)), 'everything at once': [n], 'inside the spans': mid,
            'at the span ends': ends_at_spans, 'passes of 96': list(range(96, n, 96)) + [n]}


@pytest.mark.parametrize('cls', [S.SpeechMusicNoise, S.Gender])
@pytest.mark.parametrize('spans', [SPANS, SPANS[:3], [], [(0, N)], [(N - 1, N)]], ids=['mixed', 'ends early', 'no span', 'whole', 'last slot'])
def test_smooth_landed_equals_whole_table_call(cls, spans):
    net = _net(cls)
    table = _table(N, len(cls.outlabels), seed=len(spans) + 3)
    lseg = _lseg(cls.inlabel, spans, N)
    holder = type('Ctx', (), {})()
    want = net(S._Resident(holder, 2 * N), lseg, allpred=table, ctx=holder)
    for name, ends in _chunkings(N, spans).items():
        dev = _Lander(table, ends)
        got = net.smooth_landed(dev, 7, dev.out, lseg)
        assert got == want, name
        assert [type(x) for seg in got for x in seg] == [type(x) for seg in want for x in seg], name
        if spans:
            assert dev.landed >= spans[-1][1] and dev.calls == sorted(dev.calls), name
            # nothing is waited for that no span needs: the device may still be busy behind the last span
            assert dev.landed == next(e for e in ends if e >= spans[-1][1]), name
        else:
            assert dev.calls == [] and dev.landed == 0
        # a context without wait_slots: one landing after wait
        dev = _Lander(table, ends)
        assert net.smooth_landed(_WaitOnly(dev), 7, dev.out, lseg) == want, name


class _Device:
    """The context calls Segmenter.segment_slots makes: probabilities are a function of the window's first row (so that the
    reference-semantics path, which sends the rows of its spans only, sees the same values); the asynchronous form lands in
    chunks of `chunk` slots."""
    device = 0

    def __init__(self, tables, chunk, slots_api=True):
        self.tables, self.chunk, self.live = tables, chunk, {}
        self.async_calls = 0
        if not slots_api:
            self.wait_slots = None                        # (getattr(ctx, 'wait_slots', None) is how the product asks)

    def pinned_empty(self, shape, dtype):
        return np.empty(shape, dtype)

    def pinned_free(self, a):
        pass

    def cnn_probs(self, net_id, rows):
        rows = np.asarray(rows)
        return self.tables[net_id][rows // 2].copy(), np.ones(len(rows), bool)

    def cnn_probs_async(self, net_id, rows, probs_out, finite_out):
        table = self.tables[net_id][np.asarray(rows) // 2]
        n = len(table)
        probs_out[:] = np.nan
        self.async_calls += 1
        ticket = 100 + self.async_calls
        self.live[ticket] = [table, probs_out, 0]
        return ticket, probs_out, finite_out

    def _land(self, ticket, upto):
        # one stream: everything queued before `ticket` lands first
        for t in sorted(self.live):
            table, out, landed = self.live[t]
            goal = len(table) if t < ticket else min(upto, len(table))
            while landed < goal:
                end = min(landed + self.chunk, len(table))
                out[landed:end] = table[landed:end]
                landed = end
            self.live[t][2] = landed
            if t == ticket:
                return landed
        return 2 ** 31 - 1

    def wait_slots(self, ticket, upto):
        return self._land(ticket, upto)

    def wait(self, ticket=-1):
        if not self.live:                                 # (everything retired already)
            return
        self._land(max(self.live) if ticket < 0 else ticket, 2 ** 31 - 1)
        if ticket < 0 or ticket >= max(self.live):
            self.live.clear()


@pytest.mark.parametrize('engine', ['smn', 'sm'])
@pytest.mark.parametrize('chunk,slots_api', [(1, True), (37, True), (10 ** 6, True), (37, False)])
def test_segment_slots_dense_equals_reference_semantics(engine, chunk, slots_api):
    T = 6001                                             # odd: the slot list gets its extra copy of the last window
    nslots = len(S._window_rows(T))
    nvad = 3 if engine == 'smn' else 2
    # long, decided stretches (the transition penalties are 80 and 150 decades): several speech spans, of several runs each
    tables = {0: _table(nslots + 40, nvad, seed=1, run=150, peak=60.0), 1: _table(nslots + 40, 2, seed=4, run=80, peak=200.0)}
    rng = np.random.default_rng(6)
    loge = np.repeat(np.where(rng.random(T // 100 + 1) < 0.7, 2.0, -9.0), 100)[:T].astype(np.float32) + rng.normal(0, 0.1, T).astype(np.float32)
    loge[-120:] = 2.0                                    # the recording ends inside an 'energy' span

    def segmenter(dev):
        seg = object.__new__(S.Segmenter)
        seg.energy_ratio, seg.detect_gender, seg.ctx = 0.03, True, dev
        seg.vad = _net(S.SpeechMusicNoise if engine == 'smn' else S.SpeechMusic)
        seg.gender = _net(S.Gender)
        seg.vad.ctx = seg.gender.ctx = dev
        return seg

    dev = _Device(tables, chunk, slots_api)
    seg = segmenter(dev)
    want = seg.segment_slots(S._Resident(dev, T), loge, 0, dense=False)
    got = seg.segment_slots(S._Resident(dev, T), loge, 0, dense=True)
    assert dev.async_calls == 2 and not dev.live          # both tickets were retired
    assert got == want
    labels = {lab for lab, _, _ in got}
    assert 'noEnergy' in labels and {'female', 'male'} <= labels and got[-1][2] == nslots, got
