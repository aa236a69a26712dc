"""Co-scheduling screen: a result must not depend on what runs beside the call.

The hot kernels are synchronised by hand (s_waitcnt counts, global_load_lds, register rings, wavefront-scope syncs), and the
product runs four device contexts on four streams at once (pipeline.py, DEFAULT_WORKERS), while every other test of the suite has
one stream busy.  Here four threads, each with a context of its own, run the jobs of tests/screen_jobs.py against each other
(ctypes releases the GIL: the native calls overlap) in R rounds with a different stride each, so every job meets different
neighbours and different predecessors on its own context; one neighbour slot per round is plain HBM load.  Every result must
equal the serial baseline bit for bit.  R is a fixed budget that keeps the module within seconds, not a detection guarantee.

The shared-machine rules bind the test itself: the first error in any thread aborts the barrier and nothing more is launched;
nothing is retried; a mismatch fails the case at once and is not run again."""
import threading
import time

import numpy as np
import pytest

import screen_jobs as SJ

pytestmark = pytest.mark.gpu

THREADS = 4                               # pipeline.DEFAULT_WORKERS; within the 4 hardware queues of a process
ROUNDS = 6
STRIDES = (1, 2, 3, 5, 7, 11)             # per round: thread k runs item (s + k * stride) mod J
LOAD = 'hbm_load'
MIN_OVERLAP = 0.8


class _Load:
    """The neighbour that is plain HBM traffic: the SIDEKIT front end over 20 minutes of PCM and its read-back."""
    name = LOAD

    def __init__(self):
        self.pcm = (np.random.default_rng(20).standard_normal(20 * 60 * 16000, dtype=np.float32) * 2000).astype(np.int16)

    def prepare(self, ctx):
        from inaspeechsegmenter_amd import tables
        SJ._once(ctx, 'sidekit_tables', lambda: ctx.sidekit_tables(tables.sidekit_window(), tables.sidekit_melbank()))

    def run(self, ctx):
        ctx.set_signal(self.pcm)
        ctx.sidekit()
        return ctx.get_loge(), ctx.get_mspec()


def _restore(ctx, jobs):
    """What the load's front-end run replaced on this context (resident log-mel rows): set again, off the clock."""
    ctx._screen.pop('mspec', None)
    for job in jobs:
        job.prepare(ctx)


def _overlapping(stamps):
    """Whether two or more of the (start, end) intervals hold a common instant."""
    ev = sorted([(a, 1) for a, _ in stamps] + [(b, -1) for _, b in stamps], key=lambda e: (e[0], e[1]))
    depth = 0
    for _, d in ev:
        depth += d
        if depth >= 2:
            return True
    return False


@pytest.mark.parametrize('group', SJ.GROUPS)
def test_outputs_do_not_depend_on_what_runs_beside(group):
    jobs = SJ.group_jobs(group)
    items = [(job, size) for job in jobs for size in job.sizes]
    J = len(items)
    load = _Load()
    uses_mspec = group in ('segmenter_nets', 'segmenter_switches', 'topology_families')
    ctxs = [SJ.fresh_context() for _ in range(THREADS)]
    try:
        for c in ctxs:
            for job in jobs:
                job.prepare(c)
            load.prepare(c)
        # serial: every item twice on context 0; the first is the baseline, held to the job's reference and equal to the one a
        # context of its own gave (the stale-workspace screen's)
        base, inst = {}, {}
        for job, size in items:
            job.settings(ctxs[0])
            base[job.name, size] = job.run(ctxs[0], size)
            again, inst[job.name, size] = SJ.run_profiled(ctxs[0], job, size)
            assert all(SJ.same_bits(g, w) for g, w in zip(again, base[job.name, size])), \
                SJ.mismatch_report(job, size, again, base[job.name, size], '-', 'second serial run')
            job.check(size, base[job.name, size])

        barrier = threading.Barrier(THREADS, timeout=120)
        errors, failures, stamps, loads = [], [], {}, []
        lock = threading.Lock()

        def plan(r, s, k):
            """What thread k runs in round r, step s: the load in one slot per round, else an item."""
            if s == (r * 5) % J and k == (r + 1) % THREADS:
                return LOAD
            return (s + k * STRIDES[r]) % J

        def worker(k):
            ctx = ctxs[k]
            try:
                for r in range(ROUNDS):
                    for s in range(J):
                        what = plan(r, s, k)
                        if what != LOAD:
                            job, size = items[what]
                            job.settings(ctx)
                        barrier.wait()
                        t0 = time.perf_counter()
                        out = load.run(ctx) if what == LOAD else job.run(ctx, size)
                        t1 = time.perf_counter()
                        with lock:
                            stamps.setdefault((r, s), []).append((t0, t1))
                        if what == LOAD:
                            with lock:
                                loads.append((t1 - t0, len(out[0])))
                            if uses_mspec:
                                _restore(ctx, jobs)
                            continue
                        want = base[job.name, size]
                        if not all(SJ.same_bits(g, w) for g, w in zip(out, want)):
                            beside = [LOAD if plan(r, s, q) == LOAD else f'{items[plan(r, s, q)][0].name}@{items[plan(r, s, q)][1]}'
                                      for q in range(THREADS) if q != k]
                            with lock:
                                failures.append(SJ.mismatch_report(job, size, out, want, inst[job.name, size],
                                                                   f'round {r} step {s} thread {k}, beside {beside}'))
                            barrier.abort()                      # a finding: nothing more is launched, nothing is re-run
                            return
            except threading.BrokenBarrierError:
                return
            except BaseException as e:                           # NativeError, HIP error, anything: stop every thread
                with lock:
                    errors.append((k, repr(e)))
                barrier.abort()

        threads = [threading.Thread(target=worker, args=(k,), name=f'screen-{k}') for k in range(THREADS)]
        t0 = time.perf_counter()
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        wall = time.perf_counter() - t0
        assert not errors, errors
        assert not failures, '\n'.join(failures)
        done = [v for v in stamps.values() if len(v) == THREADS]
        assert len(done) == ROUNDS * J, (len(done), ROUNDS * J)
        share = sum(_overlapping(v) for v in done) / len(done)
        assert len(loads) == ROUNDS and all(n == (len(load.pcm) - 400) // 160 + 1 for _, n in loads), loads      # one load slot per round, whole
        inside = sum(b - a for v in done for a, b in v)
        print(f'{group}: the load slot ran {len(loads)} times, {np.mean([d for d, _ in loads]) * 1e3:.1f} ms each on average; '
              f'{inside:.2f} s inside native calls over the four threads')
        print(f'{group}: {J} items x {ROUNDS} rounds on {THREADS} threads in {wall:.2f} s; two or more threads inside a native '
              f'call at the same instant in {share * 100:.1f} % of the steps')
        assert share >= MIN_OVERLAP, (group, share)
    finally:
        for c in ctxs:
            c.close()
