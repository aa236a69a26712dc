#!/usr/bin/env python3
"""Idle gaps on the GPU timeline of the LAST step of a bench run, from a rocprofv3 --kernel-trace result (rocpd SQLite):
python tools/gap_report.py <results.db> [first-kernel-substring [step-index]]   (default: sidekit_kernel starts a step; the last one is detailed)"""
import sqlite3
import sys


LANDING = ('scatter_probs_kernel', 'mask_probs_kernel')      # a pass's last kernel: it stores the result, or a copy follows it


def median(v):
    """Upper median of the values that are not NaN; NaN if there is none."""
    v = sorted(x for x in v if x == x)
    return v[len(v) // 2] if v else float('nan')


def host_share(d, starts, first):
    """Per step, the parts of the timeline in which the device waits for the host: the HEAD, from the end of the step's first
    kernel to the first kernel of the networks (row_flags_kernel and the runtime's copy kernels are not: they sit on either
    side of the host's waits), and
    the INTER-STEP GAP, from the step's last kernel to the first kernel of the next step (the tail of this step and whatever the
    host does before the next one's features).  And the idle time right behind every pass's last kernel, where copies of a
    pass's result would sit.  None of the three depends on the clock the kernels ran at."""
    print("host share per step (ms):   head   inter-step gap   idle behind the passes' last kernels (count)")
    heads, gaps, lands = [], [], []
    for j, i0 in enumerate(starts):
        sq = d[i0:starts[j + 1]] if j + 1 < len(starts) else d[i0:]
        cnn = next((x for x in sq[1:] if not any(n in x[0] for n in (first, 'row_flags_kernel', '__amd_rocclr_'))), None)
        head = (cnn[1] - sq[0][2]) / 1e6 if cnn else float('nan')
        gap = (d[starts[j + 1]][1] - max(x[2] for x in sq)) / 1e6 if j + 1 < len(starts) else float('nan')
        behind = [max(0, sq[k + 1][1] - sq[k][2]) / 1e6 for k in range(len(sq) - 1) if any(n in sq[k][0] for n in LANDING)]
        print(f"  step {j}: {head:23.3f} {gap:16.3f} {sum(behind):12.3f} ({len(behind)})")
        heads.append(head); gaps.append(gap); lands.append(sum(behind))
    print(f"  median: {median(heads):23.3f} {median(gaps):16.3f} {median(lands):12.3f}")


def main():
    db = sys.argv[1]
    first = sys.argv[2] if len(sys.argv) > 2 else 'sidekit_kernel'
    c = sqlite3.connect(db)
    d = list(c.execute("select name, start, end from kernels order by start"))
    starts = [i for i, x in enumerate(d) if first in x[0]]
    if not starts:
        raise SystemExit('no step start found')
    which = int(sys.argv[3]) if len(sys.argv) > 3 else -1
    for j, i0 in enumerate(starts):
        sq = d[i0:starts[j + 1]] if j + 1 < len(starts) else d[i0:]
        print(f"step {j}: {len(sq)} kernels, span {(max(x[2] for x in sq) - sq[0][1]) / 1e6:.2f} ms, sum of durations {sum(x[2] - x[1] for x in sq) / 1e6:.2f} ms")
    host_share(d, starts, first)
    i0 = starts[which]
    seq = d[i0:starts[which + 1]] if which != -1 and which + 1 < len(starts) else d[i0:]
    t0, t1 = seq[0][1], max(x[2] for x in seq)
    busy, cur_end, gaps = 0, seq[0][1], []
    for n, s, e in seq:
        if s > cur_end:
            gaps.append((s - cur_end, n))
        busy += max(0, e - max(s, cur_end))
        cur_end = max(cur_end, e)
    print(f"last step: {len(seq)} kernels, span {(t1 - t0) / 1e6:.2f} ms, busy {busy / 1e6:.2f} ms, idle {(t1 - t0 - busy) / 1e6:.2f} ms in {len(gaps)} gaps")
    print("largest gaps (ms, kernel that follows):")
    for g, n in sorted(gaps, reverse=True)[:12]:
        print(f"  {g / 1e6:8.3f}  {n[:70]}")
    hist = {}
    for g, n in gaps:
        k = n.split('(')[0][-50:]
        a = hist.setdefault(k, [0, 0])
        a[0] += 1; a[1] += g
    print("idle time by following kernel:")
    for k, (cnt, tot) in sorted(hist.items(), key=lambda kv: -kv[1][1])[:10]:
        print(f"  {tot / 1e6:8.3f} ms in {cnt:4d} gaps before {k}")


if __name__ == '__main__':
    main()
