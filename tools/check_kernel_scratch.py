#!/usr/bin/env python3
"""Registers, spills and scratch of the kernels of a gfx950 code object, from `llvm-readelf --notes`.

    llvm-readelf --notes unit.elf | python3 tools/check_kernel_scratch.py - 'conv_x3_wq_kernel|conv_x3_wq3h_kernel' 2

prints one line per kernel whose (mangled) name matches the pattern and exits 1 when one of them has a private segment (scratch:
spilled VGPRs or a stack), or when fewer kernels match than the last argument says.  The one-wave-per-SIMD conv kernels place
every instruction in the shadow of an MFMA; a spill reload is a memory access followed by a full wait in the middle of that
stream (profiles/conv2_scratch_ab.md).  parse_notes() is what tests/test_kernel_resources.py reads.
"""
import re
import sys

KEYS = ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count', 'agpr_count', 'sgpr_count',
        'group_segment_fixed_size')


def parse_notes(text):
    """{kernel name: {key: int}} for the keys above."""
    lines = text.splitlines()
    try:
        at = next(i for i, l in enumerate(lines) if l.strip() == 'amdhsa.kernels:')
    except StopIteration:
        return {}
    out, cur, indent = {}, None, None
    for l in lines[at + 1:]:
        if l and not l[0].isspace():
            break                                    # amdhsa.target: ...
        m = re.match(r'^(\s*)- (\.\w+):\s*(.*)$', l)
        if m and (indent is None or len(m.group(1)) == indent):
            indent = len(m.group(1))
            cur = {}
            key, val = m.group(2), m.group(3)
        else:
            m = re.match(r'^(\s*)(\.\w+):\s*(.*)$', l)
            if not m or cur is None or len(m.group(1)) != indent + 2:
                continue                             # an argument's entry, a list item
            key, val = m.group(2), m.group(3)
        if key == '.name':
            out[val.strip()] = cur
        elif key[1:] in KEYS:
            cur[key[1:]] = int(val)
    return out


def main(argv):
    src, pattern, least = argv[1], argv[2], int(argv[3]) if len(argv) > 3 else 1
    text = sys.stdin.read() if src == '-' else open(src).read()
    hit = {n: k for n, k in parse_notes(text).items() if re.search(pattern, n)}
    bad = 0
    for n, k in sorted(hit.items()):
        scratch = k.get('private_segment_fixed_size', -1)
        print(f"{'CHECK' if scratch else 'ok   '} {n}: scratch {scratch} B, spills v{k.get('vgpr_spill_count')} s{k.get('sgpr_spill_count')}, "
              f"vgpr {k.get('vgpr_count')} agpr {k.get('agpr_count')} sgpr {k.get('sgpr_count')}")
        bad += scratch != 0
    if len(hit) < least:
        print(f'CHECK only {len(hit)} kernels match {pattern!r}, expected at least {least}')
        return 1
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
