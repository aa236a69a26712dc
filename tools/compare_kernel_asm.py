#!/usr/bin/env python3
"""Compare the kernels of two gfx950 disassemblies (tools/kernel_meta.sh writes <unit>.s) instruction for instruction, kernel by
kernel, when the symbol names of the two trees differ -- a template that gained a parameter with a default changes the mangled
name of every instantiation and the addresses of everything behind it, but not an instruction of the old ones.

    python3 tools/compare_kernel_asm.py OLD.s NEW.s ['OLDNAME=NEWNAME' ...]

A kernel is the lines between its `<symbol>:` label and the next; of a line, the mnemonic with its operands and the encoding
words are compared, the address column and `<symbol+offset>` annotations are not (branches encode relative offsets).  Padding
behind a kernel (s_code_end, s_nop, objdump's `...`) is left out.  Names are demangled and compared without `(anonymous
namespace)::` and the argument list; NAME=NAME arguments are regular-expression substitutions applied to the OLD names first, e.g.
'(resample_kernel<.*)>$=\\1, false>' 'survey_kernel$=survey_kernel<false>'.  Prints one line per kernel, and exits 1 if a
kernel of OLD is missing from NEW or differs."""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        body, _, tail = line.partition('//')
        body = re.sub(r'<[^>]*>', '<sym>', body.strip())
        enc = re.sub(r'\s*<[^>]*>', '', tail.partition(':')[2].strip())
        if body.startswith(('...', 's_code_end', 's_nop')):
            continue
        cur.append(body + ' | ' + enc)
    return out


def plain(names):
    text = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return [re.sub(r'\(.*\)$', '', t.replace('(anonymous namespace)::', '')).replace('void ', '', 1) for t in text[:len(names)]]


def main(argv):
    old, new = kernels(argv[1]), kernels(argv[2])
    subs = [a.split('=', 1) for a in argv[3:]]
    old = dict(zip(plain(list(old)), old.values()))
    new = dict(zip(plain(list(new)), new.values()))
    bad = 0
    for name, code in old.items():
        to = name
        for pat, rep in subs:
            to = re.sub(pat, rep, to)
        verdict = 'missing' if to not in new else 'identical' if new[to] == code else 'DIFFERENT'
        bad += verdict != 'identical'
        print(f'{verdict:9s} {len(code):6d} instructions  {hashlib.sha256(chr(10).join(code).encode()).hexdigest()[:16]}  {name} -> {to}')
        new.pop(to, None)
    for name, code in new.items():
        print(f'{"new":9s} {len(code):6d} instructions  {hashlib.sha256(chr(10).join(code).encode()).hexdigest()[:16]}  {name}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
