#!/usr/bin/env python3
"""The conv kernel instantiations the built library holds, read from its symbol table.

Every `__global__` template instantiation leaves its mangled name in the host symbol table (the kernel handle and its
`__device_stub__` twin): weak symbols for the kernels of namespace issk (`_ZN4issk17conv_x3_fp_kernelILi5ELi3ELb1E...EEvNS_8ConvArgsE`),
local ones for those of cnn.hip's unnamed namespace (`_ZN12_GLOBAL__N_114conv_x3_kernelILi0ELb1ELi2EEEvN4issk8ConvArgsE`).  This tool
reads `.symtab` / `.dynsym` of `libiss_hip.so` (or of the unit object files) with `struct`, decodes the `Li<n>E` / `Lb<0|1>E` template
argument list with a regex -- no demangler, no LLVM tool -- and returns one canonical key per instantiation:

    conv_x3_ws_kernel<5,3,false,false,true,1,1,false,false,2>          (every template argument, defaults included)

`canonical_of_profiler_name` turns the name the library's profiler reports for a launch (conv_select.h inst_name, read through
ctx.prof_instances()) into the same key; `profiler_name_of` is its inverse on the held instantiations.  The forms of
conv_x3_ws_kernel print <KH,KW,PADDED,TR,FUSED,NH,EPI> and a word for the arguments behind them (FS, F32, NCB):

    (none) / ,plain / ,ring     false,false,2          ,fs     true,false,2
    ,f32                        false,true,2           ,ncb1   false,false,1

tests/test_conv_instantiation_ledger.py holds tests/golden/conv_instantiations.json to this list in both directions.

    python tools/list_conv_instantiations.py [libiss_hip.so | unit.o ...]
"""
import glob
import os
import re
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'inaspeechsegmenter_amd')

# <length><name>I<template arguments>E ... inside issk:: or the unnamed namespace; the stubs' names begin with __device_stub__
_SYM = re.compile(r'^_ZN(?:4issk|12_GLOBAL__N_1)(\d+)(conv[0-9a-z_]*_kernel)I((?:L[a-z]n?\d+E)+)E')
_ARG = re.compile(r'L([a-z])(n?)(\d+)E')

WS_MAXNT = 16                                     # conv_ws.h: more taps than this is the ring form
_WS_WORDS = {'': ('false', 'false', '2'), 'plain': ('false', 'false', '2'), 'ring': ('false', 'false', '2'),
             'fs': ('true', 'false', '2'), 'f32': ('false', 'true', '2'), 'ncb1': ('false', 'false', '1')}


def decode_symbol(sym):
    """Mangled symbol -> canonical instantiation, or None when it is not a conv kernel instantiation."""
    m = _SYM.match(sym)
    if not m or int(m.group(1)) != len(m.group(2)):
        return None
    args = []
    for kind, neg, val in _ARG.findall(m.group(3)):
        if kind == 'b':
            if val not in ('0', '1'):
                return None
            args.append('true' if val == '1' else 'false')
        else:
            args.append(('-' if neg else '') + str(int(val)))
    return f'{m.group(2)}<{",".join(args)}>'


def elf_symbols(path):
    """Every symbol name of .symtab and .dynsym of a little-endian ELF64 file."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:4] != b'\x7fELF' or data[4] != 2 or data[5] != 1:
        raise ValueError(f'{path}: not a little-endian ELF64 file')
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    if shnum == 0 and shoff:                                            # more than 0xff00 sections: the count is in section 0
        shnum, = struct.unpack_from('<Q', data, shoff + 0x20)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, typ, _, _, off, size, link, _, _, entsize in sections:
        if typ not in (2, 11) or not entsize:                           # SHT_SYMTAB, SHT_DYNSYM
            continue
        str_off, str_size = sections[link][4], sections[link][5]
        strtab = data[str_off:str_off + str_size]
        for k in range(size // entsize):
            st_name, = struct.unpack_from('<I', data, off + k * entsize)
            if st_name:
                names.add(strtab[st_name:strtab.index(b'\0', st_name)].decode('ascii', 'replace'))
    return names


def default_paths():
    """The built library, else the unit object files, else nothing."""
    lib = os.path.join(PKG, 'libiss_hip.so')
    if os.path.exists(lib):
        return [lib]
    return sorted(glob.glob(os.path.join(PKG, 'csrc', '*.o')))


def held_instantiations(paths=None):
    """The set of canonical conv kernel instantiations held by the files given (default: default_paths())."""
    held = set()
    for p in (default_paths() if paths is None else paths):
        for s in elf_symbols(p):
            key = decode_symbol(s)
            if key:
                held.add(key)
    return held


def _split(name):
    m = re.match(r'^(conv[0-9a-z_]*_kernel)<([^<>]*)>$', name)
    if not m:
        raise ValueError(f'not a conv kernel instantiation name: {name!r}')
    return m.group(1), m.group(2).split(',')


def canonical_of_profiler_name(name):
    """The profiler's name of a launch (conv_select.h inst_name) -> canonical instantiation."""
    kernel, args = _split(name)
    if kernel == 'conv_x3_ws_kernel':
        word = args.pop() if len(args) == 8 else ''
        if len(args) != 7 or word not in _WS_WORDS:
            raise ValueError(f'unknown form of conv_x3_ws_kernel: {name!r}')
        args = args + list(_WS_WORDS[word])
    elif kernel == 'conv_x3_pws2_kernel':                                # <SIMPLE,STRIDED,DUAL>, printed <..,..> or <..,..,dual>
        if len(args) == 3 and args[2] == 'dual':
            args = args[:2] + ['true']
        elif len(args) == 2:
            args = args + ['false']
        else:
            raise ValueError(f'unknown form of conv_x3_pws2_kernel: {name!r}')
    for a in args:
        if not re.match(r'^(true|false|-?\d+)$', a):
            raise ValueError(f'template argument {a!r} in {name!r}')
    return f'{kernel}<{",".join(args)}>'


def profiler_name_of(key):
    """Canonical instantiation -> the name the profiler reports for it (the inverse of canonical_of_profiler_name)."""
    kernel, args = _split(key)
    if kernel == 'conv_x3_ws_kernel':
        kh, kw, padded, tr, fused, nh, epi, fs, f32, ncb = args
        if (fs, f32, ncb) == ('true', 'false', '2'):
            word = ',fs'
        elif (fs, f32, ncb) == ('false', 'true', '2'):
            word = ',f32'
        elif (fs, f32, ncb) == ('false', 'false', '1'):
            word = ',ncb1'
        elif (fs, f32, ncb) != ('false', 'false', '2'):
            raise ValueError(f'no profiler name for {key!r}')
        elif int(kh) * int(kw) > WS_MAXNT:
            word = ',ring'
        elif fused == 'false' and nh == '1' and padded == 'false':       # the unpadded plain 3x3 launch (ConvKernel::WsPlainU)
            word = ',plain'
        else:
            word = ''
        return f'{kernel}<{",".join(args[:7])}{word}>'
    if kernel == 'conv_x3_pws2_kernel':
        return f'{kernel}<{args[0]},{args[1]}{",dual" if args[2] == "true" else ""}>'
    return key


def main(argv):
    held = held_instantiations(argv or None)
    for key in sorted(held):
        print(f'{key}\t{profiler_name_of(key)}')
    print(f'{len(held)} conv kernel instantiations', file=sys.stderr)
    return 0 if held else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
