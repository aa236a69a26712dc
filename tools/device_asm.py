#!/usr/bin/env python3
"""Device assembly of every HIP unit, hashed: the recipe behind a "same instructions as the parent" claim.

    python3 tools/device_asm.py OUTDIR [--only PREFIX] [-- EXTRA_FLAG ...]

Compiles each unit of the csrc Makefile's SRCS_HIP with the Makefile's own CXXFLAGS plus `--cuda-device-only -S` into
OUTDIR/<unit>.s (at most 16 jobs), drops the lines that carry the per-compilation `__hip_cuid_` symbol and prints one
sha256 per unit.  Run it on two checkouts and diff the two lists.  --only keeps the units whose name starts with PREFIX
(may be repeated); flags behind `--` are appended (e.g. -DISS_WQ3_EXP=4).  It compiles and hashes, nothing else.
"""
import argparse, hashlib, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "inaspeechsegmenter_amd", "csrc")


def make_var(text, name, env):
    value = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1)
    return re.sub(r"\$\((\w+)\)", lambda m: env[m.group(1)], value)


def main():
    argv, extra = sys.argv[1:], []
    if "--" in argv:
        argv, extra = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--only", action="append", default=[])
    args = ap.parse_args(argv)
    text = open(os.path.join(CSRC, "Makefile")).read()
    env = {"ARCH": os.environ.get("ARCH", make_var(text, "ARCH", {}))}
    hipcc = os.environ.get("HIPCC", make_var(text, "HIPCC", env))
    flags = make_var(text, "CXXFLAGS", env).split() + extra
    units = [u for u in make_var(text, "SRCS_HIP", env).split() if not args.only or u.startswith(tuple(args.only))]
    os.makedirs(args.outdir, exist_ok=True)
    print("#", subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.splitlines()[0], " ".join(extra))

    def one(unit):
        out = os.path.join(os.path.abspath(args.outdir), unit[:-4] + ".s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", unit, "-o", out], cwd=CSRC, check=True)
        lines = [l for l in open(out, "rb") if b"__hip_cuid_" not in l]
        return hashlib.sha256(b"".join(lines)).hexdigest()

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for unit, digest in zip(units, pool.map(one, units)):
            print(digest, unit)


if __name__ == "__main__":
    main()
