"""File sets and their interleaved twins for the set tests: members written by sndgen.write, and the one file that holds their
channels side by side, as many frames as the longest member, a shorter member continued with samples of value 0.0."""
import os

import numpy as np

import sndgen
import wavgen


def signals(lens, chs, seed, peak=0.9):
    """One float signal per member: (lens[m],) for a one-channel member, else (lens[m], chs[m])."""
    return [wavgen.make_signal(n, c, seed + 17 * m, peak) for m, (n, c) in enumerate(zip(lens, chs))]


def interleave(xs):
    """The twin's float samples: the members' channels side by side, zero-padded to the longest."""
    cols = [x.reshape(len(x), -1) for x in xs]
    out = np.zeros((max(len(c) for c in cols), sum(c.shape[1] for c in cols)))
    at = 0
    for c in cols:
        out[:len(c), at:at + c.shape[1]] = c
        at += c.shape[1]
    return out


def write_set(folder, stem, xs, sr, kind='i16', containers='wav', big=False, twin_container=None):
    """Members `xs` (float signals) written as <stem>.m<k>.<container> of `kind`, and their twin <stem>.twin.<container>
    -> ([member paths], twin path).  containers: one name for all members, or one per member (`big` likewise)."""
    if isinstance(containers, str):
        containers = [containers] * len(xs)
    bigs = [big] * len(xs) if isinstance(big, bool) else list(big)
    paths = []
    for k, (x, cont, b) in enumerate(zip(xs, containers, bigs)):
        paths.append(sndgen.write(os.path.join(str(folder), f'{stem}.m{k}.{cont}'), cont, kind, b, x, sr)[0])
    tc = twin_container or containers[0]
    twin = sndgen.write(os.path.join(str(folder), f'{stem}.twin.{tc}'), tc, kind, bigs[0], interleave(xs), sr)[0]
    return paths, twin


def mono_set(folder, stem, lens, sr, seed, kind='i16', containers='wav', big=False):
    """A set of one-channel members of `lens` frames -> ([member paths], twin path)."""
    return write_set(folder, stem, signals(lens, [1] * len(lens), seed), sr, kind, containers, big)
