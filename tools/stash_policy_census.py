#!/usr/bin/env python3
"""Cache-policy bits of the 16-byte global accesses in the shipped ISA, per kernel, as the shipped flags compile it
(cross-compiles, no GPU needed).  Every G16 stash access is a global_store_dwordx4 / global_load_dwordx4 (mlp_core.h:
stash_store / stash_load); the policy a call site chose shows as `sc1` (write-through store) or `nt` (non-temporal load) on
the instruction.  tests/test_cache_policy_isa.py pins the table.
    python3 tools/stash_policy_census.py [--extra "<flags>"] [file.hip ...]"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mpg_amd import build as B   # noqa: E402

ACCESS = re.compile(r'^\s*(global|buffer|flat|scratch)_(store|load)_(\w+)\s+(.*)$')
BITS = ('sc0', 'sc1', 'nt')


def asm_of(f, extra=()):
    """device assembly of translation unit f as the shipped flags compile it"""
    flags = B.COMMON + B.EXTRA.get(f, []) + list(extra) + ['-x', 'hip', '--offload-device-only', '-S']
    return subprocess.run([B.hipcc()] + flags + [os.path.join(B.CSRC, f), '-o', '-'], capture_output=True, text=True, check=True).stdout


def census_of(asm):
    """{mangled kernel: {(kind, width, bits): count}} - kind 'store' / 'load', width e.g. 'dwordx4', bits a tuple of the
    cache-policy words on the instruction (() = plain).  Scratch (spill) traffic is left out."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        a = ACCESS.match(line.split(';')[0])
        if a and cur and a.group(1) != 'scratch':
            words = a.group(4).replace(',', ' ').split()
            key = (a.group(2), a.group(3), tuple(b for b in BITS if b in words))
            out[cur][key] = out[cur].get(key, 0) + 1
    return out


def census(files=None, extra=()):
    """{(file, mangled kernel): row of census_of} over the translation units (default: all)"""
    out = {}
    for f in files or [s for s in B.sources() if s.endswith('.hip')]:
        for k, row in census_of(asm_of(f, extra)).items():
            out[(f, k)] = row
    return out


def demangle(n):
    s = subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()
    return re.sub(r'\(anonymous namespace\)::', '', s).split('(')[0].replace('void ', '')


if __name__ == '__main__':
    args = sys.argv[1:]
    extra = []
    if args and args[0] == '--extra':
        extra = args[1].split()
        args = args[2:]
    for (f, k), c in sorted(census(args or None, extra).items()):
        x4 = {key: n for key, n in c.items() if key[1] == 'dwordx4'}
        marked = {key: n for key, n in c.items() if key[2]}
        if x4 or marked:
            print('%-32s %-62s %s' % (f, demangle(k)[:62], '  '.join('%s_%s%s=%d' % (kind, w, ''.join(' ' + b for b in bits), n)
                                                                      for (kind, w, bits), n in sorted({**x4, **marked}.items()))))
