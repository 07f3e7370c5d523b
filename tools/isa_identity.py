#!/usr/bin/env python3
"""Instruction identity of the library's gfx950 kernels between a base commit and the working tree:
   tools/isa_identity.py [--base REV] [--keep DIR] [--define FLAG ...] [unit.hip ...]
                                                                       (default: HEAD, every .hip unit of the Makefile)

Each unit is compiled device-only from both trees with the Makefile's flags (derivatives.hip with -fno-slp-vectorize),
disassembled with llvm-objdump -d, and compared kernel by kernel: the instruction text and encodings (addresses
dropped, so that a kernel does not differ because an earlier one changed length), and the register / scratch / LDS
figures of the code object's notes.  --define FLAG (repeatable, e.g. --define=-DNDT_BODY_STAMPS) is passed to both builds,
so that a build variant can be compared as well.  A refactor's claim that the shipped kernels do not change is this tool printing
'identical' for every kernel.  Exit status 1 if any kernel differs."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = 'xchu_slam_amd/csrc'
LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
         '--cuda-device-only', '--no-gpu-bundle-output']
RES = ['.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size']


def units_of(tree):
    mk = open(os.path.join(tree, CSRC, 'Makefile')).read().replace('\\\n', ' ')
    return re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()


def build(tree, unit, out, defines):
    flags = FLAGS + defines + (['-fno-slp-vectorize'] if unit == 'derivatives.hip' else [])
    subprocess.run([HIPCC] + flags + ['-c', unit, '-o', out], cwd=os.path.join(tree, CSRC), check=True)


def kernels(co):
    """{symbol: [instruction lines without addresses]} and the whole disassembly minus its 'file format' line"""
    txt = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', co], check=True, capture_output=True, text=True).stdout
    whole = '\n'.join(l for l in txt.split('\n') if 'file format' not in l)
    out, cur = {}, None
    for line in txt.split('\n'):
        m = re.match(r'^[0-9a-f]+ <(\S+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r'// [0-9A-F]+:', '//', line.strip()))
    return out, whole


def resources(co):
    txt = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r'\n\s*- \.agpr_count', txt)[1:]:
        name = re.search(r'^\s*\.name:\s*(\S+)', blk, re.M)
        if name:
            out[name.group(1)] = [int(re.search(r'^\s*\%s:\s*(\d+)' % k, blk, re.M).group(1)) for k in RES]
    return out


def demangle(names):
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt', path=LLVM)
    if not filt:
        return {n: n for n in names}
    p = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, p.stdout.split('\n')))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--base', default='HEAD')
    ap.add_argument('--keep', help='directory that keeps the code objects (default: a temporary one)')
    ap.add_argument('--define', action='append', default=[], metavar='FLAG', help='compiler flag for both builds (repeatable)')
    ap.add_argument('units', nargs='*')
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix='isa_identity_')
    sha = subprocess.run(['git', 'rev-parse', '--short', a.base], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    base = os.path.join(tmp, 'base-' + sha)   # with --keep, the base's code objects are built once per commit
    if not os.path.isdir(base):
        os.makedirs(base)
        ar = subprocess.run(['git', 'archive', sha, CSRC, 'include'], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', base], input=ar, check=True)
    differs = 0
    variant = ''.join(re.sub(r'\W', '_', f) for f in a.define)  # kept code objects: one set per flag set
    for unit in a.units or units_of(ROOT):
        cos = []
        for tag, tree in (('base', base), ('new', ROOT)):
            co = os.path.join(tree if tag == 'base' else tmp, '%s%s.%s.co' % (unit[:-4], variant, tag))
            if tag == 'base' and not os.path.exists(os.path.join(tree, CSRC, unit)):
                co = None   # a unit the base does not have: its kernels, if any, are reported as 'only in new'
            elif tag == 'new' or not os.path.exists(co):
                build(tree, unit, co, a.define)
            cos.append(co)
        (kb, wb), (kn, wn) = (kernels(cos[0]) if cos[0] else ({}, None)), kernels(cos[1])
        rb, rn = (resources(cos[0]) if cos[0] else {}), resources(cos[1])
        names = demangle(sorted(set(kb) | set(kn)))
        print('## %s: %s' % (unit, 'whole disassembly identical' if wb == wn else 'not in base' if wb is None else 'DIFFERS'))
        for sym in sorted(set(kb) | set(kn)):
            if sym not in kb or sym not in kn:
                verdict = 'only in ' + ('base' if sym in kb else 'new')
            elif kb[sym] == kn[sym] and rb.get(sym) == rn.get(sym):
                verdict = 'identical'
            else:
                verdict = 'differs: %d -> %d instructions, resources %s -> %s' % (len(kb[sym]), len(kn[sym]), rb.get(sym), rn.get(sym))
            differs += verdict != 'identical'
            r = rn.get(sym) or rb.get(sym)
            res = 'vgpr %d sgpr %d scratch %d lds %d' % tuple(r) if r else ''
            print('%-10s %s  [%s]' % (verdict, names[sym].split('(')[0], res))
    sys.exit(1 if differs else 0)


if __name__ == '__main__':
    main()
