#!/usr/bin/env python3
"""Per-kernel comparison of two `make asm` trees (gym-pbn-stac_amd/build/asm of two checkouts).

Usage: tools/kernel_isa_diff.py OLD_ASM_DIR NEW_ASM_DIR [| c++filt]
For every kernel in any *gfx950.s listing below either directory: SAME / DIFF of its instruction stream
(comments stripped, the per-function numbers in local labels normalised), its instruction-line count and
SAME / DIFF of its lines in the resource reports (resource.txt: registers, scratch, LDS, occupancy);
then the kernels present on one side only. Kernels are matched by symbol, whichever file they are in.
Text comparison only. Exit status 1 on any DIFF or one-sided kernel.
"""
import glob
import re
import sys


def kernels(root):
    """symbol -> (normalised instruction lines, resource report lines)"""
    body, res = {}, {}
    for path in glob.glob(root + '/**/*gfx950.s', recursive=True):
        text = open(path).read()
        for sym in re.findall(r'^\s*\.amdhsa_kernel (\S+)', text, re.M):
            m = re.search(r'^%s:.*?^\.Lfunc_end\d+:' % re.escape(sym), text, re.M | re.S)
            lines = [re.sub(r'(\.L[A-Za-z_]+)\d+_', r'\1_', l.split(';')[0].strip()) for l in m.group(0).split('\n')[1:-1]]
            body[sym] = [l for l in lines if l]
    for path in glob.glob(root + '/**/resource.txt', recursive=True):
        sym = None
        for l in open(path):
            m = re.search(r'remark: [^ ]+ +(.*?) \[-Rpass-analysis', l)
            if not m:
                continue
            if m.group(1).startswith('Function Name: '):
                sym = m.group(1).split(': ')[1]
                res[sym] = []
            elif sym:
                res[sym].append(m.group(1))
    return body, res


def main():
    (ob, orr), (nb, nr) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for sym in sorted(set(ob) & set(nb)):
        isa = 'SAME' if ob[sym] == nb[sym] else 'DIFF'
        rs = 'SAME' if orr.get(sym) == nr.get(sym) and sym in orr else 'DIFF'
        bad += isa == 'DIFF' or rs == 'DIFF'
        print('%s isa %6d/%6d lines, resources %s  %s' % (isa, len(ob[sym]), len(nb[sym]), rs, sym))
    for side, only in (('old', set(ob) - set(nb)), ('new', set(nb) - set(ob))):
        for sym in sorted(only):
            print('ONLY in %s  %s' % (side, sym))
        bad += len(only)
    print('%d kernels old, %d new, %d in both, %d differ or are one-sided' % (len(ob), len(nb), len(set(ob) & set(nb)), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
