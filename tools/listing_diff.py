#!/usr/bin/env python3
"""Compare the device listings of two builds, kernel by kernel (no GPU):  python tools/listing_diff.py <obj dir A> <obj dir B> [name filter]
Per kernel: instructions, VGPRs, SGPRs, scratch bytes, waves per SIMD (what the register allocation admits), vector-memory instructions by
width, and how B's listing compares with A's: `identical`; `operands`: the same multiset of instructions once the operands of each one
(destination included, register numbers kept) are sorted, so only operand order inside instructions and the order of instructions may
differ; `DIFFERENT`: anything else, a mere renumbering of registers included.  A kernel whose figures differ is marked; exit status 1 when
any figure differs or a kernel exists on one side only."""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_isa_hazards as isa  # noqa: E402

VMEM = re.compile(r'^(global|flat|buffer|scratch)_(load|store|atomic)\w*')


def figures(obj):
    """{kernel: (figures tuple, listing)} of one object file"""
    with tempfile.TemporaryDirectory() as d:
        co = isa.code_object(obj, d)
        if co is None:
            return {}
        notes = subprocess.check_output([isa.TOOLS[2], '--notes', co], text=True)
        code = isa.disassembly(co)
    out = {}
    for block in notes.split('.agpr_count:')[1:]:
        f = dict(re.findall(r'\.(\w+):\s+(\S+)', block))
        sym = f['symbol'][:-len('.kd')]
        ins = code[sym]
        vgpr = int(f['vgpr_count'])
        waves = min(8, 512 // max(8, (vgpr + int(block.split()[0]) + 7) // 8 * 8))
        vmem = collections.Counter(m.group(0) for m in map(VMEM.match, ins) if m)
        out[sym] = ((len(ins), vgpr, int(f['sgpr_count']), int(f['private_segment_fixed_size']), waves, tuple(sorted(vmem.items()))), ins)
    return out


def normal(ins):
    return sorted(' '.join([i.split()[0]] + sorted(re.split(r',\s*', ' '.join(i.split()[1:])))) for i in ins)


def main(dir_a, dir_b, name=''):
    bad = 0
    for obj in sorted(glob.glob(os.path.join(dir_a, '*.o'))):
        a, b = figures(obj), figures(os.path.join(dir_b, os.path.basename(obj)))
        same = sum(1 for k in a if k in b and a[k] == b[k])
        print(f'{os.path.basename(obj)}: {len(a)} kernels in A, {len(b)} in B, {same} with identical listings')
        bad += len(set(a) ^ set(b))
        for k in sorted(set(a) & set(b)):
            if a[k] == b[k] and not (name and name in k):
                continue
            (fa, ia), (fb, ib) = a[k], b[k]
            how = 'identical' if ia == ib else 'operands' if normal(ia) == normal(ib) else 'DIFFERENT'
            bad += fa != fb
            print(f'  {k}\n    A: ins {fa[0]} vgpr {fa[1]} sgpr {fa[2]} scratch {fa[3]} waves {fa[4]} vmem {dict(fa[5])}')
            print(f'    B: ins {fb[0]} vgpr {fb[1]} sgpr {fb[2]} scratch {fb[3]} waves {fb[4]} listing {how}' + ('' if fa == fb else '   <-- FIGURES DIFFER')
                  + ('' if fa[5] == fb[5] else f' vmem {dict(fb[5])}'))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    sys.exit(main(*sys.argv[1:4]))
