"""Instruction mix of one kernel in a hipcc -S listing.

    python tools/isa_mix.py file.s name-substring [...]             the most frequent mnemonics of every matching kernel
    python tools/isa_mix.py --phases file.s name-substring [...]    counts by class, split at the kernel's barriers
    python tools/isa_mix.py --steps K file.s name-substring [...]   segment K of --phases cut into the steps of its unrolled chain

--steps cuts at the first 4x4x4 product behind an LDS write (phase 1 of k_nrb_bwd_fused: the previous step's dA1 store) and marks the pieces
that hold a 16-row product (the steps that run the dW2 sum).  The scheduler moves a few instructions across such a cut: the pieces are
approximate, their sum is the segment's count.

--phases cuts the kernel's body, in listing order, at every s_barrier and counts each segment by class only: VALU, transcendental
(v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos), MFMA, LDS (ds_*), vector memory (global_ / buffer_ / flat_ / scratch_*), SALU
and waits (s_waitcnt, s_nop, s_barrier), plus the few mnemonics the narrow block backward's audits name (packed conversions, v_perm_b32,
v_mov_b64, v_lshl_add_u64, v_readfirstlane_b32).  The counts are static: a fully unrolled loop counts every step, a rolled one its body
once; a segment that holds both paths of a branch counts both."""
import re
import sys
from collections import Counter

TRANS = ('v_exp', 'v_log', 'v_rcp', 'v_rsq', 'v_sqrt', 'v_sin', 'v_cos')
WAITS = ('s_waitcnt', 's_nop', 's_barrier', 's_sleep')
VMEM = ('global_', 'buffer_', 'flat_', 'scratch_')
NAMED = ('v_cvt_pk', 'v_perm_b32', 'v_mov_b64', 'v_lshl_add_u64', 'v_readfirstlane_b32')
CLASSES = ('VALU', 'trans', 'MFMA', 'LDS', 'VMEM', 'SALU', 'wait')


def mnemonic(line):
    m = re.match(r'^\s+([a-z][a-z_0-9]+)(\s|$)', line)
    return m.group(1) if m else None


def classify(op):
    if op.startswith(WAITS):
        return 'wait'
    if op.startswith('v_mfma') or op.startswith('v_smfma'):
        return 'MFMA'
    if op.startswith(TRANS):
        return 'trans'
    if op.startswith('ds_'):
        return 'LDS'
    if op.startswith(VMEM):
        return 'VMEM'
    if op.startswith('s_'):
        return 'SALU'
    if op.startswith('v_'):
        return 'VALU'
    return None


def kernels(lines, pat):
    starts = [(i, l.split(':')[0]) for i, l in enumerate(lines) if re.match(r'^_Z\w+:', l)]
    for k, (i, name) in enumerate(starts):
        if pat in name:
            end = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
            for j in range(i, end):                              # the body ends with the kernel's last s_endpgm
                if lines[j].startswith('\t.section') or lines[j].startswith('\t.amdhsa_kernel'):
                    end = j
                    break
            yield name, lines[i:end]


def segments(body):
    """[(first line, Counter of classes, Counter of named mnemonics)] -- one entry per stretch between two barriers"""
    segs = [(0, Counter(), Counter())]
    for j, l in enumerate(body):
        op = mnemonic(l)
        if op is None:
            continue
        cls = classify(op)
        if cls is None:
            continue
        segs[-1][1][cls] += 1
        for n in NAMED:
            if op.startswith(n):
                segs[-1][2][n] += 1
        if op == 's_barrier':
            segs.append((j + 1, Counter(), Counter()))
    return segs


def steps(body, seg):
    """segment `seg` (as numbered by --phases) cut into the steps of an unrolled pointwise chain: a new piece starts at the first 4x4x4
    product behind an LDS write (the previous step's store).  [(first line, classes, named, holds a 16-row product)]"""
    nbar, out, wrote = 0, [], True
    for j, l in enumerate(body):
        op = mnemonic(l)
        if op is None or classify(op) is None:
            continue
        if nbar == seg:
            if op.startswith('v_mfma_f32_4x4x4') and wrote:
                out.append([j, Counter(), Counter(), False])
                wrote = False
            if not out:
                out.append([j, Counter(), Counter(), False])
            out[-1][1][classify(op)] += 1
            for n in NAMED:
                if op.startswith(n):
                    out[-1][2][n] += 1
            out[-1][3] |= op.startswith('v_mfma_f32_16x16')
            wrote |= op.startswith('ds_write')
        if op == 's_barrier':
            nbar += 1
    return out


def main(argv):
    phases = argv[1:2] == ['--phases']
    nstep = int(argv[2]) if argv[1:2] == ['--steps'] else None
    args = argv[3:] if nstep is not None else argv[2:] if phases else argv[1:]
    lines = open(args[0]).read().split('\n')
    for pat in args[1:]:
        for name, body in kernels(lines, pat):
            if nstep is not None:
                print(name)
                print(' step  line ' + ' '.join('%6s' % c for c in CLASSES) + '   16-row product, named')
                for k, (first, cls, named, wide) in enumerate(steps(body, nstep)):
                    print('  %3d %5d ' % (k, first) + ' '.join('%6d' % cls[c] for c in CLASSES) + '   %s  ' % ('yes' if wide else 'no ')
                          + ', '.join('%s %d' % kv for kv in sorted(named.items())))
                continue
            if not phases:
                c = Counter(op for op in map(mnemonic, body) if op)
                top = sorted(c.items(), key=lambda kv: -kv[1])[:28]
                print(name[:70], 'total', sum(c.values()))
                print('   ', ', '.join('%s %d' % kv for kv in top))
                continue
            print(name)
            print('  seg  line ' + ' '.join('%6s' % c for c in CLASSES) + '   named')
            for k, (first, cls, named) in enumerate(segments(body)):
                print('  %3d %5d ' % (k, first) + ' '.join('%6d' % cls[c] for c in CLASSES) + '   ' + ', '.join('%s %d' % kv for kv in sorted(named.items())))


if __name__ == '__main__':
    main(sys.argv)
