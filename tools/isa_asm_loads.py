"""Audit of the global loads issued from asm statements (csrc/wide_common.h, gload_ahead) in a hipcc -S listing:

    python tools/isa_asm_loads.py file.s            # exit status 1 if a destination is touched too early

The compiler treats such a load's destination as written at the statement, while the data lands later: for every asm global load this
walks forward through the listing and counts the asm `s_waitcnt vmcnt` statements that pass before the first instruction that names one of
the destination registers.  0 waits = the register was read, copied or overwritten while the load may still be in flight.  A one-ahead load is
retired by the SECOND wait after it (the prologue request of a loop by the first), so the summary prints the count per kernel:
"(kernel, waits) loads".  The walk is textual, in listing order -- right for the unrolled straight-line loops these loads live in."""
import collections
import re
import sys

L = open(sys.argv[1]).read().split('\n')
kern, res, early = None, collections.Counter(), 0
for i, l in enumerate(L):
    m = re.match(r'^(_Z\w+):', l)
    if m:
        kern = m.group(1)
    if 'ASMSTART' in l and i + 1 < len(L):
        m = re.match(r'\s+global_load_dwordx(\d) v\[(\d+):(\d+)\], v\d+, s\[', L[i + 1])
        if not m:
            continue
        regs = set(range(int(m.group(2)), int(m.group(3)) + 1))
        waits, j = 0, i + 3
        while j < len(L) and 's_endpgm' not in L[j]:
            t = L[j]
            if re.match(r'\s+s_waitcnt vmcnt', t) and 'ASMSTART' in L[j - 1]:
                waits += 1
            elif re.match(r'\s+[a-z]', t):
                used = set()
                for a, b in re.findall(r'v\[(\d+):(\d+)\]', t):
                    used |= set(range(int(a), int(b) + 1))
                for a in re.findall(r'\bv(\d+)\b', t):
                    used.add(int(a))
                if used & regs:
                    break
            j += 1
        short = re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', kern)[:48]
        res[(short, waits)] += 1
        if waits == 0:
            early += 1
            print('TOUCHED BEFORE ANY WAIT: %s, load at line %d, first use at line %d: %s' % (short, i + 2, j + 1, L[j].strip()))
for k in sorted(res):
    print(k, res[k])
print('%d asm loads, %d touched before a wait' % (sum(res.values()), early))
sys.exit(1 if early else 0)
