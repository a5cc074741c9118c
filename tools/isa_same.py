"""Are two hipcc --cuda-device-only -S listings of one source the same device code?  python tools/isa_same.py old.s new.s
Compares per symbol, not per file (template instantiations are emitted in the order of their first reference in host code): every
function body and every .amdhsa_kernel descriptor, comments stripped, compilation-unit ids and local labels replaced by fixed tokens.
Exit status 0 = the same set of symbols and every body and descriptor identical."""
import re
import sys


def symbols(path):
    out, key = {}, None
    for line in open(path):
        line = re.sub(r'\s*;.*', '', line.rstrip())
        line = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', line)
        line = re.sub(r'\.LBB\d+_', '.LBB_', line)
        line = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', line)
        if not line:
            continue
        m = re.match(r'^\s*\.type\s+(\w+),@function', line)
        d = re.match(r'^\s*\.amdhsa_kernel\s+(\w+)', line)
        if m:
            key = m.group(1)
        elif d:
            key = 'descriptor of ' + d.group(1)
        elif re.match(r'^\s*\.(end_amdhsa_kernel|section|text|amdgpu_metadata)\b', line):
            key = None
        if key is not None:
            out.setdefault(key, []).append(line)
    return out


old, new = symbols(sys.argv[1]), symbols(sys.argv[2])
differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
for what, names in (('only in old', sorted(old.keys() - new.keys())), ('only in new', sorted(new.keys() - old.keys())), ('differs', differ)):
    for k in names:
        print('%s: %s' % (what, k))
kernels = sum(1 for k in new if k.startswith('descriptor of '))
print('%d symbols old, %d new (%d kernels), %d differ' % (len(old), len(new), kernels, len(differ)))
sys.exit(0 if old.keys() == new.keys() and not differ else 1)
