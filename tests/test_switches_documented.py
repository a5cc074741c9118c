"""csrc/common.h: tt_switch is for "the documented ones, which the tests exercise".  Every environment name the shipped
library reads -- through tt_switch or a bare getenv -- must therefore be in INTEGRATION.md and in at least one test."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# read only behind tt_tune_set(), which the shipped library compiles to false (a knob of the -DTTRAP_EXPERIMENTAL build)
TUNE_ONLY = {'TTRAP_FUSED_ABLATE'}


def test_every_switch_the_library_reads_is_documented_and_tested():
    read = lambda paths: ''.join(open(p, errors='replace').read() for p in paths)
    src = read(glob.glob(os.path.join(ROOT, 'timbre-trap_amd', 'csrc', '*')))
    names = set(re.findall(r'tt_switch\(\s*"(\w+)"', src)) | set(re.findall(r'(?<![\w.])getenv\(\s*"(TTRAP_\w+)"', src))
    names -= TUNE_ONLY
    assert {'TTRAP_GEMM_VALU', 'TTRAP_SMALL_UNFUSED_BWD'} <= names, 'the scan no longer finds the switches it is known to hold: %s' % sorted(names)
    doc = read([os.path.join(ROOT, 'INTEGRATION.md')])
    tests = read(p for p in glob.glob(os.path.join(ROOT, 'tests', '*.py')) if os.path.abspath(p) != os.path.abspath(__file__))
    for n in sorted(names):
        assert re.search(r'\b%s\b' % n, doc), '%s is read by the library and not documented in INTEGRATION.md' % n
        assert re.search(r'\b%s\b' % n, tests), '%s is read by the library and exercised by no test' % n
