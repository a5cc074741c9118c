"""
CPU-only tests of the surface of the package timbre_trap.utils.metrics (formerly the single file metrics.py): every name its callers
reach is an attribute of the package or of the family module they name, the exports are the ones of the single file, every family module
can be imported first without loading the kernel library, and no module of the evaluation side hides an import in a function body.
"""

import ast
import glob
import os
import re
import subprocess
import sys

import pytest

from timbre_trap import utils
from timbre_trap.utils import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'timbre-trap_amd')
UTILS = os.path.join(PKG, 'timbre_trap', 'utils')
FAMILIES = ('multipitch', 'mpe', 'sdr', 'notescore', 'evaluator')

# __all__ of the single file, in its order
ALL = ['resample_multipitch', 'frequencies_to_midi', 'match_count', 'multipitch_metrics', 'MultipitchEvaluator',
       'multipitch_counts_device', 'multipitch_metrics_device', 'multipitch_counts_device_notes',
       'multipitch_metrics_device_notes', 'multipitch_counts_device_track', 'multipitch_metrics_device_track', 'mpe_compact', 'MPE_MAX_EST', 'MPE_MAX_REF',
       'signal_distortion_ratio', 'signal_distortion_ratio_device', 'SignalDistortionRatio', 'SDR_CHUNK', 'SDR_MAX_FILTER',
       'note_counts', 'note_metrics', 'note_counts_device', 'note_metrics_device', 'NoteCounts', 'DeviceNoteCounts', 'NOTESCORE_MAX',
       'NOTESCORE_ROUNDS']
# what timbre_trap.utils took from the single file
FROM_UTILS = ['MultipitchEvaluator', 'multipitch_metrics', 'multipitch_metrics_device', 'multipitch_counts_device',
              'multipitch_metrics_device_notes', 'multipitch_counts_device_notes', 'multipitch_metrics_device_track',
              'multipitch_counts_device_track', 'signal_distortion_ratio', 'signal_distortion_ratio_device', 'SignalDistortionRatio',
              'note_counts', 'note_metrics', 'note_counts_device', 'note_metrics_device', 'NoteCounts', 'DeviceNoteCounts']

ATTRIBUTE = re.compile(r'\bmetrics\.([A-Za-z_]\w*)')
FROM_IMPORT = re.compile(r'^[ \t]*from (?:timbre_trap\.utils)?\.metrics(?:\.(\w+))? import (\([^)]*\)|[^\n]*)', re.M)


def _callers():
    files = glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '**', '*.py'), recursive=True)
    files += glob.glob(os.path.join(UTILS, '*.py'))
    return sorted(f for f in files if os.path.abspath(f) != os.path.abspath(__file__))


def test_every_name_the_callers_reach_is_an_attribute():
    missing, seen = [], set()
    for path in _callers():
        with open(path) as f:
            text = f.read()
        for name in ATTRIBUTE.findall(text):
            if name != 'py':                                                     # 'py': prose that names a file
                seen.add(name)
                if not hasattr(metrics, name):
                    missing.append((os.path.relpath(path, ROOT), name))
        for family, names in FROM_IMPORT.findall(text):
            where = getattr(metrics, family) if family else metrics
            for name in re.findall(r'([A-Za-z_]\w*)(?:\s+as\s+\w+)?\s*(?:,|$)', names.split('#')[0].strip('() \t').replace('\n', ' ')):
                seen.add(name)
                if not hasattr(where, name):
                    missing.append((os.path.relpath(path, ROOT), family, name))
    assert not missing, missing
    assert len(seen) >= 25, sorted(seen)                                         # the scan really read the callers


def test_exports_are_unchanged():
    assert metrics.__all__ == ALL and len(ALL) == 27
    for name in ALL:
        assert hasattr(metrics, name), name
    for name in FROM_UTILS:
        assert getattr(utils, name) is getattr(metrics, name), name
    assert len(FROM_UTILS) == 17 and set(FROM_UTILS) <= set(ALL)


@pytest.mark.parametrize('family', FAMILIES)
def test_a_family_module_can_be_imported_first(family):
    code = ('import timbre_trap.utils.metrics.%s as m; import timbre_trap._hip as h; assert h._lib is None; '
            'from timbre_trap.utils import metrics; assert m is metrics.%s and metrics.MultipitchEvaluator' % (family, family))
    if family == 'multipitch':
        # the host yardstick's own source asks for neither torch nor the kernel library (sys.modules cannot tell: the package imports torch)
        code += ('; import ast, inspect; nodes = list(ast.walk(ast.parse(inspect.getsource(m)))); '
                 'mods = [a.name for n in nodes if isinstance(n, ast.Import) for a in n.names]; '
                 'mods += [(n.module or "") + "." + a.name for n in nodes if isinstance(n, ast.ImportFrom) for a in n.names]; '
                 'assert mods and not [x for x in mods if "torch" in x.split(".") or "_hip" in x.split(".")], mods')
    subprocess.check_call([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=PKG))


def test_no_import_hides_in_a_function_body():
    files = sorted(glob.glob(os.path.join(UTILS, 'metrics', '*.py'))) + [os.path.join(UTILS, n + '.py') for n in ('pitch', 'contours', 'notes')]
    assert len(files) == len(FAMILIES) + 4, files
    hidden = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read())
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                hidden += [(os.path.relpath(path, ROOT), fn.lineno, n.lineno) for n in ast.walk(fn) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not hidden, hidden
