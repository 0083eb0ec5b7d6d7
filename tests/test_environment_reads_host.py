"""The package reads exactly two environment variables, both numerics modes that README.md "Numerics" documents: EAP_SPLIT_PLANES
(vgtk/_hip.py) and EAP_DENSE (vgtk/so3conv/functional.py).  Every other choice of kernel is a module attribute with one shipped value,
so a stray variable in a shell cannot change which kernels a run launches.  A source scan: no GPU, no library."""
import glob
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PKG = os.path.join(ROOT, 'equi-articulated-pose_amd')

USE = re.compile(r'os\.environ|getenv')
NAMED = re.compile(r'''(?:os\.environ(?:\.get\(|\.pop\(|\.setdefault\(|\[)|getenv\()\s*['"]([A-Za-z_][A-Za-z0-9_]*)['"]''')


def test_the_package_reads_two_environment_variables():
    files = sorted(glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True)) + sorted(glob.glob(os.path.join(PKG, 'csrc', '*')))
    assert any(f.endswith('_hip.py') for f in files) and any(f.endswith('.hip') for f in files)
    names = {}
    for path in files:
        if not os.path.isfile(path) or path.endswith(('.o', '.so')):
            continue
        with open(path, errors='replace') as f:
            for no, line in enumerate(f, 1):
                for m in USE.finditer(line):
                    named = NAMED.match(line, m.start())
                    # a use that names no variable (the whole environment, a computed name) counts as a name of its own
                    name = named.group(1) if named else f'<unnamed use at {os.path.relpath(path, ROOT)}:{no}>'
                    names.setdefault(name, []).append(f'{os.path.relpath(path, ROOT)}:{no}')
    assert set(names) == {'EAP_SPLIT_PLANES', 'EAP_DENSE'}, names
