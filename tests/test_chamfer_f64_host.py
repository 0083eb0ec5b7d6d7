"""CPU: the float64 chamfer forward and the two ordered backwards are declared in include/eap_hip.h at their widths and exported by
libeap_hip.so, and the Python module no longer refuses float64 (no compute calls: there is no GPU where this runs)."""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NEW_ENTRIES = {'eap_chamfer_fwd_f64': 'double', 'eap_chamfer_bwd_ordered_f32': 'float', 'eap_chamfer_bwd_ordered_f64': 'double'}


def _declarations():
    text = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_new_chamfer_entries_are_declared_at_their_width():
    text = _declarations()
    for name, scalar in NEW_ENTRIES.items():
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert decl, f'{name} is not declared in include/eap_hip.h'
        args = ' '.join(decl.group(1).split())
        other = 'float' if scalar == 'double' else 'double'
        assert f'const {scalar} *xyz1' in args and f'const {scalar} *xyz2' in args, (name, args)
        assert other not in args, (name, args)
        assert args.endswith('eap_stream_t stream'), (name, args)
        assert 'int32_t *idx1' in args and 'int32_t *idx2' in args, (name, args)
    # the ordered backwards take the argument list of eap_chamfer_bwd_f32 at their width
    old = re.search(r'\bint\s+eap_chamfer_bwd_f32\s*\(([^)]*)\)\s*;', text)
    assert old, 'eap_chamfer_bwd_f32 must stay declared'
    want = ' '.join(old.group(1).split())
    for name, scalar in (('eap_chamfer_bwd_ordered_f32', 'float'), ('eap_chamfer_bwd_ordered_f64', 'double')):
        got = ' '.join(re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text).group(1).split())
        assert got == want.replace('float', scalar), (name, got)
    fwd = ' '.join(re.search(r'\bint\s+eap_chamfer_fwd_f32\s*\(([^)]*)\)\s*;', text).group(1).split())
    got = ' '.join(re.search(r'\bint\s+eap_chamfer_fwd_f64\s*\(([^)]*)\)\s*;', text).group(1).split())
    assert got == fwd.replace('float', 'double'), got


def test_new_chamfer_entries_are_exported():
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    missing = [n for n in list(NEW_ENTRIES) + ['eap_chamfer_fwd_f32', 'eap_chamfer_bwd_f32'] if not hasattr(lib, n)]
    assert not missing, f'not exported by libeap_hip.so: {missing}'
    assert lib.eap_abi_version() == 1


def test_chamfer_module_no_longer_refuses_float64():
    src = open(os.path.join(ROOT, 'equi-articulated-pose_amd', 'chamfer.py')).read()
    assert 'float32 only' not in src
    for name in NEW_ENTRIES:
        assert name[:-3] in src, f'chamfer.py never calls {name}'
