"""CPU: the float64 twins of the four native entries that were float32 only are declared in include/eap_hip.h and exported by
libeap_hip.so (no compute calls: there is no GPU where this runs)."""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NEW_ENTRIES = ['eap_gather_points_fwd_f64', 'eap_furthest_point_sampling_f64', 'eap_anchor_query_f64', 'eap_initial_anchor_query_f64']


def test_float64_entries_are_declared_and_exported():
    text = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_ENTRIES:
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert decl, f'{name} is not declared in include/eap_hip.h'
        assert 'const double *' in decl.group(1) and 'eap_stream_t stream' in decl.group(1), name
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    missing = [n for n in NEW_ENTRIES if not hasattr(lib, n)]
    assert not missing, f'not exported by libeap_hip.so: {missing}'
    assert lib.eap_abi_version() == 1


def test_no_float32_only_refusal_is_left_in_the_wrappers():
    for mod in ('gathering.py', 'grouping.py'):
        src = open(os.path.join(ROOT, 'equi-articulated-pose_amd', 'vgtk', 'cuda', mod)).read()
        assert 'float32 only' not in src and 'float32 points only' not in src, mod
