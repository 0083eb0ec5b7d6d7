"""CPU: the float64 regime of the SO(3) conv layers (csrc/so3_f64.hip) as far as it can be held without a GPU: the entries are declared,
exported and bound with the header's arity; empty and oversize shapes return before a launch; the operator layer refuses host tensors,
mixed widths and what stays float32 only, with "float64" in the message; and the reference-made fixture tests/golden/so3_f64.npz equals
the oracle in float64 within the bars the GPU tests hold the kernels to (which pins the fixture to the oracle and shows that the
reference itself sits inside the bars)."""
import ctypes
import os
import re

import pytest
import torch

import so3_f64_cases as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ENTRIES = {'eap_so3_prep_f64': 16, 'eap_so3_inter_weights_f64': 10, 'eap_so3_inter_group_fwd_f64': 16, 'eap_inv_lists_entries': 9,
           'eap_so3_inter_group_bwd_f64': 19, 'eap_so3_intra_group_fwd_f64': 9, 'eap_so3_intra_group_bwd_f64': 9, 'eap_gemm_f64': 16,
           'eap_gemm_f64_reduce': 16}
HIP_INVALID_VALUE = 1


def test_entries_are_declared_exported_and_bound_with_the_headers_arity():
    from vgtk import _hip
    text = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so'))
    for name, arity in ENTRIES.items():
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert decl, f'{name} is not declared in include/eap_hip.h'
        params = decl.group(1).split(',')
        assert len(params) == arity and 'eap_stream_t stream' in params[-1], (name, len(params))
        assert hasattr(lib, name), f'{name} is not exported by libeap_hip.so'
        assert len(getattr(_hip.abi, name).argtypes) == arity, name
        with pytest.raises(RuntimeError, match=f'{name} takes {arity} arguments'):
            _hip._invoke(name, (0,) * (arity - 1))
    # the double scalar crosses as its bit pattern: no float parameter in the float64 entries
    for name in ENTRIES:
        assert ctypes.c_float not in getattr(_hip.abi, name).argtypes, name
    assert _hip._f64_bits(0.05) == 0x3FA999999999999A


def test_empty_shapes_return_without_a_launch_and_oversize_ones_are_refused():
    """No GPU here: an entry that reached a launch (or a memset) would return a HIP error instead of 0 / hipErrorInvalidValue."""
    from vgtk import _hip
    abi, bits = _hip.abi, _hip._f64_bits(0.05)
    P = 8                                                 # a non-null address nothing may dereference
    assert abi.eap_so3_prep_f64(0, 4, 4, 2, 60, None, None, None, None, None, None, 0, None, None, None, None) == 0
    assert abi.eap_so3_inter_weights_f64(0, 4, 2, 60, 24, bits, None, None, None, None) == 0
    assert abi.eap_so3_inter_group_fwd_f64(0, 3, 4, 4, 2, 60, 24, bits, None, None, None, None, None, None, None, None) == 0
    assert abi.eap_inv_lists_entries(0, 4, 4, 2, None, None, None, None, None) == 0
    assert abi.eap_so3_inter_group_bwd_f64(0, 3, 4, 4, 2, 60, 24, bits, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert abi.eap_so3_intra_group_fwd_f64(0, 3, 4, 60, 12, None, None, None, None) == 0
    assert abi.eap_so3_intra_group_bwd_f64(0, 3, 4, 60, 12, None, None, None, None) == 0
    assert abi.eap_gemm_f64(0, 0, 0, 5, 7, None, 7, 0, None, 5, 35, None, 5, 0, 2, None) == 0
    assert abi.eap_gemm_f64(0, 0, 3, 5, 7, None, 7, 0, None, 5, 35, None, 5, 15, 0, None) == 0
    assert abi.eap_gemm_f64_reduce(0, 1, 0, 5, 7, None, 7, 0, None, 7, 35, None, 5, 2, 0, None) == 0

    def refused(rc, words):
        assert rc == HIP_INVALID_VALUE, rc
        msg = abi.eap_last_error().decode()
        assert words in msg, msg

    refused(abi.eap_so3_prep_f64(70000, 4, 4, 2, 60, P, P, P, None, None, P, 0, P, P, None, None), '65535 clouds')
    refused(abi.eap_so3_prep_f64(1, 1 << 20, 4, 1 << 12, 60, P, P, P, None, None, P, 0, P, P, None, None), '2^31 entries')
    refused(abi.eap_so3_prep_f64(1, 4, 4, 2, 65, P, P, P, None, None, P, 0, P, P, None, None), '64 anchors')
    refused(abi.eap_so3_inter_weights_f64(70000, 4, 2, 60, 24, bits, P, P, P, None), '65535 clouds')
    refused(abi.eap_so3_inter_group_fwd_f64(1, 3, 4, 4, 2, 60, 33, bits, P, P, P, P, P, None, P, None), '32 kernel points')
    refused(abi.eap_so3_inter_group_fwd_f64(1, 3, 1 << 26, 4, 1, 60, 24, bits, P, P, P, P, P, None, P, None), 'outside the launch limits')
    refused(abi.eap_inv_lists_entries(1, 4, 16385, 2, P, P, P, P, None), '16384 support points')
    refused(abi.eap_so3_inter_group_bwd_f64(1, 3, 4, 16385, 2, 60, 24, bits, P, P, P, P, P, P, P, P, None, P, None), '16384 support points')
    refused(abi.eap_so3_inter_group_bwd_f64(70000, 3, 4, 4, 2, 60, 24, bits, P, P, P, P, P, P, P, P, None, P, None), '65535 clouds')
    refused(abi.eap_so3_intra_group_fwd_f64(1, 1, 4, 65, 12, P, P, P, None), '64 anchors')
    refused(abi.eap_gemm_f64(0, 0, 3, 5, 7, P, 7, 0, P, 5, 35, P, 5, 15, 70000, None), 'outside the launch limits')
    refused(abi.eap_gemm_f64(0, 0, 3, 5, 7, None, 7, 0, P, 5, 35, P, 5, 15, 2, None), 'null operand')
    refused(abi.eap_gemm_f64_reduce(0, 1, 1 << 23, 5, 7, P, 7, 0, P, 7, 35, P, 5, 2, 0, None), 'outside the launch limits')


def test_operator_layer_refuses_host_tensors_and_mixed_widths():
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    import vgtk.spconv as zptk
    from vgtk import _hip
    d = torch.float64
    xyz, feats = torch.zeros(1, 3, 8, dtype=d), torch.ones(1, 2, 8, 60, dtype=d)
    conv = sptk.InterSO3PoseConv(2, 4, 1, 1, 0.1, 0.01, 4).double()
    assert conv.anchors.dtype == d and conv.kernels.dtype == d and conv.basic_conv.W.dtype == d       # the tables follow .double()
    with pytest.raises(RuntimeError, match='CUDA'):
        conv(zptk.SphericalPointCloudPose(xyz, feats, None, None))
    with pytest.raises(RuntimeError, match='device'):
        L.intra_so3conv(torch.ones(1, 2, 3, 60, dtype=d), torch.ones(3, 24, dtype=d), L.get_intra_idx())
    with pytest.raises(RuntimeError, match='device'):
        L.intra_so3conv_grouping(torch.from_numpy(L.get_intra_idx()), torch.ones(1, 2, 3, 60, dtype=d))
    with pytest.raises(RuntimeError, match='CUDA'):
        L.so3_contract(torch.ones(3, 24, dtype=d), torch.ones(1, 24, 60, dtype=d))
    with pytest.raises(RuntimeError, match='CUDA'):
        L.inter_so3conv_grouping_anchor(torch.zeros(1, 3, 4, 2, dtype=d), conv.anchors, conv.kernels, 0.01)
    # mixed widths name the offender
    with pytest.raises(RuntimeError, match=r'xyz is torch\.float32 but feats is torch\.float64'):
        conv(zptk.SphericalPointCloudPose(xyz.float(), feats, None, None))
    with pytest.raises(RuntimeError, match=r'W is torch\.float64 but feats is torch\.float32'):
        conv(zptk.SphericalPointCloudPose(xyz.float(), feats.float(), None, None))
    with pytest.raises(RuntimeError, match=r'W is torch\.float32 but x is torch\.float64'):
        L.so3_contract(torch.ones(3, 24), torch.ones(1, 24, 60, dtype=d))
    with pytest.raises(RuntimeError, match=r'W is torch\.float32 but feats is torch\.float64'):
        L.intra_so3conv(torch.ones(1, 2, 3, 60, dtype=d), torch.ones(3, 24), L.get_intra_idx())
    with pytest.raises(RuntimeError, match=r'pose is torch\.float32 in a float64 call'):
        _hip._all_f64('so3_prep_f64', xyz=xyz, pose=torch.eye(4).repeat(1, 8, 1, 1))
    with pytest.raises(RuntimeError, match=r'anchors is torch\.float32 but xyz is torch\.float64'):
        L._neighbourhood_f64(xyz, None, 4, conv.anchors.float(), conv.kernels, 0.1, 0.01, False, None, None)
    # the GEMM views: all float32 or all float64
    A, Bm, C = torch.zeros(3, 4, dtype=d), torch.zeros(2, 4, 5, dtype=d), torch.zeros(2, 3, 5, dtype=d)
    assert _hip._product(A, Bm, C)[2:5] == (3, 5, 4)
    for a, b_, c in ((A.float(), Bm, C), (A, Bm.float(), C), (A, Bm, C.float())):
        with pytest.raises(RuntimeError, match='float32 view'):
            _hip._product(a, b_, c)
    big = torch.zeros(2, 4, 8, dtype=d)
    short = big[:, :, 3:]                                   # a slice whose storage then loses its last element (8 bytes)
    big.untyped_storage().resize_(big.untyped_storage().nbytes() - 8)
    with pytest.raises(RuntimeError, match='addresses 61 elements, its storage holds 63'):
        _hip._product(A, short, C)


def test_what_stays_float32_only_says_float64():
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    import vgtk.spconv as zptk
    from vgtk.so3conv.blocks import BatchNormLeakyReLU, InstanceNormLeakyReLU
    d = torch.float64
    xyz, feats = torch.zeros(1, 3, 8, dtype=d), torch.ones(1, 2, 8, 60, dtype=d)
    with pytest.raises(RuntimeError, match='use_2d.*float64'):
        sptk.InterSO3PoseConv(2, 4, 1, 1, 0.1, 0.01, 4, use_2d=True).double()(
            zptk.SphericalPointCloudPose(xyz, torch.ones(1, 2, 8, 240, dtype=d), None, None))
    with pytest.raises(RuntimeError, match='use_art_mode.*float64'):
        sptk.InterSO3PoseConv(2, 4, 1, 1, 0.1, 0.01, 4, use_art_mode=True).double()(
            zptk.SphericalPointCloudPose(torch.zeros(1, 2, 3, 8, dtype=d), feats, None, None), seg=torch.zeros(1, 8, dtype=torch.long))
    with pytest.raises(RuntimeError, match='IntraSO3Conv2D.*float64'):
        sptk.IntraSO3Conv2D(2, 4).double()(zptk.SphericalPointCloud(xyz, torch.ones(1, 2, 8, 240, dtype=d), None))
    with pytest.raises(RuntimeError, match='intra_so3conv2d.*float64'):
        L.intra_so3conv2d(torch.ones(1, 2, 8, 240, dtype=d), torch.ones(4, 24, dtype=d), torch.from_numpy(L.get_intra_idx()))
    W = torch.ones(4, 48, dtype=d)
    ep = L.FoldedEpilogue(torch.ones(4), torch.zeros(4), 0.1)
    with pytest.raises(RuntimeError, match='epilogue.*float64'):
        L.so3_contract(W, torch.ones(1, 48, 60, dtype=d), ep)
    # (these two are refused after the device check: what they say is read off the source)
    src = open(os.path.join(ROOT, 'equi-articulated-pose_amd', 'vgtk', 'so3conv', 'blocks.py')).read()
    assert src.count("float32 only -- the float64 regime covers the conv layers, not the norms") == 2
    assert isinstance(BatchNormLeakyReLU(4), torch.nn.Module) and isinstance(InstanceNormLeakyReLU(4), torch.nn.Module)
    src = open(os.path.join(ROOT, 'equi-articulated-pose_amd', 'vgtk', 'so3conv', 'functional.py')).read()
    assert 'epilogues (FoldedEpilogue, TrainEpilogue) are float32 only, a float64 conv takes none' in src
    assert 'has no float64 kernel' in src


@pytest.fixture(scope='module')
def fixture():
    return S.load_fixture()


@pytest.mark.parametrize('key', S.FIXTURE_CASES)
def test_fixture_equals_the_oracle_in_float64(fixture, key):
    c = S.fixture_case(fixture, key)
    assert not torch.equal(c['xyz'].float().double(), c['xyz']) and not torch.equal(c['feats'].float().double(), c['feats'])
    if key == 'intra':
        idx = fixture['intra_idx']
        run = lambda cast: S.intra_reference(cast(c['feats']), cast(c['W']), cast(c['gy']), idx)
    else:
        run = lambda cast: S.inter_reference(cast(c['xyz']), None if c['pose'] is None else cast(c['pose']), cast(c['feats']), cast(c['W']),
                                             cast(c['gy']), cast(c['anchors']), cast(c['kernels']), S.RADIUS, S.SIGMA, S.NNB, c['permute_modes'])
    ref = run(lambda t: t)
    S.controls(ref, run, key, neighbours=key != 'intra')
    cut = S.at_points(ref, c['points'])
    for k in ('out', 'gfeats', 'gW'):
        assert c['want'][k].dtype == torch.float64
        S.check(c['want'][k], cut[k], f'{key} fixture {k}')
    if key != 'intra':
        assert torch.equal(ref['ball_idx'], fixture['ball_idx'])
        d = float((c['inter_w'] - ref['inter_w'][:, :4]).abs().max())
        print(f'{key} fixture inter_w: {d:.3e} (bar {S.BAR_W:.0e})')
        assert d <= S.BAR_W
