"""CPU: the front-end entries as far as they go without a device -- eap_so3_dense_probe (csrc/list_probe.hip) is declared, exported and
bound, and refuses what it cannot take before anything is launched -- and the numpy restatements the GPU tests compare against
(tests/front_end_common.py) on answers written out by hand."""
import ctypes
import os

import numpy as np
import pytest

import front_end_common as FE

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INVALID_VALUE = 1           # hipErrorInvalidValue
P = 16                      # a stand-in address: the refusals below come before any pointer is read


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def test_the_probe_is_declared_exported_and_bound(hip):
    header = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    lib = ctypes.CDLL(os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so'))
    for name, arity in (('eap_so3_dense_probe', 19), ('eap_so3_dense_probe_workspace', 1)):
        assert name + '(' in header and hasattr(lib, name)
        assert len(getattr(hip.abi, name).argtypes) == arity, name
    assert [hip.abi.eap_so3_dense_probe_workspace(b) for b in (-1, 0, 1, 8)] == [0, 0, 3, 10]
    assert hip.NATIVE_LIST_PROBE is True


def _probe(hip, b=2, p=64, words=16, n_rows=P, nonident=None, dflags=P, memb=P, rot_a=None, blocks_a=0, rot_b=None, blocks_b=0,
           rot_cloud=None, norm_w=None, norm_b=None, channels=0, ratio=128.0, work=P, out=P):
    return hip.abi.eap_so3_dense_probe(b, p, words, n_rows, nonident, dflags, memb, rot_a, blocks_a, rot_b, blocks_b, rot_cloud, norm_w,
                                       norm_b, channels, ratio, work, out, None)


@pytest.mark.parametrize('kw,word', [
    (dict(b=0), 'positive'), (dict(p=0), 'positive'), (dict(b=-3), 'positive'),
    (dict(n_rows=None), 'required'), (dict(work=None), 'required'), (dict(out=None), 'required'),
    (dict(dflags=None), 'come together'), (dict(memb=None), 'come together'),
    (dict(words=17), '16 or 32'), (dict(words=0), '16 or 32'),
    (dict(norm_w=P, channels=4), 'weight and bias'), (dict(norm_b=P, channels=4), 'weight and bias'), (dict(norm_w=P, norm_b=P), 'weight and bias'),
    (dict(rot_a=P), 'at least one block'), (dict(rot_b=P, blocks_b=-1), 'at least one block'),
    (dict(memb=P + 4), '16-byte aligned'), (dict(rot_a=P + 8, blocks_a=3), '16-byte aligned')])
def test_the_probe_refuses_before_any_device_call(hip, kw, word):
    """stand-in addresses and a null stream, on a machine without a device: nothing but the argument check can have run"""
    assert _probe(hip, **kw) == INVALID_VALUE
    msg = hip.abi.eap_last_error().decode()
    assert 'so3_dense_probe' in msg and word in msg, msg


def test_the_probe_takes_only_operands_it_reads_as_they_are(hip):
    import torch
    host = torch.eye(4).repeat(2, 3, 1, 1)
    assert not hip.so3_dense_probe_takes((host,), None, None, None)                  # (not on the device)
    assert not hip.so3_dense_probe_takes((), None, torch.zeros(4), torch.zeros(4))


def test_the_split_k_entries_are_declared_exported_and_bound(hip):
    header = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    lib = ctypes.CDLL(os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so'))
    for name, arity in (('eap_gemm_f16x2_splitk_f32', 20), ('eap_gemm_f16x2_splitk_slabs', 5), ('eap_gemm_f16x2_splitk_workspace', 4)):
        assert name + '(' in header and hasattr(lib, name)
        assert len(getattr(hip.abi, name).argtypes) == arity, name
    assert hip.SPLIT_K_ONE_ROW_TILE is True


def test_the_launcher_fills_four_rounds_with_whole_k_tiles(hip):
    slabs, floats = hip.abi.eap_gemm_f16x2_splitk_slabs, hip.abi.eap_gemm_f16x2_splitk_workspace
    # the two dense layers of the benchmark on 256 CUs: 34 x 8 and 68 x 8 workgroups per slab
    assert slabs(128, 8704, 512 * 24, 8, 256) == 4                      # 2 rounds x 768 k-tiles -> 5 x 192
    assert slabs(128, 17408, 128 * 24, 8, 256) == 1                     # 3 rounds x 192 -> 5 x 96 with two slabs: not a quarter less
    assert slabs(128, 8704, 512 * 24, 8, 64) == 1                       # (272 workgroups are four rounds of 64 CUs and more)
    assert slabs(128, 256, 16 * 64, 1, 256) == 4                        # 64 k-tiles: 1, 2, 4 leave slabs of >= 16
    assert slabs(128, 256, 16 * 65 * 4, 1, 256) == 13                   # 260 k-tiles: 1, 2, 4, 5, 10, 13
    assert slabs(128, 256, 16 * 65 * 4, 1, 2) == 10                     # 8 workgroups wanted: the next divisor is 10
    assert slabs(128, 256, 16 * 65 * 4, 3, 4) == 1                      # 6 wanted -> 10 slabs: 8 rounds x 26 k-tiles against 1 x 260
    assert slabs(128, 256, 16 * 61, 1, 256) == 1                        # below 64 k-tiles
    assert slabs(256, 8704, 512 * 24, 8, 256) == 1 and slabs(64, 8704, 512 * 24, 8, 256) == 1          # not one 128-row tile
    assert slabs(128, 8704, 16 * 64 + 8, 8, 256) == 1                   # no whole k-tiles
    assert [floats(128, 256, 3, s) for s in (0, 1, 2, 13)] == [0, 0, 2 * 3 * 128 * 256, 13 * 3 * 128 * 256]


A16 = 4096                  # a 16-byte aligned stand-in address


def _split_k(hip, M=128, N=256, K=1024, A=A16, B=A16, C=A16, ldc=256, strideC=128 * 256, batch=2, abs_a=A16, abs_b=A16, grp_b=4, mult_b=1.0,
             slabs=2, work=A16, floats=2 * 2 * 128 * 256):
    return hip.abi.eap_gemm_f16x2_splitk_f32(M, N, K, A, K, B, N, K * N, C, ldc, strideC, batch, abs_a, abs_b, grp_b, mult_b, slabs, work, floats, None)


@pytest.mark.parametrize('kw,word', [
    (dict(M=0), 'positive'), (dict(N=0), 'positive'), (dict(batch=-1), 'positive'),
    (dict(A=None), 'required'), (dict(B=None), 'required'), (dict(C=None), 'required'),
    (dict(abs_a=None), 'magnitudes'), (dict(abs_b=None), 'magnitudes'), (dict(grp_b=0), 'magnitudes'), (dict(mult_b=0.0), 'magnitudes'),
    (dict(M=256), 'one 128-row tile'), (dict(K=1000), 'one 128-row tile'), (dict(A=A16 + 4), 'one 128-row tile'),
    (dict(slabs=3), 'must divide'), (dict(slabs=8), 'must divide'), (dict(slabs=-2), 'must divide'), (dict(slabs=128), 'must divide'),
    (dict(strideC=128 * 256 + 4), 'strideC = M ldc'), (dict(ldc=258, strideC=128 * 258), 'strideC = M ldc'), (dict(C=A16 + 4), 'strideC = M ldc'),
    (dict(work=A16 + 8), 'strideC = M ldc'),
    (dict(work=None), 'too small'), (dict(floats=2 * 2 * 128 * 256 - 1), 'too small'), (dict(slabs=4), 'too small')])
def test_the_split_k_entry_refuses_before_any_device_call(hip, kw, word):
    """stand-in addresses and a null stream, on a machine without a device: nothing but the argument check can have run"""
    assert _split_k(hip, **kw) == INVALID_VALUE
    msg = hip.abi.eap_last_error().decode()
    assert 'gemm_f16x2_splitk_f32' in msg and word in msg, msg


def test_matmul_leaves_other_products_to_gemm(hip, monkeypatch):
    """outside the shape class (M = 128, K >= 1024, row-major operands) nothing is asked of the library: host tensors get as far as gemm"""
    import torch
    seen = []
    monkeypatch.setattr(hip, 'gemm', lambda *a, **k: seen.append(a[:5]))
    hip.matmul(torch.zeros(64, 2048), torch.zeros(2, 2048, 256), torch.zeros(2, 64, 256))
    hip.matmul(torch.zeros(128, 512), torch.zeros(2, 512, 256), torch.zeros(2, 128, 256))
    hip.matmul(torch.zeros(128, 2048), torch.zeros(2, 256, 2048).transpose(1, 2), torch.zeros(2, 128, 256))
    hip.matmul(torch.zeros(128, 2048), torch.zeros(2, 2048, 256), torch.zeros(2, 128, 256))           # (in the class, but not on the device)
    assert seen == [(0, 0, 64, 256, 2048), (0, 0, 128, 256, 512), (0, 1, 128, 256, 2048), (0, 0, 128, 256, 2048)]


def test_row_list_restatement_by_hand():
    # rows 5 (3 times), 2 and 7 (twice: the lower index first), 0 (once); 9 = outside the support
    idx = np.array([[[5, 2, 7, 9], [5, 7, 2, 0], [5, 9, 9, 9]]])
    rows, off, cnt, n_rows = FE.row_list(idx, 8)
    assert rows.tolist() == [[5, 2, 7, 0, -1, -1, -1, -1]] and cnt.tolist() == [[3, 2, 2, 1, 0, 0, 0, 0]]
    assert off.tolist() == [[0, 3, 5, 7, 8, 8, 8, 8]] and n_rows.tolist() == [4]
    rows, off, cnt, n_rows = FE.row_list(np.full((2, 3, 4), 8), 8)
    assert (rows == -1).all() and (off == 0).all() and (cnt == 0).all() and n_rows.tolist() == [0, 0]
    assert all(a.dtype == np.int32 for a in (rows, off, cnt, n_rows))


def test_probe_restatement_by_hand():
    n_rows = np.array([3, 9], np.int32)
    assert FE.probe_words(64, n_rows).tolist() == [9, 1, 1, 0, 0]
    memb = np.zeros((2, 6, 16), np.int32)
    memb[0, 0, 0] = 0x00010001          # two halves
    memb[0, 1, 3] = -65536              # the upper half
    memb[1, 5, 15] = 0x7fff             # the lower half
    eye = np.tile(np.eye(4, dtype=np.float32), (2, 6, 1, 1))
    turned = eye.copy()
    turned[1, 2, 0, 1] = 1e-7
    shifted = eye.copy()
    shifted[0, 0, 0, 3] = 5.0           # (a translation: not part of the 3 x 3)
    w = FE.probe_words(6, n_rows, np.array([0, 2]), np.array([0, 2]), memb, [eye, turned, shifted])
    assert w.tolist() == [9, 2, 3, int(np.float32(3) * np.float32(16.0 / 6)), 0] and w[3] == 8
    r = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    r[0, 2, 0] = 2e-6
    assert FE.probe_words(6, n_rows, dflags=np.array([0, 0]), memb=memb, rot_cloud=r)[2] == 1
    r[0, 2, 0] = 5e-7
    assert FE.probe_words(6, n_rows, dflags=np.array([0, 0]), memb=memb, rot_cloud=r)[2] == 0
    r[1, 1, 1] = np.nan
    assert FE.probe_words(6, n_rows, dflags=np.array([0, 0]), memb=memb, rot_cloud=r)[2] == 0
    gamma, beta = np.array([1.0, 0.0, -0.5], np.float32), np.array([128.0, 3.0, 64.0], np.float32)
    assert FE.probe_words(6, n_rows, norm_w=gamma, norm_b=beta)[4] == 0          # (128 |gamma| reached, not passed; gamma == 0 skipped)
    beta[2] = -64.01
    assert FE.probe_words(6, n_rows, norm_w=gamma, norm_b=beta)[4] == 1
