"""CPU: the entries of the `use_2d` 'residual map' regime (csrc/so3_inter_res.hip) as far as they go without a device -- their typed
prototypes, the argument checks every entry makes on the host BEFORE it touches the device (sizes, 16-byte alignment, required pointers,
the launch limits), host tensors refused by the binding, and the byte that carries an entry's four residual indices."""
import ctypes

import pytest
import torch

INVALID_VALUE = 1           # hipErrorInvalidValue
A16 = 1 << 40               # a 16-byte aligned address nothing ever dereferences: every call below returns before it launches


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _kinds(fn):
    """the prototype in letters: i(nt), l (int64), f(loat), s(tream), or the pointee width of a pointer"""
    names = {ctypes.c_int: 'i', ctypes.c_int64: 'l', ctypes.c_float: 'f', ctypes.c_void_p: 's'}
    return ''.join(names[t] if t in names else str(t.width) for t in fn.argtypes)


def test_the_new_prototypes_bind_with_their_arity_and_types(hip):
    abi = hip.abi
    assert _kinds(abi.eap_so3_residual_index_f32) == 'iiii' + '4444' + '14' + 's' and abi.eap_so3_residual_index_f32.restype is ctypes.c_int
    assert _kinds(abi.eap_so3_inter_group_fwd_res_f32) == 'iiiiiii' + 'f' + '4444' + '1' + '4' + 's'
    assert _kinds(abi.eap_so3_inter_group_bwd_res_f32) == 'iiiiiii' + 'f' + '4444' + '1' + '44' + 's'
    assert _kinds(abi.eap_so3_inter_group_bwd_res_workspace) == 'iiiii' and abi.eap_so3_inter_group_bwd_res_workspace.restype is ctypes.c_int64
    assert abi.eap_abi_version() == 1


def _err(hip):
    return hip.abi.eap_last_error().decode()


def test_nothing_to_do_is_no_error(hip):
    abi = hip.abi
    assert abi.eap_so3_residual_index_f32(0, 8, 8, 4, A16, A16, A16, A16, A16, A16, None) == 0
    assert abi.eap_so3_inter_group_fwd_res_f32(0, 4, 8, 8, 4, 60, 24, 0.02, None, None, None, None, None, None, None) == 0
    assert abi.eap_so3_inter_group_bwd_res_f32(0, 4, 8, 8, 4, 60, 24, 0.02, None, None, None, None, None, None, None, None) == 0
    assert abi.eap_so3_inter_group_bwd_res_workspace(0, 4, 8, 8, 60) == 0


def test_the_index_entry_checks_its_arguments_on_the_host(hip):
    f = hip.abi.eap_so3_residual_index_f32
    assert f(1, 8, 8, 4, A16, None, A16, A16, A16, A16, None) == INVALID_VALUE and 'pose' in _err(hip)
    assert f(1, 8, 8, 4, A16, A16, A16, None, A16, A16, None) == INVALID_VALUE and 'residual rotations' in _err(hip)
    assert f(1, 8, 8, 4, A16, A16, A16, A16, A16, None, None) == INVALID_VALUE and 'flags' in _err(hip)
    assert f(1, 8, 0, 4, A16, A16, A16, A16, A16, A16, None) == INVALID_VALUE and 'support' in _err(hip)
    assert f(1, 8, 8, 4, None, A16, A16, A16, A16, A16, None) == INVALID_VALUE
    assert f(1, -8, 8, 4, A16, A16, A16, A16, A16, A16, None) == INVALID_VALUE and 'negative' in _err(hip)
    assert f(65536, 8, 8, 4, A16, A16, A16, A16, A16, A16, None) == INVALID_VALUE           # grid.y
    assert '65536' in _err(hip) and '65535' in _err(hip) and 'so3_residual_index' in _err(hip)


@pytest.mark.parametrize('name', ['fwd', 'bwd'])
def test_the_grouping_entries_check_their_arguments_on_the_host(hip, name):
    fn = getattr(hip.abi, f'eap_so3_inter_group_{name}_res_f32')
    tail = (None,) if name == 'fwd' else (A16, None)           # (workspace,) stream

    def call(b=1, c=4, p=8, n=8, nn=4, na=60, ks=24, t1=A16, idx=A16, gx=A16, rk=A16, shift=A16, t2=A16):
        return fn(b, c, p, n, nn, na, ks, 0.02, t1, idx, gx, rk, shift, t2, *tail)

    for bad in (dict(na=65), dict(na=0), dict(ks=33), dict(nn=-1)):
        assert call(**bad) == INVALID_VALUE and '64 anchors' in _err(hip) and '32 kernel points' in _err(hip), bad
    for bad in (dict(t1=A16 + 4), dict(t2=A16 + 8)):
        assert call(**bad) == INVALID_VALUE and '16-byte aligned' in _err(hip), bad
    for bad in (dict(t1=None), dict(idx=None), dict(gx=None), dict(rk=None), dict(shift=None), dict(t2=None)):
        assert call(**bad) == INVALID_VALUE and 'required' in _err(hip), bad
    assert call(nn=4096) == INVALID_VALUE and 'shared memory' in _err(hip)
    assert call(b=65536) == INVALID_VALUE and '65535' in _err(hip) and f'so3_inter_group_{name}_res' in _err(hip)        # grid.y / grid.z
    if name == 'bwd':
        assert fn(1, 4, 8, 8, 4, 60, 24, 0.02, A16, A16, A16, A16, A16, A16, None, None) == INVALID_VALUE and 'workspace' in _err(hip)
        assert call(c=2 ** 22, n=2 ** 10, p=16) == INVALID_VALUE and 'outside the launch limits' in _err(hip)   # c / 4 chunks along grid.y
    else:
        assert call(p=2 ** 24) == INVALID_VALUE and 'outside the launch limits' in _err(hip)                    # 2^24 blocks of 256 threads


def test_the_workspace_of_the_backward(hip):
    ws = hip.abi.eap_so3_inter_group_bwd_res_workspace
    # [cloud][chunk of 4 channels][point range][support row][4 channels][4 planes][60 anchors]; one range per 16 points at most
    assert ws(1, 5, 40, 40, 60) == 1 * 2 * 3 * 40 * 4 * 4 * 60
    assert ws(2, 64, 512, 512, 60) == 2 * 16 * 8 * 512 * 4 * 4 * 60
    assert ws(1, 5, 40, 40, 65) == 0 and ws(1, 5, 40, 40, 0) == 0
    assert ws(64, 2 ** 20, 2 ** 14, 2 ** 14, 60) > 2 ** 32                 # an int64 arrives whole


def test_host_tensors_are_refused_by_the_binding(hip):
    host_f, host_i, host_b = torch.zeros(16), torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='eap_so3_residual_index_f32: argument 5.*CUDA'):
        hip._invoke('eap_so3_residual_index_f32', (0, 1, 1, 1, host_i, None, None, None, None, None, None))
    with pytest.raises(RuntimeError, match='eap_so3_residual_index_f32: argument 9.*CUDA'):
        hip._invoke('eap_so3_residual_index_f32', (0, 1, 1, 1, None, None, None, None, host_b, None, None))
    with pytest.raises(RuntimeError, match='eap_so3_inter_group_fwd_res_f32: argument 9.*CUDA'):
        hip._invoke('eap_so3_inter_group_fwd_res_f32', (0, 1, 1, 1, 1, 60, 24, 0.02, host_f, None, None, None, None, None, None))
    with pytest.raises(RuntimeError, match='eap_so3_inter_group_fwd_res_f32: argument 13.*4 bytes.*1-byte'):      # the index is bytes
        hip._invoke('eap_so3_inter_group_fwd_res_f32', (0, 1, 1, 1, 1, 60, 24, 0.02, None, None, None, None, host_i, None, None))
    with pytest.raises(RuntimeError, match='eap_so3_inter_group_bwd_res_f32: argument 14.*CUDA'):
        hip._invoke('eap_so3_inter_group_bwd_res_f32', (0, 1, 1, 1, 1, 60, 24, 0.02, None, None, None, None, None, host_f, None, None))
    with pytest.raises(RuntimeError, match='takes 16 arguments'):
        hip._invoke('eap_so3_inter_group_bwd_res_f32', (0,) * 15)
    # the wrappers check before they allocate
    with pytest.raises(RuntimeError, match='CUDA'):
        hip.so3_residual_index(host_i.view(1, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(4, 3, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        hip.so3_inter_group_fwd_res(torch.zeros(1, 2, 4, 240), host_i.view(1, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(240, 24, 3),
                                    host_b.view(1, 4, 4), 0.02)
    with pytest.raises(RuntimeError, match='CUDA'):
        hip.so3_inter_group_bwd_res(torch.zeros(1, 2, 24, 4, 240), host_i.view(1, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(240, 24, 3),
                                    host_b.view(1, 4, 4), 0.02, 4)


def test_the_index_byte_round_trips_all_256_values(hip):
    every = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    fields = hip.residual_index_unpack(every)
    assert fields.shape == (256, 4) and fields.dtype == torch.int64 and int(fields.min()) == 0 and int(fields.max()) == 3
    for v in (0, 1, 0x1B, 0xE4, 0xFF):
        assert fields[v].tolist() == [(v >> (2 * z)) & 3 for z in range(4)]
    assert len({tuple(r) for r in fields.tolist()}) == 256
    assert torch.equal(hip.residual_index_pack(fields), every)
    assert torch.equal(hip.residual_index_pack(fields.to(torch.int32).view(4, 64, 4)), every.view(4, 64))
    assert fields[hip.RESIDUAL_IDENTITY_BYTE].tolist() == [0, 1, 2, 3]
    for bad in (torch.tensor([[0, 1, 2, 4]]), torch.tensor([[0, -1, 2, 3]]), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4)):
        with pytest.raises(RuntimeError, match='0..3'):
            hip.residual_index_pack(bad)
    with pytest.raises(RuntimeError, match='uint8'):
        hip.residual_index_unpack(torch.zeros(4, dtype=torch.int32))
