"""GPU: `_hip.call` over the typed prototypes of vgtk/_hip.py (tests/test_abi_binding_host.py holds everything that needs no device).
A launch whose arguments are bare tensors and Python numbers and the same launch with the arguments a caller wrapped by hand
(`_ptr`, `_I64`: tests and tools still do) hand the entry the same values: the outputs are compared BIT FOR BIT."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_bare_and_wrapped_arguments_launch_the_same_kernel_on_the_same_values():
    from vgtk import _hip
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    dev = torch.device('cuda:0')
    b, c, n = 2, 4, 64
    x = torch.randn(b, c, n, device=dev, generator=torch.Generator(device=dev).manual_seed(2913))
    ps, pq = _hip._partials(x, b, c, n)
    ps_w, pq_w = _hip._partials(x, b, c, n)
    for t in (ps, pq, ps_w, pq_w):
        t.fill_(float('nan'))
    _hip.call('eap_bn_stats_f32', x, b, c, n, x, ps, pq)
    _hip.call('eap_bn_stats_f32', x, b, c, _hip._I64(n), _hip._ptr(x), _hip._ptr(ps_w), _hip._ptr(pq_w))
    assert torch.equal(ps.view(torch.int32), ps_w.view(torch.int32)) and torch.equal(pq.view(torch.int32), pq_w.view(torch.int32))
    # ... and they are the moments: sums of x - pivot and of its square per channel (pivot = x[0, c, 0]), against float64.  Each of the
    # 128 differences, each square and each of the 127 additions of a channel rounds once, by at most 2^-24 of what it holds: in any
    # summation order the result is within (127 + 2) 2^-24 < 2^-16 of the sum of the magnitudes
    d = x.double() - x[0, :, 0].double()[None, :, None]
    want, want_sq = d.sum((0, 2)), d.square().sum((0, 2))
    assert float(((ps.sum(1, dtype=torch.float64) - want).abs() / d.abs().sum((0, 2))).max()) <= 2.0 ** -16
    assert float(((pq.sum(1, dtype=torch.float64) - want_sq).abs() / want_sq).max()) <= 2.0 ** -16
    # what the prototype refuses is a RuntimeError that names the entry, raised before anything is launched
    before = ps.clone()
    for args, position in (((b, c, n, x.cpu(), ps, pq), 4), ((b, c, n, x.double(), ps, pq), 4), ((b, c, _hip._F32(n), x, ps, pq), 3)):
        with pytest.raises(RuntimeError, match=f'eap_bn_stats_f32: argument {position}'):
            _hip.call('eap_bn_stats_f32', x, *args)
    for args in ((b, c, n, x, ps), (b, c, n, x, ps, pq, None)):
        with pytest.raises(RuntimeError, match='eap_bn_stats_f32 takes 7 arguments'):
            _hip.call('eap_bn_stats_f32', x, *args)
    torch.cuda.synchronize()
    assert torch.equal(ps.view(torch.int32), before.view(torch.int32))
