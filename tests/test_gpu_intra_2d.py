"""GPU: IntraSO3Conv2D on the (60, 4) anchor axis (so3conv/modules.py:L350-373; intra_so3conv_grouping_2D, so3conv/functional.py:L2606-2627,
+ BasicSO3Conv, modules.py:L48-55) as an implicit GEMM that gathers an anchor's four residuals as one 16-byte quad: the fp32-MFMA kernel
(csrc/gemm_f32.hip, GATHER == 2), the split kernels (csrc/gemm_bf16x3.hip, BMODE 2 with nr = 4) and the 2-D grouping pair
(csrc/so3_intra.hip).  Everything goes through the module; the comparator is the index_select form restated in float64 on the CPU, the
bars are the layer's own (tests/test_gpu_parity.py::test_intra_conv_implicit_gemm): 1e-5 for the output and dF, 2e-5 for dW, relative to
the largest magnitude; the split kernels also keep the bar of tests/test_gpu_split_planes.py against the fp32 kernel."""
import numpy as np
import pytest
import torch

from test_gpu_split_planes import launched, mode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def grouped_ref(f, idx):
    """intra_so3conv_grouping_2D in the reference's words: [b,c,p,240] -> [b,c,12,p,240]"""
    b, c, p, _ = f.shape
    fi = f.view(b, c, p, 60, 4).index_select(3, idx.view(-1)).view(b, c, p, 60, idx.shape[1], 4)
    return fi.permute(0, 1, 4, 2, 3, 5).reshape(b, c, idx.shape[1], p, 240)


def reference64(feats, W, gy, idx):
    """(out, dF, dW) of the layer in float64 on the CPU"""
    f = feats.detach().double().cpu().requires_grad_(True)
    w = W.detach().double().cpu().requires_grad_(True)
    b, c, p, _ = f.shape
    out = torch.matmul(w, grouped_ref(f, idx.cpu()).reshape(b, c * idx.shape[1], p * 240)).view(b, -1, p, 240)
    gf, gw = torch.autograd.grad(out, [f, w], gy.detach().double().cpu())
    return out.detach(), gf, gw


def layer(dev, c, o, seed=11):
    import vgtk.so3conv as sptk
    torch.manual_seed(seed)
    return sptk.IntraSO3Conv2D(c, o).to(dev)


def run(conv, feats, gy=None, want=('f', 'w')):
    """the module's output (and its gradients to the features / the weights) on `feats`"""
    import vgtk.spconv as zptk
    f = feats.detach().requires_grad_(True)
    y = conv(zptk.SphericalPointCloud(None, f, None)).feats
    if gy is None:
        return y
    targets = [t for k, t in (('f', f), ('w', conv.basic_conv.W)) if k in want]
    return (y,) + tuple(torch.autograd.grad(y, targets, gy))


def check_layer(conv, feats, gy):
    y, gf, gw = run(conv, feats, gy)
    out64, gf64, gw64 = reference64(feats, conv.basic_conv.W, gy, conv.intra_idx)
    errs = rel_err(y, out64), rel_err(gf, gf64), rel_err(gw, gw64)
    print(f'\nIntraSO3Conv2D {tuple(feats.shape)} -> {y.shape[1]}: out {errs[0]:.2e}, dF {errs[1]:.2e}, dW {errs[2]:.2e}')
    assert errs[0] < 1e-5 and errs[1] < 1e-5 and errs[2] < 2e-5, errs
    return y


# (2,5,7,11): a k tail (K = 60), M below one tile, a ragged last column tile (2640 = 20 * 128 + 80), tiles that cut points (128 does not
# divide 240); (1,130,8,30): K = 1560 over many k-tiles, more channels than one dW slice
@pytest.mark.parametrize('shape', [(2, 5, 7, 11), (1, 130, 8, 30)])
def test_fp32_kernel_against_float64(dev, shape):
    from vgtk import _hip
    b, c, o, p = shape
    conv = layer(dev, c, o)
    gen = torch.Generator().manual_seed(sum(shape))
    feats, gy = torch.randn(b, c, p, 240, generator=gen).to(dev), torch.randn(b, o, p, 240, generator=gen).to(dev)
    y, names = launched(lambda: check_layer(conv, feats, gy))
    assert 'eap_so3_intra_conv2d_f32' in names and 'eap_so3_intra_group2d_fwd_f32' in names, names
    assert not any(n.startswith('eap_so3_intra_conv2d_') and n != 'eap_so3_intra_conv2d_f32' for n in names), names
    with torch.no_grad():
        assert torch.equal(run(conv, feats), y)
    # the entry names its kernel for a caller without a profiler (eap_last_kernel)
    _hip.KERNEL_TIMES = rec = []
    try:
        _hip.so3_intra_conv2d(feats, conv.basic_conv.W.detach(), conv.intra_idx.int())
    finally:
        _hip.KERNEL_TIMES = None
    assert [(n, tag['kernel']) for n, tag, *_ in rec] == [('eap_so3_intra_conv2d_f32', 'gemm_f32_kernel<GATHER quad>')], rec


def test_fp32_kernel_scalar_loads_from_a_view_off_the_16_byte_grid(dev):
    """the same features as a contiguous view that starts 4 bytes past a 16-byte boundary: four dword loads per quad, the same numbers"""
    b, c, o, p = 2, 5, 7, 11
    conv = layer(dev, c, o)
    gen = torch.Generator().manual_seed(b + c + o + p)
    feats, gy = torch.randn(b, c, p, 240, generator=gen).to(dev), torch.randn(b, o, p, 240, generator=gen).to(dev)
    buf = torch.empty(feats.numel() + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + feats.numel()].view(feats.shape).copy_(feats)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    y_off = check_layer(conv, off, gy)
    assert torch.equal(y_off, run(conv, feats))              # the quad load and the four scalar loads read the same addresses


def test_against_the_reference_fixture(dev, golden):
    """the (60, 4) axis order against the reference's own IntraSO3Conv2D (tests/golden/make_golden_intra2d.py)"""
    import vgtk.so3conv.functional as L
    g = golden('intra_2d.npz')
    assert np.array_equal(g['intra_idx'], L.get_intra_idx())
    o, ck = g['W'].shape
    conv = layer(dev, ck // 12, o)
    with torch.no_grad():
        conv.basic_conv.W.copy_(torch.from_numpy(g['W']))
    y, gf, gw = run(conv, torch.from_numpy(g['feats']).to(dev), torch.from_numpy(g['gy']).to(dev))
    assert rel_err(y, torch.from_numpy(g['out'])) < 1e-5
    assert rel_err(gf, torch.from_numpy(g['gfeats'])) < 1e-5
    assert rel_err(gw, torch.from_numpy(g['gW'])) < 2e-5


def test_weight_gradient_over_a_slice_boundary_and_a_partial_slice(dev):
    """c = 40: channel slices of 16, 16 and 8 (the byte budget of 64 channels on the 60-anchor axis)"""
    import vgtk.so3conv.functional as L
    assert max(1, L.INTRA_DW_SLICE * 60 // 240) == 16
    b, c, o, p = 2, 40, 7, 3
    conv = layer(dev, c, o)
    gen = torch.Generator().manual_seed(40)
    feats, gy = torch.randn(b, c, p, 240, generator=gen).to(dev), torch.randn(b, o, p, 240, generator=gen).to(dev)
    (_, gw), names = launched(lambda: run(conv, feats, gy, want=('w',)))
    assert names.count('eap_so3_intra_group2d_fwd_f32') == 3, names
    assert rel_err(gw, reference64(feats, conv.basic_conv.W, gy, conv.intra_idx)[2]) < 2e-5


@pytest.mark.parametrize('shape', [(2, 64, 128, 16), (1, 128, 256, 8)])
def test_split_kernels_against_float64(dev, shape):
    """two fp16 planes, three bf16 planes and the fp32 pipe on operands like the path's (weights ~ N(0, 0.05), non-negative features whose
    points differ by e^+-1): each within the layer's bars, the two-plane output no further from float64 than 1.25 x the fp32 kernel's"""
    b, c, o, p = shape
    conv = layer(dev, c, o)
    gen = torch.Generator().manual_seed(sum(shape))
    with torch.no_grad():
        conv.basic_conv.W.copy_((torch.randn(o, c * 12, generator=gen) * 0.05).to(dev))
    feats = (torch.randn(b, c, p, 240, generator=gen).abs() * torch.exp(torch.randn(b, 1, p, 1, generator=gen))).to(dev)
    gy = torch.randn(b, o, p, 240, generator=gen).to(dev)
    out64, gf64, gw64 = reference64(feats, conv.basic_conv.W, gy, conv.intra_idx)
    entry = {'f16x2': 'eap_so3_intra_conv2d_f16x2_f32', 'bf16x3': 'eap_so3_intra_conv2d_bf16x3_f32', 'fp32': 'eap_so3_intra_conv2d_f32'}
    err = {}
    for name in ('f16x2', 'bf16x3', 'fp32'):
        with mode(name):
            (y, gf, gw), names = launched(lambda: run(conv, feats, gy))
        assert entry[name] in names, (name, names)
        err[name] = rel_err(y, out64), rel_err(gf, gf64), rel_err(gw, gw64)
        print(f'\nIntraSO3Conv2D {shape} {name}: out {err[name][0]:.2e}, dF {err[name][1]:.2e}, dW {err[name][2]:.2e}')
    for name, e in err.items():
        assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 2e-5, (name, e)
    assert err['f16x2'][0] <= 1.25 * err['fp32'][0] + 1e-7, err


def test_grouping_pair(dev):
    """intra_so3conv_grouping_2D on the kernels: a copy, so bit for bit the tensor expression; its backward sums without atomics"""
    import vgtk.so3conv.functional as L
    b, c, p = 2, 3, 7
    gen = torch.Generator().manual_seed(237)
    idx = torch.from_numpy(np.ascontiguousarray(L.get_intra_idx())).long().to(dev)
    f = torch.randn(b, c, p, 240, generator=gen).to(dev)
    g = torch.randn(b, c, 12, p, 240, generator=gen).to(dev)
    f1 = f.clone().requires_grad_(True)
    out, names = launched(lambda: L.intra_so3conv_grouping_2D(idx, f1))
    assert names == ['eap_so3_intra_group2d_fwd_f32'], names
    f2 = f.clone().requires_grad_(True)
    want = grouped_ref(f2, idx)
    assert out.shape == want.shape and torch.equal(out, want)
    (g1,), names = launched(lambda: torch.autograd.grad(out, [f1], g, retain_graph=True))
    assert names == ['eap_so3_intra_group2d_bwd_f32'], names
    g2, = torch.autograd.grad(want, [f2], g)
    assert rel_err(g1, g2) < 1e-6
    again, = torch.autograd.grad(out, [f1], g)
    assert torch.equal(g1, again)
    # every gathered quad lands on one feature quad: 12 reads per element
    ones, = torch.autograd.grad(L.intra_so3conv_grouping_2D(idx, f1), [f1], torch.ones_like(g))
    assert torch.equal(ones, torch.full_like(f, 12.0))


def test_no_gathered_tensor_is_allocated(dev):
    """forward + feature gradient (the weights frozen) at b = 1, c = o = 64, p = 128: the 12-tap tensor would be 94 MB and the tensor form
    holds it at least twice; the peak stays below half of it (47 MB) -- output and gradient are 7.9 MB each"""
    b, c, o, p = 1, 64, 64, 128
    conv = layer(dev, c, o).requires_grad_(False)
    gen = torch.Generator().manual_seed(64)
    feats, gy = torch.randn(b, c, p, 240, generator=gen).to(dev), torch.randn(b, o, p, 240, generator=gen).to(dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y, gf = run(conv, feats, gy, want=('f',))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    gathered = b * c * 12 * p * 240 * 4
    print(f'\npeak above the inputs {rise / 1e6:.1f} MB, the gathered tensor {gathered / 1e6:.1f} MB')
    assert rise < gathered / 2, (rise, gathered)
    assert y.shape == (b, o, p, 240) and gf.shape == feats.shape
