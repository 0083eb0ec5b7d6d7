"""GPU: a layer whose clouds reference more than 512 support rows, in the DEFAULT mode, against the reference's own numbers
(tests/golden/dense_wide_identity_o128.npz, made by running the reference: tests/golden/make_golden_dense_wide.py).  The regime the
call took is asserted; bars as tests/test_gpu_dense_golden.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_parity import _run_layer, rel_err, dev, vg  # noqa: E402,F401


def _draw(g, b, c, o, p, na=60):
    """the generator's `draw`: the layer's input and the factors of its output gradient from torch's CPU generator, checked against the
    checksums the fixture carries"""
    gen = torch.Generator().manual_seed(int(g['seed_feats']))
    feats = torch.randn(b, c, p, na, generator=gen)
    gen = torch.Generator().manual_seed(int(g['seed_gy']))
    u1, u2 = torch.randn(b, o, generator=gen), torch.randn(b, o, generator=gen)
    v1, v2 = torch.randn(b, p, na, generator=gen), torch.randn(b, p, na, generator=gen)

    def check(*ts):
        v = torch.cat([t.double().flatten() for t in ts])
        return np.concatenate([[float(v.sum()), float((v * v).sum())], v[:8].numpy()])
    np.testing.assert_allclose(check(feats), g['feats_check'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(check(u1, v1, u2, v2), g['gy_check'], rtol=1e-12, atol=0)
    return feats, u1[:, :, None, None] * v1[:, None] + u2[:, :, None, None] * v2[:, None]


def test_wide_dense_layer_golden(dev, vg, golden):
    _, _, _, L = vg
    import vgtk.cuda.grouping as G
    assert L.DENSE_MODE == 'auto'                     # the default decision, nothing forced
    g = dict(golden('dense_wide_identity_o128.npz'))
    b, _, p = g['xyz'].shape
    o, c = g['W'].shape[0], int(g['in_channels'])
    assert g['referenced_rows'].min() > 512 and g['referenced_rows'].max() <= 1024
    feats0, gy = _draw(g, b, c, o, p)
    g['feats'] = feats0.numpy()
    g['pose'] = np.tile(np.eye(4, dtype=np.float32), (b, p, 1, 1))
    xyz = torch.from_numpy(g['xyz']).to(dev)
    idx = G.ball_query(xyz, xyz, float(g['radius']), int(g['nn'])).cpu().numpy()
    assert np.array_equal(idx, g['ball_idx'].astype(np.int32))
    assert [len(np.unique(idx[i])) for i in range(b)] == list(g['referenced_rows'])
    L.BACKWARD_LOG, L.FORWARD_LOG = [], []
    try:
        conv, feats, (inter_idx, inter_w, sample_idx, y) = _run_layer(vg, dev, g)
        gf, gW = torch.autograd.grad(y.feats, [feats, conv.basic_conv.W], gy.to(dev))
        log, flog = L.BACKWARD_LOG, L.FORWARD_LOG
    finally:
        L.BACKWARD_LOG = L.FORWARD_LOG = None
    assert [r['regime'] for r in log] == ['dense rows'] and log[0]['referenced_rows_max'] > 512, log
    assert [r['dense'] for r in flog] == [True], flog
    out = y.feats.detach().cpu().numpy()
    e = (rel_err(out[:, ::16, ::31], g['out_channels16']), rel_err(out[:, :, ::256], g['out_points256']),
         rel_err(gf.cpu().numpy()[:, :, ::31], g['grad_feats_points31']), rel_err(gW.cpu().numpy(), g['grad_W']))
    print('wide golden: out (channels) %.3g, out (points) %.3g, dF %.3g, dW %.3g' % e)
    assert e[0] < 1e-5 and e[1] < 1e-5
    assert e[2] < 1e-5
    assert e[3] < 2e-5
