"""CPU: the oracle against the fixture the reference's InterSO3PoseConv(kanchor = 20 / 40, permute_modes = 1) produced with per-point
poses (tests/golden/make_golden_subsets.py).  The two anchor sets are subsets of the icosahedral rotations, not groups: the anchor
index is searched per entry and is in general no permutation.  This pins the oracle for the GPU tests of that regime
(tests/test_gpu_anchor_subsets.py)."""
import numpy as np
import pytest
import torch

from oracle import so3_ref

T = torch.from_numpy

RADIUS, SIGMA, NNB = 0.2, 0.02, 8
TIE_GAP = 2e-5        # ~20 x the fp32 rounding of a 9-term trace of magnitude <= 3: below it an fp32 arg-max may differ


def trace_gap_and_index(ball_idx, pose, anchors):
    """the oracle's expression (so3_ref.rotated_anchor_index) in float64 -> (index int64 [b,p,nn,na], smallest gap best / second best)"""
    rot = pose[:, :, :3, :3].double()
    grouped = so3_ref.batched_index_select_other(rot, ball_idx.long(), dim=1)
    rel = torch.matmul(rot.unsqueeze(2), grouped.transpose(3, 4).contiguous())
    A = anchors.double()
    top = torch.einsum('bpnji,ajk,cik->bpnac', rel, A, A).topk(2, dim=-1).values
    return so3_ref.rotated_anchor_index(rel, A), float((top[..., 0] - top[..., 1]).min())


def test_fixture_loads(golden):
    g = golden('inter_pose_subsets.npz')
    for na in (20, 40):
        assert g[f'k{na}_anchors'].shape == (na, 3, 3)
        for tag in ('random', 'parts', 'art_random'):
            key = f'k{na}_{tag}'
            assert g[f'{key}_out'].shape == (2, 4, 40, na) and g[f'{key}_gfeats'].shape == (2, 4, 40, na) and g[f'{key}_gW'].shape == (4, 96)
            idx = g[f'{key}_rotated_anchor_idx']
            assert idx.shape == (2, 40, 8, na) and idx.max() < na
            assert float(g[f'{key}_trace_gap']) >= TIE_GAP
            assert (idx != np.arange(na)).any()                                    # really permuted
    # many-to-one: some entry's index is no permutation of the anchors
    idx = g['k20_random_rotated_anchor_idx']
    assert any(len(np.unique(row)) < 20 for row in idx.reshape(-1, 20))


@pytest.mark.parametrize('na', [20, 40])
@pytest.mark.parametrize('tag', ['random', 'parts'])
def test_oracle_reproduces_the_reference(golden, na, tag):
    g = golden('inter_pose_subsets.npz')
    key = f'k{na}_{tag}'
    # the anchors as the reference's module holds them: select_anchor's strided VIEW of the 60-anchor table (L2641-2649).  torch's CPU
    # matmul rounds differently on a contiguous copy of the same numbers (out / dF / dW then agree to ~1e-6, not to the bit)
    import vgtk.so3conv.functional as L
    anchors = T(L.select_anchor(golden('constants.npz')['anchors'], na))
    assert np.array_equal(anchors.numpy(), g[f'k{na}_anchors'])
    xyz, pose, kernels = T(g['xyz']), T(g[f'{key}_pose']), T(g['kernels'])
    feats = T(g[f'{key}_feats']).requires_grad_(True)
    W = T(g[f'{key}_W']).requires_grad_(True)
    res = so3_ref.inter_so3poseconv_grouping_strided(xyz, pose, feats, NNB, anchors, kernels, RADIUS, SIGMA, permute_modes=1)
    idx64, gap = trace_gap_and_index(res['ball_idx'], pose, anchors)
    assert gap >= TIE_GAP
    assert torch.equal(res['rotated_anchor_idx'], idx64) and np.array_equal(idx64.numpy(), g[f'{key}_rotated_anchor_idx'])
    np.testing.assert_allclose(res['inter_w'][:, ::8, ::7, ::5].detach().numpy(), g[f'{key}_inter_w_sample'], rtol=0, atol=1e-6)
    out = so3_ref.basic_so3conv(W, res['new_feats'])
    np.testing.assert_array_equal(out.detach().numpy(), g[f'{key}_out'])
    gf, gW = torch.autograd.grad(out, [feats, W], T(g[f'{key}_gy']))
    np.testing.assert_array_equal(gf.numpy(), g[f'{key}_gfeats'])
    np.testing.assert_array_equal(gW.numpy(), g[f'{key}_gW'])
