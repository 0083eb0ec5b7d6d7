"""Shared by tests/test_inv_slot_head_host.py and tests/test_gpu_inv_slot_head.py: tests/golden/inv_slot_head.npz (the reference's
InvOutBlockOursWithMask run once per cloud on a point subset, tests/golden/make_golden_inv_slot.py) unpacked for the package's class."""
import numpy as np
import torch

PARAMS = {'dim_in': 24, 'mlp': [16], 'fc': [16], 'k': 16, 'kanchor': 60, 'temperature': 3.0}
# the bars of the same comparisons in tests/test_gpu_lists_and_modules.py (outputs, running statistics, d feats, parameter gradients)
BAR_OUT, BAR_RUNNING, BAR_DFEATS, BAR_DPARAM = 2e-5, 1e-5, 5e-5, 1e-4


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def make_head(tag):
    import vgtk.so3conv as sptk
    return sptk.InvOutBlockOursWithMask(PARAMS, norm=1, pooling_method='attention', use_pointnet=True, use_abs_pos=(tag == 'abs'),
                                        return_point_pooling_feature=True)


def state_of(G, tag):
    pre = f'{tag}_state_'
    return {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in G.items() if k.startswith(pre)}


def inputs_of(G):
    """-> xyz [3,3,37], feats [3,24,37,60] (the stored member points in place, seeded noise at the others, which no result may depend
    on), member bool [3,37], the three probes of the linear functional"""
    member = torch.from_numpy(np.asarray(G['member']))
    packed = torch.from_numpy(np.asarray(G['feats_members']))                        # [C, members of cloud 0, 1, 2, A]
    b, n = member.shape
    feats = torch.randn(b, packed.shape[0], n, packed.shape[2], generator=torch.Generator().manual_seed(8))
    at = 0
    for i in range(b):
        k = int(member[i].sum())
        feats[i][:, member[i]] = packed[:, at:at + k]
        at += k
    g = tuple(torch.from_numpy(np.asarray(G[k])) for k in ('g_pooled', 'g_code', 'g_logits'))
    return torch.from_numpy(np.asarray(G['xyz'])), feats, member, g


def pack_members(t, member):
    """[3,C,37,A] -> [C, members cloud after cloud, A], the layout of the fixture's feature gradients"""
    return torch.cat([t[i][:, member[i]] for i in range(member.shape[0])], 1)


def absorbed(name, tag, training):
    """parameters whose gradient a training-mode norm behind them absorbs (rounding noise in the reference): the pre-norm biases, and with
    centred coordinates the coordinate columns of the embed weight (they multiply mean(x - mean x), in both modes)"""
    if name == 'pointnet.embed.weight':
        return 'xyz columns' if tag == 'rel' else None
    return 'all' if training and name in ('linear.0.bias', 'pointnet.embed.bias') else None


def check_param_grads(named_grads, G, tag, training, bar, noise=1e-4):
    """named_grads: name -> gradient (or None) of the functional; against the fixture's.  An absorbed gradient is noise in the reference
    and zero or noise here: both below `noise` times the largest parameter gradient."""
    mode = 'train' if training else 'eval'
    refs = {k: np.asarray(G[f'{tag}_{mode}_grad_{k}']) for k in named_grads}
    top = max(np.abs(r).max() for r in refs.values())
    c = PARAMS['mlp'][-1]
    for k, got in named_grads.items():
        ref = refs[k]
        got = np.zeros_like(ref) if got is None else got.detach().cpu().numpy()
        kind = absorbed(k, tag, training)
        if kind == 'all':
            assert np.abs(ref).max() < 1e-4 * top and np.abs(got).max() <= noise * top, (mode, k)
            continue
        if kind == 'xyz columns':
            assert np.abs(ref[:, c:]).max() < 1e-4 * top and np.abs(got[:, c:]).max() <= noise * top, (mode, k)
            ref, got = ref[:, :c], got[:, :c]
        assert rel_err(got, ref) < bar, (mode, k, rel_err(got, ref))
