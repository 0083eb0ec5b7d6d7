"""tests/golden/make_golden_inv_slot.py -- golden vectors of the per-slot shape-code head by RUNNING THE REFERENCE class
InvOutBlockOursWithMask with its PointnetSO3ConvOurs (SPConvNets/utils/base_so3conv.py:L1013-1205) on CPU in the build container
(through tests/golden/ref_import.py, like make_golden_extra.inv_head and make_golden_heads.py), the way the model calls it
(...pn_38_multi_stage.py:L706-830, calls at L765-777): once per cloud, batch 1, mask=None, on the gathered subset of the cloud's points.

  inv_slot_head.npz   pooling_method='attention', use_pointnet=True, return_point_pooling_feature=True, with use_abs_pos False ('rel') and
                      True ('abs'); three clouds with 21, 4 and 1 member points out of 37; training mode (the three calls in cloud order, so
                      the running statistics hold three updates) and eval mode.  Stored per variant and mode: the three return values per
                      cloud (pooled [3,c,A], code [3,c], logits [3,A]), the gradients of a seeded linear functional of them with respect
                      to the features (member points only, cloud after cloud: the others receive none) and every parameter, and after
                      the training pass every running statistic.  Of the input features the member points alone are stored
                      (feats_members [C, 26, A], cloud after cloud).  Data only.

The input seed is the first for which every ReLU input, behind both kinds of norm and in both modes and variants, stays 2e-5 away from
zero (see make_golden_extra.inv_head); that margin is stored.

Re-run:  python tests/golden/make_golden_inv_slot.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference through ref_import)
from make_golden import save  # noqa: E402

zptk = MG.zptk
for _name, _dir in (('SPConvNets', 'SPConvNets'), ('SPConvNets.utils', 'SPConvNets/utils'), ('SPConvNets.models', 'SPConvNets/models')):
    _m = types.ModuleType(_name)
    _m.__path__ = [os.path.join('/root/reference', _dir)]
    sys.modules.setdefault(_name, _m)

_spec = importlib.util.spec_from_file_location('ref_base_so3conv', '/root/reference/SPConvNets/utils/base_so3conv.py')
REF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REF)

B, C, N, A = 3, 24, 37, 60
COUNTS = (21, 4, 1)
PARAMS = {'dim_in': C, 'mlp': [16], 'fc': [16], 'k': 16, 'kanchor': A, 'temperature': 3.0}


def build(use_abs_pos):
    torch.manual_seed(31)
    head = REF.InvOutBlockOursWithMask(PARAMS, norm=1, pooling_method='attention', use_pointnet=True, use_abs_pos=use_abs_pos,
                                       return_point_pooling_feature=True)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 2.0)
    return head


def inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, 3, N, generator=gen) * 0.3
    feats = torch.randn(B, C, N, A, generator=gen)
    member = torch.zeros(B, N, dtype=torch.bool)
    for i, k in enumerate(COUNTS):
        member[i, torch.randperm(N, generator=gen)[:k]] = True
    g = (torch.randn(B, 16, A, generator=gen), torch.randn(B, 16, generator=gen), torch.randn(B, A, generator=gen))
    return xyz, feats, member, g


def run(head, state, training, xyz, feats, member, g, seen=None):
    """the model's loop over the clouds -> outputs per cloud, gradients of sum_i <g, outputs_i>"""
    head.load_state_dict(state)
    head.train(training)
    hooks = []
    if seen is not None:
        hooks = [m.register_forward_hook(lambda mod, inp, outp: seen.append(float(outp.detach().abs().min()))) for m in head.norm]
    x = feats.clone().requires_grad_(True)
    outs, loss = [], 0.0
    for i in range(B):
        sel = member[i].nonzero().squeeze(1)
        res = head(zptk.SphericalPointCloud(xyz[i:i + 1][:, :, sel], x[i:i + 1][:, :, sel], None), None)
        outs.append(res)
        loss = loss + sum((gi[i:i + 1] * r).sum() for gi, r in zip(g, res))
    for h in hooks:
        h.remove()
    names = [n for n, _ in head.named_parameters()]
    grads = torch.autograd.grad(loss, [x] + list(head.parameters()), allow_unused=True)
    gx = torch.cat([grads[0][i][:, member[i]] for i in range(B)], 1)                      # [C, sum of the counts, A]
    assert all(float(grads[0][i][:, ~member[i]].abs().max()) == 0.0 for i in range(B) if (~member[i]).any())
    pooled, code, logits = (torch.cat([o[k] for o in outs], 0).detach() for k in range(3))
    return pooled, code, logits, gx, dict(zip(names, grads[1:]))


def main():
    heads = {'rel': build(False), 'abs': build(True)}
    states = {k: {n: v.clone() for n, v in h.state_dict().items()} for k, h in heads.items()}
    seed = 500
    while True:
        xyz, feats, member, g = inputs(seed)
        seen = []
        for k, h in heads.items():
            for training in (True, False):
                run(h, states[k], training, xyz, feats, member, g, seen)
        if min(seen) > 2e-5:
            break
        seed += 1
    print(f'inv_slot_head: input seed {seed}, smallest |ReLU input| {min(seen):.2e}')
    # the features of the member points only, cloud after cloud like the gradients: the head never sees the others (a test fills them itself)
    out = {'xyz': xyz, 'feats_members': torch.cat([feats[i][:, member[i]] for i in range(B)], 1), 'member': member, 'g_pooled': g[0], 'g_code': g[1], 'g_logits': g[2], 'x_seed': np.int32(seed),
           'relu_margin': np.float32(min(seen)), 'temperature': np.float32(PARAMS['temperature'])}
    for k, h in heads.items():
        out.update({f'{k}_state_{n}': v for n, v in states[k].items()})
        for training in (True, False):
            mode = 'train' if training else 'eval'
            pooled, code, logits, gx, gp = run(h, states[k], training, xyz, feats, member, g)
            out.update({f'{k}_{mode}_pooled': pooled, f'{k}_{mode}_code': code, f'{k}_{mode}_logits': logits, f'{k}_{mode}_grad_feats': gx})
            out.update({f'{k}_{mode}_grad_{n}': v for n, v in gp.items()})
            if training:
                out.update({f'{k}_after_{n}': v.clone() for n, v in h.state_dict().items() if 'running' in n or 'num_batches' in n})
    save('inv_slot_head.npz', **out)


if __name__ == '__main__':
    main()
