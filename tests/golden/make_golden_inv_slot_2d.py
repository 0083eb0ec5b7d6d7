"""tests/golden/make_golden_inv_slot_2d.py -- golden vectors of the per-slot shape-code head on the 240-anchor map of a `use_2d` backbone, by
RUNNING THE REFERENCE class InvOutBlockOursWithMask with its PointnetSO3ConvOurs (SPConvNets/utils/base_so3conv.py:L1013-1205) on CPU in the
build container: the sibling of make_golden_inv_slot.py, by its recipe (the reference imported through tests/golden/ref_import.py, the class
called the way the model calls it, ...pn_38_multi_stage.py:L706-830: once per cloud, batch 1, mask=None, on the gathered subset).

  inv_slot_head_2d.npz   the head built with kanchor 60 and run on a feature map of 60 x 4 = 240 anchors, so that PointnetSO3ConvOurs takes its
                         tot_anchors [240,3,3] branch (L1173-1176, L1196); pooling_method='attention', use_pointnet=True,
                         return_point_pooling_feature=True, with use_abs_pos False ('rel') and True ('abs'); three clouds with 21, 4 and 1
                         member points out of 37; training mode (the three calls in cloud order, so the running statistics hold three updates)
                         and eval mode.  Stored per variant and mode, as in inv_slot_head.npz: the three return values per cloud (pooled
                         [3,c,240], code [3,c], logits [3,240]), the gradients of a seeded linear functional of them with respect to the
                         features (member points only, cloud after cloud) and every parameter, and after the training pass every running
                         statistic.  Of the input features the member points alone are stored (feats_members [C, 26, 240]).  Data only.

Four input channels: the feature gradients are four tensors of the input's size, and the file stays under 1 MB.

The input seed is the first for which every ReLU input, behind both kinds of norm and in both modes and variants, stays 2e-5 away from zero
in the reference alone; that margin is stored.

Re-run:  python tests/golden/make_golden_inv_slot_2d.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_inv_slot as S  # noqa: E402  (imports the reference class; run() and build() read this module's sizes)
from make_golden import save  # noqa: E402

S.B, S.C, S.N, S.A = 3, 4, 37, 240
S.COUNTS = (21, 4, 1)
S.PARAMS = {'dim_in': S.C, 'mlp': [16], 'fc': [16], 'k': 16, 'kanchor': 60, 'temperature': 3.0}


def main():
    heads = {'rel': S.build(False), 'abs': S.build(True)}
    assert all(tuple(h.pointnet.tot_anchors.shape) == (240, 3, 3) for h in heads.values())
    states = {k: {n: v.clone() for n, v in h.state_dict().items()} for k, h in heads.items()}
    seed = 500
    while True:
        xyz, feats, member, g = S.inputs(seed)
        seen = []
        for k, h in heads.items():
            for training in (True, False):
                S.run(h, states[k], training, xyz, feats, member, g, seen)
        if min(seen) > 2e-5:
            break
        seed += 1
    print(f'inv_slot_head_2d: input seed {seed}, smallest |ReLU input| {min(seen):.2e}')
    out = {'xyz': xyz, 'feats_members': torch.cat([feats[i][:, member[i]] for i in range(S.B)], 1), 'member': member, 'g_pooled': g[0],
           'g_code': g[1], 'g_logits': g[2], 'x_seed': np.int32(seed), 'relu_margin': np.float32(min(seen)),
           'temperature': np.float32(S.PARAMS['temperature'])}
    for k, h in heads.items():
        out.update({f'{k}_state_{n}': v for n, v in states[k].items()})
        for training in (True, False):
            mode = 'train' if training else 'eval'
            pooled, code, logits, gx, gp = S.run(h, states[k], training, xyz, feats, member, g)
            assert pooled.shape[-1] == 240 and logits.shape[-1] == 240
            out.update({f'{k}_{mode}_pooled': pooled, f'{k}_{mode}_code': code, f'{k}_{mode}_logits': logits, f'{k}_{mode}_grad_feats': gx})
            out.update({f'{k}_{mode}_grad_{n}': v for n, v in gp.items()})
            if training:
                out.update({f'{k}_after_{n}': v.clone() for n, v in h.state_dict().items() if 'running' in n or 'num_batches' in n})
    save('inv_slot_head_2d.npz', **out)


if __name__ == '__main__':
    main()
