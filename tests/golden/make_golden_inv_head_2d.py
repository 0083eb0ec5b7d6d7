"""tests/golden/make_golden_inv_head_2d.py -- golden vectors for the per-point invariant head of the `use_2d` models, produced by RUNNING THE
REFERENCE on CPU in the build container (through tests/golden/ref_import.py), in the manner of inv_head() in make_golden_extra.py.  Data only.

  inv_head_2d.npz    InvPPOutBlock2DOurs (SPConvNets/utils/base_so3conv.py:L921-1008) on a [2,8,7,240] map (60 space anchors x 4 plane
                     anchors): attention / max / mean pooling and sel_mode = 17 (the space anchor is fixed, attention over its 4 plane
                     anchors), training and eval mode: state, outputs, the confidence where the class returns one, the running
                     statistics after the training call, and every autograd gradient of the attention and sel_mode variants

Re-run:  python tests/golden/make_golden_inv_head_2d.py"""
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
REFERENCE = '/root/reference'
for _name, _dir in (('SPConvNets', 'SPConvNets'), ('SPConvNets.utils', 'SPConvNets/utils'), ('SPConvNets.models', 'SPConvNets/models')):
    if _name not in sys.modules:
        _m = types.ModuleType(_name)
        _m.__path__ = [os.path.join(REFERENCE, _dir)]
        sys.modules[_name] = _m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PARAMS = {'dim_in': 8, 'mlp': [6], 'fc': [6], 'k': 6, 'kanchor': 60, 'temperature': 3.0}
SHAPE = (2, 8, 7, 240)
# tag -> (pooling_method, sel_mode)
MODES = {'attention': ('attention', None), 'max': ('max', None), 'mean': ('mean', None), 'sel_mode': ('max', 17)}


def inv_head_2d():
    INV = _load('ref_base_so3conv', os.path.join(REFERENCE, 'SPConvNets/utils/base_so3conv.py')).InvPPOutBlock2DOurs

    def build(tag):
        pooling, sel = MODES[tag]
        torch.manual_seed(12)
        head = INV(PARAMS, norm=1, pooling_method=pooling, sel_mode=sel)
        with torch.no_grad():
            for m in head.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
                    m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 2.0)
        return head

    def relu_margin(x):
        """Smallest |pre-activation| any ReLU of the attention head sees (training and eval mode): an input within fp32
        rounding of zero would let rounding pick the ReLU's side, and the gradients of the two sides differ by O(1)."""
        head = build('attention')
        state = {k: v.clone() for k, v in head.state_dict().items()}
        seen = []
        hooks = [m.register_forward_hook(lambda mod, inp, outp: seen.append(float(outp.detach().abs().min()))) for m in head.norm]
        for training in (True, False):
            head.load_state_dict(state)
            head.train(training)
            with torch.no_grad():
                head(zptk.SphericalPointCloud(None, x, None))
        for h in hooks:
            h.remove()
        return min(seen)

    seed = 99
    while True:                                  # the first seed whose ReLU inputs all stay 2e-5 away from zero
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.randn(*SHAPE, generator=gen)
        margin = relu_margin(x0)
        if margin > 2e-5:
            break
        seed += 1
    print(f'inv_head_2d: input seed {seed}, smallest |ReLU input| {margin:.2e}')
    out = {'x': x0, 'x_seed': np.int32(seed), 'relu_margin': np.float32(margin), 'sel_mode': np.int32(MODES['sel_mode'][1])}
    for tag in MODES:
        head = build(tag)
        state = {k: v.clone() for k, v in head.state_dict().items()}
        out.update({f'{tag}_state_{k}': v for k, v in state.items()})
        for phase in ('train', 'eval'):
            head.load_state_dict(state)
            head.train(phase == 'train')
            x = x0.clone().requires_grad_(True)
            res = head(zptk.SphericalPointCloud(None, x, None))
            if tag == 'attention':
                y, conf = res
                out[f'{tag}_{phase}_conf'] = conf.detach()
            else:
                y = res
            out[f'{tag}_{phase}_out'] = y.detach()
            if tag in ('attention', 'sel_mode'):
                g = torch.randn(y.shape, generator=gen)
                names = [n for n, _ in head.named_parameters()]
                grads = torch.autograd.grad(y, [x] + list(head.parameters()), g)
                out[f'{tag}_{phase}_grad_out'] = g
                out[f'{tag}_{phase}_grad_x'] = grads[0]
                for n, gr in zip(names, grads[1:]):
                    out[f'{tag}_{phase}_grad_{n}'] = gr
            if phase == 'train':
                for k, v in head.state_dict().items():
                    if 'running' in k:
                        out[f'{tag}_after_{k}'] = v.clone()
    save('inv_head_2d.npz', **out)


if __name__ == '__main__':
    inv_head_2d()
