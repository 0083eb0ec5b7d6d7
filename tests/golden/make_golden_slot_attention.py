"""tests/golden/make_golden_slot_attention.py -- golden vectors of the segmentation step by RUNNING THE REFERENCE class SlotAttention
(SPConvNets/utils/slot_attention_spec_v2.py:L6-193; the file imports only torch and is loaded by path) on the CPU.

  slot_attention.npz (+ slot_attention.part<k>.npz: the arrays packed into volumes below 1 MiB, `volumes` in the first names how many)
      two variants, (B, N, d, S, hidden) = 'small' (2, 37, 20, 3, 16) and 'orbit3' (1, 130, 131, 2, 128), iters = 3.  Every norm_input
      weight is drawn from N(1, 0.3) and every bias from N(0, 0.3) (at their initial 1 and 0 they could not be told from absent); the
      input is relu(randn) * 1.5 + 0.2.  Stored per variant: the state (names, float32 values), x, the noise the class drew (seed, call;
      seed again, draw the same shape), the weights of a seeded linear-plus-quadratic functional of (slots, attn_ori), the class run in
      float64 -- slots, attn_ori, dL/dx, dL/d every parameter -- and the float32 run for the record (`f32_`; of the orbit3 variant
      without its parameter gradients, which would be another three volumes), the smallest top-two gap of attn_ori over the slots.
      Data only.

The input seed is the first for which that gap, in float64, is at least 1e-4 at every point: argmax(attn_ori) is then decided by five
times the output bar of tests/slot_attention_common.py.

Re-run:  python tests/golden/make_golden_slot_attention.py [reference checkout; default: ../reference beside this repository]
(writes the same bytes every time)"""
import copy
import glob
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import slot_attention_common as C  # noqa: E402

REF_ROOT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', '..', '..', 'reference')       # a checkout beside this repository
_spec = importlib.util.spec_from_file_location('ref_slot_attention', os.path.join(REF_ROOT, 'SPConvNets', 'utils', 'slot_attention_spec_v2.py'))
REF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REF)

MIN_GAP = 1e-4
NOISE_SEED = 77
VOLUME_BYTES = 900 * 1024


def build(tag):
    b, n, d, s, hidden = C.VARIANTS[tag]
    torch.manual_seed(41 + len(tag))
    model = REF.SlotAttention(s, d, iters=C.ITERS, eps=C.EPS, hidden_dim=hidden)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in model.norm_input:
            m.weight.copy_(1.0 + 0.3 * torch.randn(d, generator=gen))
            m.bias.copy_(0.3 * torch.randn(d, generator=gen))
    return model


def run(model, x, w, dtype):
    model = copy.deepcopy(model).to(dtype)
    x = x.to(dtype).requires_grad_(True)
    torch.manual_seed(NOISE_SEED)
    slots, attn = model(x)
    names = [k for k, _ in model.named_parameters()]
    grads = torch.autograd.grad(C.functional(slots, attn, tuple(t.to(dtype) for t in w)), [x] + list(model.parameters()))
    return slots.detach(), attn.detach(), grads[0], dict(zip(names, grads[1:]))


def variant(tag):
    b, n, d, s, hidden = C.VARIANTS[tag]
    model = build(tag)
    assert list(model.state_dict()) == [k for k, _ in model.named_parameters()]
    gen = torch.Generator().manual_seed(9)
    w = (torch.randn(b, s, d, generator=gen), torch.randn(b, s, d, generator=gen) * 0.5, torch.randn(b, s, n, generator=gen),
         torch.randn(b, s, n, generator=gen) * 0.5)
    seed = 0
    while True:
        x = torch.relu(torch.randn(b, n, d, generator=torch.Generator().manual_seed(seed))) * 1.5 + 0.2
        res64 = run(model, x, w, torch.float64)
        top = res64[1].topk(min(2, s), dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        if gap >= MIN_GAP:
            break
        seed += 1
    torch.manual_seed(NOISE_SEED)
    noise = torch.randn(b, s, d)
    res32 = run(model, x, w, torch.float32)
    out = {f'{tag}_state_{k}': v for k, v in model.state_dict().items()}
    out.update({f'{tag}_x': x, f'{tag}_noise': noise, f'{tag}_input_seed': np.int64(seed), f'{tag}_gap': np.float64(gap)})
    out.update({f'{tag}_{k}': v for k, v in zip(('a_slots', 'q_slots', 'a_attn', 'q_attn'), w)})
    for pre, res, with_params in (('', res64, True), ('f32_', res32, tag == 'small')):
        out.update({f'{tag}_{pre}slots': res[0], f'{tag}_{pre}attn': res[1], f'{tag}_{pre}dx': res[2]})
        if with_params:
            out.update({f'{tag}_{pre}grad_{k}': v for k, v in res[3].items()})
    print(f'{tag}: input seed {seed}, smallest top-two gap {gap:.3e}; float32 run against float64: slots '
          f'{C.rel_err(res32[0], res64[0]):.1e}, attn {C.rel_err(res32[1], res64[1]):.1e}, dx {C.rel_err(res32[2], res64[2]):.1e}')
    return out


def write_volume(path, arrays):
    """an .npz np.load reads, with the fixed timestamp that makes a re-run write the same bytes"""
    with zipfile.ZipFile(path, 'w') as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, v if v.ndim == 0 else np.ascontiguousarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    arrays = {}
    for tag in C.VARIANTS:
        arrays.update({k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in variant(tag).items()})
    volumes, size = [{}], 0
    for k, v in arrays.items():
        if size + v.nbytes > VOLUME_BYTES and volumes[-1]:
            volumes.append({})
            size = 0
        volumes[-1][k] = v
        size += v.nbytes
    volumes[0] = dict(volumes=np.int64(len(volumes)), **volumes[0])
    for old in glob.glob(os.path.join(HERE, C.FIXTURE.replace('.npz', '.part*.npz'))):
        os.remove(old)
    for i, vol in enumerate(volumes):
        name = C.FIXTURE if i == 0 else C.FIXTURE.replace('.npz', f'.part{i}.npz')
        write_volume(os.path.join(HERE, name), vol)
        print(f'{name}: {os.path.getsize(os.path.join(HERE, name)) / 1024:.0f} KiB, {len(vol)} arrays')


if __name__ == '__main__':
    main()
