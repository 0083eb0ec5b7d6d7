"""tools/lists2_only.py [B] (was tools/lists2_ablation.py) -- the two-tile grouping kernel (csrc/so3_inter_lists2.hip) alone: the deepest layer's backward
(O = 512, real inverse lists) and forward (C = 128) launches.
Median of 5 runs.  (The timing ablations that switched parts of the kernel off are recorded in profiles/r0[234]_lists2_ablation.txt;
their code left the tree with the ablation build.)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'equi-articulated-pose_amd'))
import torch
import synth_clouds
import vgtk.cuda.grouping as G
import vgtk.so3conv as sptk
import vgtk.so3conv.functional as L
from vgtk import _hip

B, P, NN, NA, KS = (int(sys.argv[1]) if len(sys.argv) > 1 else 8), 4096, 64, 60, 24
dev = torch.device('cuda:0')
xyz = torch.from_numpy(synth_clouds.laptop_batch(0, B, P)[0]).to(dev)
c, o, r, s = synth_clouds.backbone_layers(P)[2]
conv = sptk.InterSO3PoseConv(c, 8, 1, 1, r, s, NN, kanchor=NA, permute_modes=1).to(dev)
idx = G.ball_query(xyz, xyz, r, NN)
gx, nonident = _hip.so3_prep(xyz, xyz, idx, None, None, conv.anchors, 29)
rk = L.rotated_kernels(conv.anchors, conv.kernels)
rows, off, cnt, ent_p, ent_gx, rcap, _ = L._inverse_lists(idx, gx, P, 29, nonident)
gy = torch.randn(B, o, P, NA, device=dev)
feats = torch.randn(B, c, P, NA, device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def inv():
    return _hip.so3_inter_group_inv(gy, rows, off, cnt, ent_p, ent_gx, rk, None, s, NN)


def fwd():
    return _hip.so3_inter_group_fwd(feats, idx, gx, rk, None, s, blocked=2)


for name, fn, fl in (('backward Z, O = 512', inv, 2.0 * B * o * KS * P * NN * NA), ('forward X (transposed), C = 128', fwd, 2.0 * B * c * KS * P * NN * NA)):
    v = sorted(timed(fn) for _ in range(6))[:5]
    print(f'{name}: median {v[2]:7.2f} ms = {fl / v[2] / 1e9 / 157.3:.3f} of peak (algorithmic)', flush=True)
