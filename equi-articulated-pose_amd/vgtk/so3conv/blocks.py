"""Block-layer epilogue of the SO(3) conv blocks: BatchNorm2d + leaky_relu in one pass.

Reference: `feat = self.norm(x.feats); feat = self.relu(feat)` in
SPConvNets/utils/base_so3poseconv.py:L214-221 (`norm = nn.BatchNorm2d(dim_out)`, `relu =
F.leaky_relu` for the shipped 'leaky_relu' activation, L196-201).  SURVEY.md 8(f) row 1.

`BatchNormLeakyReLU` has nn.BatchNorm2d's parameters and buffers under the same names (weight,
bias, running_mean, running_var, num_batches_tracked), so a reference checkpoint's `norm.*`
entries load into it; its forward equals `F.leaky_relu(bn(x), negative_slope)`.
The arithmetic runs in csrc/bn_act.hip (no CPU / eager fallback).
"""
import torch
from torch import nn

from vgtk.spconv import SphericalPointCloud, SphericalPointCloudPose

from .. import _hip
from . import norm_fold
from .functional import FoldedEpilogue, TrainEpilogue, so3_contract
from .norm_fold import _syncing, affine_from_moments, all_reduce_sums, batch_moments, update_running_stats  # noqa: F401  (re-exported)


class _BNAct(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, slope, sync, residual=None, pre_bias=None):
        """pre_bias [C]: act(bn(x + pre_bias)) without the pass that would add it -- a per-channel constant in front of a
        BatchNorm moves the batch mean and nothing else (training: it only enters the running mean, its gradient is
        exactly zero; eval: it shifts the pre-activation like beta)."""
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
            if residual.shape != x.shape:
                raise RuntimeError('BatchNormLeakyReLU: residual must have the shape of the input')
        b, c = x.shape[0], x.shape[1]
        n = x.numel() // (b * c)
        sums = (*_hip.bn_stats(x, b, c, n), x.reshape(b, c, n)[0, :, 0].double(), b * n) if training else None
        scale, shift, mean, invstd, count = norm_fold.fold(sums, weight, bias, running_mean, running_var, training, momentum, eps, pre_bias, sync)
        y = _hip.bn_act_fwd(x, b, c, n, scale, shift, slope, residual)
        ctx.has_res = residual is not None
        ctx.has_pre_bias = pre_bias is not None
        ctx.save_for_backward(x, scale, shift, mean.float(), invstd.float())
        ctx.training, ctx.slope, ctx.dims, ctx.sync, ctx.count = training, slope, (b, c, n), sync, count
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, shift, mean, invstd = ctx.saved_tensors
        b, c, n = ctx.dims
        gy = gy.contiguous()
        sg, sgx = _hip.bn_act_bwd_reduce(gy, x, b, c, n, scale, shift, mean, invstd, ctx.slope)
        g_x = None
        if ctx.needs_input_grad[0]:
            k2, k3 = norm_fold.backward_coefficients(scale, sg, sgx, ctx.count, ctx.training, ctx.sync)
            g_x = _hip.bn_act_bwd_apply(gy, x, b, c, n, scale, shift, mean, invstd, k2, k3, ctx.slope)
        g_pre = norm_fold.pre_bias_grad(sg, scale, ctx.training) if ctx.has_pre_bias else None
        return g_x, sgx.float(), sg.float(), None, None, None, None, None, None, None, (gy if ctx.has_res else None), g_pre


class BatchNormLeakyReLU(nn.BatchNorm2d):
    """nn.BatchNorm2d followed by leaky_relu, fused.  Input [B, C, P, A] (any trailing shape whose
    product is a multiple of 4)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, negative_slope=0.01, sync=False):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=True, track_running_stats=True)
        self.negative_slope = negative_slope
        self.sync = sync          # batch statistics over all ranks (what nn.SyncBatchNorm does for the reference)

    def forward(self, x, residual=None, pre_bias=None):
        """leaky_relu(BatchNorm(x + pre_bias)) (+ residual: the separable block's `x.feats + skip_feature`,
        base_so3poseconv.py:L319-328, added in the same pass).  pre_bias [C]: the bias of the 1x1 conv in front, folded into
        the mean instead of a pass of its own.  In eval mode the normalisation is already folded into one per-channel
        scale / shift (no statistics pass): a single read + write of the tensor."""
        if not x.is_cuda:
            raise RuntimeError('BatchNormLeakyReLU: tensor must be a CUDA(HIP) tensor (no CPU fallback)')
        if x.dtype == torch.float64:
            raise RuntimeError('BatchNormLeakyReLU: float32 only -- the float64 regime covers the conv layers, not the norms')
        if self.training:
            self.num_batches_tracked.add_(1)
        return _BNAct.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.training,
                            self.momentum, self.eps, self.negative_slope, self.sync, residual, pre_bias)

    def folded(self, pre_bias=None, residual=None):
        """The layer in inference mode as one per-channel affine map + activation ("inference-mode BN
        folds into W"): leaky_relu(scale * x + shift) (+ residual), scale = gamma / sqrt(running_var + eps),
        shift = beta - (running_mean - pre_bias) * scale, computed in float64 exactly as the eval-mode forward does."""
        if self.training:
            raise RuntimeError('BatchNormLeakyReLU.folded: training-mode statistics depend on the data; call .eval() first')
        mean, var = norm_fold.eval_moments(self.running_mean, self.running_var, pre_bias)
        scale, shift, _ = affine_from_moments(mean, var, self.weight.detach(), self.bias.detach(), self.eps)
        return FoldedEpilogue(scale, shift, self.negative_slope, residual)


def conv_norm_act(conv, norm, x, **conv_kwargs):
    """The block layer's `x = conv(x); feat = relu(norm(x.feats))` (SPConvNets/utils/base_so3poseconv.py:L205-222) for an
    InterSO3Conv / InterSO3PoseConv and a BatchNormLeakyReLU -> (inter_idx, inter_w, sample_idx, cloud with the activated
    features).  In inference (norm in eval mode, gradients off) the normalisation and the activation ride in the
    contraction's epilogue -- the feature map is written once, no pass of its own; in training the norm joins the conv's autograd
    node where the conv runs the dense product, or where it has at most 32 contraction indices and an input without gradient (the
    first layer: regime 'narrow input'); otherwise conv and norm run as usual."""
    fold = not norm.training and not torch.is_grad_enabled()
    ep = norm.folded() if fold else None
    if ep is None and norm.training and isinstance(norm, BatchNormLeakyReLU) and norm.negative_slope > 0:
        # training: where the conv runs the dense product, and at the first layer, the normalisation joins its autograd node (no pass of
        # its own in either direction, the conv output is never written: vgtk/so3conv/functional.py TrainEpilogue)
        ep = TrainEpilogue(norm)
    if ep is not None:
        conv_kwargs = dict(conv_kwargs, epilogue=ep)
    inter_idx, inter_w, sample_idx, y = conv(x, **conv_kwargs)
    if ep is not None and ep.applied:
        feats = y.feats
        if norm.training:
            norm.num_batches_tracked.add_(1)
    else:
        feats = norm(y.feats)
    pose = getattr(y, 'pose', None)
    out = SphericalPointCloudPose(y.xyz, feats, y.anchors, pose) if pose is not None else SphericalPointCloud(y.xyz, feats, y.anchors)
    return inter_idx, inter_w, sample_idx, out


def pointwise_norm_act(conv1x1, norm, x, residual=None):
    """relu(norm(conv1x1(x))) (+ residual): the separable block's skip branch and sum (base_so3poseconv.py:L319-328) for an
    nn.Conv2d(c, o, 1) and a BatchNormLeakyReLU.  The conv bias always rides in the norm's mean; in inference the whole
    norm + activation + sum ride in the contraction's epilogue."""
    b, c, n, a = x.shape
    W = conv1x1.weight.view(conv1x1.out_channels, c)
    ep = norm.folded(pre_bias=conv1x1.bias, residual=residual) if (not norm.training and not torch.is_grad_enabled()) else None
    y = so3_contract(W, x.reshape(b, c, n * a), ep).view(b, conv1x1.out_channels, n, a)
    if ep is not None and ep.applied:
        return y
    return norm(y, residual=residual, pre_bias=conv1x1.bias)


class InstanceNormLeakyReLU(nn.Module):
    """nn.InstanceNorm2d(affine=False) followed by leaky_relu, fused: the norm of the intra blocks
    (`self.norm = nn.InstanceNorm2d(dim_out, affine=False)`, base_so3poseconv.py:L88).  Instance
    statistics are batch statistics of a [1, B*C, P, A] view, so the same kernels serve it."""

    def __init__(self, num_features, eps=1e-5, negative_slope=0.01):
        super().__init__()
        self.num_features, self.eps, self.negative_slope = num_features, eps, negative_slope

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('InstanceNormLeakyReLU: tensor must be a CUDA(HIP) tensor (no CPU fallback)')
        if x.dtype == torch.float64:
            raise RuntimeError('InstanceNormLeakyReLU: float32 only -- the float64 regime covers the conv layers, not the norms')
        b, c = x.shape[0], x.shape[1]
        ones = torch.ones(b * c, dtype=torch.float32, device=x.device)
        y = _BNAct.apply(x.contiguous().view(1, b * c, *x.shape[2:]), ones, torch.zeros_like(ones), None, None, True,
                         0.0, self.eps, self.negative_slope, False)
        return y.view_as(x)
