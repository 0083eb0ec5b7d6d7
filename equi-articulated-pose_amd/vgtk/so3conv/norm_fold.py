"""The per-channel float64 bookkeeping of a BatchNorm folded into one map y = scale x + shift, shared by every norm + activation node
(blocks._BNAct, functional.TrainEpilogue, heads._SubsetBNAct / _NormActPointMean and the heads' torch fallbacks).  Pure torch on [C] or
[R, C] tensors (R = one row per cloud), a leaf module: it imports nothing from the package and runs without the HIP library.
csrc/norm_fold.hip is the one-launch version of the same arithmetic (_hip.norm_fold_train / _hip.norm_fold_bwd)."""
import torch
import torch.distributed as dist


def _syncing(sync):
    return bool(sync) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def batch_moments(s1, s2, pivot, count, sync=False):
    """Per-channel mean and biased variance from pivoted sums  s1 = sum(x - pivot), s2 = sum((x - pivot)^2)
    over `count` elements: float64 [C] with a scalar count, or [R, C] with a float64 count [R, 1] (the statistics of R clouds, never
    synchronised).  With `sync` (the reference wraps its models in
    nn.SyncBatchNorm for multi-GPU training, trainer_unsup_arti_align.py:L430) the raw moments of
    all ranks are summed by ONE all-reduce of 2C+1 doubles, so every rank normalises with the
    statistics of the whole batch.  Returns (mean, var, total_count)."""
    assert s1.dim() == 1 or not sync, 'per-cloud statistics are not synchronised'
    if not _syncing(sync):
        m = s1 / count
        return pivot + m, (s2 / count - m * m).clamp_(min=0.0), count
    raw = torch.cat([s1 + count * pivot, s2 + 2.0 * pivot * s1 + count * pivot * pivot,
                     torch.full((1,), float(count), dtype=torch.float64, device=s1.device)])
    dist.all_reduce(raw)
    c = s1.numel()
    total = raw[2 * c]
    mean = raw[:c] / total
    var = (raw[c:2 * c] / total - mean * mean).clamp_(min=0.0)
    return mean, var, total


def affine_from_moments(mean, var, weight, bias, eps):
    """BatchNorm as one per-channel map y = scale x + shift, formed in float64 from the (float64) mean and biased variance:
    -> (scale float32, shift float32, invstd float64)."""
    invstd = torch.rsqrt(var + eps)
    scale64 = weight.double() * invstd
    return scale64.float(), (bias.double() - mean * scale64).float(), invstd


def update_running_stats(running_mean, running_var, mean, var, count, momentum):
    """nn.BatchNorm2d's running statistics after a training batch of `count` elements per channel (unbiased variance).  mean / var [R, C]
    (count [R, 1] or a scalar): the R updates r <- (1 - momentum) r + momentum v_i of R batch-1 calls in row order, in closed form."""
    with torch.no_grad():
        if mean.dim() == 1:
            running_mean.mul_(1.0 - momentum).add_(mean.to(running_mean.dtype), alpha=momentum)
            running_var.mul_(1.0 - momentum).add_((var * (count / (count - 1))).to(running_var.dtype), alpha=momentum)
            return
        r = mean.shape[0]
        count = torch.as_tensor(count, dtype=torch.float64)
        unb = var * (count / (count - 1.0).clamp_min(1.0))
        keep = (1.0 - momentum) ** torch.arange(r - 1, -1, -1, device=mean.device, dtype=torch.float64).view(r, 1)
        running_mean.mul_((1.0 - momentum) ** r).add_((momentum * (keep * mean).sum(0)).to(running_mean.dtype))
        running_var.mul_((1.0 - momentum) ** r).add_((momentum * (keep * unb).sum(0)).to(running_var.dtype))


def eval_moments(running_mean, running_var, pre_bias=None):
    """The float64 (mean, var) an eval-mode norm of x + pre_bias normalises x with: the constant in front only moves the mean."""
    mean = running_mean.double()
    return (mean if pre_bias is None else mean - pre_bias.detach().double()), running_var.double()


def fold(sums, weight, beta, running_mean, running_var, training, momentum, eps, pre_bias=None, sync=False):
    """act(norm(x + pre_bias)) as y = scale x + shift.  Training: sums = (s1, s2, pivot, count) of x as batch_moments takes them; the
    running buffers (None: not tracked) are updated with the mean of x + pre_bias -- a per-channel constant in front of a BatchNorm moves
    the batch mean and nothing else.  Eval: sums = None, the running statistics.
    -> (scale float32, shift float32, mean float64 of x, invstd float64, count), shaped [C], or [R, C] from [R, C] sums."""
    count = None
    if training:
        mean, var, count = batch_moments(*sums, sync)                 # biased variance, as BatchNorm normalises with
        if running_mean is not None:
            update_running_stats(running_mean, running_var, mean if pre_bias is None else mean + pre_bias.detach().double(), var, count, momentum)
    else:
        mean, var = eval_moments(running_mean, running_var, pre_bias)
    scale, shift, invstd = affine_from_moments(mean, var, weight, beta, eps)
    return scale, shift, mean, invstd, count


def backward_coefficients(scale, sg, sgx, count, training, sync=False):
    """(k2, k3), float32 like the nodes' `scale`, of the input gradient gx = scale g - k2 - k3 xhat from the float64 sums sg = sum(g), sgx = sum(g xhat):
    scale sum / count in training mode, zeros in eval mode.  [C] sums are summed over the ranks first (SyncBatchNorm backward); [B, C] sums
    stay per cloud with a count [B, 1] and are summed over the clouds with a scalar count (whole-batch statistics)."""
    if not training:
        return torch.zeros_like(scale), torch.zeros_like(scale)
    if sg.dim() == 1:
        sg, sgx = all_reduce_sums(sg, sgx, sync=sync)
    elif not (torch.is_tensor(count) and count.dim() == 2):
        sg, sgx = sg.sum(0, keepdim=True), sgx.sum(0, keepdim=True)
    return (scale.double() * sg / count).to(scale.dtype).contiguous(), (scale.double() * sgx / count).to(scale.dtype).contiguous()


def pre_bias_grad(sg, scale, training):
    """d pre_bias [C]: exactly zero in training mode (the batch mean absorbs the constant); in eval mode it shifts the pre-activation like
    beta does, sum(g) scale (summed over the clouds of [B, C] operands)."""
    if training:
        return torch.zeros(scale.shape[-1], dtype=torch.float32, device=scale.device)
    g = sg * scale.double()
    return (g.sum(0) if g.dim() == 2 else g).float()


def all_reduce_sums(*tensors, sync=False):
    """Sum float64 per-channel reductions over the ranks (one all-reduce); identity without sync."""
    if not _syncing(sync):
        return tensors
    flat = torch.cat([t.reshape(-1) for t in tensors])
    dist.all_reduce(flat)
    out, o = [], 0
    for t in tensors:
        out.append(flat[o:o + t.numel()].view_as(t))
        o += t.numel()
    return tuple(out)
