"""SlotAttention, the model's segmentation step (SPConvNets/utils/slot_attention_spec_v2.py:L6-193, built at
SPConvNets/models/unsup_seg_so3_pose_conv_pn_38_multi_stage.py:L142 and called at L621), on csrc/slot_attention.hip.

The reference normalises the [B,N,d] input once per slot (L149), writes keys and values as [B,S,N,d] tensors (L153-154) and reads both
again in every iteration (L167, L175).  All of that is linear in z[n] = (x[n] - mean_n) rstd_n, the same for every slot:

    dots[s,n] = z[n] . u_s + c0_s          u_s = scale g_s o (Wk_s^T q_s),   c0_s = scale q_s . (Wk_s beta_s + bk_s)
    updates_s = Wv_s (g_s o m_s + beta_s) + bv_s,       m_s = sum_n attn_ori[s,n] z[n] / sum_n attn_ori[s,n]

(g_s, beta_s: norm_input[s]'s weight and bias), so an iteration is two passes over x on the device -- scores, pool -- and a handful of
[B,S,d] operations, which stay torch layers as the heads' regressors do.  No tensor of B S N d elements exists."""
import torch
from torch import nn
from torch.nn import init

from vgtk import _hip

MAX_KERNEL_SLOTS = 8           # csrc/slot_attention.hip MAXS; more slots run the same algebra as device tensor ops


class _AttendStep(torch.autograd.Function):
    """x [B,d,N], mean, rstd [B,N] (data), u [B,S,d], c0 [B,S] -> attn_ori [B,S,N], msum [B,S,d] = sum_n attn_ori z, wsum [B,S] = sum_n attn_ori
    (slot_attention_spec_v2.py:L167-175).  The gradient reaches x (through z and its statistics), u and c0."""

    @staticmethod
    def forward(ctx, x, mean, rstd, u, c0, eps):
        attn = _hip.slot_attn_scores_fwd(x, mean, rstd, u, c0, eps)
        msum, wsum = _hip.slot_attn_pool(x, mean, rstd, attn)
        ctx.eps = eps
        ctx.set_materialize_grads(False)
        if any(ctx.needs_input_grad):                      # x, mean, rstd by reference; attn is an output
            ctx.save_for_backward(x, mean, rstd, attn, u)
        return attn, msum, wsum

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_attn, g_msum, g_wsum):
        x, mean, rstd, attn, u = ctx.saved_tensors
        g_msum = torch.zeros_like(u) if g_msum is None else g_msum.contiguous()
        g_wsum = attn.new_zeros(attn.shape[:2]) if g_wsum is None else g_wsum.contiguous()
        g_attn = None if g_attn is None else g_attn.contiguous()
        gdots = _hip.slot_attn_scores_bwd(x, mean, rstd, attn, g_msum, g_wsum, g_attn, ctx.eps)
        du, dc0 = _hip.slot_attn_pool(x, mean, rstd, gdots)
        gx = None
        if ctx.needs_input_grad[0]:                        # gz[n] = sum_s attn[s,n] g_msum_s + gdots[s,n] u_s
            gx = _hip.slot_attn_input_grad(x, mean, rstd, torch.cat([attn, gdots], 1), torch.cat([g_msum, u], 1))
        return gx, None, None, du, dc0, None


def _attend_tensor_ops(x, ln_eps, u, c0, eps):
    """_AttendStep (with its statistics) as device tensor ops, for more slots than a launch takes"""
    mean = x.mean(1, keepdim=True)
    z = (x - mean) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + ln_eps)
    attn = (torch.einsum('bsd,bdn->bsn', u, z) + c0.unsqueeze(-1)).softmax(dim=1) + eps
    return attn, torch.einsum('bsn,bdn->bsd', attn, z), attn.sum(-1)


class SlotAttention(nn.Module):
    """The reference class: its constructor, its parameter names (a reference checkpoint loads with strict=True) and its results.
    Float32 device tensors only (no CPU path); the per-slot norm_input modules must share one eps."""

    def __init__(self, num_slots, dim, iters=3, eps=1e-8, hidden_dim=128):
        super().__init__()
        self.num_slots = num_slots
        self.iters = iters
        self.eps = eps
        self.scale = dim ** -0.5
        self.slots_mu = nn.Parameter(torch.randn(1, num_slots, dim))
        self.slots_logsigma = nn.Parameter(torch.zeros(1, num_slots, dim))
        init.xavier_uniform_(self.slots_logsigma)
        per_slot = lambda make: nn.ModuleList([make() for _ in range(num_slots)])
        self.to_q = per_slot(lambda: nn.Linear(dim, dim))
        self.to_k = per_slot(lambda: nn.Linear(dim, dim))
        self.to_v = per_slot(lambda: nn.Linear(dim, dim))
        self.gru = per_slot(lambda: nn.GRUCell(dim, dim))
        hidden_dim = max(dim, hidden_dim)
        self.mlp = per_slot(lambda: nn.Sequential(nn.Linear(dim, hidden_dim), nn.ReLU(inplace=True), nn.Linear(hidden_dim, dim)))
        self.norm_input = per_slot(lambda: nn.LayerNorm(dim))
        self.norm_slots = per_slot(lambda: nn.LayerNorm(dim))
        self.norm_pre_ff = per_slot(lambda: nn.LayerNorm(dim))

    @staticmethod
    def _per_slot(mods, *feats):
        """mods[s](f[:, s] for f in feats), stacked on the slot axis (apply_to_q, apply_gru, apply_layer_norm_slot_feats: L94-130)"""
        return torch.stack([mod(*(f[:, i] for f in feats)) for i, mod in enumerate(mods)], 1)

    def forward(self, inputs, num_slots=None, *, noise=None):
        """inputs [B,N,d] -> slots [B,S,d], attn_ori [B,S,N] (softmax over the slots + eps, of the last iteration).

        The kernels read channel-major storage: a transposed view of a contiguous [B,d,N] tensor (what InvPPOutBlockOurs returns and
        the model hands over as `ppinv_out.transpose(1, 2)`) is used in place; a point-major contiguous [B,N,d] tensor costs one
        transposing copy.  noise [B,S,d] replaces the reference's torch.randn draw (L146); None draws on the device as it does."""
        assert num_slots is None
        if not inputs.is_cuda or inputs.dtype != torch.float32:
            raise RuntimeError('SlotAttention: float32 device tensors only (there is no CPU path)')
        b, n, d = inputs.shape
        n_s = self.num_slots
        ln_eps = {m.eps for m in self.norm_input}
        if len(ln_eps) != 1:
            raise RuntimeError('SlotAttention: the per-slot norm_input modules must share one eps')
        ln_eps = ln_eps.pop()
        mu = self.slots_mu.expand(b, n_s, -1)
        sigma = self.slots_logsigma.exp().expand(b, n_s, -1)
        slots = mu + sigma * (torch.randn(mu.shape, device=inputs.device) if noise is None else noise)
        x = inputs.transpose(1, 2)
        if not x.is_contiguous():
            x = x.contiguous()
        fused = n_s <= MAX_KERNEL_SLOTS
        if fused:
            mean, rstd = _hip.slot_attn_stats(x.detach(), ln_eps)
        g = torch.stack([m.weight for m in self.norm_input])                       # [S, d]
        beta = torch.stack([m.bias for m in self.norm_input])
        Wk = torch.stack([m.weight for m in self.to_k])                            # [S, d, d]
        Wv = torch.stack([m.weight for m in self.to_v])
        bv = torch.stack([m.bias for m in self.to_v])
        k_const = torch.einsum('sij,sj->si', Wk, beta) + torch.stack([m.bias for m in self.to_k])      # Wk_s beta_s + bk_s
        for _ in range(self.iters):
            slots_prev = slots
            q = self._per_slot(self.to_q, self._per_slot(self.norm_slots, slots))
            u = (self.scale * g) * torch.einsum('sij,bsi->bsj', Wk, q)
            c0 = self.scale * (q * k_const).sum(-1)
            if fused:
                attn_ori, msum, wsum = _AttendStep.apply(x, mean, rstd, u.contiguous(), c0.contiguous(), self.eps)
            else:
                attn_ori, msum, wsum = _attend_tensor_ops(x, ln_eps, u, c0, self.eps)
            m = msum / wsum.unsqueeze(-1)
            updates = torch.einsum('sij,bsj->bsi', Wv, g * m + beta) + bv
            slots = self._per_slot(self.gru, updates, slots_prev)
            slots = slots + self._per_slot(self.mlp, self._per_slot(self.norm_pre_ff, slots))
        return slots, attn_ori
