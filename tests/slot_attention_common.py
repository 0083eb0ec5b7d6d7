"""Shared by tests/test_slot_attention_host.py, tests/test_gpu_slot_attention.py, tests/golden/make_golden_slot_attention.py and
tools/slot_attention_time.py: the fixture of the reference's SlotAttention (SPConvNets/utils/slot_attention_spec_v2.py:L6-193) unpacked,
and a batched torch restatement of the algebra the package's class runs (any dtype, any device).  The restatement is the tests'
comparator; the package does not import it.

    z[n]       = (x[n] - mean_n) rstd_n                           the same for every slot
    dots[s,n]  = z[n] . u_s + c0_s       u_s = scale g_s o (Wk_s^T q_s),   c0_s = scale q_s . (Wk_s beta_s + bk_s)
    updates_s  = Wv_s (g_s o m_s + beta_s) + bv_s,      m_s = sum_n attn_ori[s,n] z[n] / sum_n attn_ori[s,n]
"""
import numpy as np
import torch
import torch.nn.functional as F

# the bars of tests/inv_slot_common.py: outputs, input gradient, parameter gradients, each relative to the largest reference value
BAR_OUT, BAR_DX, BAR_DPARAM = 2e-5, 5e-5, 1e-4

# tag -> (B, N, d, S, hidden); iters = 3, eps = 1e-8.  d = 131 = 128 + 3 is the orbit_attn == 3 width.
VARIANTS = {'small': (2, 37, 20, 3, 16), 'orbit3': (1, 130, 131, 2, 128)}
ITERS, EPS, LN_EPS = 3, 1e-8, 1e-5
FIXTURE = 'slot_attention.npz'


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def load_fixture(golden):
    """the fixture's volumes (slot_attention.npz names how many follow as slot_attention.part<k>.npz: no file above 1 MiB) as one dict"""
    G = dict(golden(FIXTURE))
    for k in range(1, int(G['volumes'])):
        G.update(golden(FIXTURE.replace('.npz', f'.part{k}.npz')))
    return G


def state_of(G, tag):
    pre = f'{tag}_state_'
    return {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in G.items() if k.startswith(pre)}


def param_names(state):
    return list(state.keys())                  # the reference class has no buffers: every entry of the state is a parameter


def functional(slots, attn, w):
    """the seeded linear-plus-quadratic functional of (slots, attn_ori); w = (a_slots, q_slots, a_attn, q_attn)"""
    a_s, q_s, a_a, q_a = w
    return (a_s * slots).sum() + 0.5 * (q_s * slots * slots).sum() + (a_a * attn).sum() + 0.5 * (q_a * attn * attn).sum()


def functional_weights(G, tag, dtype=torch.float64, device='cpu'):
    return tuple(torch.from_numpy(np.asarray(G[f'{tag}_{k}'])).to(device=device, dtype=dtype) for k in ('a_slots', 'q_slots', 'a_attn', 'q_attn'))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def _stack(P, fmt, S):
    return torch.stack([P[fmt.format(i)] for i in range(S)])


def _per_slot_linear(W, b, t):
    """W [S,o,i], b [S,o], t [B,S,i] -> [B,S,o]"""
    return torch.einsum('soi,bsi->bso', W, t) + b


def _per_slot_norm(P, name, S, t):
    return F.layer_norm(t, t.shape[-1:], eps=LN_EPS) * _stack(P, name + '.{}.weight', S) + _stack(P, name + '.{}.bias', S)


def restated_forward(P, x, noise, S, iters=ITERS, eps=EPS):
    """P: name -> tensor (the reference's state names), x [B,N,d], noise [B,S,d] -> slots [B,S,d], attn_ori [B,S,N]"""
    d = x.shape[-1]
    scale = d ** -0.5
    g, beta = _stack(P, 'norm_input.{}.weight', S), _stack(P, 'norm_input.{}.bias', S)
    Wk, bk = _stack(P, 'to_k.{}.weight', S), _stack(P, 'to_k.{}.bias', S)
    Wv, bv = _stack(P, 'to_v.{}.weight', S), _stack(P, 'to_v.{}.bias', S)
    Wq, bq = _stack(P, 'to_q.{}.weight', S), _stack(P, 'to_q.{}.bias', S)
    Wih, Whh = _stack(P, 'gru.{}.weight_ih', S), _stack(P, 'gru.{}.weight_hh', S)
    bih, bhh = _stack(P, 'gru.{}.bias_ih', S), _stack(P, 'gru.{}.bias_hh', S)
    W1, b1 = _stack(P, 'mlp.{}.0.weight', S), _stack(P, 'mlp.{}.0.bias', S)
    W2, b2 = _stack(P, 'mlp.{}.2.weight', S), _stack(P, 'mlp.{}.2.bias', S)
    z = F.layer_norm(x, (d,), eps=LN_EPS)                                             # [B,N,d], no affine
    k_const = torch.einsum('sij,sj->si', Wk, beta) + bk
    slots = P['slots_mu'] + P['slots_logsigma'].exp() * noise
    attn = None
    for _ in range(iters):
        prev = slots
        q = _per_slot_linear(Wq, bq, _per_slot_norm(P, 'norm_slots', S, slots))
        u = scale * g * torch.einsum('sij,bsi->bsj', Wk, q)
        c0 = scale * (q * k_const).sum(-1)
        attn = (torch.einsum('bnd,bsd->bsn', z, u) + c0.unsqueeze(-1)).softmax(dim=1) + eps
        m = torch.einsum('bsn,bnd->bsd', attn, z) / attn.sum(-1, keepdim=True)
        updates = _per_slot_linear(Wv, bv, g * m + beta)
        i_r, i_z, i_n = _per_slot_linear(Wih, bih, updates).chunk(3, -1)             # nn.GRUCell
        h_r, h_z, h_n = _per_slot_linear(Whh, bhh, prev).chunk(3, -1)
        r, zg = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        cand = torch.tanh(i_n + r * h_n)
        slots = (1 - zg) * cand + zg * prev
        hidden = torch.relu(_per_slot_linear(W1, b1, _per_slot_norm(P, 'norm_pre_ff', S, slots)))
        slots = slots + _per_slot_linear(W2, b2, hidden)
    return slots, attn


def restated_run(state, x, noise, S, w, dtype, device='cpu'):
    """forward and the gradients of the functional -> slots, attn, dx, {name: gradient}"""
    P = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in state.items()}
    x = x.to(device=device, dtype=dtype).requires_grad_(True)
    slots, attn = restated_forward(P, x, noise.to(device=device, dtype=dtype), S)
    names = list(P)
    grads = torch.autograd.grad(functional(slots, attn, tuple(t.to(device=device, dtype=dtype) for t in w)), [x] + [P[k] for k in names])
    return slots.detach(), attn.detach(), grads[0], dict(zip(names, grads[1:]))


# ---- the five entries as torch expressions (any dtype): x [b,d,n], mean / rstd [b,n] ------------------------------------------------

def _z(x, mean, rstd):
    return (x - mean.unsqueeze(1)) * rstd.unsqueeze(1)


def ref_stats(x, ln_eps=LN_EPS):
    mean = x.mean(1)
    return mean, 1.0 / torch.sqrt(((x - mean.unsqueeze(1)) ** 2).mean(1) + ln_eps)


def ref_scores_fwd(x, mean, rstd, u, c0, eps=EPS):
    return (torch.einsum('bsd,bdn->bsn', u, _z(x, mean, rstd)) + c0.unsqueeze(-1)).softmax(dim=1) + eps


def ref_pool(x, mean, rstd, w):
    return torch.einsum('bsn,bdn->bsd', w, _z(x, mean, rstd)), w.sum(-1)


def ref_scores_bwd(x, mean, rstd, attn, gmsum, gwsum, gattn, eps=EPS):
    ga = torch.einsum('bsd,bdn->bsn', gmsum, _z(x, mean, rstd)) + gwsum.unsqueeze(-1)
    if gattn is not None:
        ga = ga + gattn
    p = attn - eps
    return p * (ga - (p * ga).sum(1, keepdim=True))


def ref_input_grad(x, mean, rstd, rows, vecs):
    z = _z(x, mean, rstd)
    gz = torch.einsum('bjn,bjd->bdn', rows, vecs)
    return rstd.unsqueeze(1) * (gz - gz.mean(1, keepdim=True) - z * (gz * z).mean(1, keepdim=True))
