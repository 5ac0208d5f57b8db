"""fp64 Adam on the CPU: the reference the optimizer tests hold vsrcap.optim.Adam (and, for the bound, torch's fused kernel) to.
torch.optim.Adam semantics, amsgrad = maximize = False, L2 weight decay.  tests/test_optim_logic.py checks it against torch's own
float64 optimizer."""
import math

import torch


def adam_step_fp64(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """one step on float64 tensors (g None: nothing moves) -> (p, m, v), new tensors"""
    if g is None:
        return p, m, v
    b1, b2 = betas
    if weight_decay:
        g = g + weight_decay * p
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def run_fp64(params, grads_per_step, lrs, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """params: dict name -> fp32 tensor; grads_per_step: list of dicts name -> fp32 tensor or None; lrs: the lr of each step.
    -> list, one entry per step, of dict name -> (p, exp_avg, exp_avg_sq) in float64.  A tensor's own step count advances only when it
    has a gradient (torch's rule)."""
    st = {k: (p.detach().cpu().double(), torch.zeros_like(p, dtype=torch.float64, device="cpu"), torch.zeros_like(p, dtype=torch.float64, device="cpu"), 0)
          for k, p in params.items()}
    out = []
    for grads, lr in zip(grads_per_step, lrs):
        for k, (p, m, v, n) in st.items():
            g = grads.get(k)
            if g is None:
                continue
            p, m, v = adam_step_fp64(p, g.detach().cpu().double(), m, v, n + 1, lr, betas, eps, weight_decay)
            st[k] = (p, m, v, n + 1)
        out.append({k: s[:3] for k, s in st.items()})
    return out
