"""Shared by the SinkhornNet training tests and tests/golden/make_golden_sinkhorn_train.py: the location targets of
coco_scripts/train_sinkhorn.py:190-205 on synthetic items, the fp64 / fp32 oracle run of its three loss lines (:207-211), and the
summary of the four large weight gradients the fixture stores."""
import numpy as np
import torch
from torch import nn

import ssp_oracle as so

BIG = ("W1_txt.weight", "W1_vis.weight", "W2_vis.weight", "W_fc_pos.weight")      # stored as row norms, column norms and one block
BLOCK = {"W1_txt.weight": (64, 128), "W1_vis.weight": (256, 1024), "W2_vis.weight": (32, 192), "W_fc_pos.weight": (128, 240)}   # top-left corner of the 16 x 16 block


def make_locs(n_filled, N, seed):
    """tr_locs, gt_locs_ (Q, N) fp32 as train_sinkhorn.py:190-205 builds them: the item's slot positions in ascending order, padded
    with 10; the arg-sort of the ground-truth positions of those slots (a permutation), padded with 10."""
    rng = np.random.RandomState(1000 + seed)
    Q = len(n_filled)
    tr_locs = np.full((Q, N), 10.0, dtype=np.float32)
    gt_locs_ = np.full((Q, N), 10.0, dtype=np.float32)
    for q, n in enumerate(n_filled):
        n = int(n)
        tr_locs[q, :n] = np.sort(rng.choice(max(N, 10), n, replace=False))
        gt = np.full(N, 10.0)
        gt[:n] = rng.permutation(n)                       # this_idx_list[loc]
        gt_locs_[q, :n] = np.argsort(gt, kind="stable")[:n]
    return tr_locs, gt_locs_


def reference_loss(tr, tr_locs, gt_locs, scale):
    """train_sinkhorn.py:207-211 on a (Q, N, N) tr: one torch.mm and one nn.MSELoss per item, added in item order"""
    criterion = nn.MSELoss()
    loss, items = 0., []
    for q in range(tr.shape[0]):
        resort_locs = torch.mm(tr_locs[q].unsqueeze(0), tr[q]).squeeze()
        items.append(criterion(resort_locs, gt_locs[q]))
        loss = loss + items[-1]
    return loss * scale, torch.stack(items)


def oracle_run(w, seq, tr_locs, gt_locs, n_iters, tau, dtype, scale):
    """forward + the three loss lines + backward of SinkhornOracle in `dtype`; everything returned as fp64"""
    o = so.SinkhornOracle(w, n_iters=n_iters, tau=tau, dtype=dtype)
    for k in o.p:
        o.p[k] = o.p[k].clone().requires_grad_(True)
    tr = o.forward(torch.as_tensor(seq).to(dtype))
    loss, items = reference_loss(tr, torch.as_tensor(tr_locs).to(dtype), torch.as_tensor(gt_locs).to(dtype), scale)
    loss.backward()
    return dict(loss=float(loss.item()), items=items.detach().double(), tr=tr.detach().double(),
                grads={k: o.p[k].grad.detach().double() for k in o.p})


def summarise(run):
    """the tensors g16_sinkhorn_train.npz holds of one run: per-item losses, tr, the five bias gradients and W_fc.weight's in full,
    row norms / column norms / one 16 x 16 block of the four large weight gradients"""
    out = {"items": run["items"], "tr": run["tr"]}
    for k, g in run["grads"].items():
        g = torch.as_tensor(g).double()
        if k in BIG:
            r0, c0 = BLOCK[k]
            out[k + "/rows"] = g.pow(2).sum(1).sqrt()
            out[k + "/cols"] = g.pow(2).sum(0).sqrt()
            out[k + "/block"] = g[r0:r0 + 16, c0:c0 + 16].clone()
        else:
            out[k] = g
    return out
