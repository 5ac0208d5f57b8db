#!/usr/bin/env python3
"""Golden vectors of SinkhornNet TRAINING from the REAL reference (build container only):

    python tests/golden/make_golden_sinkhorn_train.py            # writes tests/golden/g16_sinkhorn_train.npz

The reference's SinkhornNet (models/sinkhorn_network.py) in fp64 on closed-form weights and inputs (vsrcap.synth), called one item
at a time as coco_scripts/train_sinkhorn.py:207 does, its three loss lines (:207-209, :211) and backward().  The fixture holds
results only: per-item losses, tr, the gradients of the five biases and of W_fc.weight in full, and of the four large weights their
row norms, column norms and one fixed 16 x 16 block (tests/sinkhorn_train_ref.py: summarise)."""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(os.path.join(ROOT, "vsr-guided-cic_amd"))

from vsrcap import synth  # noqa: E402
import sinkhorn_train_ref as ref  # noqa: E402


def reference_run(Q, seed, scale):
    from models.sinkhorn_network import SinkhornNet
    net = SinkhornNet(10, 20, 0.1)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sinkhorn_weights(seed).items()})
    net = net.double().train()
    x, n = synth.make_sinkhorn_inputs(Q, seed)
    tr_locs, gt_locs_ = ref.make_locs(n, 10, seed)
    x, tr_locs, gt_locs_ = torch.from_numpy(x).double(), torch.from_numpy(tr_locs).double(), torch.from_numpy(gt_locs_).double()
    criterion = nn.MSELoss()
    loss, items, trs = 0., [], []
    for q in range(Q):
        tr_matrix = net(x[q].unsqueeze(0)).squeeze()                                   # train_sinkhorn.py:207
        resort_locs = torch.mm(tr_locs[q].unsqueeze(0), tr_matrix).squeeze()           # :208
        items.append(criterion(resort_locs, gt_locs_[q]))                              # :209
        loss += items[-1]
        trs.append(tr_matrix)
    loss = loss * scale                                                                # :211 (1 / batch size)
    loss.backward()
    return dict(loss=float(loss.item()), items=torch.stack(items).detach(), tr=torch.stack(trs).detach(),
                grads={k: p.grad.detach() for k, p in net.named_parameters()})


def main():
    Q, seed, scale = 6, 0, 0.25
    run = reference_run(Q, seed, scale)
    s = ref.summarise(run)
    path = os.path.join(HERE, "g16_sinkhorn_train.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(dict(Q=Q, seed=seed, scale=scale, N=10, n_iters=20, tau=0.1, loss=run["loss"]))),
                        **{k.replace("/", "__"): v.numpy().astype(np.float64) for k, v in s.items()})
    print("wrote %s (%.1f KB), loss %.6f" % (path, os.path.getsize(path) / 1024, run["loss"]))


if __name__ == "__main__":
    main()
