#!/usr/bin/env python3
"""Time one SinkhornNet training step (forward + location loss + backward + Adam) at Q = 256 items, N = 10, three ways:

  (a) models.SinkhornNet.loc_loss: all Q items in one call (one forward, one fused loss, one hand-written backward)
  (b) the same items as Q calls of one item each through forward(), with torch.mm / nn.MSELoss per item and the losses added on the
      host side of autograd - the call pattern of coco_scripts/train_sinkhorn.py:189-215
  (c) oracle/ssp_oracle.py's SinkhornOracle under torch autograd on the same GPU, all Q items in one batch

    python tools/sinkhorn_train_bench.py [--q 256] [--steps 20] [--warmup 5] [--variants abc] [--out profiles/NAME.json]

Each figure is the median over --steps steps of a device-synchronised wall time (torch.cuda.synchronize() on both sides of the step),
after --warmup untimed steps - the same two settings for all three variants; the inputs stay on the device.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vsr-guided-cic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from vsrcap import synth  # noqa: E402
import ssp_oracle as so  # noqa: E402
from sinkhorn_train_ref import make_locs  # noqa: E402  (the location targets the tests use)

DEV = "cuda"


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", default="abc", help="which of the three to run (the device path alone: --variants a)")
    a = ap.parse_args()
    from models import SinkhornNet
    N, Q, scale = 10, a.q, 1.0 / 16
    w = synth.make_sinkhorn_weights(0, N)
    x, n = synth.make_sinkhorn_inputs(Q, 0, N)
    tr_locs, gt_locs = make_locs(n, N, 0)
    x, tr_locs, gt_locs = (torch.from_numpy(t).to(DEV) for t in (x, tr_locs, gt_locs))
    criterion = nn.MSELoss()

    def fresh():
        m = SinkhornNet(N, 20, 0.1)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        m = m.to(DEV).train()
        return m, torch.optim.Adam(m.parameters(), lr=1e-4)

    res = {}
    m, opt = fresh()

    def step_a():
        opt.zero_grad()
        loss = m.loc_loss(x, tr_locs, gt_locs, scale)
        loss.backward()
        opt.step()
    if "a" in a.variants:
        res["a_one_call_ms"], res["a_min_ms"] = timed(step_a, a.steps, a.warmup)

    m, opt = fresh()

    def step_b():
        opt.zero_grad()
        loss = 0.
        for q in range(Q):
            tr = m(x[q].unsqueeze(0)).squeeze()
            loss += criterion(torch.mm(tr_locs[q].unsqueeze(0), tr).squeeze(), gt_locs[q])
        loss = loss * scale
        loss.backward()
        opt.step()
    if "b" in a.variants:
        res["b_per_item_ms"], res["b_min_ms"] = timed(step_b, a.steps, a.warmup)

    o = so.SinkhornOracle({k: torch.from_numpy(v).to(DEV) for k, v in w.items()})
    for k in o.p:
        o.p[k] = o.p[k].clone().requires_grad_(True)
    opt_c = torch.optim.Adam(list(o.p.values()), lr=1e-4)

    def step_c():
        opt_c.zero_grad()
        tr = o.forward(x)
        resort = torch.bmm(tr_locs.unsqueeze(1), tr).squeeze(1)
        loss = ((resort - gt_locs) ** 2).mean(1).sum() * scale
        loss.backward()
        opt_c.step()
    if "c" in a.variants:
        res["c_torch_autograd_ms"], res["c_min_ms"] = timed(step_c, a.steps, a.warmup)

    res.update(Q=Q, N=N, n_iters=20, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count, torch=torch.__version__)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
