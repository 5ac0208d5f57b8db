#!/usr/bin/env python3
"""Time one S_SSP training step (forward + backward + Adam, .train() mode: dropout on) at S = 256 sequences, three ways:

  (a) models.S_SSP.forward: all S sequences in one call (one device forward, one hand-written backward)
  (b) the same sequences as S calls of one sequence each, the losses added under autograd and divided by S
  (c) tests/ssp_train_ref.py's oracle in fp32 under torch autograd on the same GPU, all S sequences in one batch, its 33 keep masks
      drawn with torch.rand on the device each step

    python tools/ssp_train_bench.py [--s 256] [--steps 20] [--warmup 5] [--variants abc] [--out profiles/NAME.json]

Each figure is the median over --steps steps of a device-synchronised wall time (torch.cuda.synchronize() on both sides of the step),
after --warmup untimed steps - the same two settings for all three variants; the inputs stay on the device.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vsr-guided-cic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from vsrcap import synth  # noqa: E402
import ssp_train_ref as ref  # noqa: E402  (the oracle and the ground-truth orders the tests use)

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
    ap.add_argument("--s", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", default="abc", help="which of the three to run (a kernel trace of the device path alone: --variants a)")
    a = ap.parse_args()
    from models import S_SSP
    S = a.s
    w = synth.make_ssp_weights(0)
    verbs, roles = synth.make_ssp_inputs(S, 0)
    gt = ref.make_gt(roles, 0)
    verbs, roles, gt = (torch.from_numpy(t).to(DEV) for t in (verbs, roles, gt))

    def fresh():
        m = S_SSP()
        sd = m.state_dict()
        alias = {"encoder.sr_embed_layer.weight": "sr_embed_layer.weight", "decoder.embed_layer.weight": "sr_embed_layer.weight",
                 "encoder.v_embed_layer.weight": "v_embed_layer.weight"}
        for k in sd:
            if alias.get(k, k) in w:
                sd[k] = torch.from_numpy(w[alias.get(k, k)])
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        return m, torch.optim.Adam([p for k, p in m.named_parameters() if "cross_attention" not in k], lr=1e-5)

    res = {}
    m, opt = fresh()

    def step_a():
        opt.zero_grad()
        m(verbs.unsqueeze(1), roles, gt).backward()
        opt.step()
    if "a" in a.variants:
        res["a_one_call_ms"], res["a_min_ms"] = timed(step_a, a.steps, a.warmup)

    m, opt = fresh()

    def step_b():
        opt.zero_grad()
        loss = 0.
        for i in range(S):
            loss = loss + m(verbs[i:i + 1].unsqueeze(1), roles[i:i + 1], gt[i:i + 1])
        (loss / S).backward()
        opt.step()
    if "b" in a.variants:
        res["b_per_sequence_ms"], res["b_min_ms"] = timed(step_b, a.steps, a.warmup)

    o = ref.TrainOracle({k: torch.from_numpy(v).to(DEV) for k, v in w.items()})
    used = [k for k in o.p if "cross_attention" not in k]
    for k in used:
        o.p[k] = o.p[k].clone().requires_grad_(True)
    opt_c = torch.optim.Adam([o.p[k] for k in used], lr=1e-5)
    shapes = ref.site_shapes(S)

    def step_c():
        opt_c.zero_grad()
        masks = [torch.rand(sh, device=DEV) >= ref.P_DROP for sh in shapes]
        o.run(verbs, roles, gt, masks).backward()
        opt_c.step()
    if "c" in a.variants:
        res["c_torch_autograd_ms"], res["c_min_ms"] = timed(step_c, a.steps, a.warmup)

    res.update(S=S, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count, torch=torch.__version__)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
