#!/usr/bin/env python3
"""Time the step in front of the ordering models' two training calls - building the batch from the loader's integer annotations - at
N = 80 caption rows, L = 10, MV = 3, annotations as host arrays (as a DataLoader hands them over), feature rows on the device:

  (a) the numpy yardsticks of vsrcap.trainbatch (the reference's loops as a port would write them), the upload of their tables and, for
      the Sinkhorn items, a torch gather of the feature rows
  (b) vsrcap.trainbatch.build_device (two launches, one 16-byte read-back, vsr_gather_rows)
  (c) a whole training step (batch building + forward + backward + Adam; S_SSP in .train() mode) of S_SSP and of SinkhornNet, fed by (a)
      and fed by (b)

    python tools/train_batch_bench.py [--n 80] [--mv 3] [--steps 20] [--warmup 5] [--out profiles/NAME.json]

Each figure is the median over --steps repetitions of a device-synchronised wall time (torch.cuda.synchronize() on both sides), after
--warmup untimed ones - the same two settings for every variant.  There is no threshold: the values are what they are.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vsr-guided-cic_amd"))

from vsrcap import synth, trainbatch as tb  # noqa: E402

DEV = "cuda"
L = tb.L


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
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80)
    ap.add_argument("--mv", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=16, help="images of the loader batch: the divisor of the Sinkhorn loss")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from models import S_SSP, SinkhornNet
    N = a.n
    cv, dv, dsr, feats = synth.make_rank_batch(N, a.mv, 3)
    rng = np.random.RandomState(3)
    idx = np.stack([rng.permutation(L) for _ in range(N)])
    gv, gsr = np.zeros_like(dv), np.zeros_like(dsr)
    for n in range(N):
        gv[n, idx[n]], gsr[n, idx[n]] = dv[n], dsr[n]
    feats = torch.from_numpy(feats).to(DEV)
    rows = feats.reshape(N * L, -1)

    w = synth.make_ssp_weights(0)
    ssp = S_SSP()
    sd = ssp.state_dict()
    alias = {"encoder.sr_embed_layer.weight": "sr_embed_layer.weight", "decoder.embed_layer.weight": "sr_embed_layer.weight",
             "encoder.v_embed_layer.weight": "v_embed_layer.weight"}
    for k in sd:
        if alias.get(k, k) in w:
            sd[k] = torch.from_numpy(w[alias.get(k, k)])
    ssp.load_state_dict(sd)
    ssp = ssp.to(DEV).train()
    n_verbs = ssp.v_embed_layer.weight.shape[0]
    opt_ssp = torch.optim.Adam([p for k, p in ssp.named_parameters() if "cross_attention" not in k], lr=1e-5)
    sh = SinkhornNet(10, 20, 0.1)
    sh.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sinkhorn_weights(0).items()})
    sh = sh.to(DEV).train()
    opt_sh = torch.optim.Adam(sh.parameters(), lr=1e-5)

    def host_ssp():
        verbs, det, gt = tb.ssp_train_batch(cv, dv, dsr, gv, gsr)
        return tuple(torch.from_numpy(x).to(DEV, non_blocking=True) for x in (verbs[:, None], det, gt))

    def host_sinkhorn():
        gather, tr, gl, _ = tb.sinkhorn_train_items(cv, dv, dsr, idx, 10)
        g, tr, gl = (torch.from_numpy(x).to(DEV, non_blocking=True) for x in (gather, tr, gl))
        return (rows[g.clamp(min=0)] * (g >= 0).unsqueeze(-1)).contiguous(), tr, gl

    def dev_both():
        return tb.build_device(DEV, cv, dv, dsr, gv, gsr, idx, feats, n_verbs=n_verbs)

    def dev_ssp():
        return tb.build_device(DEV, cv, dv, dsr, gv, gsr, n_verbs=n_verbs)

    def dev_sinkhorn():
        return tb.build_device(DEV, cv, dv, dsr, idx_list=idx, seqs_perm=feats, n_verbs=n_verbs)

    def ssp_step(batch):
        def step():
            opt_ssp.zero_grad()
            ssp(*batch()).backward()
            opt_ssp.step()
        return step

    def sinkhorn_step(items):
        def step():
            opt_sh.zero_grad()
            sh.loc_loss(*items(), scale=1.0 / a.batch_size).backward()
            opt_sh.step()
        return step

    b = dev_both()
    res = dict(N=N, L=L, MV=a.mv, S=b.n_seqs, Q=b.n_items)
    for name, fn in (("a_host_ssp_ms", host_ssp), ("a_host_sinkhorn_ms", host_sinkhorn), ("a_host_both_ms", lambda: (host_ssp(), host_sinkhorn())),
                     ("b_device_ssp_ms", dev_ssp), ("b_device_sinkhorn_ms", dev_sinkhorn), ("b_device_both_ms", dev_both),
                     ("c_ssp_step_from_host_ms", ssp_step(host_ssp)),
                     ("c_ssp_step_from_device_ms", ssp_step(lambda: (lambda t: (t.verbs, t.det_roles, t.gt_roles))(dev_ssp()))),
                     ("c_sinkhorn_step_from_host_ms", sinkhorn_step(host_sinkhorn)),
                     ("c_sinkhorn_step_from_device_ms", sinkhorn_step(lambda: (lambda t: (t.seq, t.tr_locs, t.gt_locs))(dev_sinkhorn())))):
        res[name], res[name.replace("_ms", "_min_ms")] = timed(fn, a.steps, a.warmup)
    res.update(steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
               torch=torch.__version__)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
