#!/usr/bin/env python3
"""One sha256 per output of the ordering models' device paths on fixed vsrcap.synth inputs and weights: what two builds of the library
must agree on bit for bit when only their host code (or shared device code) was rearranged.

  generate        S_SSP.generate_batch: pred, logp
  ssp-train       S_SSP.forward + backward in eval() mode: the loss and every gradient of SSP_PARAM_KEYS, once without masks and once
                  with the library's masks of seed 7 (SspEngine.ssp_dropout_masks)
  sinkhorn        SinkhornNet: tr of the training forward, tr and the assignment of assign(), the ten gradients of loc_loss
  rank            evalbatch.rank_captions_device: rank, status

    python tools/ordering_digest.py [--s 1,13,64,96] [--q all|smallest] [--out FILE]

S: the sequence counts of generate and ssp-train.  The Sinkhorn cases (Q, N, n_iters, seed) are those of
tests/test_gpu_sinkhorn_train.py; `smallest` keeps the one with the smallest Q.  The rank batch is tests/test_gpu_rank_device.py's
(N = 40, MV = 3, RandomState(3)).  Prints `sha256  name` lines in a fixed order; compare two builds with diff."""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vsr-guided-cic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from vsrcap import evalbatch, synth  # noqa: E402
from vsrcap.ssp import SSP_PARAM_KEYS  # noqa: E402
from vsrcap._lib import SINKHORN_FIELDS  # noqa: E402
import ssp_train_ref  # noqa: E402  (the ground-truth orders the tests use)
from sinkhorn_train_ref import make_locs  # noqa: E402  (the location targets the tests use)

DEV = "cuda"
SINKHORN_CASES = [(1, 10, 20, 2), (13, 10, 20, 3), (70, 10, 20, 1), (5, 16, 3, 4), (4, 2, 1, 5), (3, 10, 0, 6)]
MASK_SEED = 7
LINES = []


def emit(name, t):
    h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    LINES.append("%s  %s" % (h, name))
    print(LINES[-1], flush=True)


def ssp_net():
    from models import S_SSP
    m = S_SSP()
    w = synth.make_ssp_weights(0)
    sd = m.state_dict()
    alias = {"encoder.sr_embed_layer.weight": "sr_embed_layer.weight", "decoder.embed_layer.weight": "sr_embed_layer.weight",
             "encoder.v_embed_layer.weight": "v_embed_layer.weight"}
    for k in sd:
        if alias.get(k, k) in w:
            sd[k] = torch.from_numpy(w[alias.get(k, k)])
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def sinkhorn_net(N, n_iters, seed):
    from models import SinkhornNet
    m = SinkhornNet(N, n_iters, 0.1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sinkhorn_weights(seed, N).items()})
    return m.to(DEV).train()


def ssp_sections(m, S):
    verbs, roles = synth.make_ssp_inputs(S, 1)
    gt = ssp_train_ref.make_gt(roles, 1)
    verbs, roles, gt = (torch.from_numpy(t).to(DEV) for t in (verbs, roles, gt))
    with torch.no_grad():
        pred, logp = m.generate_batch(verbs, roles)
    emit("generate S=%d pred" % S, pred)
    emit("generate S=%d logp" % S, logp)
    named = dict(m.named_parameters())
    eng = m._engine(torch.device(DEV))
    for label, masks in (("nomask", None), ("masks", eng.ssp_dropout_masks(S, MASK_SEED))):
        m.zero_grad(set_to_none=True)
        loss = m(verbs.unsqueeze(1), roles, gt, dropout_masks=masks)
        loss.backward()
        emit("ssp-train S=%d %s loss" % (S, label), loss)
        for k in SSP_PARAM_KEYS:
            emit("ssp-train S=%d %s d %s" % (S, label, k), named[k].grad)


def sinkhorn_section(Q, N, n_iters, seed):
    m = sinkhorn_net(N, n_iters, seed)
    x, n = synth.make_sinkhorn_inputs(Q, seed, N)
    tr_locs, gt_locs = make_locs(n, N, seed)
    x, tr_locs, gt_locs = (torch.from_numpy(t).to(DEV) for t in (x, tr_locs, gt_locs))
    tag = "sinkhorn Q=%d N=%d iters=%d" % (Q, N, n_iters)
    emit(tag + " train tr", m(x))
    with torch.no_grad():
        tr, assign = m.assign(x)
    emit(tag + " assign tr", tr)
    emit(tag + " assign", assign)
    m.zero_grad(set_to_none=True)
    loss = m.loc_loss(x, tr_locs, gt_locs, 0.25)
    loss.backward()
    emit(tag + " loss", loss)
    for f in SINKHORN_FIELDS:
        name, wb = f.rsplit("_", 1)
        emit("%s d %s" % (tag, f), getattr(getattr(m, name), "weight" if wb == "w" else "bias").grad)


def rank_section(ssp):
    sh = sinkhorn_net(10, 20, 0).eval()
    cv, dv, dsr, feats = synth.make_rank_batch(40, 3, 3)
    with torch.no_grad():
        rank, status = evalbatch.rank_captions_device(ssp, sh, cv, dv, dsr, torch.from_numpy(feats).to(DEV))
    emit("rank N=40 MV=3 rank", rank)
    emit("rank N=40 MV=3 status", status)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", default="1,13,64,96", help="comma-separated sequence counts of generate and ssp-train")
    ap.add_argument("--q", default="all", choices=["all", "smallest"], help="which of the Sinkhorn cases to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ssp = ssp_net()
    for S in (int(v) for v in a.s.split(",")):
        ssp_sections(ssp, S)
    cases = SINKHORN_CASES if a.q == "all" else [min(SINKHORN_CASES)]
    for c in cases:
        sinkhorn_section(*c)
    rank_section(ssp)
    torch.cuda.synchronize()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
