#!/usr/bin/env python3
"""Golden vectors of S_SSP TRAINING from the REAL reference (build container only):

    python tests/golden/make_golden_ssp_train.py            # writes tests/golden/g17_ssp_train.npz

The reference's S_SSP (models/sort_model.py) in fp64 on closed-form weights and inputs (vsrcap.synth, tests/ssp_train_ref.py:
make_gt), called as coco_scripts/train_region_sort.py:181 calls it, and backward():
  run a  .eval(): no dropout
  run b  .train() with nn.Dropout.forward replaced, for the run, by a function that applies the hashed keep masks of
         ssp_train_ref.hash_masks in CALL ORDER and records the shapes it sees - exactly 33 calls with the shapes of
         ssp_train_ref.site_shapes, which pins the site table to the reference
The fixture holds results only: the loss and, per gradient tensor, its L2 norm and 32 hashed positions (ssp_train_ref.summarise,
packed into one array per run by ssp_train_ref.pack)."""
import json
import os
import sys
import tempfile

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
import ssp_train_ref as ref  # noqa: E402


def _reference_model(seed):
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "datasets/coco"))
    for n in ("verb_2_vob_all_refine.json", "verb_2_vob.json"):          # read by the package's import, not by S_SSP
        json.dump({}, open(os.path.join(tmp, "datasets/coco", n), "w"))
    os.chdir(tmp)
    try:
        from models.sort_model import S_SSP
    finally:
        os.chdir(cwd)
    net = S_SSP()
    w = synth.make_ssp_weights(seed)
    sd = net.state_dict()
    for k in sd:                                     # shared embeddings appear under several keys (encoder.*, decoder.*)
        key = k
        if k.startswith("encoder.sr_embed_layer.") or k.startswith("decoder.embed_layer."):
            key = "sr_embed_layer." + k.split(".")[-1]
        if k.startswith("encoder.v_embed_layer."):
            key = "v_embed_layer." + k.split(".")[-1]
        if key in w:
            sd[k] = torch.from_numpy(w[key])
    net.load_state_dict(sd)
    return net.double()


def reference_run(S, seed, masks=None):
    """one S_SSP.forward + backward of the reference in fp64; masks: None -> .eval(), else .train() on the 33 injected keep arrays"""
    net = _reference_model(seed)
    verbs, roles = synth.make_ssp_inputs(S, seed)
    gt = ref.make_gt(roles, seed)
    args = (torch.from_numpy(verbs).unsqueeze(1), torch.from_numpy(roles), torch.from_numpy(gt))     # (S,1), (S,10), (S,10)
    if masks is None:
        loss = net.eval()(*args)
    else:
        seen = []

        def injected(self, x):
            seen.append(tuple(x.shape))
            return ref.apply_keep(x, torch.from_numpy(masks[len(seen) - 1]))
        real = nn.Dropout.forward
        nn.Dropout.forward = injected
        try:
            loss = net.train()(*args)
        finally:
            nn.Dropout.forward = real
        assert seen == ref.site_shapes(S), "the reference's dropout calls are not the 33 sites of the table"
    loss.backward()
    return dict(loss=float(loss.item()), grads={k: p.grad.detach() for k, p in net.named_parameters() if p.grad is not None})


def main():
    S, seed = 24, 0
    runs = {"a": reference_run(S, seed), "b": reference_run(S, seed, ref.hash_masks(S, seed))}
    names = sorted(runs["a"]["grads"])
    assert names == sorted(runs["b"]["grads"])
    arrays = {tag: ref.pack(ref.summarise(run), names) for tag, run in runs.items()}
    path = os.path.join(HERE, "g17_ssp_train.npz")
    meta = dict(S=S, seed=seed, p=ref.P_DROP, names=names, loss_a=runs["a"]["loss"], loss_b=runs["b"]["loss"])
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote %s (%.1f KB), loss eval %.6f, loss with masks %.6f, %d gradients" % (path, os.path.getsize(path) / 1024, runs["a"]["loss"], runs["b"]["loss"], len(names)))


if __name__ == "__main__":
    main()
