#!/usr/bin/env python3
"""Time the eval loop's caption ranking (eval_coco.py:141-221) for one loader batch of N = 80 caption rows (16 images x 5), L = 10 slots,
MV = 3 verb columns, three ways:

  (a) vsrcap.evalbatch.rank_captions: integer bookkeeping on the host, one S-SSP and one Sinkhorn call with a read-back each
  (b) vsrcap.evalbatch.rank_captions_device: one stream of launches, nothing read back - at the default max_items (the static maximum
      N * MV * 10 items) and, as b_bound, with max_items = the batch's item count (what a caller who knows its data passes)
  (c) each of them followed by the slot re-ordering and model.beam_search_v (beam 5) at the eval caller's shapes (100 detections x 2048,
      10 slots x 20 regions, index-list regions), with set_valid_rows_bound set: c_host = rank_captions + beam_search_v_indexed,
      c_device = beam_search_v_ranked (default max_items), c_device_bound = the same with the item count as the bound

    python tools/rank_bench.py [--n 80] [--mv 3] [--steps 20] [--warmup 5] [--variants abc] [--b-mode both] [--out profiles/NAME.json]

Each figure is the median over --steps repetitions of a device-synchronised wall time (torch.cuda.synchronize() on both sides), after
--warmup untimed repetitions; the annotations are host arrays (as the loader delivers them) in every variant, the features stay on the
device.  The batch is the generator of tests/test_gpu_rank_device.py (RandomState(3)).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vsr-guided-cic_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

from vsrcap import evalbatch, synth  # noqa: E402

DEV = "cuda"
L = 10


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


make_batch = synth.make_rank_batch          # the generator of tests/test_gpu_ssp.py's rank_captions test, kept in one place


def models():
    from models import S_SSP, SinkhornNet
    w = synth.make_ssp_weights(0)
    m = S_SSP()
    sd = m.state_dict()
    alias = {"encoder.sr_embed_layer.weight": "sr_embed_layer.weight", "decoder.embed_layer.weight": "sr_embed_layer.weight",
             "encoder.v_embed_layer.weight": "v_embed_layer.weight"}
    for k in sd:
        if alias.get(k, k) in w:
            sd[k] = torch.from_numpy(w[alias.get(k, k)])
    m.load_state_dict(sd)
    sh = SinkhornNet(10, 20, 0.1)
    sh.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sinkhorn_weights(0).items()})
    return m.to(DEV).eval(), sh.to(DEV).eval()


def captioner(nv):
    from models import ControllableCaptioningModel
    c = dict(V=10000, D=2048, E=1000, H=1000, A=512, T=20)
    w = synth.make_weights(c["V"], c["D"], c["E"], c["H"], c["A"], seed=0)
    m = ControllableCaptioningModel(c["T"], c["V"], 2, det_feat_size=c["D"], input_encoding_size=c["E"], rnn_size=c["H"], att_size=c["A"],
                                    verb_2_vob_all=synth.make_verb_table(nv, c["V"], seed=0))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.to(DEV).eval(), c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80, help="caption rows (a multiple of 5: five captions per image)")
    ap.add_argument("--mv", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", default="abc", help="which to run (a kernel trace of the device path alone: --variants b)")
    ap.add_argument("--b-mode", default="both", choices=["both", "default", "bound"], help="variant (b): which max_items to time")
    a = ap.parse_args()
    N, MV = a.n, a.mv
    ssp, sh = models()
    cv, dv, dsr, feats = make_batch(N, MV, 3)
    feats = torch.from_numpy(feats).to(DEV)
    with torch.no_grad():
        host_ranks = evalbatch.rank_captions(ssp, sh, cv, dv, dsr, feats)
        rank, status = evalbatch.rank_captions_device(ssp, sh, cv, dv, dsr, feats)
    n_items = int(ssp._engine(torch.device(DEV)).rank_plan(cv, dv, dsr)[3].ge(0).any(1).sum())       # (outside the timed region: it reads back)
    same = sum([int(x) for x in row if x >= 0] == hr[:L] for row, hr in zip(rank.cpu().numpy(), host_ranks))
    res = dict(N=N, L=L, MV=MV, job_slots=N * MV, items=n_items, default_max_items=N * MV * 10, status_nonzero=int((status != 0).sum()),
               captions_ranked_like_the_host_path=same)

    def no_grad(f):
        def g():
            with torch.no_grad():
                return f()
        return g
    if "a" in a.variants:
        res["a_host_ms"], res["a_min_ms"] = timed(no_grad(lambda: evalbatch.rank_captions(ssp, sh, cv, dv, dsr, feats)), a.steps, a.warmup)
    if "b" in a.variants and a.b_mode != "bound":
        res["b_device_ms"], res["b_min_ms"] = timed(no_grad(lambda: evalbatch.rank_captions_device(ssp, sh, cv, dv, dsr, feats)), a.steps, a.warmup)
    if "b" in a.variants and a.b_mode != "default":
        res["b_bound_ms"], res["b_bound_min_ms"] = timed(no_grad(lambda: evalbatch.rank_captions_device(ssp, sh, cv, dv, dsr, feats, max_items=n_items)), a.steps, a.warmup)
    if "c" in a.variants:
        nv, n_caps, R0, R = 8, 5, 100, 20
        n_img = N // n_caps
        m, c = captioner(nv)
        det = torch.from_numpy(synth.make_detections(n_img, R0, c["D"], seed=3000)).to(DEV)
        idx = torch.from_numpy(synth.make_slot_indices(N, L, R, R0, seed=3000)).to(DEV)
        row_img = torch.arange(N, dtype=torch.int32, device=DEV) // n_caps
        verbs_host = synth.make_verbs(N, L, nv, seed=3000, p=0.15)
        verbs_dev = torch.from_numpy(verbs_host).to(DEV)
        m.set_valid_rows_bound(n_img * R0)            # every bank row may be non-zero: prepare() then never waits for the host
        eos = [3, -1]

        def c_host():
            ranks = evalbatch.rank_captions(ssp, sh, cv, dv, dsr, feats)
            return evalbatch.beam_search_v_indexed(m, det, det, idx, row_img, ranks, verbs_host, eos, beam_size=5)

        def c_device(max_items=None):
            return evalbatch.beam_search_v_ranked(m, ssp, sh, det, det, idx, row_img, cv, dv, dsr, feats, verbs_dev, eos, beam_size=5, max_items=max_items)
        res["c_host_ms"], res["c_host_min_ms"] = timed(no_grad(c_host), a.steps, a.warmup)
        res["c_device_ms"], res["c_device_min_ms"] = timed(no_grad(c_device), a.steps, a.warmup)
        res["c_device_bound_ms"], res["c_device_bound_min_ms"] = timed(no_grad(lambda: c_device(n_items)), a.steps, a.warmup)
        res["c_decode_alone_ms"], _ = timed(no_grad(lambda: evalbatch.beam_search_v_indexed(m, det, det, idx, row_img, host_ranks, verbs_host, eos, beam_size=5)),
                                            a.steps, a.warmup)
    res.update(steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
               torch=torch.__version__)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
