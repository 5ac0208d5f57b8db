#!/usr/bin/env python3
"""Time one SCST training step at BASELINE configs[4] (100 images x 5 samples, 10 slots x 36 regions x 2048-d, vocabulary 10 000) on one
GPU, composed three ways.  A step is decode(s) + device CIDEr-D rewards + replay forward + hand-written backward + Adam(fused=True):

  (a) bench.py's composition: eval() / test() / train() for the greedy baseline, then sample_rl on 5-times repeated images
  (b) the same greedy baseline call, then sample_rl(..., samples_per_image=5) - the images' statics shared among their samples
  (c) sample_rl(..., samples_per_image=5, greedy_baseline=True): the baseline is one more decoder row per image in the sampling call -
      no mode switch (two rebuilds of the derived weight state), no second prepare, no decode of 100 rows of its own

    python tools/scst_bench.py [--steps 20] [--warmup 5] [--variants abc] [--dtype f16x2] [--out profiles/NAME.json]

Each figure is over --steps steps of a device-synchronised wall time (torch.cuda.synchronize() on both sides of the step) after --warmup
untimed steps: median, and min / max as the spread.  The three variants run in one process, each on a fresh model and optimizer, over
the same two alternating batches that stay on the device.  Prints one JSON line."""
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

from vsrcap import parallel, synth  # noqa: E402
from vsrcap.reward import CiderD, clean_ids  # noqa: E402

DEV = "cuda"
CFG = dict(V=10000, B=100, R0=36, R=36, D=2048, L=10, T=20, E=1000, H=1000, A=512)
NS, EOS = 5, 3


def timed(step, steps, warmup):
    for i in range(warmup):
        step(i)
    ms = []
    for i in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--dtype", default="f16x2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from models import ControllableCaptioningModel
    c = CFG
    weights = synth.make_weights(c["V"], c["D"], c["E"], c["H"], c["A"], seed=0, gains={k: 1.0 for k in synth.DEFAULT_GAINS})
    batches = []
    for i in range(2):
        seed = 2000 + i
        det = torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed)).contiguous().to(DEV)
        reg = torch.from_numpy(synth.make_ctrl(c["B"], c["L"], c["R"], c["D"], seed=seed)).contiguous().to(DEV)
        caps = torch.from_numpy(synth.make_captions(c["B"], c["T"], c["V"], seed=seed)).contiguous().to(DEV)
        batches.append((det, reg, caps))
    rl_batches = [(det.repeat_interleave(NS, 0).contiguous(), reg.repeat_interleave(NS, 0).contiguous()) for det, reg, _ in batches]
    corpus = [[clean_ids(cap, eos=EOS)] for cap in synth.make_captions(2000, c["T"], c["V"], seed=77)]
    cider = CiderD(corpus, c["V"])
    refs = [caps.unsqueeze(1).contiguous() for _, _, caps in batches]            # (B, 1, T): one reference per image
    refs5 = [r.repeat_interleave(NS, 0).contiguous() for r in refs]

    def fresh():
        m = ControllableCaptioningModel(c["T"], c["V"], 2, det_feat_size=c["D"], input_encoding_size=c["E"], rnn_size=c["H"],
                                        att_size=c["A"], verb_2_vob_all={})
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
        m = m.to(DEV).train()
        m.set_compute_dtype(a.dtype)
        opt = torch.optim.Adam(m.parameters(), lr=5e-4, fused=True)
        return m, parallel.DataParallelStep(m, opt, sample_fn=lambda d, ct, **kw: m.sample_rl(d, ct, **kw))

    def greedy_reward(m, i):
        det, reg, _ = batches[i & 1]
        with torch.no_grad():
            m.eval()
            base_words, _ = m.test(det, reg)
            m.train()
        return cider.rewards(base_words, refs[i & 1], EOS).repeat_interleave(NS, 0)

    def variant(which):
        m, step = fresh()

        def step_a(i):
            r_base = greedy_reward(m, i)
            det5, reg5 = rl_batches[i & 1]
            return step.scst_step(det5, reg5, lambda words: (cider.rewards(words, refs5[i & 1], EOS), r_base))

        def step_b(i):
            r_base = greedy_reward(m, i)
            det, reg, _ = batches[i & 1]
            return step.scst_step(det, reg, lambda words: (cider.rewards(words, refs5[i & 1], EOS), r_base), samples_per_image=NS)

        def step_c(i):
            det, reg, _ = batches[i & 1]
            return step.scst_step(det, reg, lambda words, base_words: (cider.rewards(words, refs5[i & 1], EOS),
                                                                       cider.rewards(base_words, refs[i & 1], EOS)),
                                  samples_per_image=NS, greedy_baseline=True)
        out = timed({"a": step_a, "b": step_b, "c": step_c}[which], a.steps, a.warmup)
        step.close()
        del m, step
        torch.cuda.empty_cache()
        return out

    names = {"a": "a_test_then_repeated_rows", "b": "b_test_then_samples_per_image", "c": "c_greedy_baseline_row"}
    res = {names[v]: variant(v) for v in "abc" if v in a.variants}
    res.update(images=c["B"], samples_per_image=NS, steps=a.steps, warmup=a.warmup, dtype=a.dtype, device=torch.cuda.get_device_name(0),
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count, torch=torch.__version__)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
