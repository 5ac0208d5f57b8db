"""SCST step with samples_per_image = 5 (statics shared) against the repeated-image form, alternating inside ONE process.

    python tools/scst_multi.py [--steps 12] [--warmup 3] [--dtype f16x2] [--only shared|repeated] [--out FILE.json]

The workload is bench.py's `scst` line: 100 images, resident synthetic batches, greedy baseline, 5 samples per image, CIDEr-D rewards on
the device, torch.optim.Adam(fused=True).  Form "repeated" is what bench.py times (det / regions repeat_interleave(5, 0), 500 images
through prepare); form "shared" is scst_step(det, regions, reward_fn, samples_per_image=5).  Each form has its own model and optimizer
(same initial weights); the timed steps alternate shared / repeated so that clock and temperature drift hit both alike, every step is
timed with a device synchronisation on both sides.  Reported per form: median, min, max, the inter-quartile spread of the step times
and the form's peak memory (torch.cuda.max_memory_allocated above what was resident before the form was built).  --only runs one form (for a rocprofv3 --kernel-trace --stats pass)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vsr-guided-cic_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

NS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="f16x2")
    ap.add_argument("--only", choices=["shared", "repeated"])
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from vsrcap import parallel, synth
    from vsrcap.reward import CiderD, clean_ids
    c, EOS = bench.CFG, bench.EOS
    dev = torch.device("cuda", 0)
    batches = []
    for i in range(2):
        seed = 2000 + i
        batches.append((torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed)).contiguous().to(dev),
                        torch.from_numpy(synth.make_ctrl(c["B"], c["L"], c["R"], c["D"], seed=seed)).contiguous().to(dev),
                        torch.from_numpy(synth.make_captions(c["B"], c["T"], c["V"], seed=seed)).contiguous().to(dev)))
    corpus = [[clean_ids(cap, eos=EOS)] for cap in synth.make_captions(2000, c["T"], c["V"], seed=77)]
    cider = CiderD(corpus, c["V"])
    refs = [caps.unsqueeze(1).contiguous() for _, _, caps in batches]
    refs5 = [r.repeat_interleave(NS, 0).contiguous() for r in refs]

    forms, base_mem = {}, {}
    for name in ([args.only] if args.only else ["shared", "repeated"]):
        torch.cuda.synchronize()
        base_mem[name] = torch.cuda.memory_allocated()     # (what is resident before this form exists: the batches, the other form)
        m, _ = bench.make_model(torch, synth, dev, True, args.dtype)
        opt = torch.optim.Adam(m.parameters(), lr=5e-4, fused=True)
        step = parallel.DataParallelStep(m, opt, sample_fn=lambda d, ct, _m=m, **kw: _m.sample_rl(d, ct, **kw))
        rep = [(d.repeat_interleave(NS, 0).contiguous(), r.repeat_interleave(NS, 0).contiguous()) for d, r, _ in batches] if name == "repeated" else None
        forms[name] = (m, step, rep)

    def one_step(name, i):
        m, step, rep = forms[name]
        det, reg, _ = batches[i & 1]
        with torch.no_grad():
            m.eval()
            base_words, _ = m.test(det, reg)
            m.train()
        r_base = cider.rewards(base_words, refs[i & 1], EOS).repeat_interleave(NS, 0)
        reward_fn = lambda words: (cider.rewards(words, refs5[i & 1], EOS), r_base)
        if name == "shared":
            return step.scst_step(det, reg, reward_fn, samples_per_image=NS)
        return step.scst_step(rep[i & 1][0], rep[i & 1][1], reward_fn)

    times = {n: [] for n in forms}
    peak = {}
    for n in forms:
        # this form's own footprint: model + Adam state + workspaces + the transients of a step, above what was resident before it was built
        # (its parameters were allocated after base_mem was read; the peak counter restarts from the current allocation)
        torch.cuda.reset_peak_memory_stats()
        for i in range(args.warmup):
            one_step(n, i)
        torch.cuda.synchronize()
        peak[n] = torch.cuda.max_memory_allocated() - base_mem[n]
    for i in range(args.steps):
        for n in forms:                      # alternate: shared, repeated, shared, ...
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_step(n, i)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3)
    res = {"workload": "SCST step, 100 images x %d samples, greedy baseline, device CIDEr-D, Adam(fused)" % NS, "dtype": args.dtype,
           "steps": args.steps, "warmup": args.warmup, "forms": {}}
    for n, t in times.items():
        a = np.sort(np.array(t))
        q1, q3 = np.percentile(a, [25, 75])
        res["forms"][n] = {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "iqr_ms": float(q3 - q1),
                           "images_per_s": float(c["B"] / (np.median(a) * 1e-3)), "peak_memory_bytes": int(peak[n]), "ms": [round(x, 3) for x in t]}
    if len(res["forms"]) == 2:
        s, r = res["forms"]["shared"], res["forms"]["repeated"]
        res["shared_over_repeated_median"] = s["median_ms"] / r["median_ms"]
        res["shared_not_slower_beyond_repeated_spread"] = bool(s["median_ms"] <= r["median_ms"] + (r["max_ms"] - r["min_ms"]))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
