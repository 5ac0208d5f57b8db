"""A/B of the XE training step under torch.optim.Adam(fused=True) and under vsrcap.optim.Adam, in ONE process.

    python tools/optim_ab.py [--dtypes f16x2,bf16] [--leg-seconds 2.0] [--alternations 3] [--out FILE.json]

The step is bench.py's `--workload xe`: the same shapes (bench.CFG), the same model and batches (bench.make_model, the two synthetic
batches of train_bench), the same parallel.DataParallelStep at world 1.  Per compute dtype two models are built, one per optimizer, and
their legs ALTERNATE (torch, vsrcap, torch, vsrcap, ...): every leg is a few warm-up steps, then at least --leg-seconds of steps timed
by the host clock between two device synchronisations.  Reported: ms per step of every leg, per optimizer the mean and the SPREAD (max -
min over its repeated legs), the gap between the two means - to be called a difference only where it exceeds the spread - and, from a
separate short traced phase after the timing (a profiler slows the host), the kernel launches per step: all of them, and those of the
optimizer and of the refresh of the derived weight state, by kernel name.  The GEMM launches per step are vsr_profile_seen's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vsr-guided-cic_amd"))

WARMUP_FIRST, WARMUP_LEG, CHUNK = 6, 4, 20
# kernels of the optimizer step and of the refresh that follows a torch step, by substrings of their names
STEP_KERNELS = ("adam", "Adam", "multi_tensor_apply", "k_absmax_multi", "k_row_l1_max", "k_h2_exps", "k_h2_head_init", "k_f32_to_h2", "k_f32_to_bf16")


def build(torch, synth, bench, parallel, dtype, which, dev):
    m, _ = bench.make_model(torch, synth, dev, True, dtype)
    if which == "torch":
        opt = torch.optim.Adam(m.parameters(), lr=5e-4, fused=True)          # bench.py's
    else:
        from vsrcap.optim import Adam
        opt = Adam(m, lr=5e-4)
    step = parallel.DataParallelStep(m, opt, forward_fn=lambda d, cp, sq: m((d,), (cp, sq)), all_reduce_fn=None,
                                     exchange_dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    return m, step


def make_batches(torch, synth, bench, dev):
    c = bench.CFG
    out = []
    for i in range(2):
        seed = 2000 + i
        out.append((torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed)).contiguous().to(dev),
                    torch.from_numpy(synth.make_ctrl(c["B"], c["T"], c["R"], c["D"], seed=seed)).contiguous().to(dev),
                    torch.from_numpy(synth.make_captions(c["B"], c["T"], c["V"], seed=seed)).contiguous().to(dev),
                    torch.from_numpy(synth.make_gate_gts(c["B"], c["T"], seed=seed)).contiguous().to(dev)))
    return out


def launches_per_step(torch, one_step, eng, dev, steps=3):
    """kernel launches per step from a traced run of `steps` steps: (all kernels, those of STEP_KERNELS by name, GEMM launches)"""
    out = {}
    one_step(0)                                  # (the other leg's optimizer has stepped since: this model's one refresh happens here, untraced)
    eng.profile_begin(every=1 << 20)             # (counts every GEMM launch, times next to none)
    seen0 = eng.profile_seen()
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for i in range(steps):
                one_step(i)
            torch.cuda.synchronize(dev)
        names = {}
        for e in prof.events():
            # device-side events that are kernels: no copies, no annotations (the profiler mirrors "Optimizer.step#..." onto the device)
            if str(e.device_type).endswith("CUDA") and "#" not in e.name and not e.name.startswith(("Memcpy", "Memset", "hipMemcpy", "hipMemset")):
                names[e.name] = names.get(e.name, 0) + 1
        out["kernels_per_step"] = sum(names.values()) / steps
        of_step = {}
        for n, k in sorted(names.items()):
            if any(s in n for s in STEP_KERNELS):
                of_step[n[:80]] = of_step.get(n[:80], 0) + k / steps         # (template instances of one kernel share the prefix)
        out["optimizer_and_refresh_kernels_per_step"] = sum(of_step.values())
        out["optimizer_and_refresh_kernels"] = of_step
    except Exception as e:                       # the trace is an extra: the timing stands without it
        out["trace_error"] = repr(e)
        for i in range(steps):
            one_step(i)
        torch.cuda.synchronize(dev)
    out["gemm_launches_per_step"] = (eng.profile_seen() - seen0) / steps
    eng.profile_end(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtypes", default="f16x2,bf16")
    ap.add_argument("--leg-seconds", type=float, default=2.0)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.alternations < 3 or args.leg_seconds < 2.0:
        ap.error("at least three alternations of legs of at least 2 s: fewer measures the clock and the scheduler")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_ab.py measures on the GPU: no device found (there is no CPU fallback)")
    import bench
    from vsrcap import parallel, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    batches = make_batches(torch, synth, bench, dev)
    result = {"tool": "tools/optim_ab.py", "workload": "bench.py --workload xe, one GPU", "cfg": bench.CFG, "device": torch.cuda.get_device_name(dev),
              "torch": torch.__version__, "leg_seconds": args.leg_seconds, "alternations": args.alternations, "dtypes": {}}
    for dtype in args.dtypes.split(","):
        legs = {"torch": [], "vsrcap": []}
        runs = {}
        for which in legs:
            m, step = build(torch, synth, bench, parallel, dtype, which, dev)
            one = (lambda step: lambda i: step.xe_step(batches[i & 1][0], batches[i & 1][2], batches[i & 1][1], batches[i & 1][3]))(step)
            for i in range(WARMUP_FIRST):
                one(i)
            runs[which] = (m, step, one)
        torch.cuda.synchronize(dev)
        for alt in range(args.alternations):
            for which in ("torch", "vsrcap"):
                one = runs[which][2]
                for i in range(WARMUP_LEG):
                    one(i)
                torch.cuda.synchronize(dev)
                n, t0 = 0, time.perf_counter()
                while True:
                    for i in range(CHUNK):
                        one(n + i)
                    n += CHUNK
                    torch.cuda.synchronize(dev)
                    dt = time.perf_counter() - t0
                    if dt >= args.leg_seconds:
                        break
                legs[which].append({"steps": n, "seconds": dt, "ms_per_step": 1e3 * dt / n})
                print("%s %s leg %d: %d steps, %.4f ms/step" % (dtype, which, alt, n, 1e3 * dt / n), flush=True)
        block = {}
        for which, ls in legs.items():
            ms = [l["ms_per_step"] for l in ls]
            block[which] = {"legs": ls, "mean_ms_per_step": sum(ms) / len(ms), "spread_ms": max(ms) - min(ms)}
            block[which]["launches"] = launches_per_step(torch, runs[which][2], runs[which][0]._eng, dev)
        gap = block["torch"]["mean_ms_per_step"] - block["vsrcap"]["mean_ms_per_step"]
        spread = max(block["torch"]["spread_ms"], block["vsrcap"]["spread_ms"])
        block["gap_ms_torch_minus_vsrcap"] = gap
        block["largest_spread_ms"] = spread
        block["gap_exceeds_spread"] = abs(gap) > spread
        result["dtypes"][dtype] = block
        for _, step, _ in runs.values():
            step.close()
        del runs
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
