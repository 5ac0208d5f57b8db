#!/usr/bin/env python3
"""bench.py - headline benchmark of the VSR captioning decoder hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload beam5|beam5idx|greedy|xe|xeidx|scst]
                    [--scaling weak|strong] [--dtype f16x2|f32x3|f32|bf16] [--dump-outputs DIR]
                    [--full [--no-cpu] [--no-secondary] [--no-alt]]

A plain run sets up, warms up, times the K steps of the chosen workload, writes the last step's outputs if --dump-outputs
is given, and prints the result line.  --full adds everything beside the headline: the GEMM roofline (HIP events around
every 5th GEMM launch of the timed region), the CPU baseline, the XE step and the other GEMM flavours and workloads of the
default line, and the dense-format comparison of beam5idx.
--dump-outputs DIR: what the timed path returned to its caller in the last timed step (rank 0), as DIR/<name>.npy in
float32 / float64: word and gate ids (and beam log-probs) of a decode call, the losses of a training step and a fixed
seeded sample of 4 096 elements per parameter after it.  The inputs are synthetic and seeded: the same arguments give the
same inputs from run to run.

Headline (BASELINE.json metric, configs[2]): beam-5 decode through ControllableCaptioningModel.beam_search, batch 100
images per GPU, 36 regions x 2048-d, 10 slots, seq_len 20, vocab 10 000, fp32 operands and accumulation (the reference's
precision; token parity holds: every GPU test runs in this flavour and in the exact-chain one).  A "step" = ONE full decode call on one batch of synthetic inputs already resident in HBM: hoisted
statics (vsr_prepare) + 20 timesteps + back-tracking.  tokens/s = B_total * T * steps / wall time (top-1 hypothesis
tokens).  The --full line also carries the second half of the BASELINE metric as "secondary": the XE
training step (configs[3] shapes; forward + NLL losses + hand-written BPTT + Adam [+ RCCL gradient all-reduce]).

Multi-GPU (one process per GPU, RCCL):  `--gpus N` with no torch.distributed environment starts the N ranks itself
(child processes; the parent never touches the GPU); under `python -m torch.distributed.run` each process is a rank.
  --scaling weak    every rank owns a batch of 100 (decode: no data-path collective; XE: gradient all-reduce)
  --scaling strong  ONE batch of 100 split 13,13,13,13,12,12,12,12 (parallel.shard_bounds); decode gathers the ids
The timed region is bracketed by barrier + synchronize on both sides; the time is the MAX over ranks.
"""
import argparse
import json
import os
import platform
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "vsr-guided-cic_amd"))

CFG = dict(V=10000, B=100, R0=36, R=36, D=2048, L=10, T=20, E=1000, H=1000, A=512)
BEAM = 5
EOS = 3
PROFILE_EVERY = 5
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4_f32, dense, spec
PEAK_BF16_MFMA_TFLOPS = 2500.0   # dense bf16 (never the 2:1-sparsity figure)
PEAK_HBM_GBS = 8000.0
PARAM_SAMPLE = 4096              # --dump-outputs: elements per trained parameter


def host_outputs(named):
    """{name: tensor} of the last timed step -> {name: host array}: float64 stays float64, everything else (ids < 2^24,
    fp32 log-probs) becomes float32"""
    out = {}
    for k, t in named.items():
        a = t.detach().cpu().numpy()
        out[k] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    return out


def param_sample(torch, model):
    """a fixed, seeded sample of PARAM_SAMPLE elements of every parameter (all of a smaller one)"""
    out = {}
    for k, p in model.named_parameters():
        flat = p.detach().reshape(-1)
        if flat.numel() > PARAM_SAMPLE:
            idx = np.sort(np.random.default_rng(0).choice(flat.numel(), PARAM_SAMPLE, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        out["param_" + k] = flat
    return out


def dump_outputs(outdir, arrays):
    os.makedirs(outdir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(outdir, k + ".npy"), a)


# ---------------------------------------------------------------------------------------------- rank launch
def launch_ranks(args):
    """Parent of a `--gpus N` run outside torch.distributed.run: start N rank processes and relay rank 0's line.
    Nothing here initialises the GPU (no HIP call, no torch.cuda.*): the children do."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = p.wait() or rc
    return rc


def traffic_from_profiles(kind):
    """HBM bytes per launch of the dominant kernel from the newest committed PMC passes (rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE on this same command, FETCH_SIZE doubled per the guide's gfx950 correction).  Returns (bytes, file):
    the figure is QUOTED from that file, not measured in this run (PMC collection needs rocprofv3 around the process)."""
    pdir = os.path.join(ROOT, "profiles")
    best = (None, None)
    if os.path.isdir(pdir):
        for f in sorted(os.listdir(pdir)):
            if f.endswith(kind + "_hbm_traffic.json"):
                try:
                    best = (json.load(open(os.path.join(pdir, f)))["hbm_bytes_per_launch"], "profiles/" + f)
                except Exception:
                    pass
    return best


def cpu_info():
    model = platform.processor() or "unknown"
    phys = set()
    try:
        pid = cid = None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
            elif ln.startswith("physical id"):
                pid = ln.split(":", 1)[1].strip()
            elif ln.startswith("core id"):
                cid = ln.split(":", 1)[1].strip()
                phys.add((pid, cid))
    except OSError:
        pass
    return model, (len(phys) or os.cpu_count() or 1)


# ---------------------------------------------------------------------------------------------- CPU baseline legs
def cpu_baseline(weights, sample_B, beam, torch, synth, full_B=0):
    """the CPU oracle (PyTorch CPU, fp32) on the same synthetic workload, in the reference's AS-WRITTEN
    op order (per-step recompute of the pooled descriptor / region projection, statics re-gather per beam step, full sort)
    and HOISTED beside it, torch.set_num_threads(physical cores).  Both flavours are timed the SAME way on the SAME inputs:
    full_B > 0 (default): the GPU leg's own first batch (B = 100, M = 500 rows), one warm-up call, then 2 timed calls as written and
    3 hoisted; `value` / `hoisted_value` = tokens/s at the MEDIAN call time, `*_best` at the fastest.  full_B = 0: a bounded sample
    of sample_B images (1 warm-up on 2 images, median of 3)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vsr_oracle as vo
    c = CFG
    model, cores = cpu_info()
    torch.set_num_threads(cores)
    B = full_B if full_B > 0 else sample_B
    seed = 1000 if full_B > 0 else 77                      # (1000 = the GPU leg's first batch)
    det = torch.from_numpy(synth.make_detections(B, c["R0"], c["D"], seed=seed))
    ctrl = torch.from_numpy(synth.make_ctrl(B, c["L"], c["R"], c["D"], seed=seed))
    name = "beam-%d" % beam if beam > 1 else "greedy"
    out = {}
    for flavour, n_timed in (("as_written", 2 if full_B > 0 else 3), ("hoisted", 3)):
        o = vo.Oracle(weights, c["T"], 2, as_written=flavour == "as_written")
        run = (lambda d, r: o.beam_search(d, r, [EOS, -1], beam, 1)) if beam > 1 else (lambda d, r: o.test(d, r))
        ts = []
        with torch.no_grad():
            t0 = time.time()
            run(det, ctrl) if full_B > 0 else run(det[:2], ctrl[:2])          # warm-up (allocator, thread pool at these shapes)
            warm = time.time() - t0
            for _ in range(n_timed):
                t0 = time.time()
                run(det, ctrl)
                ts.append(time.time() - t0)
        ts.sort()
        med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
        out[flavour] = dict(med=med, best=ts[0], warm=warm, n=n_timed)
    tok = B * c["T"]
    aw, ho = out["as_written"], out["hoisted"]
    return dict(value=tok / aw["med"], unit="tokens/s", cores=torch.get_num_threads(), kind="port", cpu_model=model, torch=torch.__version__,
                value_best=tok / aw["best"], hoisted_value=tok / ho["med"], hoisted_value_best=tok / ho["best"], sample_B=B,
                timed_calls={"as_written": aw["n"], "hoisted": ho["n"]},
                sample="oracle/vsr_oracle.py, %s, fp32, %s%d images x %d steps; as written (the reference's op order): 1 warm-up call (%.1f s) + %d timed, "
                       "median %.1f s / best %.1f s per call = value / value_best; hoisted variant on the same inputs: warm-up %.1f s + %d timed, median %.1f s / best "
                       "%.1f s = hoisted_value / hoisted_value_best" %
                       (name, "the GPU leg's own first batch, " if full_B > 0 else "bounded sample, ", B, c["T"], aw["warm"], aw["n"], aw["med"], aw["best"],
                        ho["warm"], ho["n"], ho["med"], ho["best"]))


def cpu_baseline_xe(weights, sample_B, torch, synth):
    """XE step of coco_scripts/train.py:103-113 on the CPU oracle (autograd backward + Adam), bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vsr_oracle as vo
    c = CFG
    model, cores = cpu_info()
    torch.set_num_threads(cores)
    o = vo.Oracle(weights, c["T"], 2, as_written=True)
    params = [o.p[k].requires_grad_(True) for k in o.p]
    opt = torch.optim.Adam(params, lr=5e-4)
    det = torch.from_numpy(synth.make_detections(sample_B, c["R0"], c["D"], seed=77))
    seq = torch.from_numpy(synth.make_ctrl(sample_B, c["T"], c["R"], c["D"], seed=78))
    caps = torch.from_numpy(synth.make_captions(sample_B, c["T"], c["V"], seed=77))
    gts = torch.from_numpy(synth.make_gate_gts(sample_B, c["T"], seed=77))
    ts = []
    for _ in range(3):
        t0 = time.time()
        opt.zero_grad()
        out, gate = o.forward(det, caps, seq)
        vo.xe_loss(out, gate, caps, gts)[0].backward()
        opt.step()
        ts.append(time.time() - t0)
    med = sorted(ts[1:])[0]
    return dict(value=sample_B / med, unit="samples/s", cores=torch.get_num_threads(), kind="port", cpu_model=model,
                torch=torch.__version__,
                sample="oracle/vsr_oracle.py as_written XE step (forward + NLL losses + autograd backward + Adam), %d images x %d steps, "
                       "fp32, %.1f s (best of two steps after one warm-up step)" % (sample_B, c["T"], med))


# ---------------------------------------------------------------------------------------------- shared pieces
class Dist:
    """backend "nccl" (= RCCL over xGMI): one GPU per rank, collectives on the device.  backend "gloo" is a SELF-TEST of the
    multi-rank code path on a box with fewer GPUs than ranks: ranks share the visible devices and the collectives are staged
    through host memory; its numbers are not a measurement of anything."""

    def __init__(self, torch, dist, backend="nccl"):
        self.torch, self.dist, self.backend = torch, dist, backend
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        index = self.local_rank if backend == "nccl" else self.local_rank % max(1, torch.cuda.device_count())
        if self.world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            torch.cuda.set_device(index)
            if backend == "nccl":
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=torch.device("cuda", index))
            else:
                dist.init_process_group("gloo", rank=self.rank, world_size=self.world)
        torch.cuda.set_device(index)
        self.dev = torch.device("cuda", index)

    def all_reduce_fn(self):
        """None for RCCL; a host-staged SUM for the gloo self-test (DataParallelStep's all_reduce_fn hook)"""
        if self.backend == "nccl" or self.world == 1:
            return None

        def host(t):
            c = t.detach().float().cpu()          # (a bf16 wire buffer is summed in fp32 here: gloo's bf16 support varies by build)
            self.dist.all_reduce(c)
            t.copy_(c)
        return host

    def gather_ids(self, parallel, w, n_total):
        if self.backend == "nccl":
            return parallel.gather_ids(w, n_total)
        return parallel.gather_ids(w.cpu(), n_total).to(self.dev)

    def barrier(self):
        self.torch.cuda.synchronize(self.dev)
        if self.world > 1:
            self.dist.barrier()
        self.torch.cuda.synchronize(self.dev)

    def max_time(self, dt):
        if self.world > 1:
            t = self.torch.tensor([dt], dtype=self.torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    def observed_world(self):
        """what the collective library itself sees: the sum of a ones-vector over the ranks"""
        if self.world == 1:
            return 1
        t = self.torch.ones(1, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t)
        return int(t.item())


def make_model(torch, synth, dev, train, dtype, verb_table=None):
    from models import ControllableCaptioningModel
    c = CFG
    gains = {k: 1.0 for k in synth.DEFAULT_GAINS} if train else None
    weights = synth.make_weights(c["V"], c["D"], c["E"], c["H"], c["A"], seed=0, gains=gains)
    m = ControllableCaptioningModel(c["T"], c["V"], 2, det_feat_size=c["D"], input_encoding_size=c["E"], rnn_size=c["H"],
                                    att_size=c["A"], verb_2_vob_all=verb_table or {})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    m = m.to(dev)
    m = m.train() if train else m.eval()
    m.set_compute_dtype(dtype)
    return m, weights


def roofline_block(dtype, gemm_ms, gemm_n, gemm_seen, gemm_flops, dt, traffic=None, traffic_source=None, gemm_bytes=0.0):
    achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    if dtype == "bf16":
        # bf16 operands take the matrix pipe out of the picture (16x the fp32 rate): the GEMMs are bound by the bytes they move
        gbs = gemm_bytes / (gemm_ms * 1e-3) / 1e9 if gemm_ms > 0 else 0.0
        return {"bound": "hbm", "kernel": "gemm_nt_b16a_kernel (v_mfma_f32_32x32x16_bf16; bf16 W copies and producer-written bf16 A images, both global -> LDS by DMA) and, for launches with an fp32-only A operand, gemm_nt_bf16w_kernel (A converted on the way into LDS)",
                "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS, "traffic": None,
                "algorithmic_bytes_per_launch": gemm_bytes / max(gemm_n, 1), "launches": gemm_seen, "launches_timed": gemm_n,
                "avg_launch_us": gemm_ms * 1e3 / max(gemm_n, 1), "gemm_share_of_wall": gemm_ms * 1e-3 / max(gemm_n, 1) * gemm_seen / dt,
                "mfma_tflops_for_reference": achieved, "mfma_frac_of_dense_bf16_peak": achieved / PEAK_BF16_MFMA_TFLOPS}
    peak = PEAK_F32_MFMA_TFLOPS
    if dtype in ("f32x3", "f16x2"):
        # fp32-equivalent peak = the dense bf16 / fp16 MFMA peak over the MFMAs one fp32 product costs (six / three)
        nmfma = 6.0 if dtype == "f32x3" else 3.0
        kernel = ("gemm_nt_x3_kernel<2,2> / <2,1> (128 x 256 / 128 x 128 tiles; from 193 / up to 128 rows) and gemm_nt_x3s_kernel (weight streaming, "
                  "<= 80 rows): fp32 operands split into 3 bf16 terms in the kernel, 6 x v_mfma_f32_*_bf16 per product; launches of 129-192 rows: "
                  "the exact fp32 kernels of gemm_f32.h") if dtype == "f32x3" else \
                 ("gemm_nt_h2a_kernel<2,2> / <2,1> (128 x 256 / 128 x 128 tiles, > 80 rows; both operands are fp16-pair images moved global -> LDS by DMA: "
                  "weights pre-split per weight version, A images written by the kernels that produce h1 / h2 / s_t / g_t / the attended vector), "
                  "gemm_nt_h2_kernel (same tiles, fp32 A split in the kernel: prepare(), the backward pass of training with gradient bounds measured "
                  "by their producers) and gemm_nt_h2s_kernel (weight streaming, <= 80 rows): fp32 operands as 2 fp16 terms under a power-of-two "
                  "scale, 3 x v_mfma_f32_*_f16 per product")
        r = {"bound": "mfma", "kernel": kernel,
             "achieved": achieved, "peak": PEAK_BF16_MFMA_TFLOPS / nmfma, "unit": "TFLOP/s (fp32-equivalent)", "frac": achieved / (PEAK_BF16_MFMA_TFLOPS / nmfma),
             "traffic": traffic, "launches": gemm_seen, "launches_timed": gemm_n, "avg_launch_us": gemm_ms * 1e3 / max(gemm_n, 1),
             "gemm_share_of_wall": gemm_ms * 1e-3 / max(gemm_n, 1) * gemm_seen / dt, "algorithmic_flops_per_launch": gemm_flops / max(gemm_n, 1),
             "vs_fp32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS}
        if dtype == "f16x2":
            # the peak above is quoted at 2.4 GHz; under this load the chip holds ~1.5 GHz (profiles/r04_s_h2a_ablations.txt: the kernel with no
            # global traffic in its k loop reaches 85 % of the MFMA rate AT THAT CLOCK), so `frac` tops out near 0.6 here
            r["sustained_clock_note"] = ("peak quoted at 2.4 GHz; the chip holds ~1.74 GHz in these launches (power limit: 1.90 GHz without the weight DMAs, 2.14 GHz with idle "
                                         "matrix pipes; profiles/r05_k_h2a_phase_stamps_and_fragment_read_ablation.txt part 3): 604 TFLOP/s fp32-equivalent at that clock")
            r["frac_of_peak_at_sustained_clock"] = achieved / (PEAK_BF16_MFMA_TFLOPS / nmfma * 1.74 / 2.4)
            # the same launches against the HBM roofline (algorithmic bytes: every operand and output element once)
            gbs = gemm_bytes / (gemm_ms * 1e-3) / 1e9 if gemm_ms > 0 else 0.0
            r["hbm_view"] = {"achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                             "algorithmic_bytes_per_launch": gemm_bytes / max(gemm_n, 1)}
        if traffic_source:
            r["traffic_source"] = traffic_source + " (quoted from the committed rocprofv3 PMC passes of this command, not re-measured in this run)"
        return r
    r = {"bound": "mfma",
         "kernel": "gemm_nt_f32_kernel (v_mfma_f32_32x32x2_f32; problems of <= 80 rows: gemm_nt_f32_r16_kernel, v_mfma_f32_16x16x4_f32)",
         "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak, "traffic": traffic,
         "launches": gemm_seen, "launches_timed": gemm_n, "avg_launch_us": gemm_ms * 1e3 / max(gemm_n, 1),
         "gemm_share_of_wall": gemm_ms * 1e-3 / max(gemm_n, 1) * gemm_seen / dt,
         "algorithmic_flops_per_launch": gemm_flops / max(gemm_n, 1)}
    if traffic_source:
        r["traffic_source"] = traffic_source + " (quoted from the committed rocprofv3 PMC passes of this command, not re-measured in this run)"
    return r


# ---------------------------------------------------------------------------------------------- decode
def decode_bench(args, D, torch, dist, synth):
    from vsrcap import parallel
    c = CFG
    dev, rank, world = D.dev, D.rank, D.world
    m, weights = make_model(torch, synth, dev, False, args.dtype)
    beam = BEAM if args.workload in ("beam5", "beam5idx") else 1
    indexed = args.workload == "beam5idx"
    strong = args.scaling == "strong" and world > 1
    lo, hi = parallel.shard_bounds(c["B"], world, rank) if strong else (0, c["B"])
    # two distinct resident batches, alternated, so no step can reuse the previous step's prepare()
    batches = []
    valid_rows = 0
    for i in range(2):
        seed = 1000 + i + (0 if strong else 10 * rank)
        if indexed:
            # index-list region format: the slots name rows of the image's own detection matrix
            from vsrcap.regions import IndexedRegions
            det = torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed, min_valid=c["R0"])[lo:hi]).to(dev)
            idx = torch.from_numpy(synth.make_slot_indices(c["B"], c["L"], c["R"], c["R0"], seed=seed)[lo:hi]).contiguous().to(dev)
            batches.append((det, IndexedRegions(det, idx)))
        else:
            ctrl_np = synth.make_ctrl(c["B"], c["L"], c["R"], c["D"], seed=seed)[lo:hi]
            valid_rows = max(valid_rows, int((ctrl_np.sum(-1) != 0).sum()))       # known on the host, like the eval script's own tensors
            batches.append((torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed)[lo:hi]).contiguous().to(dev),
                            torch.from_numpy(ctrl_np).contiguous().to(dev)))
    if args.rows_bound and valid_rows > 0:
        m.set_valid_rows_bound(valid_rows)      # vsr_prepare() then never waits for the host (include/vsrcap.h, vsr_set_valid_rows_bound)

    def one_step(i):
        det, ctrl = batches[i & 1]
        with torch.no_grad():
            if beam > 1:
                (w, g), (lw, lg) = m.beam_search((det, ctrl), [EOS, -1], beam, 1)
                out = {"words": w, "gates": g, "logp_words": lw, "logp_gates": lg}
            else:
                w, g = m.test(det, ctrl)
                out = {"words": w, "gates": g}
            if strong:      # the one exchange of a sharded decode: (B, T) ids of every shard
                out["words"] = D.gather_ids(parallel, w, c["B"])
            return out

    for i in range(args.warmup):
        one_step(i)
    eng = m._engine(dev)
    D.barrier()
    if args.full:
        # HIP events around every 5th GEMM launch of the timed region (3 launch kinds per timestep: every kind is sampled
        # equally often); an event pair on EVERY launch costs the timed region 3 %
        eng.profile_begin(every=PROFILE_EVERY)
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = one_step(i)
    D.barrier()
    dt = time.perf_counter() - t0
    if args.full:
        gemm_seen = eng.profile_seen()
        gemm_bytes = eng.profile_bytes()
        gemm_ms, gemm_n, gemm_flops = eng.profile_end(dev)
    dt = D.max_time(dt)
    images = c["B"] if strong else world * c["B"]
    name = "beam-5" if beam > 1 else "greedy"
    traffic, tsrc = (None, None)
    if args.full and beam > 1 and not indexed:                          # the workloads the committed PMC passes were taken on
        traffic, tsrc = traffic_from_profiles({"f32": "gemm", "bf16": "gemm_bf16", "f32x3": "gemm_f32x3", "f16x2": "gemm_f16x2"}[args.dtype])
    line = {
        "metric": ("decoded tokens/sec at batch=100, beam=5, 36x2048 regions" + (", index-list region format" if indexed else ""))
                  if beam > 1 else "decoded tokens/sec, greedy, batch=100, 36x2048 regions",
        "value": images * c["T"] * args.steps / dt, "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "%s decode, batch %s, %d regions x 2048-d, 10 slots, seq_len 20, vocab 10000 (BASELINE configs[%d])" %
                               (name, "%d images split over the ranks (13/12 per GPU at 8)" % c["B"] if strong else "%d images/GPU" % c["B"], c["R"], 2 if beam > 1 else 1),
                   "beam": beam, "batch_per_gpu": hi - lo, "seq_len": c["T"],
                   "parallelism": "images sharded, dp%d%s" % (world, ", ids all-gathered (%s)" % ("RCCL" if args.backend == "nccl" else "gloo self-test") if strong else ", no data-path collective"),
                   "rccl_world_size_observed": D.observed_world(), "collective_backend": args.backend,
                   "host_sync_per_call": "none (caller-supplied bound on the non-padding region rows)" if (args.rows_bound and valid_rows > 0) else "one 8-byte read-back in vsr_prepare (the number of non-padding region rows)",
                   "decode_cache": "prebuilt, weight-only (embedding rows through the x columns of the LSTM1 / gate input weights, "
                                   "240 MB, built once per weight version outside the timed call; all per-image hoisting is inside)"},
    }
    if args.full:
        line["roofline"] = roofline_block(args.dtype, gemm_ms, gemm_n, gemm_seen, gemm_flops, dt, traffic, tsrc, gemm_bytes)
    if getattr(args, "emit_ids", False) and rank == 0:
        line["config"]["ids"] = last["words"].cpu().tolist()
    outputs = host_outputs(last) if args.dump_outputs and rank == 0 else None
    if args.full and indexed and rank == 0:
        dense = [(d, r.dense().contiguous()) for d, r in batches]
        with torch.no_grad():
            for i in range(2):
                m.beam_search(dense[i & 1], [EOS, -1], beam, 1)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for i in range(args.steps):
                m.beam_search(dense[i & 1], [EOS, -1], beam, 1)
            torch.cuda.synchronize(dev)
        line["config"]["dense_format_same_data_tokens_per_s"] = (hi - lo) * c["T"] * args.steps / (time.perf_counter() - t1)
        line["config"]["region_bytes_per_batch"] = {"index_lists": int(batches[0][1].slot_idx.numel() * 4), "dense": int(dense[0][1].numel() * 4)}
    del m, batches
    torch.cuda.empty_cache()
    return line, weights, beam, outputs


# ---------------------------------------------------------------------------------------------- eval-side caller (C3 / N1)
def eval_bench(args, D, torch, dist, synth):
    """coco_scripts/eval_coco.py:240-247 at the shapes the real caller feeds: per image the pooled detections (100 x 2048), n_caps = 5
    caption rows of 10 slots x 20 regions and a verb list; 16 images of a loader batch decoded by ONE beam_search_v call through
    vsrcap.evalbatch.beam_search_v_batched (M = 80 / 400 rows).  tokens/s = caption rows x T / wall time."""
    from vsrcap import evalbatch
    c = dict(CFG, R0=100, R=20, L=10)
    n_img, n_caps, nv = 16, 5, 8
    dev = D.dev
    m, weights = make_model(torch, synth, dev, False, args.dtype, verb_table=synth.make_verb_table(nv, c["V"], seed=0))
    batches = []
    for i in range(2):
        seed = 3000 + i + 10 * D.rank
        det = torch.from_numpy(synth.make_detections(n_img, c["R0"], c["D"], seed=seed)).to(dev)
        seqs = torch.from_numpy(synth.make_ctrl(n_img * n_caps, c["L"], c["R"], c["D"], seed=seed)).to(dev)
        verbs = torch.from_numpy(synth.make_verbs(n_img * n_caps, c["L"], nv, seed=seed, p=0.15)).to(dev)
        batches.append([(det[j], seqs[j * n_caps:(j + 1) * n_caps], verbs[j * n_caps:(j + 1) * n_caps]) for j in range(n_img)])

    def one_step(i):
        with torch.no_grad():
            return evalbatch.beam_search_v_batched(m, batches[i & 1], [EOS, -1], BEAM, 1, gt=False)

    for i in range(args.warmup):
        one_step(i)
    eng = m._engine(dev)
    D.barrier()
    if args.full:
        eng.profile_begin(every=PROFILE_EVERY)
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = one_step(i)
    D.barrier()
    dt = time.perf_counter() - t0
    if args.full:
        gemm_seen, gemm_bytes = eng.profile_seen(), eng.profile_bytes()
        gemm_ms, gemm_n, gemm_flops = eng.profile_end(dev)
    dt = D.max_time(dt)
    rows = n_img * n_caps * D.world
    line = {"metric": "decoded tokens/sec, beam_search_v at the eval caller's shapes (16 images x 5 caption rows, beam 5)",
            "value": rows * c["T"] * args.steps / dt, "unit": "tokens/s", "n_gpus": D.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "beam_search_v (verb forcing, gt=False) through evalbatch.beam_search_v_batched: 16 images x 5 caption rows per GPU, 100 pooled "
                                   "detections x 2048-d, 10 slots x 20 regions, seq_len 20, vocab 10000, beam 5 (eval_coco.py:55-57,240-247; data/field.py:18,115)",
                       "beam": BEAM, "rows_per_gpu": n_img * n_caps, "seq_len": c["T"], "parallelism": "dp%d, no data-path collective" % D.world}}
    if args.full:
        line["roofline"] = roofline_block(args.dtype, gemm_ms, gemm_n, gemm_seen, gemm_flops, dt, None, None, gemm_bytes)
    outputs = None
    if args.dump_outputs and D.rank == 0:       # per image ([words, gates], [lp_w, lp_g]), concatenated over the images' caption rows
        outputs = host_outputs({k: torch.cat([r[j][i] for r in last], 0) for k, j, i in
                                (("words", 0, 0), ("gates", 0, 1), ("logp_words", 1, 0), ("logp_gates", 1, 1))})
    del m, batches
    torch.cuda.empty_cache()
    return line, weights, outputs


# ---------------------------------------------------------------------------------------------- training
def train_bench(args, D, torch, dist, synth, steps, warmup):
    """XE step (BASELINE configs[3]) / SCST step (configs[4]): forward + losses + hand-written BPTT backward + Adam,
    data-parallel over ranks with RCCL gradient all-reduce overlapped with the weight-gradient phase and global loss
    normalisation (vsrcap/parallel.py)."""
    from vsrcap import parallel
    c = CFG
    dev, rank, world = D.dev, D.rank, D.world
    m, weights = make_model(torch, synth, dev, True, args.dtype)
    opt = torch.optim.Adam(m.parameters(), lr=5e-4, fused=True)      # train.py:77 Adam(lr=5e-4); one fused launch per step
    xe = args.workload != "scst"
    indexed = args.workload == "xeidx"          # index-list regions on the training path: slot entries name detection rows
    strong = args.scaling == "strong" and world > 1
    lo, hi = parallel.shard_bounds(c["B"], world, rank) if strong else (0, c["B"])
    L = c["T"] if xe else c["L"]
    batches = []
    for i in range(2):
        seed = 2000 + i + (0 if strong else 10 * rank)
        if indexed:
            from vsrcap.regions import IndexedRegions
            det = torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed, min_valid=c["R0"])[lo:hi]).contiguous().to(dev)
            reg = IndexedRegions(det, torch.from_numpy(synth.make_slot_indices(c["B"], L, c["R"], c["R0"], seed=seed)[lo:hi]).contiguous().to(dev))
        else:
            det = torch.from_numpy(synth.make_detections(c["B"], c["R0"], c["D"], seed=seed)[lo:hi]).contiguous().to(dev)
            reg = torch.from_numpy(synth.make_ctrl(c["B"], L, c["R"], c["D"], seed=seed)[lo:hi]).contiguous().to(dev)
        batches.append((det, reg,
                        torch.from_numpy(synth.make_captions(c["B"], c["T"], c["V"], seed=seed)[lo:hi]).contiguous().to(dev),
                        torch.from_numpy(synth.make_gate_gts(c["B"], c["T"], seed=seed)[lo:hi]).contiguous().to(dev)))
    if getattr(args, "rows_bound", False) and not indexed:
        # the loader pads on the host (data/field.py:44-61), so the number of non-padding region rows is known there: with it vsr_prepare()
        # never waits for the device (include/vsrcap.h, vsr_set_valid_rows_bound).  An option, not the default line: the reference's loop does not pass it.
        m.set_valid_rows_bound(max(int((b[1].sum(-1) != 0).sum()) for b in batches))
    step = parallel.DataParallelStep(m, opt, forward_fn=lambda d, cp, sq: m((d,), (cp, sq)),
                                     sample_fn=lambda d, ct: m.sample_rl(d, ct), all_reduce_fn=D.all_reduce_fn(),
                                     exchange_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    NS = 5                          # samples per image (BASELINE configs[4]); the reference has no such loop, the caller
    rl_batches = []                 # repeats every image NS times
    if not xe:
        for det, reg, _, _ in batches:
            rl_batches.append((det.repeat_interleave(NS, 0).contiguous(), reg.repeat_interleave(NS, 0).contiguous()))
        # rewards: per-sample CIDEr-D on the device (vsrcap/reward.py; train.py:169-170) of the sampled /
        # greedy captions against the batch's synthetic reference caption, document frequencies from a synthetic corpus
        from vsrcap.reward import CiderD, clean_ids
        corpus = [[clean_ids(cap, eos=EOS)] for cap in synth.make_captions(2000, c["T"], c["V"], seed=77)]
        cider = CiderD(corpus, c["V"])
        refs = [caps.unsqueeze(1).contiguous() for _, _, caps, _ in batches]               # (B, 1, T): one reference per sample
        refs5 = [r.repeat_interleave(NS, 0).contiguous() for r in refs]

    def one_step(i):
        det, reg, caps, gts = batches[i & 1]
        if xe:
            return step.xe_step(det, caps, reg, gts)
        with torch.no_grad():       # greedy baseline of train.py:127-138 (model.test), then NS samples per image
            m.eval()
            base_words, _ = m.test(det, reg)
            m.train()
        r_base = cider.rewards(base_words, refs[i & 1], EOS).repeat_interleave(NS, 0)
        det5, reg5 = rl_batches[i & 1]
        return step.scst_step(det5, reg5, lambda words: (cider.rewards(words, refs5[i & 1], EOS), r_base))

    for i in range(warmup):
        one_step(i)
    eng = m._engine(dev)
    D.barrier()
    if args.full:
        eng.profile_begin(every=PROFILE_EVERY)
    t0 = time.perf_counter()
    last = None
    for i in range(steps):
        last = one_step(i)
    D.barrier()
    dt = time.perf_counter() - t0
    if args.full:
        gemm_seen = eng.profile_seen()
        gemm_bytes = eng.profile_bytes()
        gemm_ms, gemm_n, gemm_flops = eng.profile_end(dev)
    dt = D.max_time(dt)
    images = c["B"] if strong else world * c["B"]
    line = {
        "metric": ("XE-step samples/sec" + (", index-list region format" if indexed else "")) if xe else "SCST-step images/sec (5 samples/image + greedy baseline, CIDEr-D rewards on device)",
        "value": images * steps / dt, "unit": "samples/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": ("XE training step (fp16-pair / bf16 weight images refreshed from the live weights + forward + NLL losses + BPTT backward + torch.optim.Adam(fused=True)), batch %s, %d pooled detections, 20 slots x %d regions x 2048-d, "
                                "seq_len 20, vocab 10000 (%s)" % ("100 split over the ranks" if strong else "100/GPU", c["R0"], c["R"],
                                                                   "BASELINE configs[3] shapes" if (c["R0"], c["R"]) == (36, 36) else "the real callers' shapes: data/field.py:18,115, coco_scripts/train.py:39-41")) if xe else
                               ("SCST step: greedy baseline (100 images) + sample_rl on 500 rows (5 samples/image) + replayed forward + BPTT "
                                "backward + Adam(fused=True), rewards = device CIDEr-D vs synthetic references, 10 slots x 36 x 2048 (BASELINE configs[4])"),
                   "batch_per_gpu": hi - lo, "seq_len": c["T"],
                   "parallelism": "dp%d, %s gradient all-reduce (%s on the wire) in buckets on a side stream, overlapped with the weight-gradient GEMMs" % (world, "RCCL" if args.backend == "nccl" else "gloo (self-test, host-staged)", "bf16, 142 MB" if args.dtype == "bf16" else "fp32, 285 MB"),
                   "rccl_world_size_observed": D.observed_world()},
    }
    if args.full:
        line["roofline"] = roofline_block(args.dtype, gemm_ms, gemm_n, gemm_seen, gemm_flops, dt,
                                          *((traffic_from_profiles("f16x2_xe_step") if xe and not indexed and args.dtype == "f16x2" else (None, None))),
                                          gemm_bytes=gemm_bytes)
    outputs = None
    if args.dump_outputs and rank == 0:         # the step's global losses (XE: loss, loss_cap, loss_gate; SCST: loss) + the trained weights
        outputs = host_outputs(dict({"losses": last.reshape(-1)}, **param_sample(torch, m)))
    del m, opt, step, batches
    torch.cuda.empty_cache()
    return line, weights, outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="beam5", choices=["beam5", "beam5idx", "greedy", "xe", "xeidx", "scst", "xe_real", "beam5_eval"],
                    help="xe_real / beam5_eval: the XE step and the eval-side beam_search_v call at the shapes the reference's real callers feed "
                         "(100 pooled detections, slots of 20 regions; 16 images x 5 caption rows)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--dtype", default="f16x2", choices=["f32", "f32x3", "f16x2", "bf16"],
                    help="f16x2 = parity mode (headline): fp32 operands in memory, fp32 accumulation, every product from two fp16 terms per operand "
                         "under a power-of-two scale (3 MFMAs), weights pre-split per weight version (csrc/gemm_h2.h); f32x3 = the same with three "
                         "bf16 terms (6 MFMAs, csrc/gemm_x3.h; launches of 129-192 rows on the exact kernels); f32 = the exact fp32 fma chain for "
                         "every launch; bf16 = throughput mode (bf16 operands, fp32 accumulate, fp32 master weights).  Every parity test runs in "
                         "f16x2, f32x3 and f32 (tests/conftest.py)")
    ap.add_argument("--full", action="store_true", help="also measure everything beside the headline: roofline, CPU baseline, the default line's "
                                                        "XE step and other flavours / workloads, beam5idx's dense-format comparison")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the XE-step leg of the default line")
    ap.add_argument("--no-alt", action="store_true", help="with --full: skip the other-flavour legs (f32 / f32x3 / f16x2 / bf16) and the greedy / 13-image legs of the default line")
    ap.add_argument("--cpu-sample", type=int, default=12)
    ap.add_argument("--cpu-full", type=int, default=1, help="1: the CPU baseline's value is ONE as-written call at the workload's own batch size (0: the bounded sample only)")
    ap.add_argument("--batch", type=int, default=0, help="images per batch instead of 100 (experiments only: not the BASELINE workload)")
    ap.add_argument("--rows-bound", action="store_true", help="decode workloads with dense regions: hand the library the host-known number of non-padding region rows "
                                                              "(model.set_valid_rows_bound): the decode call then has no host synchronisation at all")
    ap.add_argument("--emit-ids", action="store_true", help="decode workloads: put the (B, T) word ids of the last timed step into config.ids (tests compare a sharded run with a single-process run)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL, one GPU per rank (the measurement); gloo = self-test of the multi-rank path on fewer GPUs than ranks")
    args = ap.parse_args()

    if args.batch > 0:
        CFG["B"] = args.batch
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))

    import torch
    import torch.distributed as dist
    from vsrcap import synth
    torch.manual_seed(0)        # the SCST step draws its sampling seed from torch's generator: same arguments, same draws
    D = Dist(torch, dist, args.backend)
    if args.gpus != D.world and D.rank == 0:
        print("bench.py: --gpus %d but the launcher started %d ranks; reporting n_gpus = %d" % (args.gpus, D.world, D.world), file=sys.stderr)

    if args.workload == "beam5_eval":
        line, weights, outputs = eval_bench(args, D, torch, dist, synth)
    elif args.workload == "xe_real":
        CFG.update(R0=100, R=20)
        args.workload = "xe"
        line, weights, outputs = train_bench(args, D, torch, dist, synth, args.steps, args.warmup)
        line["metric"] = "XE-step samples/sec at the real callers' shapes (100 pooled detections, 20 slots x 20 regions)"
    elif args.workload in ("xe", "xeidx", "scst"):
        line, weights, outputs = train_bench(args, D, torch, dist, synth, args.steps, args.warmup)
        if args.full and D.rank == 0 and D.world == 1 and not args.no_cpu and args.workload == "xe":
            line["cpu_baseline"] = cpu_baseline_xe(weights, min(args.cpu_sample, 16), torch, synth)
    else:
        line, weights, beam, outputs = decode_bench(args, D, torch, dist, synth)
        def optional(what, fn):
            # the legs below ride along with the headline: a failure in one of them (the same code on every rank, so a Python-level
            # error is raised by all ranks together) is reported in its place instead of costing the run its headline value
            try:
                return fn()
            except Exception as e:                              # noqa: BLE001 - reported, not swallowed
                print("bench.py: optional leg %s failed: %r" % (what, e), file=sys.stderr)
                return {"error": "%s: %r" % (what, e)}

        def xe_leg(dt, full):
            xb = argparse.Namespace(**vars(args))
            xb.workload, xb.dtype, xb.dump_outputs = "xe", dt, None
            bl, _, _ = train_bench(xb, D, torch, dist, synth, max(5, args.steps // 2), 2)
            keys = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "scaling", "dtype", "config", "roofline") if full \
                else ("value", "unit", "ms_per_step", "steps", "dtype", "roofline")
            return {k: bl[k] for k in keys}

        def decode_leg(dt):
            aa = argparse.Namespace(**vars(args))
            aa.dtype, aa.dump_outputs = dt, None
            aa.steps, aa.warmup = max(5, args.steps // 2), 2
            al, _, _, _ = decode_bench(aa, D, torch, dist, synth)
            return {k: al[k] for k in ("value", "unit", "ms_per_step", "steps", "dtype", "roofline")}

        if args.full and args.workload == "beam5" and not args.no_secondary:
            # the other half of BASELINE.json's metric in the same driver-timed run
            line["secondary"] = optional("secondary XE step", lambda: xe_leg(args.dtype, True))
            if not args.no_alt and "error" not in line["secondary"]:
                # configs[3] names bf16: the same XE step in the throughput mode, and in the exact-chain flavour, side by side
                line["secondary"]["alt_modes"] = {dt: optional("XE step " + dt, lambda dt=dt: xe_leg(dt, False))
                                                  for dt in ("f32", "bf16") if dt != args.dtype}
        if args.full and args.workload == "beam5" and not args.no_alt:
            # the same workload in the other GEMM flavours, always printed side by side (never the headline `value`):
            #   f32   = the exact k-ordered fp32 fma chain for every launch (v_mfma_f32_32x32x2_f32)
            #   f32x3 = fp32 products from three bf16 terms per operand, f16x2 = from two fp16 terms (same fixtures, same bounds: the GPU
            #           suite runs in every one of them)
            #   bf16  = throughput mode (tests/test_gpu_bf16.py states its deviation)
            line["alt_modes"] = {dt: optional("beam-5 " + dt, lambda dt=dt: decode_leg(dt)) for dt in ("f32", "f32x3", "f16x2", "bf16") if dt != args.dtype}
            # the regimes the one-m-tile kernels serve, driver-timed: greedy decoding (configs[1], M = 100) and the 13-image shard of a
            # strong-scaled batch (M = 13 / 65): short legs in the headline's flavour, never the headline `value`
            def workload_leg(workload, batch):
                aa = argparse.Namespace(**vars(args))
                aa.workload, aa.dump_outputs = workload, None
                aa.steps, aa.warmup = max(10, args.steps), 3
                old_b = CFG["B"]
                CFG["B"] = batch
                try:
                    al, _, _, _ = decode_bench(aa, D, torch, dist, synth)
                finally:
                    CFG["B"] = old_b
                return {k: al[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "dtype")} | {"batch": batch, "gemm_avg_launch_us": al["roofline"]["avg_launch_us"]}
            def real_xe_leg():
                xb = argparse.Namespace(**vars(args))
                xb.workload, xb.dump_outputs = "xe", None
                old = (CFG["R0"], CFG["R"])
                CFG.update(R0=100, R=20)
                try:
                    bl, _, _ = train_bench(xb, D, torch, dist, synth, max(5, args.steps // 2), 2)
                finally:
                    CFG.update(R0=old[0], R=old[1])
                return {k: bl[k] for k in ("value", "unit", "ms_per_step", "steps", "dtype")} | {"workload": bl["config"]["workload"], "roofline_frac": bl["roofline"]["frac"]}

            def eval_leg():
                aa = argparse.Namespace(**vars(args))
                aa.steps, aa.warmup, aa.dump_outputs = max(10, args.steps), 3, None
                bl, _, _ = eval_bench(aa, D, torch, dist, synth)
                return {k: bl[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "dtype")} | {"workload": bl["config"]["workload"]}
            if args.batch == 0 and D.world == 1:
                line["alt_workloads"] = {"greedy": optional("greedy leg", lambda: workload_leg("greedy", CFG["B"])),
                                         "beam5_batch13": optional("13-image leg", lambda: workload_leg("beam5", 13)),
                                         "xe_real": optional("real-shape XE leg", real_xe_leg),
                                         "beam5_eval": optional("eval-caller leg", eval_leg)}
        if args.full and D.rank == 0 and D.world == 1 and not args.no_cpu and args.workload != "beam5idx":
            line["cpu_baseline"] = cpu_baseline(weights, args.cpu_sample, beam, torch, synth, full_B=CFG["B"] if args.cpu_full else 0)
        # The driver's record keeps the standard top-level keys and `config`: the other half of BASELINE.json's metric (XE samples/s), the
        # exact-chain flavour and the one-m-tile regimes are therefore ALSO summarised inside `config` (full legs: `secondary`, `alt_modes`,
        # `alt_workloads` of this same line).  `vs_baseline` stays null (BASELINE.md holds no published number for this metric); the ratio to
        # the CPU baseline timed in this run - BASELINE.md section 4's ">= 50x" target - is config.vs_cpu_baseline.
        def pick(d, *keys):
            for k in keys:
                d = d.get(k) if isinstance(d, dict) else None
            return d
        cfgk = line["config"]
        sec = line.get("secondary")
        if pick(sec, "value") is not None:
            cfgk["xe_samples_per_s"], cfgk["xe_ms_per_step"] = sec["value"], sec["ms_per_step"]
            cfgk["xe_roofline_frac"] = pick(sec, "roofline", "frac")
            for dt in ("f32", "bf16"):
                if pick(sec, "alt_modes", dt, "value") is not None:
                    cfgk["xe_%s_samples_per_s" % dt] = sec["alt_modes"][dt]["value"]
        for dt, key in (("f32", "f32_exact_tokens_per_s"), ("f32x3", "f32x3_tokens_per_s"), ("bf16", "bf16_tokens_per_s")):
            if pick(line, "alt_modes", dt, "value") is not None:
                cfgk[key] = line["alt_modes"][dt]["value"]
        for wl, key, field in (("greedy", "greedy_tokens_per_s", "value"), ("beam5_batch13", "batch13_ms", "ms_per_step"),
                               ("xe_real", "xe_real_samples_per_s", "value"), ("beam5_eval", "beam5_eval_tokens_per_s", "value")):
            if pick(line, "alt_workloads", wl, field) is not None:
                cfgk[key] = line["alt_workloads"][wl][field]
        if pick(line, "cpu_baseline", "value"):
            # two significant digits: the CPU leg is 2 / 3 timed calls of ~20 s and moves +-10 % from box to box (84.7 .. 104.8 tokens/s
            # over three boxes); the number of timed calls rides beside it
            sig2 = lambda x: float("%.2g" % x)
            cfgk["vs_cpu_baseline"] = sig2(line["value"] / line["cpu_baseline"]["value"])
            cfgk["vs_cpu_baseline_hoisted"] = sig2(line["value"] / line["cpu_baseline"]["hoisted_value"])
            cfgk["cpu_baseline_timed_calls"] = line["cpu_baseline"].get("timed_calls")
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)
    if D.rank == 0:
        print(json.dumps(line), flush=True)
    if D.world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
