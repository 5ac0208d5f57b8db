"""The hand-written BPTT on every kernel route, element by element against the fp64 oracle (tests/grad_compare.py).

The other element-wise gradient checks run where every per-step launch has 3 to 24 rows; the fixtures that reach the routes below
compare 28 norms.  Here the shapes are what decides a route - rows and the threshold sizes - and everything else stays tiny:

  rows    41 first past gemm_r16_max; 81 first past x3s_max (with R = 72: softmax passes of k_attend / k_attend_bwd over more than
          64 entries, weighted sum in 4 chunks of 18); 128 the last launch with two attention parts and one m-tile, 129 the first
          without; 193 the first past gemm_x3_min_rows and the exact kernels' tm.  The weight-gradient K is B T = 123, 243, 384,
          387, 579: all but 384 are zero-filled to a multiple of 8.
  sizes   D = 2048 (k_attend<512>, QN = 5, a second score pass: R + 1 = 42 > 8 waves x 5), A = 512 (k_attend_bwd<512>), V = 4104
          (k_vocab<.., 512>, Vp = up8(V) padding of the dh2 product), H = 256 (weight-gradient products with M = 4H = 1024 and
          6H = 1536: the 128 x 128 tiles, k-aligned pieces); the same at 130 rows with D = 256 (one workgroup per attention row).
  SCST    samples_per_image = 5 at 130 rows (k_attend_bwd<.., true> with one part per row, k_dP_rows_sum past 128 rows) and at 40
          rows (two parts per row, below the rows-16 boundary).

The cases are named after the thresholds in csrc/gemm_route.h (GemmBuilder::finish) and csrc/vsrcap.hip (attend_parts, the
512-thread launches) as the source states them; no test here observes which kernel a launch took.  The GEMM kernels themselves
are fuzzed per kernel in tests/test_gpu_gemm_fuzz.py; this module checks the training pass's wiring around them.

All sizes are multiples of 8, so the f16x2 flavour really takes its kernels.  Gains 1.0.  Every case asserts that a region row is
padding and that a word id repeats within a step (the zero-row and the segmented-sum paths).

Bounds: grad_compare.compare at margin 16 x the fp32 oracle's own error against fp64, per tensor and metric, plus the older
2e-3 (SCST 3e-3) of max |ref| ceiling; loss 1e-4, log-probs 2e-4 against fp64.

conftest.py multiplies the modules it lists by the three fp32 GEMM flavours; this module does the same for itself (`flavour`)."""
import os

import numpy as np
import pytest
import torch

import grad_compare as gc
import helpers
import vsr_oracle as vo
from vsrcap import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

GAINS = {k: 1.0 for k in synth.DEFAULT_GAINS}
BASE = dict(V=56, R0=6, R=6, D=64, L=3, T=3, E=32, H=64, A=32)
SIZES = dict(V=4104, R0=6, R=41, D=2048, L=3, T=3, E=64, H=256, A=512)

XE_CASES = {
    "rows41": (dict(BASE, B=41), 23),
    "rows81-R72": (dict(BASE, B=81, R=72), 23),
    "rows128": (dict(BASE, B=128), 23),
    "rows129": (dict(BASE, B=129), 23),
    "rows193": (dict(BASE, B=193), 23),
    "sizes": (dict(SIZES, B=4), 51),                # the first seed at which two of the 4 rows read the same word at a step
    "sizes-rows130": (dict(SIZES, B=130, D=256), 23),
}
SCST_CASES = {
    "scst-rows130": (dict(BASE, B=26, T=5), 12),
    "scst-rows40": (dict(BASE, B=8, T=5), 12),
}
SCST_K = 5

# Per-tensor factors on the margin-16 bound: (case, flavour) -> {tensor: factor}, each with its named cause and measured ratio.
FACTORS = {}


@pytest.fixture(params=("f16x2", "f32x3", "f32"), autouse=True)
def flavour(request):
    import models
    old = models.set_default_compute_dtype(request.param)
    old_env = os.environ.get("VSR_COMPUTE_DTYPE")
    os.environ["VSR_COMPUTE_DTYPE"] = request.param
    yield request.param
    models.set_default_compute_dtype(old)
    if old_env is None:
        os.environ.pop("VSR_COMPUTE_DTYPE", None)
    else:
        os.environ["VSR_COMPUTE_DTYPE"] = old_env


_oracle_cache = {}


def _oracles(key, w, T, det, loss_fn, **kw):
    """(fp64 reference, fp32 yardstick) of one case, computed once and shared by the flavours; never modified"""
    if key not in _oracle_cache:
        _oracle_cache[key] = tuple(gc.oracle_grads(w, T, det, dt, loss_fn, **kw) for dt in (torch.float64, torch.float32))
    return _oracle_cache[key]


def _assert_edges(regions, words):
    """regions (..., R, D): some region row is padding; words (rows, steps): some id repeats within a step"""
    assert bool((regions.abs().sum(-1) == 0).any()), "no padding region row"
    assert any(len(set(words[:, t].tolist())) < words.shape[0] for t in range(words.shape[1])), "no word id repeats within a step"


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("case", list(XE_CASES))
def test_xe_gradients_vs_fp64_oracle(case, flavour):
    cfg, seed = XE_CASES[case]
    assert all(cfg[k] % 8 == 0 for k in ("V", "D", "E", "H", "A"))
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, seed)
    _assert_edges(ctrl_seq, caps)
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    out, gate = m((det.to(DEV),), (caps.to(DEV), ctrl_seq.to(DEV)))
    assert out.requires_grad and gate.requires_grad
    loss = vo.xe_loss(out, gate, caps.to(DEV), gts.to(DEV))[0]
    loss.backward()
    ref, yard = _oracles(case, w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    label = "%s %s" % (case, flavour)
    gc.check_outputs(loss.item(), out, gate, ref, label)
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 2e-3, FACTORS.get((case, flavour)), label)


@pytest.mark.parametrize("case", list(SCST_CASES))
def test_scst_gradients_vs_fp64_oracle(case, flavour):
    cfg, seed = SCST_CASES[case]
    assert all(cfg[k] % 8 == 0 for k in ("V", "D", "E", "H", "A"))
    K, M = SCST_K, cfg["B"] * SCST_K
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl = helpers.decode_inputs(cfg, seed)
    reward = torch.from_numpy(synth.hash_u01(M, 70, 1).astype(np.float32))
    base = torch.from_numpy(synth.hash_u01(M, 71, 1).astype(np.float32))
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    (sw, sg), (lw, lg) = m.sample_rl(det.to(DEV), ctrl.to(DEV), samples_per_image=K, seed=11)
    assert lw.requires_grad and lg.requires_grad and tuple(sw.shape) == (M, cfg["T"])
    loss = vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV))
    loss.backward()
    sw, sg = sw.cpu(), sg.cpu()
    _assert_edges(ctrl, sw[:, :-1])                                         # the words that steps 1 .. T-1 read (step 0 reads bos)
    key = (case, sw.numpy().tobytes(), sg.numpy().tobytes())                # a flavour may draw other samples
    ref, yard = _oracles(key, w, cfg["T"], det.repeat_interleave(K, 0), gc.scst_loss_fn(reward, base),
                         ctrl=ctrl.repeat_interleave(K, 0), forced=(sw, sg))
    label = "%s %s" % (case, flavour)
    gc.check_outputs(loss.item(), lw, lg, ref, label)
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 3e-3, FACTORS.get((case, flavour)), label)
