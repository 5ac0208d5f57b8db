"""The all-DMA f16x2 kernel (csrc/gemm_h2a.h) in both MFMA shapes of its multipliers: v_mfma_f32_16x16x32_f16 (the default) and
v_mfma_f32_32x32x16_f16 (VSR_H2_MFMA=32 in the library, H2_MFMA=32 in tools/gemm_bench).  The default shape is what every other
f16x2 test runs; here the 32x32 path keeps its fuzz coverage, and the headline decode keeps the reference's tokens in both."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden
import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gemm_bench")


@pytest.mark.parametrize("variant", ["5400 1", "5400 21", "5400 21 nw4"])
def test_h2a_mfma32_on_random_ragged_launches(variant):
    if not os.path.exists(TOOL):
        pytest.skip("tools/gemm_bench not built (python vsr-guided-cic_amd/build.py --tool, or __graft_entry__.build())")
    v = variant.split()
    env = dict(os.environ, H2_MFMA="32")
    if v[-1] == "nw4":
        env["H2_NW"] = "4"
    r = subprocess.run([TOOL, "fuzz"] + v[:2] + ["16", "5"], capture_output=True, text=True, timeout=600, env=env)
    tail = "\n".join(r.stdout.splitlines()[-20:])
    assert r.returncode == 0 and "0 of 16 cases failed" in r.stdout, tail + r.stderr[-2000:]


@pytest.mark.parametrize("mfma", ["16", "32"])
def test_beam5_batch100_both_mfma_shapes_vs_reference(mfma, monkeypatch):
    """beam-5 and greedy at the headline shape (batch 100) on the fixture rows test_gpu_headline.py pins, in each shape."""
    monkeypatch.setenv("VSR_H2_MFMA", mfma)
    monkeypatch.setenv("VSR_COMPUTE_DTYPE", "f16x2")                 # the flavour whose wide launches take the all-DMA kernel
    meta, g = load_golden("g3_beam")
    _, gg = load_golden("g2_greedy")
    cfg = meta["cfg"]
    w = helpers.weights_for(cfg, wseed=meta.get("wseed", 0))
    m = helpers.build_model(cfg, w, DEV, bos=meta["bos"])         # a fresh model -> a fresh handle that reads the environment
    det, ctrl = helpers.decode_inputs(cfg, meta["seed"])
    solid = g["agree64"].astype(bool)
    lo, hi = 0, 100
    d, c = det[lo:hi].contiguous().to(DEV), ctrl[lo:hi].contiguous().to(DEV)
    with torch.no_grad():
        (bw, bg), _ = m.beam_search((d, c), meta["eos"], 5, 1)
        gw, ggate = m.test(d, c)
    bw, bg = bw.cpu().numpy(), bg.cpu().numpy()
    same = (bw == g["words"][lo:hi]).all(1) & (bg == g["gates"][lo:hi]).all(1)
    assert same[solid[lo:hi]].all(), "VSR_H2_MFMA=%s: beam-5 rows %s differ" % (mfma, np.nonzero(~same & solid[lo:hi])[0][:10])
    assert same.mean() >= 0.98
    np.testing.assert_array_equal(gw.cpu().numpy(), gg["words"][lo:hi].astype(np.int64))
    np.testing.assert_array_equal(ggate.cpu().numpy(), gg["gates"][lo:hi].astype(np.int64))
