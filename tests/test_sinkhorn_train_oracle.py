"""Pin the yardstick of the SinkhornNet training tests to the reference: oracle/ssp_oracle.py's SinkhornOracle in fp64, with
requires_grad_ on its parameters and the three loss lines of coco_scripts/train_sinkhorn.py:207-211, reproduces what the reference's
own SinkhornNet gives under autograd (tests/golden/make_golden_sinkhorn_train.py -> g16_sinkhorn_train.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import sinkhorn_train_ref as ref
from vsrcap import synth

REFERENCE = "/root/reference"


def _oracle_summary(meta):
    w = synth.make_sinkhorn_weights(meta["seed"])
    x, n = synth.make_sinkhorn_inputs(meta["Q"], meta["seed"])
    tr_locs, gt_locs = ref.make_locs(n, meta["N"], meta["seed"])
    run = ref.oracle_run(w, x, tr_locs, gt_locs, meta["n_iters"], meta["tau"], torch.float64, meta["scale"])
    return run, ref.summarise(run)


def _assert_close(got, want, what):
    for k in want:
        g, r = got[k].double(), torch.as_tensor(want[k]).double()
        assert g.shape == r.shape, (what, k)
        err = float((g - r).abs().max()) / float(r.abs().max())
        assert err <= 1e-10, "%s %s: %.3e of max |ref|" % (what, k, err)


def test_fp64_oracle_reproduces_the_reference_fixture():
    meta, g = load_golden("g16_sinkhorn_train")
    run, s = _oracle_summary(meta)
    assert abs(run["loss"] - meta["loss"]) <= 1e-10 * abs(meta["loss"])
    want = {k.replace("__", "/"): v for k, v in g.items()}
    assert set(want) == set(s) and len(want) == 2 + 6 + 3 * 4
    _assert_close(s, want, "fixture")
    assert float(s["W1_vis.weight/rows"].max()) > 0 and float(s["W_fc.bias"].abs().max()) > 0        # the gradients are alive


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "models")), reason="the reference tree is not on this machine")
def test_fp64_oracle_matches_a_live_reference_run():
    meta, _ = load_golden("g16_sinkhorn_train")
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    saved_path, saved_mods = list(sys.path), {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved_mods:
        del sys.modules[k]
    sys.path.insert(0, here)
    try:
        import make_golden_sinkhorn_train as mk          # (puts the reference tree in front of sys.path)
        live = mk.reference_run(meta["Q"], meta["seed"], meta["scale"])
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved_mods)
        sys.path[:] = saved_path
    run, s = _oracle_summary(meta)
    assert abs(run["loss"] - live["loss"]) <= 1e-10 * abs(live["loss"])
    _assert_close(s, ref.summarise(live), "live reference")
