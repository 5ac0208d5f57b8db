"""Pin the yardstick of the S-SSP training tests to the reference: tests/ssp_train_ref.py's oracle in fp64 - oracle/ssp_oracle.py's
stacks with the 33 dropout sites and the label-smoothed KL loss of models/sort_model.py:80-103 - reproduces what the reference's own
S_SSP gives under autograd, without dropout and with injected masks (tests/golden/make_golden_ssp_train.py -> g17_ssp_train.npz),
and the library's mask layout is the site table."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import ssp_train_ref as ref
from vsrcap import synth

REFERENCE = "/root/reference"


def _oracle_run(meta, with_masks):
    w = synth.make_ssp_weights(meta["seed"])
    verbs, roles = synth.make_ssp_inputs(meta["S"], meta["seed"])
    gt = ref.make_gt(roles, meta["seed"])
    masks = ref.hash_masks(meta["S"], meta["seed"]) if with_masks else None
    return ref.oracle_run(w, verbs, roles, gt, masks, torch.float64)


def _assert_close(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        g, r = got[k].double(), torch.as_tensor(want[k]).double()
        assert g.shape == r.shape, (what, k)
        err, scale = float((g - r).abs().max()), float(r.abs().max())        # (scale 0: 32 positions of v_embed rows no sequence reads)
        assert err <= 1e-10 * scale, "%s %s: %.3e against max |ref| %.3e" % (what, k, err, scale)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fp64_oracle_reproduces_the_reference_fixture(tag):
    meta, g = load_golden("g17_ssp_train")
    run = _oracle_run(meta, tag == "b")
    want_loss = meta["loss_" + tag]
    assert abs(run["loss"] - want_loss) <= 1e-10 * abs(want_loss)
    assert sorted(run["grads"]) == meta["names"] and len(meta["names"]) == 112
    assert not any("cross_attention" in k for k in run["grads"])              # never called: no gradient, here as under the reference
    _assert_close(ref.summarise(run), ref.unpack(g[tag], meta["names"], want_loss), "fixture run " + tag)
    assert all(float(v.abs().max()) > 0 for k, v in run["grads"].items())     # every gradient is alive


def test_masks_change_the_run():
    meta, g = load_golden("g17_ssp_train")
    assert abs(meta["loss_a"] - meta["loss_b"]) > 1e-3 * abs(meta["loss_a"])
    assert not np.array_equal(g["a"], g["b"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "models")), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("tag", ["a", "b"])
def test_fp64_oracle_matches_a_live_reference_run(tag):
    """in full and element-wise: every gradient tensor, not its summary"""
    meta, _ = load_golden("g17_ssp_train")
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    saved_path, saved_mods = list(sys.path), {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved_mods:
        del sys.modules[k]
    sys.path.insert(0, here)
    try:
        import make_golden_ssp_train as mk           # (puts the reference tree in front of sys.path)
        live = mk.reference_run(meta["S"], meta["seed"], ref.hash_masks(meta["S"], meta["seed"]) if tag == "b" else None)
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.") or k == "make_golden_ssp_train"]:
            del sys.modules[k]                       # (the generator too: its import is what puts the reference in front)
        sys.modules.update(saved_mods)
        sys.path[:] = saved_path
    run = _oracle_run(meta, tag == "b")
    assert abs(run["loss"] - live["loss"]) <= 1e-10 * abs(live["loss"])
    _assert_close(run["grads"], live["grads"], "live reference run " + tag)


@pytest.mark.parametrize("S", [1, 3, 24])
def test_mask_layout_is_the_site_table(S):
    """pure host functions of the library: the 33 sites one after the other, each from a 16-byte boundary, nothing else in the buffer"""
    from vsrcap import _lib
    from vsrcap.ssp import ssp_site_shapes
    lib = _lib.load()
    shapes = ref.site_shapes(S)
    assert ssp_site_shapes(S) == shapes and len(shapes) == ref.N_SITES
    sizes = [int(np.prod(sh)) for sh in shapes]
    offs = [lib.vsr_ssp_mask_offset(S, i) for i in range(ref.N_SITES)]
    total = lib.vsr_ssp_mask_bytes(S)
    gaps = 0
    for i, (o, n) in enumerate(zip(offs, sizes)):
        assert o % 16 == 0
        end = offs[i + 1] if i + 1 < ref.N_SITES else total
        assert 0 <= end - (o + n) < 16, i                                     # the next site starts on the first boundary behind this one
        gaps += end - (o + n)
    assert offs[0] == 0 and sum(sizes) == total - gaps
    assert lib.vsr_ssp_mask_bytes(0) == 0 and lib.vsr_ssp_tape_bytes(0) == 0 and lib.vsr_ssp_train_workspace_bytes(0) == 0
    assert lib.vsr_ssp_tape_bytes(S) > 0 and lib.vsr_ssp_train_workspace_bytes(S) > 0
