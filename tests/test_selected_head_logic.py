"""The torch side of the sparse vocabulary head (vsrcap/train.py: xe_targets, xe_loss_from_selected) on the CPU: the XE loss computed
from one log-prob per (row, step) is the reference's loss computed from the dense (B, T, V) tensor (oracle/vsr_oracle.py: xe_loss =
coco_scripts/train.py:106-110)."""
import torch

import vsr_oracle as vo
from vsrcap import train

B, T, V = 3, 4, 7


def _case(seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.log_softmax(torch.randn(B, T, V, dtype=torch.float64, generator=g), -1)
    gate = torch.log_softmax(torch.randn(B, T, 2, dtype=torch.float64, generator=g), -1)
    caps = torch.randint(0, V, (B, T), generator=g)
    gts = torch.randint(0, 2, (B, T), generator=g)
    gts[0, 1] = gts[2, 3] = gts[1, 0] = -1               # ignore_index entries of the gate loss
    return out, gate, caps, gts


def test_xe_targets_shift_the_captions_and_leave_the_last_step_unselected():
    _, _, caps, _ = _case(0)
    tgt = train.xe_targets(caps)
    assert tgt.shape == caps.shape and tgt.dtype == caps.dtype
    assert torch.equal(tgt[:, :-1], caps[:, 1:])
    assert bool((tgt[:, -1] == -1).all())
    assert bool((tgt[:, :-1] >= 0).all()), "-1 in the last column only"


def test_xe_loss_from_selected_is_the_dense_loss():
    for seed in range(4):
        out, gate, caps, gts = _case(seed)
        tgt = train.xe_targets(caps)
        lp_sel = out.gather(2, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)       # (what sits at the unselected entries must not matter)
        got = train.xe_loss_from_selected(lp_sel, gate, tgt, gts)
        want = vo.xe_loss(out, gate, caps, gts)
        for g, w, name in zip(got, want, ("loss", "loss_cap", "loss_gate")):
            assert abs(float(g) - float(w)) <= 1e-12, "%s: %.15f vs %.15f (seed %d)" % (name, float(g), float(w), seed)


def test_gate_weight_scales_the_gate_term_only():
    out, gate, caps, gts = _case(5)
    tgt = train.xe_targets(caps)
    lp_sel = out.gather(2, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    loss, cap, gl = train.xe_loss_from_selected(lp_sel, gate, tgt, gts, gate_weight=2.5)
    assert abs(float(loss) - (float(cap) + 2.5 * float(gl))) <= 1e-12
