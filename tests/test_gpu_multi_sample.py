"""sample_rl(..., samples_per_image=K): K samples of every image in one call, the image's statics shared forward and backward.

The reference draws one sample per image and its SCST caller repeats every image K times (coco_scripts/train.py:151-178).  Here row
b * K + j is sample j of image b - the order of repeat_interleave(K, 0) - so everything is checked against the repeated-image form:
the CPU oracle's autograd on the repeated tensors (bounds of tests/test_gpu_train.py::test_scst_step_gradients_vs_oracle, which pin
the K = 1 path), and the K = 1 call of this build on the repeated tensors.

Bounds: |loss - oracle loss| < 1e-4, lp_w atol 2e-4, every one of the 28 gradients within 3e-3 of its scale (max |reference|).

conftest.py multiplies the modules it lists by the three fp32 GEMM flavours; this module does the same for itself (`flavour`)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import helpers
import vsr_oracle as vo
from vsrcap import _lib, synth
from vsrcap.regions import IndexedRegions

pytestmark = pytest.mark.gpu
DEV = "cuda"

CFG_B = dict(V=61, B=3, R0=6, R=7, D=128, L=3, T=7, E=32, H=48, A=16)          # M = 15 rows at K = 5; L < T: late steps share the last slot
GAINS_B = {k: 1.5 for k in synth.DEFAULT_GAINS}


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


def _setup(which, B=None, **flags):
    """(cfg, weights, det, ctrl) of one of the two configurations, on the CPU"""
    if which == "a":
        meta, _ = load_golden("g3_beam_small")
        cfg, seed = dict(meta["cfg"]), meta["seed"]
        w = helpers.weights_for(cfg)
    else:
        cfg, seed = dict(CFG_B), 12
        w = synth.make_weights(cfg["V"], cfg["D"], cfg["E"], cfg["H"], cfg["A"], seed=4, gains=GAINS_B, **flags)
    det, ctrl = helpers.decode_inputs(cfg, seed, n=B)
    if B is not None:
        cfg["B"] = B
    return cfg, w, det, ctrl


def _rewards(M):
    reward = torch.from_numpy(synth.hash_u01(M, 70, 1).astype(np.float32))
    base = torch.from_numpy(synth.hash_u01(M, 71, 1).astype(np.float32))
    return reward, base


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def _check(got, want, rtol):
    """a ceiling against the fp32 oracle; the tight bound (fp64 oracle, per kernel route) lives in tests/test_gpu_grad_routes.py"""
    for k in want:
        g, r = got[k].double(), want[k].double()
        scale = r.abs().max().item() + 1e-12
        err = (g - r).abs().max().item()
        assert err <= rtol * scale + 1e-9, "%s: max err %.3e vs scale %.3e" % (k, err, scale)


def _slots(gates, L):
    """slot read at step t: clamped running sum of the earlier gates"""
    z = torch.zeros_like(gates[:, :1])
    return torch.cat([z, torch.clamp(torch.cumsum(gates[:, :-1], 1), max=L - 1)], 1)


def _assert_not_degenerate(sw, sg, B, K, L):
    """the K rows of an image are not all the same caption, and at some t > 0 two rows of one image read the same slot"""
    w, s = sw.reshape(B, K, -1).cpu(), _slots(sg.cpu(), L).reshape(B, K, -1)
    assert all(len({tuple(r.tolist()) for r in w[b]}) > 1 for b in range(B)), "all K samples of an image are equal"
    shared = any(len(set(s[b, :, t].tolist())) < K for b in range(B) for t in range(1, s.shape[2]))
    assert shared, "no two rows of an image share a slot after step 0"
    distinct = any(len(set(s[b, :, t].tolist())) > 1 for b in range(B) for t in range(1, s.shape[2]))
    assert distinct, "the rows of every image always read the same slot"


def _step(m, det, ctrl, K, reward, base, **kw):
    """one forward + backward of the SCST loss; returns (samples, detached log-probs, loss, gradients)"""
    m.train()
    m.zero_grad()
    (sw, sg), (lw, lg) = m.sample_rl(det, ctrl, samples_per_image=K, **kw)
    assert lw.requires_grad and lg.requires_grad
    loss = vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV))
    loss.backward()
    return (sw, sg), (lw.detach(), lg.detach()), loss.item(), _grads(m)


CASES = [("a", 5, None, {}), ("a", 8, 2, {}), ("b", 5, None, {}), ("b", 8, 2, {}),
         ("b", 5, None, dict(img_second_lstm=True)), ("b", 5, None, dict(h2_first_lstm=False))]


@pytest.mark.parametrize("which,K,B,flags", CASES, ids=["a-K5", "a-K8", "b-K5", "b-K8", "b-K5-img2", "b-K5-noh2"])
def test_gradients_vs_oracle_on_repeated_images(which, K, B, flags):
    cfg, w, det, ctrl = _setup(which, B, **flags)
    M = cfg["B"] * K
    m = helpers.build_model(cfg, w, DEV, **flags)
    reward, base = _rewards(M)
    (sw, sg), (lw, lg), loss, got = _step(m, det.to(DEV), ctrl.to(DEV), K, reward, base, seed=11)
    assert tuple(sw.shape) == (M, cfg["T"]) and tuple(lw.shape) == (M, cfg["T"])
    _assert_not_degenerate(sw, sg, cfg["B"], K, cfg["L"])
    o = vo.Oracle(w, cfg["T"], 2, as_written=True, **flags)
    for k in o.p:
        o.p[k].requires_grad_(True)
    _, (olw, olg) = o.sample_rl(det.repeat_interleave(K, 0), ctrl.repeat_interleave(K, 0), forced=(sw.cpu(), sg.cpu()))
    oloss = vo.scst_loss(olw, olg, reward, base)
    oloss.backward()
    print("K=%d loss %.6f oracle %.6f  max |dlp_w| %.2e" % (K, loss, oloss.item(), float((lw.cpu() - olw.detach()).abs().max())))
    assert abs(loss - oloss.item()) < 1e-4
    np.testing.assert_allclose(lw.cpu().numpy(), olw.detach().numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(lg.cpu().numpy(), olg.detach().numpy(), atol=2e-4, rtol=0)
    _check(got, {k: o.p[k].grad for k in o.p}, 3e-3)


def test_shared_statics_equal_repeated_images():
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    det_r, ctrl_r = det.repeat_interleave(K, 0).contiguous(), ctrl.repeat_interleave(K, 0).contiguous()
    m = helpers.build_model(cfg, w, DEV).train()
    reward, base = _rewards(cfg["B"] * K)
    with torch.no_grad():
        (sw, sg), _ = m.sample_rl(det, ctrl, samples_per_image=K, seed=11)
        (rw, _), _ = m.sample_rl(det_r, ctrl_r, seed=11)          # the same Philox keys (seed, row, t)
    print("freely sampled captions equal in both forms: %d of %d" % (int((sw == rw).all(1).sum()), sw.shape[0]))
    _, (lw_s, lg_s), loss_s, g_s = _step(m, det, ctrl, K, reward, base, forced=(sw, sg))
    _, (lw_r, lg_r), loss_r, g_r = _step(m, det_r, ctrl_r, 1, reward, base, forced=(sw, sg))
    assert abs(loss_s - loss_r) < 1e-4
    assert float((lw_s - lw_r).abs().max()) <= 2e-4 and float((lg_s - lg_r).abs().max()) <= 2e-4
    _check(g_s, g_r, 3e-3)


def test_runs_repeat_bit_for_bit_and_seeds_name_the_noise():
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    m = helpers.build_model(cfg, w, DEV).train()
    reward, base = _rewards(cfg["B"] * K)
    (w1, g1), (lw1, lg1), _, gr1 = _step(m, det, ctrl, K, reward, base, seed=11)
    (w2, g2), (lw2, lg2), _, gr2 = _step(m, det, ctrl, K, reward, base, seed=11)
    assert torch.equal(w1, w2) and torch.equal(g1, g2)
    assert torch.equal(lw1, lw2) and torch.equal(lg1, lg2)
    for k in gr1:
        assert torch.equal(gr1[k], gr2[k]), k
    with torch.no_grad():
        (w3, _), _ = m.sample_rl(det, ctrl, samples_per_image=K, seed=12)
    assert not torch.equal(w1, w3)


def test_index_lists_equal_dense():
    K = 5
    cfg = dict(V=60, B=3, R0=9, R=7, D=128, L=4, T=8, E=32, H=48, A=16)
    w = helpers.weights_for(cfg, gains=GAINS_B)
    det = torch.from_numpy(synth.make_detections(cfg["B"], cfg["R0"], cfg["D"], seed=44, min_valid=4)).to(DEV)
    idx = torch.from_numpy(synth.make_slot_indices(cfg["B"], cfg["L"], cfg["R"], cfg["R0"], seed=44)).to(DEV)
    reg = IndexedRegions(det, idx)
    dense = reg.dense().contiguous()
    m = helpers.build_model(cfg, w, DEV).train()
    reward, base = _rewards(cfg["B"] * K)
    with torch.no_grad():
        (sw, sg), _ = m.sample_rl(det, dense, samples_per_image=K, seed=5)
    _, (lw_d, lg_d), loss_d, g_d = _step(m, det, dense, K, reward, base, forced=(sw, sg))
    _, (lw_i, lg_i), loss_i, g_i = _step(m, det, reg, K, reward, base, forced=(sw, sg))
    assert abs(loss_i - loss_d) < 1e-4
    assert float((lw_i - lw_d).abs().max()) <= 2e-4 and float((lg_i - lg_d).abs().max()) <= 2e-4
    _check(g_i, g_d, 3e-3)
    assert float(g_i["att_va.weight"].abs().max()) > 0


def test_interface():
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    m = helpers.build_model(cfg, w, DEV).train()
    for bad in (0, _lib.MAX_BEAM + 1):
        with pytest.raises(ValueError, match="samples_per_image"):
            m.sample_rl(det, ctrl, samples_per_image=bad)
    # K = 1 is the call without the argument, bit for bit
    reward1, base1 = _rewards(cfg["B"])
    a = _step(m, det, ctrl, 1, reward1, base1, seed=11)
    m.zero_grad()
    (bw, bg), (blw, blg) = m.sample_rl(det, ctrl, seed=11)
    vo.scst_loss(blw, blg, reward1.to(DEV), base1.to(DEV)).backward()
    assert torch.equal(a[0][0], bw) and torch.equal(a[0][1], bg) and torch.equal(a[1][0], blw.detach()) and torch.equal(a[1][1], blg.detach())
    gb = _grads(m)
    for k in gb:
        assert torch.equal(a[3][k], gb[k]), k
    # no graph under no_grad
    with torch.no_grad():
        (sw, sg), (lw, lg) = m.sample_rl(det, ctrl, samples_per_image=K, seed=11)
    assert lw.grad_fn is None and lg.grad_fn is None and not lw.requires_grad
    assert tuple(sw.shape) == (cfg["B"] * K, cfg["T"])
    # a row -> image map still cannot train
    idx = torch.from_numpy(synth.make_slot_indices(cfg["B"], cfg["L"], cfg["R"], cfg["R0"], seed=3)).to(DEV)
    mapped = IndexedRegions(det, idx, torch.arange(cfg["B"], dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="one decoder row per image"):
        m.sample_rl(det, mapped, samples_per_image=K, seed=11)


def test_decode_between_the_forward_and_its_backward_and_a_rows_bound():
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    m = helpers.build_model(cfg, w, DEV).train()
    reward, base = _rewards(cfg["B"] * K)
    (sw, sg), _, _, want = _step(m, det, ctrl, K, reward, base, seed=11)
    # a greedy decode (the SCST baseline) between the K-row forward and its backward
    m.zero_grad()
    _, (lw, lg) = m.sample_rl(det, ctrl, samples_per_image=K, forced=(sw, sg))
    with torch.no_grad():
        m.eval()
        words, _ = m.test(det, ctrl)
        m.train()
    vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV)).backward()
    got = _grads(m)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert tuple(words.shape) == (cfg["B"], cfg["T"])
    # a safe bound on the non-padding region rows: no read-back, the same gradients.
    # (i) the tightest safe bound, the count itself: every launch has the rows it has without a bound, so the gradients are the same
    #     bits - but for att_va's, whose weight-gradient GEMM reads its rows through the device-side limit (the rule of
    #     tests/test_gpu_rows_bound.py: 0, and 2e-5 of the scale for att_va).
    # (ii) a loose bound, every slot entry: att_va's projection in prepare() then runs over 63 rows instead of 25 and may take another
    #     GEMM kernel and k split (the exact-fp32 flavour routes launches of <= 40 rows to its rows-16 kernel), so P - and through it
    #     every gradient - is the same sum in another order: the bounds this file holds two GEMM plans of one computation to
    #     (test_shared_statics_equal_repeated_images).
    exact = int((ctrl.sum(-1) != 0).sum())
    total = cfg["B"] * cfg["L"] * cfg["R"]
    assert exact + 16 < total
    m.set_valid_rows_bound(exact)
    _, _, _, tight = _step(m, det, ctrl, K, reward, base, forced=(sw, sg))
    m.set_valid_rows_bound(total)
    _, (lw_b, _), loss_b, loose = _step(m, det, ctrl, K, reward, base, forced=(sw, sg))
    m.set_valid_rows_bound(None)
    for k in want:
        tol = 0.0 if k != "att_va.weight" else 2e-5 * (float(want[k].abs().max()) + 1e-30)
        err = float((tight[k] - want[k]).abs().max())
        print("bound = count: %s max |dg| %.3e" % (k, err))
        assert err <= tol, k
    assert abs(loss_b - vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV)).item()) < 1e-4
    assert float((lw_b - lw.detach()).abs().max()) <= 2e-4
    _check(loose, want, 3e-3)


def test_scst_step_with_samples_per_image_equals_the_repeated_step():
    from vsrcap import parallel
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    det_r, ctrl_r = det.repeat_interleave(K, 0).contiguous(), ctrl.repeat_interleave(K, 0).contiguous()
    M = cfg["B"] * K
    reward, base = (x.to(DEV) for x in _rewards(M))
    seen = []

    def reward_fn(words):
        seen.append(tuple(words.shape))
        return reward, base
    with torch.no_grad():
        (sw, sg), _ = helpers.build_model(cfg, w, DEV).sample_rl(det, ctrl, samples_per_image=K, seed=11)
    after = []
    for shared in (True, False):
        m = helpers.build_model(cfg, w, DEV).train()
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        # the samples are replayed in both forms: a freely sampled token may differ between them (other GEMM row counts)
        step = parallel.DataParallelStep(m, opt, sample_fn=lambda d, c, **kw: m.sample_rl(d, c, forced=(sw, sg), **kw))
        if shared:
            loss = step.scst_step(det, ctrl, reward_fn, samples_per_image=K)
        else:
            loss = step.scst_step(det_r, ctrl_r, reward_fn)
        step.close()
        after.append((float(loss), {k: p.detach().cpu().clone() for k, p in m.named_parameters()}))
    assert seen == [(M, cfg["T"])] * 2
    assert abs(after[0][0] - after[1][0]) < 1e-4
    moved = 0.0
    for k, a in after[1][1].items():
        err = float((after[0][1][k] - a).abs().max())
        assert err <= 1e-6 * max(float(a.abs().max()), 1e-3) + 1e-6, "%s: max |dw| %.3e" % (k, err)      # 1e-6 relative
        moved = max(moved, float((a - torch.from_numpy(np.ascontiguousarray(w[k]))).abs().max()))
    assert moved > 1e-4, "the step did not move the weights"
