"""sample_rl(..., samples_per_image=K, greedy_baseline=True): the greedy decode of every image - SCST's self-critical baseline - as one
more decoder row per image in the same call as its K samples (include/vsrcap.h, vsr_sample_rows_baseline).

Decoder row b (K + 1) is the baseline of image b, the K rows behind it are its samples; the samples land in the (B K, T) tensors of
the samples_per_image=K call (row b K + j, which also keys their noise and names their forced ids), the baseline in (B, T) tensors of its
own.  K = 5 on three images = 18 decoder rows: the row map, rows of one image on different slots, the last-slot clamp (L = 3 < T = 7) and
the per-destination writes all occur.

Configurations "a" (g3_beam_small's) and "b" (CFG_B) are those of tests/test_gpu_multi_sample.py, and the bounds are that file's:
|loss - oracle loss| < 1e-4, log-probs atol 2e-4, every one of the 28 gradients within 3e-3 of its scale; the step test's are 1e-4 on the
loss and 1e-6 relative on the weights.

Input condition of the token comparisons (checked on the CPU when these inputs were chosen): on every input used for a baseline
comparison here - "a", "b" and the index-list configuration - the fp32 as-written oracle and the fp64 oracle give the same greedy
tokens on every row, so a token is not decided by fp32 rounding.  No row is excluded.

conftest.py multiplies the modules it lists by the three fp32 GEMM flavours; this module does the same for itself (`flavour`)."""
import ctypes as C
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

CFG_B = dict(V=61, B=3, R0=6, R=7, D=128, L=3, T=7, E=32, H=48, A=16)          # L < T: late steps share the last slot
GAINS_B = {k: 1.5 for k in synth.DEFAULT_GAINS}
CFG_IDX = dict(V=60, B=3, R0=9, R=7, D=128, L=4, T=8, E=32, H=48, A=16)        # (test_index_lists_equal_dense's)


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


_SETUPS, _GREEDY = {}, {}


def _setup(which):
    """(cfg, weights, det, ctrl) of one of the two configurations, on the CPU (built once, never written)"""
    if which not in _SETUPS:
        if which == "a":
            meta, _ = load_golden("g3_beam_small")
            cfg, seed = dict(meta["cfg"]), meta["seed"]
            w = helpers.weights_for(cfg)
        else:
            cfg, seed = dict(CFG_B), 12
            w = synth.make_weights(cfg["V"], cfg["D"], cfg["E"], cfg["H"], cfg["A"], seed=4, gains=GAINS_B)
        det, ctrl = helpers.decode_inputs(cfg, seed)
        _SETUPS[which] = (cfg, w, det, ctrl)
    return _SETUPS[which]


def _oracle_greedy(which):
    """the CPU oracle's greedy tokens of a configuration: computed once, shared"""
    if which not in _GREEDY:
        cfg, w, det, ctrl = _setup(which)
        with torch.no_grad():
            _GREEDY[which] = vo.Oracle(w, cfg["T"], 2, as_written=True).test(det, ctrl)
    return _GREEDY[which]


def _rewards(M):
    reward = torch.from_numpy(synth.hash_u01(M, 70, 1).astype(np.float32))
    base = torch.from_numpy(synth.hash_u01(M, 71, 1).astype(np.float32))
    return reward, base


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def _check(got, want, rtol):
    for k in want:
        g, r = got[k].double(), want[k].double()
        scale = r.abs().max().item() + 1e-12
        err = (g - r).abs().max().item()
        assert err <= rtol * scale + 1e-9, "%s: max err %.3e vs scale %.3e" % (k, err, scale)


def _slots(gates, L):
    z = torch.zeros_like(gates[:, :1])
    return torch.cat([z, torch.clamp(torch.cumsum(gates[:, :-1], 1), max=L - 1)], 1)


def _step(m, det, ctrl, K, reward, base, baseline, **kw):
    """one forward + backward of the SCST loss; returns (samples, detached log-probs, loss, gradients, baseline tokens or None)"""
    m.train()
    m.zero_grad()
    res = m.sample_rl(det, ctrl, samples_per_image=K, **(dict(kw, greedy_baseline=True) if baseline else kw))
    assert len(res) == (3 if baseline else 2)
    (sw, sg), (lw, lg) = res[0], res[1]
    assert lw.requires_grad and lg.requires_grad
    loss = vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV))
    loss.backward()
    return (sw, sg), (lw.detach(), lg.detach()), loss.item(), _grads(m), (res[2] if baseline else None)


# ---------------------------------------------------------------------------------------------------- 1. baseline = greedy
@pytest.mark.parametrize("which,K", [("a", 5), ("b", 5), ("b", 1)], ids=["a-K5", "b-K5", "b-K1"])
def test_baseline_rows_are_the_greedy_decode(which, K):
    cfg, w, det, ctrl = _setup(which)
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    B, T = cfg["B"], cfg["T"]
    m = helpers.build_model(cfg, w, DEV)
    # .train() under grad: no decode cache, the selection kernel of its own
    m.train()
    (sw, sg), (lw, lg), (bw_t, bg_t) = m.sample_rl(det, ctrl, samples_per_image=K, greedy_baseline=True, seed=11)
    assert lw.requires_grad and lg.requires_grad
    assert tuple(sw.shape) == tuple(lw.shape) == (B * K, T) and tuple(bw_t.shape) == tuple(bg_t.shape) == (B, T)
    assert bw_t.dtype == torch.int64 and bg_t.dtype == torch.int64
    # .eval() under no_grad: the selection rides in the next step's LSTM1 kernel
    m.eval()
    with torch.no_grad():
        _, _, (bw_e, bg_e) = m.sample_rl(det, ctrl, samples_per_image=K, greedy_baseline=True, seed=11)
        tw, tg = m.test(det, ctrl)
    ow, og = _oracle_greedy(which)
    for name, (bw, bg) in (("train", (bw_t, bg_t)), ("eval", (bw_e, bg_e))):
        assert torch.equal(bw, tw) and torch.equal(bg, tg), "%s mode: the baseline rows differ from test() of this build" % name
        assert torch.equal(bw.cpu(), ow) and torch.equal(bg.cpu(), og), "%s mode: the baseline rows differ from the oracle's greedy decode" % name


# ---------------------------------------------------------------------------------------------------- 2. samples under replay
@pytest.mark.parametrize("which", ["a", "b"])
def test_replayed_samples_vs_oracle_and_vs_the_call_without_baseline(which):
    K = 5
    cfg, w, det, ctrl = _setup(which)
    M, L = cfg["B"] * K, cfg["L"]
    m = helpers.build_model(cfg, w, DEV).train()
    reward, base = _rewards(M)
    dd, cc = det.to(DEV), ctrl.to(DEV)
    with torch.no_grad():
        (sw, sg), _ = m.sample_rl(dd, cc, samples_per_image=K, seed=11)
    s = _slots(sg.cpu(), L).reshape(cfg["B"], K, -1)
    assert any(len(set(s[b, :, t].tolist())) > 1 for b in range(cfg["B"]) for t in range(1, s.shape[2])), "rows of an image never part"
    (fw, fg), (lw, lg), loss, got, (bw, bg) = _step(m, dd, cc, K, reward, base, True, forced=(sw, sg))
    assert torch.equal(fw, sw) and torch.equal(fg, sg)
    ow, og = _oracle_greedy(which)
    assert torch.equal(bw.cpu(), ow) and torch.equal(bg.cpu(), og)          # (a forced launch: the baseline rows are still greedy)
    # the CPU oracle on the repeated images
    o = vo.Oracle(w, cfg["T"], 2, as_written=True)
    for k in o.p:
        o.p[k].requires_grad_(True)
    _, (olw, olg) = o.sample_rl(det.repeat_interleave(K, 0), ctrl.repeat_interleave(K, 0), forced=(sw.cpu(), sg.cpu()))
    oloss = vo.scst_loss(olw, olg, reward, base)
    oloss.backward()
    print("loss %.6f oracle %.6f  max |dlp_w| %.2e  max |dlp_g| %.2e" % (loss, oloss.item(), float((lw.cpu() - olw.detach()).abs().max()),
                                                                       float((lg.cpu() - olg.detach()).abs().max())))
    assert abs(loss - oloss.item()) < 1e-4
    np.testing.assert_allclose(lw.cpu().numpy(), olw.detach().numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(lg.cpu().numpy(), olg.detach().numpy(), atol=2e-4, rtol=0)
    _check(got, {k: o.p[k].grad for k in o.p}, 3e-3)
    # this build's samples_per_image=K call on the same forced samples
    _, (lw_k, lg_k), loss_k, g_k, _ = _step(m, dd, cc, K, reward, base, False, forced=(sw, sg))
    assert abs(loss - loss_k) < 1e-4
    assert float((lw - lw_k).abs().max()) <= 2e-4 and float((lg - lg_k).abs().max()) <= 2e-4
    _check(got, g_k, 3e-3)
    same = [k for k in g_k if torch.equal(got[k], g_k[k])]
    print("gradients bitwise equal with and without the baseline rows in the decode: %d of %d" % (len(same), len(g_k)))
    # the baseline rows took no part in the replay: the same forward over the same K rows per image, the same backward
    for k in g_k:
        assert torch.equal(got[k], g_k[k]), "%s differs with the baseline rows present: max |dg| %.3e" % (k, float((got[k] - g_k[k]).abs().max()))


# ---------------------------------------------------------------------------------------------------- 3. noise
def test_noise_is_keyed_by_the_sample_index_and_baseline_rows_draw_none():
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    B = cfg["B"]
    for mode in ("train", "eval"):
        m = helpers.build_model(cfg, w, DEV).train(mode == "train")
        with torch.no_grad():
            call = lambda seed: m.sample_rl(det, ctrl, samples_per_image=K, greedy_baseline=True, seed=seed)
            (w1, g1), (lw1, lg1), (bw1, bg1) = call(11)
            (w2, g2), (lw2, lg2), (bw2, bg2) = call(11)
            (w3, g3), _, (bw3, bg3) = call(12)
            (kw, kg), _ = m.sample_rl(det, ctrl, samples_per_image=K, seed=11)
        for x, y in ((w1, w2), (g1, g2), (lw1, lw2), (lg1, lg2), (bw1, bw2), (bg1, bg2)):
            assert torch.equal(x, y), "%s mode: the same seed gave other bytes" % mode
        assert not torch.equal(w1, w3), "%s mode: another seed gave the same samples" % mode
        assert torch.equal(bw1, bw3) and torch.equal(bg1, bg3), "%s mode: the baseline rows depend on the seed" % mode
        rows = w1.reshape(B, K, -1).cpu()
        assert all(len({tuple(r.tolist()) for r in rows[b]}) > 1 for b in range(B)), "all K samples of an image are equal"
        # the key rule: at step 0 the state is zero, so sample j of image b sees the logits and the noise (seed, b K + j, 0) of the
        # samples_per_image=K call - the same word and gate but for a rounding near-tie (seed 11 has none in any flavour)
        assert torch.equal(w1[:, 0], kw[:, 0]) and torch.equal(g1[:, 0], kg[:, 0]), "%s mode: step-0 samples differ from the K-row call's" % mode
        # (later steps: the two calls have other GEMM row counts, a freely sampled token may differ)
        print("%s mode: whole captions equal to the samples_per_image=%d call: %d of %d" % (mode, K, int(((w1 == kw).all(1) & (g1 == kg).all(1)).sum()), B * K))


# ---------------------------------------------------------------------------------------------------- 4. region formats and interface
def test_index_lists_equal_dense():
    K = 5
    cfg = CFG_IDX
    w = helpers.weights_for(cfg, gains=GAINS_B)
    det = torch.from_numpy(synth.make_detections(cfg["B"], cfg["R0"], cfg["D"], seed=44, min_valid=4)).to(DEV)
    idx = torch.from_numpy(synth.make_slot_indices(cfg["B"], cfg["L"], cfg["R"], cfg["R0"], seed=44)).to(DEV)
    reg = IndexedRegions(det, idx)
    dense = reg.dense().contiguous()
    m = helpers.build_model(cfg, w, DEV).train()
    reward, base = _rewards(cfg["B"] * K)
    with torch.no_grad():
        (sw, sg), _ = m.sample_rl(det, dense, samples_per_image=K, seed=5)
    _, (lw_d, lg_d), loss_d, g_d, (bw_d, bg_d) = _step(m, det, dense, K, reward, base, True, forced=(sw, sg))
    _, (lw_i, lg_i), loss_i, g_i, (bw_i, bg_i) = _step(m, det, reg, K, reward, base, True, forced=(sw, sg))
    assert torch.equal(bw_i, bw_d) and torch.equal(bg_i, bg_d)
    assert abs(loss_i - loss_d) < 1e-4
    assert float((lw_i - lw_d).abs().max()) <= 2e-4 and float((lg_i - lg_d).abs().max()) <= 2e-4
    _check(g_i, g_d, 3e-3)
    assert float(g_i["att_va.weight"].abs().max()) > 0


def test_interface():
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    B, T = cfg["B"], cfg["T"]
    m = helpers.build_model(cfg, w, DEV).train()
    with pytest.raises(ValueError, match="samples_per_image.*greedy_baseline"):
        m.sample_rl(det, ctrl, samples_per_image=_lib.MAX_BEAM, greedy_baseline=True)
    # no graph under no_grad
    with torch.no_grad():
        (sw, sg), (lw, lg), (bw, bg) = m.sample_rl(det, ctrl, samples_per_image=K, greedy_baseline=True, seed=11)
    assert lw.grad_fn is None and lg.grad_fn is None and not lw.requires_grad
    assert tuple(sw.shape) == (B * K, T) and tuple(bw.shape) == (B, T)
    # a row -> image map still cannot train
    idx = torch.from_numpy(synth.make_slot_indices(B, cfg["L"], cfg["R"], cfg["R0"], seed=3)).to(DEV)
    mapped = IndexedRegions(det, idx, torch.arange(B, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="one decoder row per image"):
        m.sample_rl(det, mapped, samples_per_image=K, greedy_baseline=True, seed=11)
    # the library's own refusals, after a prepare with a smaller beam
    eng = m._engine(det.device)
    eng.prepare(det, ctrl, 3)
    with pytest.raises(RuntimeError, match="exceed the prepared beam 3"):
        eng.sample(B, det.device, 11, None, 3, greedy_baseline=True)
    out = [torch.empty(B * 2, T, dtype=dt, device=DEV) for dt in (torch.int64, torch.int64, torch.float32, torch.float32)]
    base = [torch.empty(B, T, dtype=torch.int64, device=DEV) for _ in range(2)]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(det.device).cuda_stream)
    assert eng.lib.vsr_sample_rows_baseline(eng.h, 0, C.c_uint64(11), None, None, *[ptr(t) for t in out], ptr(base[0]), ptr(base[1]), stream) != 0
    assert b"rows_per_image 0 < 1" in eng.lib.vsr_last_error()
    for bad in ((None, ptr(base[1])), (ptr(base[0]), None)):
        assert eng.lib.vsr_sample_rows_baseline(eng.h, 2, C.c_uint64(11), None, None, *[ptr(t) for t in out], bad[0], bad[1], stream) != 0
        assert b"vsr_sample_rows_baseline: null output" in eng.lib.vsr_last_error()
    assert eng.lib.vsr_sample_rows_baseline(eng.h, 2, C.c_uint64(11), ptr(out[0]), None, *[ptr(t) for t in out], ptr(base[0]), ptr(base[1]), stream) != 0
    assert b"go together" in eng.lib.vsr_last_error()
    # ... and the call it accepts on that handle: two samples + the baseline within the beam of 3
    (w2, _), _, (b2, _) = eng.sample(B, det.device, 11, None, 2, greedy_baseline=True)
    assert tuple(w2.shape) == (B * 2, T) and torch.equal(b2, bw)


# ---------------------------------------------------------------------------------------------------- 5. scst_step
def test_scst_step_with_greedy_baseline_equals_the_step_without():
    from vsrcap import parallel
    K = 5
    cfg, w, det, ctrl = _setup("b")
    det, ctrl = det.to(DEV), ctrl.to(DEV)
    B, T, M = cfg["B"], cfg["T"], cfg["B"] * K
    reward = torch.from_numpy(synth.hash_u01(M, 70, 1).astype(np.float32)).to(DEV)
    base_img = torch.from_numpy(synth.hash_u01(B, 71, 1).astype(np.float32)).to(DEV)       # one baseline reward per image
    seen = []

    def reward_fn_baseline(words, base_words):
        seen.append((tuple(words.shape), tuple(base_words.shape)))
        return reward, base_img

    def reward_fn(words):
        seen.append(tuple(words.shape))
        return reward, base_img.repeat_interleave(K)
    with torch.no_grad():
        (sw, sg), _ = helpers.build_model(cfg, w, DEV).sample_rl(det, ctrl, samples_per_image=K, seed=11)
    after = []
    for baseline in (True, False):
        m = helpers.build_model(cfg, w, DEV).train()
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        step = parallel.DataParallelStep(m, opt, sample_fn=lambda d, c, **kw: m.sample_rl(d, c, forced=(sw, sg), **kw))
        if baseline:
            loss = step.scst_step(det, ctrl, reward_fn_baseline, samples_per_image=K, greedy_baseline=True)
        else:
            loss = step.scst_step(det, ctrl, reward_fn, samples_per_image=K)
        step.close()
        after.append((float(loss), {k: p.detach().cpu().clone() for k, p in m.named_parameters()}))
    assert seen == [((M, T), (B, T)), (M, T)]
    print("loss with the baseline rows %.6f, without %.6f" % (after[0][0], after[1][0]))
    assert abs(after[0][0] - after[1][0]) < 1e-4
    moved = 0.0
    for k, a in after[1][1].items():
        err = float((after[0][1][k] - a).abs().max())
        assert err <= 1e-6 * max(float(a.abs().max()), 1e-3) + 1e-6, "%s: max |dw| %.3e" % (k, err)
        moved = max(moved, float((a - torch.from_numpy(np.ascontiguousarray(w[k]))).abs().max()))
    assert moved > 1e-4, "the step did not move the weights"
