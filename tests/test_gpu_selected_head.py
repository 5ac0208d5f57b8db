"""The sparse vocabulary head (vsr_train_forward_selected / vsr_train_backward_selected, model.forward_selected / xe_loss /
sample_rl(sparse_head=True), DataParallelStep(sparse_head=True)): one log-prob per (row, step) leaves the library, the (T B, V)
log_softmax rows stay in the training workspace and the backward turns them into dlogits in place.

Shapes: the smallest that reach each branch of k_vocab_select / k_dlogits_sel (csrc/train_kernels.h) - 256 and 512 threads, the LDS row
and the slab re-read past VOCAB_LDS_MAX = 12288, 16-byte and scalar accesses, pad columns [V, up8(V)) - everything else as BASE of
tests/test_gpu_grad_routes.py.  Gains 1.0.

Bounds are the project's: grad_compare.compare at MARGIN against the fp64 oracle with the fp32 oracle as yardstick, ceiling 2e-3 (SCST
3e-3); loss 1e-4 and the selected log-probs 2e-4 against fp64.  bf16 is not a parity mode: its test holds the two heads to each other."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import grad_compare as gc
import helpers
import vsr_oracle as vo
from vsrcap import synth, train
from vsrcap.regions import IndexedRegions

pytestmark = pytest.mark.gpu
DEV = "cuda"

GAINS = {k: 1.0 for k in synth.DEFAULT_GAINS}
BASE = dict(V=56, R0=6, R=6, D=64, L=3, T=3, E=32, H=64, A=32)

XE_CASES = {
    "V56-rows41": (dict(BASE, B=41), 23),                    # 256 threads, LDS row, 16-byte accesses
    "V4104-rows4": (dict(BASE, V=4104, B=4), 23),            # 512 threads
    "V12296-rows3": (dict(BASE, V=12296, B=3, T=2), 23),     # past VOCAB_LDS_MAX: the slabs are re-read
    "V58-rows5": (dict(BASE, V=58, B=5), 23),                # scalar accesses, six pad columns
}
SCST_CFG, SCST_SEED, SCST_K = dict(BASE, B=8, T=5), 12, 5
SMALL = dict(BASE, B=9)


@pytest.fixture(params=("f16x2", "f32x3", "f32"))
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


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _check_selected(lp_sel, gate, targets, ref, label):
    """the selected log-probs within 2e-4 of the fp64 oracle's entries, exactly 0.0 where nothing is selected; gate log-probs 2e-4"""
    lp, tg = lp_sel.detach().double().cpu(), targets.cpu()
    want = ref["logp_words"].gather(2, tg.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    sel = tg >= 0
    dw = float((lp - want)[sel].abs().max()) if bool(sel.any()) else 0.0
    dg = float((gate.detach().double().cpu() - ref["logp_gates"]).abs().max())
    print("%s max |dlogp_sel| %.2e  max |dlogp_gates| %.2e" % (label, dw, dg))
    assert bool((lp_sel.detach()[~sel.to(lp_sel.device)] == 0).all()), "%s: an unselected entry is not exactly 0.0" % label
    assert dw <= 2e-4 and dg <= 2e-4, "%s log-probs off by %.3e (selected words) / %.3e (gates)" % (label, dw, dg)


# ------------------------------------------------------------------------------------------------------------------ 1. XE
@pytest.mark.parametrize("case", list(XE_CASES))
def test_xe_loss_gradients_vs_fp64_oracle(case, flavour):
    cfg, seed = XE_CASES[case]
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, seed)
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    d, s, c, g = _dev(det, ctrl_seq, caps, gts)
    loss, loss_cap, loss_gate = m.xe_loss(d, c, s, g)
    assert loss.requires_grad
    loss.backward()
    ref, yard = _oracles(case, w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    label = "%s %s" % (case, flavour)
    want = vo.xe_loss(ref["logp_words"], ref["logp_gates"], caps, gts)
    for got, wnt, name in zip((loss, loss_cap, loss_gate), want, ("loss", "loss_cap", "loss_gate")):
        print("%s |d%s| %.2e" % (label, name, abs(got.item() - float(wnt))))
        assert abs(got.item() - float(wnt)) < 1e-4, "%s %s %.7f vs fp64 %.7f" % (label, name, got.item(), float(wnt))
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 2e-3, None, label)
    V, Vp, TB = cfg["V"], (cfg["V"] + 7) // 8 * 8, cfg["T"] * cfg["B"]
    if Vp != V:                                              # the pad columns of the in-place dlogits rows
        dl = m._engine(torch.device(DEV)).debug_buffer("dlogits", (TB, Vp), torch.device(DEV))
        assert bool((dl[:, V:] == 0).all()), "pad columns [V, up8(V)) of dlogits are not exactly 0 after the backward"
        assert float(dl[:, :V].abs().max()) > 0
    # the same values without a graph (validation loss)
    tg = train.xe_targets(c)
    with torch.no_grad():
        lp_sel, gate = m.forward_selected((d,), (c, s), tg)
    assert not lp_sel.requires_grad and not gate.requires_grad and tuple(lp_sel.shape) == (cfg["B"], cfg["T"])
    _check_selected(lp_sel, gate, tg, ref, label)
    m.eval()
    lp_e, gate_e = m.forward_selected((d,), (c, s), tg)
    assert torch.equal(lp_e.detach(), lp_sel) and torch.equal(gate_e.detach(), gate)


# ------------------------------------------------------------------------------------------------------------------ 2. SCST
def test_scst_gradients_vs_fp64_oracle(flavour):
    cfg, seed, K = SCST_CFG, SCST_SEED, SCST_K
    M = cfg["B"] * K
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl = helpers.decode_inputs(cfg, seed)
    reward = torch.from_numpy(synth.hash_u01(M, 70, 1).astype(np.float32))
    base = torch.from_numpy(synth.hash_u01(M, 71, 1).astype(np.float32))
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    (sw, sg), (lw, lg) = m.sample_rl(det.to(DEV), ctrl.to(DEV), samples_per_image=K, seed=11, sparse_head=True)
    assert lw.requires_grad and lg.requires_grad and tuple(sw.shape) == (M, cfg["T"]) and tuple(lw.shape) == (M, cfg["T"])
    loss = vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV))
    loss.backward()
    sw, sg = sw.cpu(), sg.cpu()
    key = ("scst", sw.numpy().tobytes(), sg.numpy().tobytes())              # a flavour may draw other samples
    ref, yard = _oracles(key, w, cfg["T"], det.repeat_interleave(K, 0), gc.scst_loss_fn(reward, base),
                         ctrl=ctrl.repeat_interleave(K, 0), forced=(sw, sg))
    label = "scst-rows40 %s" % flavour
    gc.check_outputs(loss.item(), lw, lg, ref, label)
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 3e-3, None, label)


# ------------------------------------------------------------------------------------------------------------------ 3. unselected entries
def test_unselected_entries_are_zero_and_carry_no_gradient(flavour):
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, 23)
    m = helpers.build_model(cfg, w, DEV).train()
    d, s, c = _dev(det, ctrl_seq, caps)
    ref, _ = _oracles("small", w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    tg = torch.from_numpy(synth.make_captions(cfg["B"], cfg["T"], cfg["V"], seed=5))
    drop = torch.from_numpy(synth.hash_u01(cfg["B"] * cfg["T"], 72, 1).reshape(cfg["B"], cfg["T"])) < 1.0 / 3
    assert 0 < int(drop.sum()) < drop.numel()
    tg[drop] = -1
    lp_sel, gate = m.forward_selected((d,), (c, s), tg.to(DEV))
    assert lp_sel.requires_grad
    _check_selected(lp_sel, gate, tg, ref, "a third unselected %s" % flavour)
    assert bool((lp_sel.detach()[~drop.to(DEV)] < 0).all())
    del lp_sel, gate
    # nothing selected, no gate gradient: every parameter gradient is exactly 0 whatever arrives for the (unselected) log-probs
    m.zero_grad()
    none = torch.full_like(tg, -1).to(DEV)
    lp_sel, gate = m.forward_selected((d,), (c, s), none)
    assert bool((lp_sel.detach() == 0).all())
    (lp_sel * 3.0).sum().backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and bool((p.grad == 0).all()), "%s: a gradient without a selected entry" % k
    assert len(list(m.named_parameters())) == 28


# ------------------------------------------------------------------------------------------------------------------ 4. bad target ids
@pytest.mark.parametrize("bad", ["V", "-2"])
def test_bad_target_ids_raise(bad, flavour):
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl_seq, caps, _ = helpers.train_inputs(cfg, 23)
    m = helpers.build_model(cfg, w, DEV).train()
    d, s, c = _dev(det, ctrl_seq, caps)
    m._engine(torch.device(DEV)).check_ids = True
    tg = train.xe_targets(c)
    tg[1, 1] = cfg["V"] if bad == "V" else -2
    with pytest.raises(IndexError, match="train_forward_selected"):
        m.forward_selected((d,), (c, s), tg)
    lp_sel, _ = m.forward_selected((d,), (c, s), train.xe_targets(c))       # the count was read and reset: good ids pass
    assert bool(torch.isfinite(lp_sel).all())


# ------------------------------------------------------------------------------------------------------------------ 5. live forwards, kinds
def _two_batches(cfg):
    b1 = helpers.train_inputs(cfg, 23)
    b2 = helpers.train_inputs(cfg, 40)
    b2 = (b2[0] * 1.75, b2[1] * 1.75, b2[2], b2[3])          # other feature bounds: the f16x2 exponent rows of the two batches differ
    return _dev(*b1), _dev(*b2)


def _snap(m):
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    m.zero_grad()
    return g


def test_dense_and_sparse_forwards_alive_together(flavour):
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    m = helpers.build_model(cfg, w, DEV).train()
    (d1, s1, c1, g1), (d2, s2, c2, g2) = _two_batches(cfg)
    # each alone
    m.zero_grad()
    out, gate = m((d1,), (c1, s1))
    vo.xe_loss(out, gate, c1, g1)[0].backward()
    dense_alone = _snap(m)
    m.xe_loss(d2, c2, s2, g2)[0].backward()
    sparse_alone = _snap(m)
    del out, gate
    # both alive, differentiated in the opposite order
    out, gate = m((d1,), (c1, s1))
    l1 = vo.xe_loss(out, gate, c1, g1)[0]
    l2 = m.xe_loss(d2, c2, s2, g2)[0]
    assert m._engine(torch.device(DEV)).live_forwards() == 2
    l2.backward(retain_graph=True)
    sparse_mixed = _snap(m)
    l1.backward()
    dense_mixed = _snap(m)
    for k in dense_alone:
        assert torch.equal(dense_mixed[k], dense_alone[k]), "dense forward, %s" % k
        assert torch.equal(sparse_mixed[k], sparse_alone[k]), "sparse forward, %s" % k
    # the sparse backward consumed its log-prob rows in place: a second one must not return gradients
    with pytest.raises(RuntimeError, match="consumed"):
        l2.backward()


def test_backward_kinds_do_not_mix(flavour):
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    m = helpers.build_model(cfg, w, DEV).train()
    (d, s, c, g), _ = _two_batches(cfg)
    dev = torch.device(DEV)
    eng = m._engine(dev)
    B, T, V = cfg["B"], cfg["T"], cfg["V"]
    sink = [torch.zeros_like(p) for p in train._params_in_abi_order(m)]
    gw = train._lib.VsrWeights(*[t.data_ptr() for t in sink])
    g_dense, g_sel, g_gate = torch.zeros(B, T, V, device=DEV), torch.zeros(B, T, device=DEV), torch.zeros(B, T, 2, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    lp_sel, gate = m.forward_selected((d,), (c, s), train.xe_targets(c))                 # a sparse forward is the current one
    assert eng.lib.vsr_train_backward(eng.h, ptr(g_dense), ptr(g_gate), C.byref(gw), stream) != 0
    msg = eng.lib.vsr_last_error().decode()
    assert "vsr_train_backward_selected" in msg and "sparse" in msg, msg
    lp_sel.sum().backward()                                                              # ... and is still differentiable by its own call
    out, gate = m((d,), (c, s))                                                          # a dense forward is the current one
    assert eng.lib.vsr_train_backward_selected(eng.h, ptr(g_sel), ptr(g_gate), C.byref(gw), stream) != 0
    msg = eng.lib.vsr_last_error().decode()
    assert "call vsr_train_backward " in msg and "dense" in msg, msg
    vo.xe_loss(out, gate, c, g)[0].backward()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 6. index lists
def test_xe_loss_on_index_lists_vs_oracle_on_the_dense_regions(flavour):
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    det = torch.from_numpy(synth.make_detections(cfg["B"], cfg["R0"], cfg["D"], seed=33, min_valid=max(2, cfg["R0"] // 2)))
    idx = torch.from_numpy(synth.make_slot_indices(cfg["B"], cfg["T"], cfg["R"], cfg["R0"], seed=33))
    caps = torch.from_numpy(synth.make_captions(cfg["B"], cfg["T"], cfg["V"], seed=33))
    gts = torch.from_numpy(synth.make_gate_gts(cfg["B"], cfg["T"], seed=33))
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    reg = IndexedRegions(det.to(DEV), idx.to(DEV))
    dense = reg.dense().contiguous().cpu()
    loss = m.xe_loss(det.to(DEV), caps.to(DEV), reg, gts.to(DEV))[0]
    loss.backward()
    ref, yard = _oracles("indexed", w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=dense)
    label = "index lists %s" % flavour
    print("%s |dloss| %.2e" % (label, abs(loss.item() - ref["loss"])))
    assert abs(loss.item() - ref["loss"]) < 1e-4
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 2e-3, None, label)


# ------------------------------------------------------------------------------------------------------------------ 7. DataParallelStep
def test_data_parallel_xe_step_with_the_sparse_head(flavour):
    from vsrcap import parallel
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, 23)
    ref, _ = _oracles("small", w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    want = vo.xe_loss(ref["logp_words"], ref["logp_gates"], caps, gts)
    m = helpers.build_model(cfg, w, DEV).train()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    step = parallel.DataParallelStep(m, opt, sparse_head=True)
    try:
        stats = step.xe_step(*_dev(det, caps, ctrl_seq, gts))
    finally:
        step.close()
    assert tuple(stats.shape) == (3,)
    for got, wnt, name in zip(stats.tolist(), want, ("loss", "loss_cap", "loss_gate")):
        assert abs(got - float(wnt)) < 1e-4, "%s %.7f vs fp64 %.7f" % (name, got, float(wnt))
    # plain Adam moves every parameter whose gradient is not zero
    still = [k for k, p in m.named_parameters() if float(ref["grads"][k].abs().max()) > 0 and torch.equal(p.detach(), before[k])]
    assert not still, "parameters the step left untouched: %s" % still
    assert not torch.equal(m.out_fc.weight.detach(), before["out_fc.weight"])


def test_sparse_head_needs_the_hip_model():
    from vsrcap import parallel
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="sparse_head"):
        parallel.DataParallelStep(p, torch.optim.SGD(p, lr=0.1), sparse_head=True)


# ------------------------------------------------------------------------------------------------------------------ 8. bf16 mode
def test_bf16_sparse_and_dense_heads_agree():
    cfg = SMALL
    w = helpers.weights_for(cfg, gains=GAINS)
    det, ctrl_seq, caps, gts = helpers.train_inputs(cfg, 23)
    m = helpers.build_model(cfg, w, DEV).set_compute_dtype("bf16").train()
    d, s, c, g = _dev(det, ctrl_seq, caps, gts)
    m.zero_grad()
    out, gate = m((d,), (c, s))
    cap_dense = vo.xe_loss(out, gate, c, g)[1].item()
    loss, cap_sparse, _ = m.xe_loss(d, c, s, g)
    print("bf16 loss_cap dense %.7f sparse %.7f" % (cap_dense, cap_sparse.item()))
    assert abs(cap_sparse.item() - cap_dense) <= 2e-4
    loss.backward()
    for k, p in m.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), k
    assert float(m.out_fc.weight.grad.abs().max()) > 0
