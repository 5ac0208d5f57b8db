"""step() under autograd: a manual decode loop from init_state is taped and ONE hand-written backward differentiates it through the
recurrence (vsrcap/steptape.py, vsrcap/train.py, include/vsrcap.h vsr_train_tape_*).  The reference's step
(models/controllable_captioning.py:117-190) is plain autograd and its forward (models/CaptioningModel.py:22-36) a loop over it.

Shapes: test_gpu_grad_routes.BASE, gains 1.0, rows B = 4, 41 and 129 - both sides of the rows-16 boundary and the first launch without
two attention parts; the per-step x-projection and vocabulary launches exist only here at M = B.  Every case asserts that a region row is
padding and that a word id repeats within a step.

Bounds are the project's own: grad_compare.compare at margin 16 x the fp32 oracle's own error against fp64 plus the 2e-3 (SCST 3e-3)
of max |ref| ceiling; loss 1e-4 and log-probs 2e-4 against fp64 (grad_compare.check_outputs); step-vs-whole-call log-probs 2e-5
(test_gpu_parity.test_teacher_forcing_step_matches_forward).  bf16 is not a parity mode: tests/test_gpu_bf16.py's stated bounds.

The module multiplies itself by the three fp32 GEMM flavours (`flavour`), as test_gpu_grad_routes does."""
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
# rows -> input seed: the first from 23 on at which the first two steps already repeat a word id and step 3 reads ids they do not
SEEDS = {4: 24, 41: 23, 129: 23}
ROWS = sorted(SEEDS)
FACTORS = {}                             # (case, flavour) -> {tensor: factor}: none needed


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


_cache = {}


def _case(B):
    """weights and inputs of one row count, built once"""
    if ("case", B) not in _cache:
        cfg = dict(BASE, B=B)
        _cache[("case", B)] = (cfg, helpers.weights_for(cfg, gains=GAINS)) + tuple(helpers.train_inputs(cfg, SEEDS[B]))
    return _cache[("case", B)]


def _oracles(key, w, T, det, loss_fn, **kw):
    """(fp64 reference, fp32 yardstick), computed once per case and shared by the flavours; never modified"""
    if key not in _cache:
        _cache[key] = tuple(gc.oracle_grads(w, T, det, dt, loss_fn, **kw) for dt in (torch.float64, torch.float32))
    return _cache[key]


def _assert_edges(regions, words):
    assert bool((regions.abs().sum(-1) == 0).any()), "no padding region row"
    assert any(len(set(words[:, t].tolist())) < words.shape[0] for t in range(words.shape[1])), "no word id repeats within a step"


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def gc_collect():
    import gc
    gc.collect()                         # (a raised backward leaves its frames - and the tape they hold - in a reference cycle)


def _eng(m):
    return m._engine(torch.device(DEV))


def _tf_loop(m, det, caps, ctrl_seq, steps, between=None):
    """`steps` teacher-forced steps from init_state, as CaptioningModel.forward unrolls them; -> stacked (out, gate)"""
    state = m.init_state(det.size(0), torch.device(DEV))
    outs, ow, og = None, [], []
    for t in range(steps):
        outs, state = m.step(t, state, outs, (det,), (caps, ctrl_seq), mode="teacher_forcing")
        assert outs[0].requires_grad and outs[1].requires_grad, "step %d returned outputs without a graph" % t
        ow.append(outs[0])
        og.append(outs[1])
        if between is not None:
            between(t)
    return torch.stack(ow, 1), torch.stack(og, 1)


def _run_case1(B):
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    live = []
    out, gate = _tf_loop(m, det.to(DEV), caps.to(DEV), ctrl_seq.to(DEV), cfg["T"], between=lambda t: live.append(_eng(m).live_forwards()))
    loss = vo.xe_loss(out, gate, caps.to(DEV), gts.to(DEV))[0]
    loss.backward()
    return m, loss, out, gate, live


@pytest.mark.parametrize("B", ROWS)
def test_teacher_forced_loop_vs_fp64_oracle(B, flavour):
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    _assert_edges(ctrl_seq, caps)
    m, loss, out, gate, live = _run_case1(B)
    assert live == [1] * cfg["T"], "one tape is ONE live forward, however many steps it holds: %s" % live
    assert _eng(m).live_forwards() == 0
    ref, yard = _oracles(("xe", B), w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    label = "step-loop rows%d %s" % (B, flavour)
    gc.check_outputs(loss.item(), out, gate, ref, label)
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 2e-3, FACTORS.get(("xe%d" % B, flavour)), label)


@pytest.mark.parametrize("B", ROWS)
def test_partial_loop_two_of_three_steps(B, flavour):
    """2 of the model's 3 steps, loss on those two: the oracle run with T = 2; what only step 3 would read gets exactly nothing"""
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    caps2, seq2, gts2 = caps[:, :2].contiguous(), ctrl_seq[:, :2].contiguous(), gts[:, :2].contiguous()
    _assert_edges(seq2, caps2)
    only3 = sorted(set(caps[:, 2].tolist()) - set(caps2.flatten().tolist()))
    assert only3, "no word id that only step 3 reads"
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    out, gate = _tf_loop(m, det.to(DEV), caps.to(DEV), ctrl_seq.to(DEV), 2)          # the full sequences, two steps taken
    assert tuple(out.shape) == (B, 2, cfg["V"])
    loss = vo.xe_loss(out, gate, caps2.to(DEV), gts2.to(DEV))[0]
    loss.backward()
    ref, yard = _oracles(("xe2", B), w, 2, det, gc.xe_loss_fn(caps2, gts2), caps=caps2, ctrl_seq=seq2)
    label = "partial step-loop rows%d %s" % (B, flavour)
    gc.check_outputs(loss.item(), out, gate, ref, label)
    got = _grads(m)
    gc.compare(got, ref["grads"], yard["grads"], gc.MARGIN, 2e-3, FACTORS.get(("xe2-%d" % B, flavour)), label)
    assert float(got["embed.weight"][only3].abs().max()) == 0.0, "an embedding row that only the step not taken reads got a gradient"


def _draw_samples(m, det, ctrl, B):
    """forced words / gates: sample_rl's own draw under no_grad, at the first seed whose words repeat an id within a step they feed"""
    for seed in range(11, 75):
        with torch.no_grad():
            (sw, sg), _ = m.sample_rl(det, ctrl, seed=seed)
        sw, sg = sw.cpu(), sg.cpu()
        if any(len(set(sw[:, t].tolist())) < B for t in range(sw.shape[1] - 1)):
            return sw, sg
    raise AssertionError("no seed in [11, 75) draws a word id twice within a step")


@pytest.mark.parametrize("B", ROWS)
def test_feedback_loop_vs_fp64_oracle(B, flavour):
    cfg, w = _case(B)[:2]
    T, L = cfg["T"], cfg["L"]
    det, ctrl = helpers.decode_inputs(cfg, 12)
    reward = torch.from_numpy(synth.hash_u01(B, 70, 1).astype(np.float32))
    base = torch.from_numpy(synth.hash_u01(B, 71, 1).astype(np.float32))
    m = helpers.build_model(cfg, w, DEV).train()
    d, c = det.to(DEV), ctrl.to(DEV)
    sw, sg = _draw_samples(m, d, c, B)
    _assert_edges(ctrl, sw[:, :-1])                       # the words that steps 1 .. T-1 read (step 0 reads bos)
    with torch.no_grad():
        _, (want_w, want_g) = m.sample_rl(d, c, forced=(sw.to(DEV), sg.to(DEV)))
    m.zero_grad()
    state = m.init_state(B, torch.device(DEV))
    prev, lw, lg = None, [], []
    for t in range(T):
        (ow, og), state = m.step(t, state, prev, (d, c), None, mode="feedback")
        assert ow.requires_grad and og.requires_grad
        prev = (sw[:, t].to(DEV), sg[:, t].to(DEV))
        lw.append(ow.gather(1, prev[0].unsqueeze(1)).squeeze(1))
        lg.append(og.gather(1, prev[1].unsqueeze(1)).squeeze(1))
        assert torch.equal(state[2].cpu(), torch.clamp(sg[:, :t].sum(1), max=L - 1)), "slot pointer read by step %d" % t
    lw, lg = torch.stack(lw, 1), torch.stack(lg, 1)
    dw, dg = float((lw.detach() - want_w).abs().max()), float((lg.detach() - want_g).abs().max())
    print("feedback loop rows%d %s: max |dlogp| against sample_rl(forced) words %.2e gates %.2e" % (B, flavour, dw, dg))
    assert dw <= 2e-5 and dg <= 2e-5
    loss = vo.scst_loss(lw, lg, reward.to(DEV), base.to(DEV))
    loss.backward()
    key = ("scst", B, sw.numpy().tobytes(), sg.numpy().tobytes())       # a flavour may draw other samples
    ref, yard = _oracles(key, w, T, det, gc.scst_loss_fn(reward, base), ctrl=ctrl, forced=(sw, sg))
    label = "feedback step-loop rows%d %s" % (B, flavour)
    gc.check_outputs(loss.item(), lw, lg, ref, label)
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 3e-3, FACTORS.get(("scst%d" % B, flavour)), label)


def _sum_oracle(w, T, batches, dtype):
    o = vo.Oracle(w, T, 2, as_written=True, dtype=dtype)
    for k in o.p:
        o.p[k].requires_grad_(True)
    total = 0
    for det, ctrl_seq, caps, gts in batches:
        lw, lg = o.forward(det.to(dtype), caps, ctrl_seq.to(dtype))
        total = total + vo.xe_loss(lw, lg, caps, gts)[0]
    total.backward()
    return dict(loss=float(total.item()), grads={k: o.p[k].grad.detach().double() for k in o.p})


def test_two_tapes_interleaved_with_a_decode(flavour):
    """a no_grad decode of another batch between step 1 and step 2, a second tape alive at the same time, (l1 + l2).backward()"""
    B = 41
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    b1 = (det, ctrl_seq, caps, gts)
    b2 = helpers.train_inputs(cfg, SEEDS[B] + 17)
    b2 = (b2[0] * 1.75, b2[1] * 1.75, b2[2], b2[3])      # other feature bounds: the f16x2 exponent rows of the two batches differ
    _assert_edges(ctrl_seq, caps)
    _assert_edges(b2[1], b2[2])
    m = helpers.build_model(cfg, w, DEV).train()
    m.zero_grad()
    eng = _eng(m)
    d1, s1, c1, g1 = (x.to(DEV) for x in b1)
    d2, s2, c2, g2 = (x.to(DEV) for x in b2)
    dev = torch.device(DEV)
    st1, st2 = m.init_state(B, dev), m.init_state(B, dev)
    o1, o2 = [], []
    outs, st1 = m.step(0, st1, None, (d1,), (c1, s1), mode="teacher_forcing")
    o1.append(outs)
    prev1, prev2 = outs, None
    assert eng.live_forwards() == 1
    with torch.no_grad():
        words, _ = m.test(d2, s2[:, :cfg["L"]].contiguous())
    assert eng.live_forwards() == 1
    for t in range(cfg["T"]):                             # tape 2 runs ahead, tape 1 follows
        prev2, st2 = m.step(t, st2, prev2, (d2,), (c2, s2), mode="teacher_forcing")
        o2.append(prev2)
        assert eng.live_forwards() == 2
        if t + 1 < cfg["T"]:
            prev1, st1 = m.step(t + 1, st1, prev1, (d1,), (c1, s1), mode="teacher_forcing")
            o1.append(prev1)
    stack = lambda o: (torch.stack([x[0] for x in o], 1), torch.stack([x[1] for x in o], 1))
    (w1, q1), (w2, q2) = stack(o1), stack(o2)
    l1, l2 = vo.xe_loss(w1, q1, c1, g1)[0], vo.xe_loss(w2, q2, c2, g2)[0]
    (l1 + l2).backward()
    assert eng.live_forwards() == 0
    if ("sum", B) not in _cache:
        _cache[("sum", B)] = tuple(_sum_oracle(w, cfg["T"], [b1, b2], dt) for dt in (torch.float64, torch.float32))
    ref, yard = _cache[("sum", B)]
    assert abs((l1 + l2).item() - ref["loss"]) < 2e-4     # two losses of 1e-4 each
    gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 2e-3, None, "two tapes %s" % flavour)
    fresh = helpers.build_model(cfg, w, DEV)
    with torch.no_grad():
        w_alone, _ = fresh.test(d2, s2[:, :cfg["L"]].contiguous())
    assert torch.equal(words, w_alone), "the decode between two steps saw the tape's state"


def test_what_a_tape_cannot_express_raises(flavour):
    """every limit raises a RuntimeError that names forward() / sample_rl(); after each the model trains as before"""
    B = 4
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    d, s, c, g = det.to(DEV), ctrl_seq.to(DEV), caps.to(DEV), gts.to(DEV)
    dev = torch.device(DEV)
    m = helpers.build_model(cfg, w, DEV, verb_table={"0": [1, 2, 3]}).train()
    ref, yard = _oracles(("xe", B), w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    tf = dict(mode="teacher_forcing")
    names = r"forward\(\) / sample_rl\(\)"

    def still_trains(after):
        m.zero_grad()
        out, gate = m((d,), (c, s))
        vo.xe_loss(out, gate, c, g)[0].backward()
        gc.compare(_grads(m), ref["grads"], yard["grads"], gc.MARGIN, 2e-3, None, "forward() after '%s' %s" % (after, flavour))

    # a first step whose state did not come from init_state
    z = lambda: torch.zeros(B, cfg["H"], device=DEV)
    with pytest.raises(RuntimeError, match=names):
        m.step(0, ((z(), z()), (z(), z()), torch.zeros(B, dtype=torch.long, device=DEV)), None, (d,), (c, s), **tf)
    still_trains("state from nowhere")
    # a branch, then an edited state
    st0 = m.init_state(B, dev)
    o0, st1 = m.step(0, st0, None, (d,), (c, s), **tf)
    o1, st2 = m.step(1, st1, o0, (d,), (c, s), **tf)
    with pytest.raises(RuntimeError, match="branching.*" + names):
        m.step(1, st1, o0, (d,), (c, s), **tf)
    with torch.no_grad():
        st2[0][0].mul_(0.5)
    with pytest.raises(RuntimeError, match="modified in place.*" + names):
        m.step(2, st2, o1, (d,), (c, s), **tf)
    del o0, o1, st1, st2
    still_trains("branch / edited state")
    # more than seq_len steps
    st, o = m.init_state(B, dev), None
    for t in range(cfg["T"]):
        o, st = m.step(t, st, o, (d,), (c, s), **tf)
    with pytest.raises(RuntimeError, match="limit is %d steps.*%s" % (cfg["T"], names)):
        m.step(cfg["T"], st, o, (d,), (c, s), **tf)
    del o, st
    still_trains("step count")
    # step_v under grad
    verbs = torch.zeros(B, cfg["L"], device=DEV)
    with pytest.raises(RuntimeError, match="step_v.*" + names):
        m.step_v(0, m.init_state(B, dev), None, (d, s[:, :cfg["L"]].contiguous(), verbs), None, mode="feedback")
    still_trains("step_v")
    # a gradient for a returned state tensor
    o, st = m.step(0, m.init_state(B, dev), None, (d,), (c, s), **tf)
    with pytest.raises(RuntimeError, match="state tensor.*" + names):
        (o[0].sum() + st[1][0].sum()).backward()
    del o, st
    still_trains("state gradient")
    # create_graph=True
    o, st = m.step(0, m.init_state(B, dev), None, (d,), (c, s), **tf)
    with pytest.raises(RuntimeError, match="create_graph.*" + names):
        o[0].sum().backward(create_graph=True)
    del o, st
    still_trains("create_graph")
    # the second backward of a tape, as the second backward of a forward
    o, st = m.step(0, m.init_state(B, dev), None, (d,), (c, s), **tf)
    l = o[0].sum()
    l.backward()
    with pytest.raises(RuntimeError, match="second time"):
        l.backward()
    still_trains("second backward")
    del o, st, l
    gc_collect()
    assert _eng(m).live_forwards() == 0


def test_two_runs_give_the_same_bits(flavour):
    a = _grads(_run_case1(41)[0])
    b = _grads(_run_case1(41)[0])
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between two runs" % k


def test_no_grad_step_is_the_old_path(flavour):
    B = 4
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    d, s, c = det.to(DEV), ctrl_seq.to(DEV), caps.to(DEV)
    m = helpers.build_model(cfg, w, DEV).train()
    eng = _eng(m)
    before = (eng.live_forwards(), eng.train_generation())
    with torch.no_grad():
        state, outs = m.init_state(B, torch.device(DEV)), None
        for t in range(cfg["T"]):
            outs, state = m.step(t, state, outs, (d,), (c, s), mode="teacher_forcing")
            assert outs[0].grad_fn is None and outs[1].grad_fn is None and not outs[0].requires_grad
            assert all(x.grad_fn is None for x in (state[0] + state[1]))
            assert eng.live_forwards() == before[0]
    assert eng.train_generation() == before[1] or eng.train_generation() == 0      # no forward was saved
    for p in m.parameters():                              # frozen parameters: no graph either, grad mode on
        p.requires_grad_(False)
    outs, state = m.step(0, m.init_state(B, torch.device(DEV)), None, (d,), (c, s), mode="teacher_forcing")
    assert outs[0].grad_fn is None and eng.live_forwards() == before[0]


def test_bf16_loop_within_the_throughput_modes_bounds():
    """bf16 is not a parity mode (tests/test_gpu_bf16.py): log-probs within 0.15, loss within 1 %, every gradient's cosine with the
    fp64 oracle's >= 0.99 and its norm within 3 %"""
    B = 41
    cfg, w, det, ctrl_seq, caps, gts = _case(B)
    m = helpers.build_model(cfg, w, DEV).train()
    m.set_compute_dtype("bf16")
    m.zero_grad()
    out, gate = _tf_loop(m, det.to(DEV), caps.to(DEV), ctrl_seq.to(DEV), cfg["T"])
    loss = vo.xe_loss(out, gate, caps.to(DEV), gts.to(DEV))[0]
    loss.backward()
    ref, _ = _oracles(("xe", B), w, cfg["T"], det, gc.xe_loss_fn(caps, gts), caps=caps, ctrl_seq=ctrl_seq)
    d_out = float((out.detach().double().cpu() - ref["logp_words"]).abs().max())
    d_gate = float((gate.detach().double().cpu() - ref["logp_gates"]).abs().max())
    print("bf16 step-loop: max |dlogp| words %.3e gates %.3e, loss %.6f vs %.6f" % (d_out, d_gate, loss.item(), ref["loss"]))
    assert d_out < 0.15 and d_gate < 0.15
    assert abs(loss.item() - ref["loss"]) < 1e-2 * abs(ref["loss"])
    for k, p in m.named_parameters():
        a, b = ref["grads"][k].flatten(), p.grad.detach().cpu().double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm() + 1e-30))
        assert cos >= 0.99, (k, cos)
        assert abs(float(b.norm() / (a.norm() + 1e-30)) - 1.0) < 0.03, k
