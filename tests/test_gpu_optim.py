"""vsrcap.optim.Adam on the device: one vsr_adam_step per step that updates the 28 tensors AND leaves the state the engine derives from
them (csrc/optim_kernels.h; the books: vsrcap/derived.py, models/controllable_captioning.py "the weights' GENERATION").

Everything runs on the g14_xe_traj_small configuration (V 50, B 4, D 512, E 64, H 64, A 32, T 12: a 50-element bias, (1, 32) vectors, a
3 200-element embedding table) and picks its compute dtype itself.  The update is held element-wise to an fp64 Adam on the CPU from the
same fp32 inputs (tests/optim_ref.py); the bound is computed here from the reference, never from the code under test: the error of
torch.optim.Adam(fused=True) on the device against the same fp64 run, times 4 (the two kernels round in a different order at a handful
of places - the idea of tests/grad_compare.py)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import helpers
import optim_ref
import vsr_oracle as vo
from vsrcap import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = "g14_xe_traj_small"
FLAVOURS = ("f16x2", "f32x3", "f32")
KEYS = [k for _, k in _lib.WEIGHT_FIELDS]
LR = 5e-4
SLACK = 4.0
GUARD = 0x5A5A5A5A


@functools.lru_cache(None)
def _fixture():
    meta, g = load_golden(NAME)
    return meta, g, helpers.weights_for(meta["cfg"], gains=meta["gains"])


def _model(dtype):
    meta, _, w = _fixture()
    m = helpers.build_model(meta["cfg"], w, DEV)
    m.set_compute_dtype(dtype)
    return m.train()


def _batch(seed):
    meta, _, _ = _fixture()
    det, ctrl_seq, caps, gts = helpers.train_inputs(meta["cfg"], seed)
    fs = meta["feat_scale"]
    return (det * fs).to(DEV), (ctrl_seq * fs).to(DEV), caps.to(DEV), gts.to(DEV)


def _grads(step, none_key=None):
    """fixed random gradients of step `step`, on the CPU: magnitudes from 1e-1 down to 1e-4 across the tensors"""
    _, _, w = _fixture()
    gen = torch.Generator().manual_seed(1000 + step)
    return {k: None if k == none_key else torch.randn(w[k].shape, generator=gen) * 10.0 ** -(1 + i % 4) for i, k in enumerate(KEYS)}


def _errors(values, ref):
    """values: name -> (p, exp_avg, exp_avg_sq) fp32; ref: the same in fp64 -> name -> the three max |difference|s"""
    return {k: tuple(float((a.detach().cpu().double() - b).abs().max()) for a, b in zip(values[k], ref[k])) for k in ref}


def _values(params, opt):
    return {k: (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for k, p in params.items()}


@functools.lru_cache(None)
def _reference(wd, sched=False, none_key=None, steps=4):
    """computed once per case and shared: the gradients, the fp64 run, and what torch's fused kernel makes of the same steps on the
    device -> (grads per step, fp64 results per step, torch's errors per step)"""
    _, _, w = _fixture()
    params = {k: torch.from_numpy(np.ascontiguousarray(w[k])) for k in KEYS}
    grads = [_grads(i, none_key) for i in range(steps)]
    lrs = [LR * (0.5 ** i if sched else 1.0) for i in range(steps)]
    ref = optim_ref.run_fp64(params, grads, lrs, weight_decay=wd)
    tp = {k: torch.nn.Parameter(p.to(DEV)) for k, p in params.items()}
    opt = torch.optim.Adam(list(tp.values()), lr=LR, weight_decay=wd, fused=True)
    sc = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5) if sched else None
    errs = []
    for i in range(steps):
        for k, p in tp.items():
            p.grad = None if grads[i][k] is None else grads[i][k].to(DEV)
        opt.step()
        if sc:
            sc.step()
        live = {k: p for k, p in tp.items() if p in opt.state and len(opt.state[p])}
        errs.append(_errors(_values(live, opt), {k: ref[i][k] for k in live}))
    return grads, ref, errs


def _hold(errs, bound, what):
    worst = 0.0
    for k in errs:
        for name, e, b in zip(("p", "exp_avg", "exp_avg_sq"), errs[k], bound[k]):
            ratio = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
            worst = max(worst, ratio)
            print("%s %-24s %-10s this %.3e  torch fused %.3e  ratio %.2f" % (what, k, name, e, b, ratio))
    print("%s: worst ratio to torch's fused kernel %.3f (bound %.0f)" % (what, worst, SLACK))
    for k in errs:
        for name, e, b in zip(("p", "exp_avg", "exp_avg_sq"), errs[k], bound[k]):
            assert e <= SLACK * b, "%s %s: error %.3e against fp64, torch's fused kernel %.3e" % (k, name, e, b)


def _assign(params, grads):
    for k, p in params.items():
        p.grad = None if grads[k] is None else grads[k].to(DEV)


def _named(m):
    named = dict(m.named_parameters())
    return {k: named[k] for k in KEYS}


def _derived_bytes(m):
    """the engine's flavour product as bytes: (exponent slots 0 .. 15, everything from byte 4096 on) of the fp16-pair image buffer, or
    the bf16 copies.  Both buffers end in 256 bytes of slack that no kernel ever writes (vsr_h2_weight_bytes / vsr_bf16_weight_bytes):
    whatever the allocator left there is not compared."""
    eng = m._eng
    torch.cuda.synchronize()
    if m.compute_dtype == "f16x2":
        b = eng._wbuf["h2"]
        return b[:64].clone(), b[4096:b.numel() - 256].clone()
    b = eng._wbuf["bf16"]
    return (b[:b.numel() - 256].clone(),)


def _assert_derived_is_what_a_refresh_builds(m):
    """the buffer as the step left it == the buffer after the ordinary refresh from the same weights, byte for byte (the max and the
    split do not depend on the order of evaluation)"""
    got = _derived_bytes(m)
    eng = m._eng
    eng.refresh_h2(True) if m.compute_dtype == "f16x2" else eng.refresh_bf16(True)
    want = _derived_bytes(m)
    m.invalidate_cache()                                   # (a refresh behind the books' back: the test's own doing)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    return got


# ------------------------------------------------------------------------------------------------ 1. the update, element-wise
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("dtype", FLAVOURS + ("bf16",))
def test_three_steps_against_fp64_within_four_times_torchs_own_error(dtype, wd):
    from vsrcap.optim import Adam
    grads, ref, bound = _reference(wd)
    m = _model(dtype)
    params = _named(m)
    opt = Adam(m, lr=LR, weight_decay=wd)
    for i in range(3):                                     # no forward: the kernel alone
        _assign(params, grads[i])
        opt.step()
    assert all(float(opt.state[p]["step"]) == 3 for p in params.values())
    _hold(_errors(_values(params, opt), ref[2]), bound[2], "%s wd=%g" % (dtype, wd))


# ------------------------------------------------------------------------------------------------ 2. tails and alignment
def _flat(sizes, guard, align):
    """one int32 buffer full of the guard pattern with room for tensors of `sizes` elements, `guard` pattern words before and after
    each, every tensor starting at a multiple of `align` words -> (buffer, offsets)"""
    offs, off = [], 0
    for n in sizes:
        off += guard
        off = (off + align - 1) // align * align
        offs.append(off)
        off += n
    buf = torch.full((off + guard + align,), GUARD, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, offs


def _guards_intact(buf, offs, sizes):
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = False
    return bool((buf[mask] == GUARD).all())


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("dtype", FLAVOURS + ("bf16",))
def test_unaligned_views_tails_and_a_missing_gradient(dtype, wd):
    """gradients and moments are views of flat buffers packed word-tight (one guard word between neighbours: most tensors are only
    4-byte aligned, and out_fc.bias with 50 elements shifts everything behind it); the parameters sit in a guarded buffer too, 16-byte
    aligned as every kernel of the library needs its weights.  One tensor has no gradient."""
    from vsrcap.optim import Adam
    none_key = "att_ga.weight"
    grads, ref, bound = _reference(wd, none_key=none_key)
    m = _model(dtype)
    params = _named(m)
    sizes = [p.numel() for p in params.values()]
    assert any(n % 4 for n in sizes)
    bufs = {"p": _flat(sizes, 4, 4), "g": _flat(sizes, 1, 1), "m": _flat(sizes, 1, 1), "v": _flat(sizes, 1, 1)}
    view = lambda kind, i, p: bufs[kind][0].view(torch.float32)[bufs[kind][1][i]:bufs[kind][1][i] + p.numel()].view_as(p)
    assert sum(o % 4 != 0 for o in bufs["g"][1]) >= 8, "several tensors must be only 4-byte aligned"
    opt = Adam(m, lr=LR, weight_decay=wd)
    gviews = {}
    for i, (k, p) in enumerate(params.items()):
        pv = view("p", i, p)
        pv.copy_(p.data)
        p.data = pv                                        # (new storage: the next call binds it)
        mv, vv = view("m", i, p), view("v", i, p)
        mv.zero_(); vv.zero_()
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": mv, "exp_avg_sq": vv}
        gviews[k] = view("g", i, p)
    before = {k: tuple(t.clone() for t in (p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])) for k, p in params.items()}
    for i in range(3):
        for k, p in params.items():
            if grads[i][k] is None:
                p.grad = None
            else:
                gviews[k].copy_(grads[i][k])
                p.grad = gviews[k]
        opt.step()
    torch.cuda.synchronize()
    for kind, (buf, offs) in bufs.items():
        assert _guards_intact(buf, offs, sizes), "guard words of the %s buffer were overwritten" % kind
    for a, b in zip(before[none_key], _values(params, opt)[none_key]):
        assert torch.equal(a, b), "a tensor without a gradient must not move"
    moved = [k for k, p in params.items() if k != none_key and not torch.equal(before[k][0], p.data)]
    assert len(moved) == len(KEYS) - 1
    live = {k: p for k, p in params.items() if k != none_key}
    _hold(_errors(_values(live, opt), {k: ref[2][k] for k in live}), bound[2], "views %s wd=%g" % (dtype, wd))
    if dtype in ("f16x2", "bf16"):                         # the tensor without a gradient is still measured and converted
        _assert_derived_is_what_a_refresh_builds(m)


# ------------------------------------------------------------------------------------------------ 3. the derived state, bitwise
@pytest.mark.parametrize("dtype", ["f16x2", "bf16"])
def test_derived_state_after_a_step_is_bitwise_what_a_refresh_builds(dtype):
    from vsrcap.optim import Adam
    grads, _, _ = _reference(0.0)

    def run():
        m = _model(dtype)
        params = _named(m)
        with torch.no_grad():
            # att_va.weight with max |x| = 1 exactly, and a gradient that pushes that element across the power of two: the step changes
            # the tensor's scale exponent, not only the low bits of its image
            w = params["att_va.weight"]
            at = w.abs().argmax()
            w.mul_(0.5 / w.abs().max())
            w.view(-1)[at] = torch.sign(w.view(-1)[at])
            assert float(w.abs().max()) == 1.0
        opt = Adam(m, lr=LR)
        g0 = {k: v.clone() for k, v in grads[0].items()}
        g0["att_va.weight"].view(-1)[at] = -10.0 * torch.sign(w.detach().view(-1)[at]).cpu()
        m._engine(torch.device(DEV, torch.cuda.current_device()))
        exps0 = _derived_bytes(m)[0].clone()
        for g in (g0, grads[1]):
            _assign(params, g)
            opt.step()
        got = _assert_derived_is_what_a_refresh_builds(m)
        return exps0, got
    exps0, first = run()
    _, second = run()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "two runs must leave identical bytes"
    if dtype == "f16x2":
        e0, e1 = exps0.view(torch.int32), first[0].view(torch.int32)
        assert int(e0[2]) - int(e1[2]) == 1, "att_va.weight (slot 2) must have crossed a power of two: %s -> %s" % (e0.tolist(), e1.tolist())


# ------------------------------------------------------------------------------------------------ 4. no refresh in the loop
class _Refreshes:
    """counts Engine.refresh_h2(True) / refresh_bf16(True) on one engine instance"""

    def __init__(self, eng):
        self.n = 0
        for name in ("refresh_h2", "refresh_bf16"):
            setattr(eng, name, self._wrap(getattr(eng, name)))

    def _wrap(self, fn):
        def counted(on):
            self.n += bool(on)
            return fn(on)
        return counted

    def take(self):
        n, self.n = self.n, 0
        return n


def _xe_step(m, opt, seed):
    det, ctrl_seq, caps, gts = _batch(seed)
    out, gate = m((det,), (caps, ctrl_seq))
    loss = vo.xe_loss(out, gate, caps, gts)[0]
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def _foreign_writes(m):
    dummy = torch.nn.Parameter(torch.zeros(4, device=DEV))
    dummy.grad = torch.ones_like(dummy)
    other = torch.optim.SGD([dummy], lr=0.1)

    def inplace():
        with torch.no_grad():
            m.out_fc.bias.add_(0.0)

    def rebind():
        m.s_fc.weight.data = m.s_fc.weight.data.clone()
    return {"an in-place torch op": inplace, "another optimizer's step": other.step, "invalidate_cache()": m.invalidate_cache,
            "load_state_dict()": lambda: m.load_state_dict(m.state_dict()), "eval() / train()": lambda: (m.eval(), m.train()),
            "set_compute_dtype()": lambda: m.set_compute_dtype(m.compute_dtype), "a rebind of the pointers": rebind}


@pytest.mark.parametrize("dtype", ["f16x2", "bf16"])
def test_no_refresh_in_the_training_loop_and_one_after_every_foreign_write(dtype):
    from vsrcap.optim import Adam
    seed = _fixture()[0]["seed"]
    # today: one per step
    m = _model(dtype)
    topt = torch.optim.Adam(m.parameters(), lr=LR, fused=True)
    _xe_step(m, topt, seed)
    count = _Refreshes(m._eng)
    for i in (1, 2):
        _xe_step(m, topt, seed + i)
        assert count.take() == 1, "torch.optim.Adam: one refresh per step, as before"
    # this optimizer: none after the first forward
    m = _model(dtype)
    opt = Adam(m, lr=LR)
    l0 = _xe_step(m, opt, seed)
    count = _Refreshes(m._eng)
    l1 = _xe_step(m, opt, seed + 1)
    l2 = _xe_step(m, opt, seed + 2)
    assert count.take() == 0, "no refresh call between fused steps"
    assert abs(float(l1) - float(l0)) > 1e-3 and abs(float(l2) - float(l1)) > 1e-3
    for what, write in _foreign_writes(m).items():
        write()
        _xe_step(m, opt, seed + 3)
        assert count.take() == 1, "%s between two steps must bring back exactly one refresh" % what
        _xe_step(m, opt, seed + 4)
        assert count.take() == 0, "the step after %s runs without a refresh again" % what


# ------------------------------------------------------------------------------------------------ 5. trajectory
def _trajectory(dtype):
    """the loop of tests/test_gpu_traj.py::_run with this optimizer"""
    from vsrcap.optim import Adam
    meta, g, _ = _fixture()
    m = _model(dtype)
    w0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = Adam(m, lr=meta["lr"])
    losses = []
    for i in range(meta["steps"]):
        det, ctrl_seq, caps, gts = _batch(meta["seed"] + i)
        out, gate = m((det,), (caps, ctrl_seq))
        loss, lc, lg = vo.xe_loss(out, gate, caps, gts)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append([loss.item(), lc.item(), lg.item()])
    dn = np.array([float((p.detach() - w0[k]).double().norm()) for k, p in m.named_parameters()])
    m.eval()
    det, ctrl_seq, caps, gts = _batch(meta["seed"] + meta["steps"])
    with torch.no_grad():
        out, gate = m((det,), (caps, ctrl_seq))
        held = [x.item() for x in vo.xe_loss(out, gate, caps, gts)]
    return g, np.array(losses), dn, np.array(held)


@pytest.mark.parametrize("dtype", FLAVOURS)
def test_five_xe_steps_follow_the_reference(dtype):
    """the bounds of tests/test_gpu_traj.py::test_five_xe_steps_follow_the_reference; a step on stale images fails from step 2 on"""
    g, losses, dn, held = _trajectory(dtype)
    print("trajectory %s: max |loss - reference| %s" % (dtype, np.abs(losses - g["losses"]).max(0).tolist()))
    np.testing.assert_allclose(losses[:, 1], g["losses"][:, 1], atol=1e-4, rtol=0)
    np.testing.assert_allclose(losses[:, 2], g["losses"][:, 2], atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(losses[:, 0], g["losses"][:, 0], atol=1e-4, rtol=2e-5)
    np.testing.assert_allclose(dn, g["delta_norm"], rtol=2e-3, atol=1e-9)
    np.testing.assert_allclose(held, g["heldout_losses"], atol=1e-4, rtol=2e-5)


def test_five_xe_steps_bf16_within_the_stated_deviation():
    """the bounds of tests/test_gpu_traj.py::test_five_xe_steps_bf16_deviation_stated"""
    g, losses, dn, held = _trajectory("bf16")
    d = np.abs(losses - g["losses"])
    print("bf16 trajectory deviation per step (total, cap, gate):", d.tolist(), "held-out:", np.abs(held - g["heldout_losses"]).tolist())
    assert d[:, 1].max() < 5e-5
    assert (d[:, 2] / np.maximum(1.0, g["losses"][:, 2])).max() < 1e-2
    np.testing.assert_allclose(dn, g["delta_norm"], rtol=5e-2)


# ------------------------------------------------------------------------------------------------ 6. checkpoints, schedulers
@pytest.mark.parametrize("first", ["torch", "vsrcap"])
def test_checkpoints_interchange_with_torch_adam(first):
    """two steps of one class, state_dict() -> load_state_dict() of the other, two more steps == four steps of torch.optim.Adam on the
    same gradients, within the bound of the element-wise test"""
    from vsrcap.optim import Adam
    grads, ref, bound = _reference(0.0)
    m = _model("f32x3")
    params = _named(m)
    make = {"torch": lambda: torch.optim.Adam(m.parameters(), lr=LR, fused=True), "vsrcap": lambda: Adam(m, lr=LR)}
    a = make[first]()
    for i in (0, 1):
        _assign(params, grads[i])
        a.step()
    sd = a.state_dict()
    b = make["vsrcap" if first == "torch" else "torch"]()
    b.load_state_dict(sd)
    for i in (2, 3):
        _assign(params, grads[i])
        b.step()
    assert all(float(b.state[p]["step"]) == 4 for p in params.values())
    _hold(_errors(_values(params, b), ref[3]), bound[3], "checkpoint %s first" % first)


def test_steplr_changes_the_applied_lr():
    from vsrcap.optim import Adam
    grads, ref, bound = _reference(0.0, sched=True)
    grads_c, ref_c, _ = _reference(0.0)
    m = _model("f32x3")
    params = _named(m)
    opt = Adam(m, lr=LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for i in range(3):
        _assign(params, grads[i])
        opt.step()
        sched.step()
    assert opt.param_groups[0]["lr"] == LR * 0.125
    _hold(_errors(_values(params, opt), ref[2]), bound[2], "StepLR")
    # the schedule is visible: far from the constant-lr run, in units of the bound
    k = "lstm_cell_1.weight_ih"
    assert float((params[k].detach().cpu().double() - ref_c[2][k][0]).abs().max()) > 100 * bound[2][k][0]


def test_step_closure_and_hooks_behave_as_on_any_optimizer():
    from vsrcap.optim import Adam
    grads, _, _ = _reference(0.0)
    m = _model("f32x3")
    params = _named(m)
    opt = Adam(m, lr=LR)
    seen = []
    opt.register_step_pre_hook(lambda o, a, k: seen.append("pre"))
    opt.register_step_post_hook(lambda o, a, k: seen.append("post"))

    def closure():
        assert torch.is_grad_enabled()
        _assign(params, grads[0])
        seen.append("closure")
        return torch.tensor(1.5)
    assert float(opt.step(closure)) == 1.5
    assert seen == ["pre", "closure", "post"]
    opt.zero_grad()
    assert all(p.grad is None for p in params.values())
    with pytest.raises(ValueError, match="one parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, device=DEV))], "lr": 1.0})
    m.out_fc.bias = torch.nn.Parameter(m.out_fc.bias.detach().clone())
    _assign(_named(m), grads[0])
    with pytest.raises(RuntimeError, match="replaced"):
        opt.step()


# ------------------------------------------------------------------------------------------------ 7. DataParallelStep
@pytest.mark.parametrize("dtype", FLAVOURS)
def test_data_parallel_step_keeps_the_shortcut(dtype):
    from vsrcap.optim import Adam
    from vsrcap.parallel import DataParallelStep
    seed = _fixture()[0]["seed"]

    def run(make_opt):
        m = _model(dtype)
        dp = DataParallelStep(m, make_opt(m), forward_fn=lambda det, caps, ctrl: m((det,), (caps, ctrl)), all_reduce_fn=lambda t: None)
        count = _Refreshes(m._eng)
        out = []
        for i in (0, 1):
            det, ctrl_seq, caps, gts = _batch(seed + i)
            out.append(dp.xe_step(det, caps, ctrl_seq, gts).cpu().numpy())
            n = count.take()
        dp.close()
        return np.array(out), n
    ours, n_ours = run(lambda m: Adam(m, lr=LR))
    theirs, n_theirs = run(lambda m: torch.optim.Adam(m.parameters(), lr=LR))
    print("DataParallelStep %s: |loss difference| %s" % (dtype, np.abs(ours - theirs).max(0).tolist()))
    np.testing.assert_allclose(ours[:, 1], theirs[:, 1], atol=1e-4, rtol=0)
    np.testing.assert_allclose(ours[:, 2], theirs[:, 2], atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(ours[:, 0], theirs[:, 0], atol=1e-4, rtol=2e-5)
    assert n_ours == 0, "no refresh in the second step with this optimizer"
    assert n_theirs == (1 if dtype == "f16x2" else 0), "torch optimizers see no difference: invalidate_cache() after every step"
