"""SinkhornNet training on the device (coco_scripts/train_sinkhorn.py:137-215): forward with a grad_fn, the hand-written backward
and the fused location loss against oracle/ssp_oracle.py's SinkhornOracle under torch autograd in fp64 (pinned to the reference by
tests/test_sinkhorn_train_oracle.py), with the fp32 oracle's own error as the yardstick (tests/grad_compare.py)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import grad_compare as gc
import sinkhorn_train_ref as ref
from vsrcap import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAU, SCALE = 0.1, 0.25

# (Q, N, n_iters, seed): R = Q N rows go through the layers
CASES = [(1, 10, 20, 2),       # one item, R = 10
         (13, 10, 20, 3),      # R = 130 crosses a 128-row tile
         (70, 10, 20, 1),      # R = 700: more than one m-tile and a long k for dW
         (5, 16, 3, 4),        # the widest matrix the kernels admit
         (4, 2, 1, 5),         # the narrowest
         (3, 10, 0, 6)]        # no normalisation


def _net(N, n_iters, seed):
    from models import SinkhornNet
    m = SinkhornNet(N, n_iters, TAU)
    w = synth.make_sinkhorn_weights(seed, N)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.to(DEV).train(), w


@functools.lru_cache(maxsize=None)
def _case(Q, N, n_iters, seed):
    """inputs and the two oracle runs of one case, computed once and shared (nothing below writes into them)"""
    x, n = synth.make_sinkhorn_inputs(Q, seed, N)
    tr_locs, gt_locs = ref.make_locs(n, N, seed)
    w = synth.make_sinkhorn_weights(seed, N)
    r64 = ref.oracle_run(w, x, tr_locs, gt_locs, n_iters, TAU, torch.float64, SCALE)
    r32 = ref.oracle_run(w, x, tr_locs, gt_locs, n_iters, TAU, torch.float32, SCALE)
    return x, tr_locs, gt_locs, r64, r32


def _dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _grads(m):
    return {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}


def _step(m, x, tr_locs, gt_locs, fused):
    """one forward + loss + backward from zeroed gradients; fused: loc_loss, else the reference's torch lines on forward()'s tr"""
    m.zero_grad(set_to_none=True)
    if fused:
        loss = m.loc_loss(x, tr_locs, gt_locs, SCALE)
    else:
        loss, _ = ref.reference_loss(m(x), tr_locs, gt_locs, SCALE)
    loss.backward()
    return loss.detach()


def test_forward_has_a_grad_fn_and_assigns_bits():
    Q, N, n_iters, seed = CASES[1]
    m, _ = _net(N, n_iters, seed)
    x, = _dev(_case(Q, N, n_iters, seed)[0])
    tr = m(x)
    assert tr.grad_fn is not None and tr.requires_grad            # (fails without the feature: forward returned a leaf)
    with torch.no_grad():
        tr0 = m(x)
        tra, _ = m.assign(x)
    assert tr0.grad_fn is None and not tr0.requires_grad
    assert torch.equal(tr.detach(), tra) and torch.equal(tr0, tra)
    for p in m.parameters():
        p.requires_grad_(False)
    assert m(x).grad_fn is None                                    # nothing to train: today's path


@pytest.mark.parametrize("Q,N,n_iters,seed", CASES)
def test_gradients_match_the_fp64_oracle(Q, N, n_iters, seed):
    m, _ = _net(N, n_iters, seed)
    xa, tla, gla, r64, r32 = _case(Q, N, n_iters, seed)
    x, tr_locs, gt_locs = _dev(xa, tla, gla)
    label = "Q %d N %d iters %d" % (Q, N, n_iters)
    la = _step(m, x, tr_locs, gt_locs, fused=False)
    assert len(r64["grads"]) == 10
    gc.compare(_grads(m), r64["grads"], r32["grads"], label=label + " torch loss:")
    lb = _step(m, x, tr_locs, gt_locs, fused=True)
    gc.compare(_grads(m), r64["grads"], r32["grads"], label=label + " loc_loss:  ")
    la, lb = float(la), float(lb)
    print("%s loss torch lines %.7f  loc_loss %.7f  fp64 oracle %.7f  fp32 oracle %.7f" % (label, la, lb, r64["loss"], r32["loss"]))
    assert abs(la - lb) <= 1e-6 * abs(la)
    # the loss itself: one more scalar under the yardstick rule
    unit = max(abs(r32["loss"] - r64["loss"]), gc.ULP_FLOOR / gc.MARGIN * abs(r64["loss"]))
    assert abs(lb - r64["loss"]) <= gc.MARGIN * unit and abs(la - r64["loss"]) <= gc.MARGIN * unit


def test_reference_fixture():
    """the fp64 REFERENCE run (g16_sinkhorn_train.npz) is the reference here, the fp32 oracle run of the same inputs the yardstick"""
    meta, g = load_golden("g16_sinkhorn_train")
    want = {k.replace("__", "/"): torch.from_numpy(v) for k, v in g.items()}
    Q, N, n_iters, seed = meta["Q"], meta["N"], meta["n_iters"], meta["seed"]
    m, w = _net(N, n_iters, seed)
    xa, n = synth.make_sinkhorn_inputs(Q, seed, N)
    tla, gla = ref.make_locs(n, N, seed)
    r32 = ref.oracle_run(w, xa, tla, gla, n_iters, meta["tau"], torch.float32, meta["scale"])
    x, tr_locs, gt_locs = _dev(xa, tla, gla)
    m.zero_grad(set_to_none=True)
    tr = m(x)
    loss, items = ref.reference_loss(tr, tr_locs, gt_locs, meta["scale"])
    loss.backward()
    got = ref.summarise(dict(items=items.detach().double().cpu(), tr=tr.detach().double().cpu(), grads=_grads(m)))
    gc.compare(got, want, ref.summarise(r32), label="fixture, torch loss:")
    m.zero_grad(set_to_none=True)
    m.loc_loss(x, tr_locs, gt_locs, meta["scale"]).backward()
    items_f = m._engine(x.device).sinkhorn_loc_loss(tr.detach(), tr_locs, gt_locs, meta["scale"], want_grad=False)[0]
    got = ref.summarise(dict(items=items_f.double().cpu(), tr=tr.detach().double().cpu(), grads=_grads(m)))
    gc.compare(got, want, ref.summarise(r32), label="fixture, loc_loss:  ")


def _ulp_close(got, want, what):
    for k in want:
        bound = gc.ULP_FLOOR * float(want[k].abs().max())
        err = float((got[k] - want[k]).abs().max())
        assert err <= bound, "%s %s: %.3e > %.3e" % (what, k, err, bound)


def test_live_forwards_accumulation_and_an_assign_in_between():
    Q, N, n_iters, _ = CASES[1]
    m, _ = _net(N, n_iters, 3)
    x1, tl1, gl1 = _dev(*_case(Q, N, n_iters, 3)[:3])
    x2, tl2, gl2 = _dev(*_case(*CASES[2])[:3])                      # 70 items: another Q, another tape size
    _step(m, x1, tl1, gl1, fused=True)
    g1 = _grads(m)
    _step(m, x2, tl2, gl2, fused=False)
    g2 = _grads(m)
    want = {k: (g1[k].float() + g2[k].float()).double() for k in g1}
    # two forwards alive, one backward
    m.zero_grad(set_to_none=True)
    l1 = m.loc_loss(x1, tl1, gl1, SCALE)
    l2, _ = ref.reference_loss(m(x2), tl2, gl2, SCALE)
    (l1 + l2).backward()
    _ulp_close(_grads(m), want, "(l1 + l2).backward()")
    # two successive backward() calls accumulate into .grad, with an assign() between each forward and its backward
    m.zero_grad(set_to_none=True)
    l1 = m.loc_loss(x1, tl1, gl1, SCALE)
    with torch.no_grad():
        tra, a = m.assign(x2)
    l1.backward()
    _ulp_close(_grads(m), g1, "assign() before backward")
    l2, _ = ref.reference_loss(m(x2), tl2, gl2, SCALE)
    with torch.no_grad():
        m.assign(x1)
    l2.backward()
    _ulp_close(_grads(m), want, "micro-batch accumulation")
    assert sorted(a[0].tolist()) == list(range(N))


def test_two_runs_give_the_same_bits():
    Q, N, n_iters, seed = CASES[2]
    m, _ = _net(N, n_iters, seed)
    x, tl, gl = _dev(*_case(Q, N, n_iters, seed)[:3])
    runs = []
    for _ in range(2):
        loss = _step(m, x, tl, gl, fused=True)
        runs.append((loss.clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert len(runs[0][1]) == 10
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_backward_takes_n_iters_and_tau_from_the_tape():
    """the library level, below the Python check of the binding: the tape records the n_iters and tau of its forward, and the backward
    walks it with those (the divisor stride is 2 n_iters N) whatever is bound by then"""
    Q, N, n_iters, seed = CASES[1]
    m, _ = _net(N, n_iters, seed)
    x, = _dev(_case(Q, N, n_iters, seed)[0])
    eng = m._engine(x.device)
    sd = {k: v.data for k, v in m.state_dict(keep_vars=True).items()}
    tr, tape = eng.sinkhorn_train_forward(x)
    d_tr = torch.linspace(-1, 1, tr.numel(), device=DEV).reshape(tr.shape)
    want = eng.sinkhorn_train_backward(x, tape, d_tr)
    eng.bind_sinkhorn(sd, N, 3, 2 * TAU)
    got = eng.sinkhorn_train_backward(x, tape, d_tr)
    assert len(got) == 10 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(eng.sinkhorn_train_backward(x, eng.sinkhorn_train_forward(x)[1], d_tr)[0], want[0])      # the new binding differs


def _oracle_trajectory(w, dtype, train, held, n_iters):
    """three Adam steps (lr 1e-4) of the location loss on the CPU oracle in `dtype`: the three losses and the held-out loss afterwards"""
    import ssp_oracle as so
    o = so.SinkhornOracle(w, n_iters=n_iters, tau=TAU, dtype=dtype)
    for k in o.p:
        o.p[k] = o.p[k].clone().requires_grad_(True)
    opt = torch.optim.Adam(list(o.p.values()), lr=1e-4)
    losses = []
    t = [torch.as_tensor(a).to(dtype) for a in train]
    h = [torch.as_tensor(a).to(dtype) for a in held]
    for _ in range(3):
        opt.zero_grad()
        loss, _ = ref.reference_loss(o.forward(t[0]), t[1], t[2], SCALE)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    with torch.no_grad():
        losses.append(float(ref.reference_loss(o.forward(h[0]), h[1], h[2], SCALE)[0].item()))
    return np.array(losses, dtype=np.float64)


def test_adam_trajectory_plain_and_fused():
    """Bound: 16 x the fp32 oracle trajectory's own deviation from the fp64 one (its largest relative deviation over the four losses),
    floored at ULP_FLOOR of the loss - grad_compare's rule applied to a scalar.  The engine reads the parameters' storage live, so the
    optimizers' in-place steps (fused=True leaves Tensor._version untouched) need no refresh: a stale weight would show here."""
    Q, N, n_iters, seed = CASES[1]
    train, held = _case(Q, N, n_iters, seed)[:3], _case(Q, N, n_iters, 7)[:3]
    w = synth.make_sinkhorn_weights(seed, N)
    t64 = _oracle_trajectory(w, torch.float64, train, held, n_iters)
    t32 = _oracle_trajectory(w, torch.float32, train, held, n_iters)
    unit = max(float((np.abs(t32 - t64) / np.abs(t64)).max()), gc.ULP_FLOOR / gc.MARGIN)
    got = {}
    for fused in (False, True):
        m, _ = _net(N, n_iters, seed)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, fused=fused)
        tx, hx = _dev(*train), _dev(*held)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = m.loc_loss(*tx, SCALE)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            losses.append(float(m.loc_loss(*hx, SCALE)))
        got[fused] = np.array(losses, dtype=np.float64)
        dev = float((np.abs(got[fused] - t64) / np.abs(t64)).max())
        print("Adam(fused=%s) losses %s  fp64 %s  deviation / fp32-oracle deviation: %.2f (unit %.2e)" % (fused, got[fused], t64, dev / unit, unit))
        assert t64[2] < t64[0]                                    # the steps do train
        assert dev <= gc.MARGIN * unit, (got[fused], t64)
    both = float((np.abs(got[True] - got[False]) / np.abs(t64)).max())
    print("fused vs plain: %.2f of the unit" % (both / unit))
    assert both <= gc.MARGIN * unit


def test_loud_errors():
    Q, N, n_iters, seed = CASES[0]
    m, _ = _net(N, n_iters, seed)
    xa, tla, gla = _case(Q, N, n_iters, seed)[:3]
    x, tl, gl = _dev(xa, tla, gla)
    with pytest.raises(RuntimeError):
        m(torch.from_numpy(xa))                                     # CPU tensor
    with pytest.raises(RuntimeError):
        m.loc_loss(torch.from_numpy(xa), tl, gl)
    for bad in (N - 1, N + 1):
        with pytest.raises(RuntimeError):
            m(torch.zeros(Q, bad, 2352, device=DEV))
        with pytest.raises(RuntimeError):
            m.loc_loss(torch.zeros(Q, bad, 2352, device=DEV), tl, gl)
    with pytest.raises(RuntimeError, match="seq"):
        m(x.clone().requires_grad_(True))
    for k in ("tr_locs", "gt_locs"):                                # data, like seq: no silent None gradient
        locs = dict(tr_locs=tl, gt_locs=gl)
        locs[k] = locs[k].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=k):
            m.loc_loss(x, scale=SCALE, **locs)
    with pytest.raises(RuntimeError, match="create_graph"):
        ref.reference_loss(m(x), tl, gl, SCALE)[0].backward(create_graph=True)
    with pytest.raises(RuntimeError, match="create_graph"):
        m.loc_loss(x, tl, gl, SCALE).backward(create_graph=True)
    from models import SinkhornNet
    deep = SinkhornNet(N, SinkhornNet.TRAIN_MAX_ITERS + 1, TAU).to(DEV)
    with pytest.raises(RuntimeError, match="n_iters"):
        deep(x)
    with torch.no_grad():
        assert deep(x).shape == (Q, N, N)                           # inference binds any n_iters
    # the library's own check behind the Python one
    eng = deep._engine(x.device)
    with pytest.raises(RuntimeError, match="training cap"):
        eng.sinkhorn_train_forward(x)
    # a re-bind between a forward and its backward: the tape belongs to the earlier binding
    loss = m.loc_loss(x, tl, gl, SCALE)
    eng = m._engine(x.device)
    eng.bind_sinkhorn({k: v.data for k, v in m.state_dict(keep_vars=True).items()}, N, 3, TAU)
    with pytest.raises(RuntimeError, match="bind_sinkhorn"):
        loss.backward()
    eng.bind_sinkhorn({k: v.data for k, v in m.state_dict(keep_vars=True).items()}, N, n_iters, TAU)
    m.zero_grad(set_to_none=True)
    m.loc_loss(x, tl, gl, SCALE).backward()                         # ... and the device is still fine
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
