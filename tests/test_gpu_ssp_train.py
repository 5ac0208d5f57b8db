"""S_SSP training on the device (coco_scripts/train_region_sort.py:181-185): the loss of models/sort_model.py:80-103 with a grad_fn
and the hand-written backward against tests/ssp_train_ref.py's oracle under torch autograd in fp64 (pinned to the reference by
tests/test_ssp_train_oracle.py), with the fp32 oracle's own error as the yardstick (tests/grad_compare.py).

Cases S = 1 (Rd = 11 and Re = 10 rows: no multiple of 4), 13 (Rd = 143 crosses a 128-row tile), 64 (several m-tiles, k = 704 for dW).
The gradients of w_1 / b_1 jump where a ReLU pre-activation crosses zero, and at these sizes a handful of the 8.3 M pre-activations do so
between ANY two roundings of the forward: both oracles are therefore run on the device's side of the kinks that lie within rounding
error of zero (ssp_train_ref.pinned_reference, which states the band), and are untouched everywhere else.
Between them the inputs hold a sequence of one role, one of ten roles (its EOS target sits at the last position) and a ground truth
shorter than the detected roles; S = 13 and S = 64 each hold all three, S = 1 is the ten-role one."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import grad_compare as gc
import ssp_train_ref as ref
from vsrcap import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(1, 1), (13, 1), (64, 1)]            # (S, seed of the inputs)
WSEED = 0                                     # seed of the weights


def _net():
    from models import S_SSP
    m = S_SSP()
    w = synth.make_ssp_weights(WSEED)
    sd = m.state_dict()
    alias = {"encoder.sr_embed_layer.weight": "sr_embed_layer.weight", "decoder.embed_layer.weight": "sr_embed_layer.weight",
             "encoder.v_embed_layer.weight": "v_embed_layer.weight"}
    for k in sd:
        if alias.get(k, k) in w:
            sd[k] = torch.from_numpy(w[alias.get(k, k)])
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _inputs(S, seed):
    verbs, roles = synth.make_ssp_inputs(S, seed)
    return verbs, roles, ref.make_gt(roles, seed)


@functools.lru_cache(maxsize=None)
def _oracle(S, seed, mask_kind, dtype):
    """one oracle run, computed once and shared (nothing below writes into it); mask_kind: None, or "hash" = the generator's masks"""
    verbs, roles, gt = _inputs(S, seed)
    masks = ref.hash_masks(S, seed) if mask_kind == "hash" else None
    return ref.oracle_run(synth.make_ssp_weights(WSEED), verbs, roles, gt, masks, dtype)


def _dev(S, seed):
    verbs, roles, gt = _inputs(S, seed)
    return torch.from_numpy(verbs).to(DEV).unsqueeze(1), torch.from_numpy(roles).to(DEV), torch.from_numpy(gt).to(DEV)     # (S,1), (S,10), (S,10)


def _grads(m):
    return {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None}


def _mask_buffer(eng, S, masks):
    """33 keep arrays -> the library's byte buffer"""
    layout, total = eng.ssp_mask_layout(S)
    buf = np.zeros(total, dtype=np.uint8)
    for (off, shape), keep in zip(layout, masks):
        assert tuple(keep.shape) == tuple(shape)
        buf[off:off + keep.size] = keep.reshape(-1)
    return torch.from_numpy(buf).to(DEV)


def _split_buffer(eng, S, buf):
    layout, _ = eng.ssp_mask_layout(S)
    b = buf.cpu().numpy()
    return [b[off:off + int(np.prod(shape))].reshape(shape) for off, shape in layout]


def _check_loss(got, r64, r32, label):
    """the scalar form of grad_compare's rule, as tests/test_gpu_sinkhorn_train.py holds its loss"""
    unit = max(abs(r32 - r64), gc.ULP_FLOOR / gc.MARGIN * abs(r64))
    print("%s loss %.8f  fp64 oracle %.8f  fp32 oracle %.8f  error / unit %.2f" % (label, got, r64, r32, abs(got - r64) / unit))
    assert abs(got - r64) <= gc.MARGIN * unit, (label, got, r64, r32)


def _step(m, args, **kw):
    """one forward + backward from zeroed gradients -> (loss, the six ReLU gate patterns of this forward, from its tape)"""
    m.zero_grad(set_to_none=True)
    loss = m(*args, **kw)
    gates = [g.cpu() for g in loss.grad_fn.eng.ssp_relu_gates(args[1].size(0), loss.grad_fn.tape)]
    loss.backward()
    return loss.detach(), gates


def _reference(S, seed, kind, gates, masks=None):
    """(fp64 reference, fp32 yardstick) of one case on the device's side of the ReLU kinks within rounding error of zero.
    kind: None / "hash" (cached oracle runs) or "given" with the 33 keep arrays in `masks`"""
    verbs, roles, gt = _inputs(S, seed)
    w = synth.make_ssp_weights(WSEED)
    if kind == "given":
        r64, r32 = (ref.oracle_run(w, verbs, roles, gt, masks, dt) for dt in (torch.float64, torch.float32))
    else:
        masks = ref.hash_masks(S, seed) if kind == "hash" else None
        r64, r32 = _oracle(S, seed, kind, torch.float64), _oracle(S, seed, kind, torch.float32)
    r64, r32, moved = ref.pinned_reference(r64, r32, gates, lambda dt, pin: ref.oracle_run(w, verbs, roles, gt, masks, dt, pin), masks)
    print("S %d %s: %d pinned units changed side" % (S, kind, moved))
    return r64, r32


def _used(m):
    return [k for k, _ in m.named_parameters() if "cross_attention" not in k]


def test_the_inputs_hold_the_three_kinds_of_sequence():
    seen = set()
    for S, seed in CASES:
        _, roles, gt = _inputs(S, seed)
        n, ng = (roles != 0).sum(1), (gt != 0).sum(1)
        kinds = {"one role": bool((n == 1).any()), "ten roles": bool((n == 10).any()), "shortened gt": bool((ng < n).any())}
        assert S == 1 or all(kinds.values()), (S, kinds)
        seen |= {k for k, v in kinds.items() if v}
        assert all(set(gt[s][:ng[s]]) <= set(roles[s][:n[s]]) and len(set(gt[s][:ng[s]])) == ng[s] for s in range(S))     # an order of (some of) the roles
    assert len(seen) == 3
    assert (_inputs(1, 1)[1] != 0).sum() == 10 and _inputs(1, 1)[2][0, 9] != 0       # S = 1: the target of position 10 is the EOS behind ten roles


def test_forward_returns_a_loss_with_a_grad_fn_and_leaves_generate_alone():
    S, seed = CASES[1]
    m = _net()
    args = _dev(S, seed)
    with torch.no_grad():
        before = m.generate_batch(args[0].reshape(-1), args[1])
    loss = m(*args)                                                 # (fails without the feature: NotImplementedError)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None and loss.requires_grad
    with torch.no_grad():
        plain = m(*args)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, loss.detach())
    loss.backward()
    with torch.no_grad():
        after = m.generate_batch(args[0].reshape(-1), args[1])
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(m(args[0].reshape(-1), args[1], args[2]).detach(), plain)          # this_verb (S,) as well as (S,1)
    for p in m.parameters():
        p.requires_grad_(False)
    frozen = m(*args)
    assert frozen.grad_fn is None and torch.equal(frozen, plain)    # nothing to train: a plain tensor with the same bits


@pytest.mark.parametrize("S,seed", CASES)
def test_eval_gradients_match_the_fp64_oracle(S, seed):
    m = _net()
    loss, gates = _step(m, _dev(S, seed))
    r64, r32 = _reference(S, seed, None, gates)
    got = _grads(m)
    assert len(got) == len(_used(m)) == len(r64["grads"]) == 112
    assert all(p.grad is None for k, p in m.named_parameters() if "cross_attention" in k)
    gc.compare(got, r64["grads"], r32["grads"], label="S %d eval:" % S)
    _check_loss(float(loss), r64["loss"], r32["loss"], "S %d eval" % S)


@pytest.mark.parametrize("S,seed", CASES)
def test_injected_masks_match_the_fp64_oracle(S, seed):
    m = _net()
    buf = _mask_buffer(m._engine(torch.device(DEV)), S, ref.hash_masks(S, seed))
    loss, gates = _step(m, _dev(S, seed), dropout_masks=buf)
    r64, r32 = _reference(S, seed, "hash", gates)
    got = _grads(m)
    assert len(got) == len(r64["grads"]) == 112
    gc.compare(got, r64["grads"], r32["grads"], label="S %d masks:" % S)
    _check_loss(float(loss), r64["loss"], r32["loss"], "S %d masks" % S)
    assert abs(r64["loss"] - _oracle(S, seed, None, torch.float64)["loss"]) > 1e-4         # the masks do something


def test_reference_fixture():
    """the fp64 REFERENCE runs (g17_ssp_train.npz) are the reference here, the fp32 oracle's summaries the yardstick"""
    meta, g = load_golden("g17_ssp_train")
    S, seed = meta["S"], meta["seed"]
    assert WSEED == seed
    m = _net()
    args = _dev(S, seed)
    buf = _mask_buffer(m._engine(torch.device(DEV)), S, ref.hash_masks(S, seed))
    for tag, kind, kw in (("a", None, {}), ("b", "hash", dict(dropout_masks=buf))):
        loss, gates = _step(m, args, **kw)
        got = ref.summarise(dict(loss=float(loss), grads=_grads(m)))
        want = ref.unpack(g[tag], meta["names"], meta["loss_" + tag])
        # the fixture moved to the device's side of the kinks by what that move does to the fp64 oracle (which reproduces it to 1e-10)
        r64, r32 = _reference(S, seed, kind, gates)
        here, there = ref.summarise(r64), ref.summarise(_oracle(S, seed, kind, torch.float64))
        want = {k: v + (here[k] - there[k]) for k, v in want.items()}
        gc.compare(got, want, ref.summarise(r32), label="fixture run %s:" % tag)


def test_library_masks():
    S, seed = CASES[2]
    m = _net()
    eng = m._engine(torch.device(DEV))
    a, b, c = eng.ssp_dropout_masks(S, 7), eng.ssp_dropout_masks(S, 7), eng.ssp_dropout_masks(S, 8)
    assert a.dtype == torch.uint8 and torch.equal(a, b) and not torch.equal(a, c)
    sites = _split_buffer(eng, S, a)
    assert [s.shape for s in sites] == ref.site_shapes(S)
    for i, keep in enumerate(sites):
        assert set(np.unique(keep)) <= {0, 1}
        n = keep.size
        assert n >= 32768
        share, sd = float(keep.mean()), (0.9 * 0.1 / n) ** 0.5              # 5 binomial standard deviations: +- 0.0083 at most (n = 32 768)
        assert abs(share - 0.9) <= 5 * sd, (i, share, 5 * sd)
    assert not np.array_equal(sites[3], sites[5])                           # two sites of one shape draw different bits
    # .train() with a seed IS the library's masks of that seed: the same bits in loss and gradients
    args = _dev(S, seed)
    m.train()
    l1, gates = _step(m, args, seed=7)
    g1 = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    l2, _ = _step(m, args, dropout_masks=a)
    assert torch.equal(l1, l2) and len(g1) == 112
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(g1[k], p.grad), k
    m.eval()
    assert not torch.equal(_step(m, args)[0], l1)                            # .eval(): no dropout
    r64, r32 = _reference(S, seed, "given", gates, sites)
    gc.compare({k: v.double().cpu() for k, v in g1.items()}, r64["grads"], r32["grads"], label="S %d library masks:" % S)
    _check_loss(float(l1), r64["loss"], r32["loss"], "S %d library masks" % S)


def test_accumulation_live_forwards_and_the_same_bits_twice():
    m = _net()
    a1, a2 = _dev(*CASES[1]), _dev(*CASES[0])                              # two S: two tape sizes
    _step(m, a1)
    g1 = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    m(*a1).backward()                                                      # a second backward accumulates: exactly twice
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, 2 * g1[k]), k
    _step(m, a1)                                                           # a re-run of the same step: no atomics, the same bits
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g1[k]), k
    _step(m, a2)
    g2 = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    l1, l2 = m(*a1), m(*a2)                                                # two forwards alive, one backward
    with torch.no_grad():
        m.generate_batch(a1[0].reshape(-1), a1[1])                         # ... and a generate() in between
    (l1 + l2).backward()
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g1[k] + g2[k]), k


def test_one_sgd_step_then_the_next_loss():
    """the library reads the parameters' storage live: the optimizer's in-place step is seen by the next forward with no refresh"""
    S, seed = CASES[1]
    lr = 0.003                                  # (the oracle's loss falls from 4.33 to 3.69 at this step size)
    verbs, roles, gt = _inputs(S, seed)
    w = synth.make_ssp_weights(WSEED)
    nxt = {}
    for dtype in (torch.float64, torch.float32):
        g = _oracle(S, seed, None, dtype)["grads"]
        np_t = np.float64 if dtype == torch.float64 else np.float32
        w2 = {k: (v.astype(np_t) - np_t(lr) * g[k].numpy().astype(np_t)) if k in g else v for k, v in w.items()}
        nxt[dtype] = ref.oracle_run(w2, verbs, roles, gt, None, dtype)["loss"]
    m = _net()
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    args = _dev(S, seed)
    opt.zero_grad()
    first = m(*args)
    first.backward()
    opt.step()
    with torch.no_grad():
        second = m(*args)
    assert nxt[torch.float64] < _oracle(S, seed, None, torch.float64)["loss"]            # the step does train
    _check_loss(float(second), nxt[torch.float64], nxt[torch.float32], "after one SGD step")


def test_loud_errors():
    S, seed = CASES[1]
    m = _net()
    verbs, roles, gt = _dev(S, seed)
    with pytest.raises(RuntimeError):
        m(verbs.cpu(), roles, gt)                                           # CPU tensors
    with pytest.raises(RuntimeError):
        m(verbs, roles.cpu(), gt)
    bad = roles.clone()
    bad[0, 0] = 26
    with pytest.raises(IndexError):
        m(verbs, bad, gt)
    bad = gt.clone()
    bad[0, 0] = -1
    with pytest.raises(IndexError):
        m(verbs, roles, bad)
    with pytest.raises(IndexError):
        m(torch.full_like(verbs, 2663), roles, gt)                          # a verb outside the table
    with pytest.raises(RuntimeError):
        m(verbs[:-1], roles, gt)                                            # mismatched S
    with pytest.raises(RuntimeError):
        m(verbs, roles, gt[:, :9])
    with pytest.raises(RuntimeError):
        m(verbs, roles, gt, dropout_masks=torch.ones(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="create_graph"):
        m(verbs, roles, gt).backward(create_graph=True)
    from models import S_SSP
    with pytest.raises(NotImplementedError):
        S_SSP(pos_enc=True)
    # a re-bind between a forward and its backward: the tape belongs to the earlier binding
    loss = m(verbs, roles, gt)
    eng = m._engine(torch.device(DEV))
    eng.bind_ssp({k: v.data for k, v in m.state_dict(keep_vars=True).items()})
    with pytest.raises(RuntimeError, match="bind_ssp"):
        loss.backward()
    _step(m, (verbs, roles, gt))                                            # ... and the device is still fine
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
