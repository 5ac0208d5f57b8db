"""The books of the library's own optimizer (vsrcap/optim.py) without a library or a GPU, in the style of tests/test_derived_logic.py:
Derived's new event - stepped(): the optimizer rebuilt the flavour product for the weights as they are now - against that module's fake
handle, under enumerated event sequences; the model's side of the rule (models/controllable_captioning.py, "the weights' GENERATION")
transcribed next to it; the constructor's refusals; and the fp64 reference of the update the GPU tests use (tests/optim_ref.py) against
torch's own float64 Adam.  The GPU side is tests/test_gpu_optim.py."""
import itertools

import pytest
import torch

import optim_ref
from test_derived_logic import FakeHandle, World
from vsrcap.derived import Derived


class StepHandle(FakeHandle):
    """... plus vsr_adam_step: writes the weights; rebuilds the product that is on from them; voids what a refresh voids"""

    def adam_step(self):
        self.calls.append(("adam_step",))
        self.world.content += 1
        if self.bf16_on:
            self.bf16_from = self.world.content
        if self.h2_on:
            self.h2_from = self.world.content
        if self.bf16_on or self.h2_on:
            self._void(False)
        else:
            self.cache = None


class Model:
    """the model's rules around a Derived: a graph-building forward bumps the version unless the optimizer's step left it exactly there;
    the step bumps it and files the rebuilt product under the new one"""

    def __init__(self):
        self.world = World()
        self.world.training = True
        self.handle, self.derived = StepHandle(self.world), Derived()
        self.stepped_at = None
        self.prep_key = None

    def forward(self, graph=True):
        w = self.world
        if graph:
            if self.stepped_at is None or self.stepped_at != w.version:
                w.version += 1
            self.stepped_at = None
        if self.derived.sync(w.target(), self.handle):
            self.prep_key = None
        if self.prep_key != (w.ptrs, w.version):
            self.handle.prepare()
            self.prep_key = (w.ptrs, w.version)
        if w.training:
            self.handle.saved = True

    def fused_step(self):
        w = self.world
        if self.derived.ptrs != w.ptrs:
            self.forward(graph=False)            # bind first
        w.version += 1
        self.stepped_at = None
        self.handle.adam_step()
        self.derived.stepped(w.ptrs, w.version)
        self.prep_key = None
        self.stepped_at = w.version

    # ---- what else can move the weights between a step and the next forward
    def inplace_op(self):                        # sum(p._version), another optimizer's step (_OPT_STEPS), load_state_dict(): the version moves
        self.world.version += 1
        self.world.content += 1

    def invalidate_cache(self):
        self.world.version += 1
        self.world.content += 1
        self.derived.invalidate(self.handle)

    def train_eval(self):                        # eval() and back
        self.world.version += 2

    def set_compute_dtype(self, dtype=None):
        self.world.dtype = dtype or self.world.dtype
        self.stepped_at = None

    def rebind(self):
        self.world.ptrs = (self.world.ptrs[0] + "'",)
        self.world.content += 1


FOREIGN = ("inplace_op", "invalidate_cache", "train_eval", "set_compute_dtype", "rebind")
REFRESH = {"f16x2": ("refresh_h2", True), "bf16": ("refresh_bf16", True)}


def _refreshes(calls):
    return [c for c in calls if c[0] in ("refresh_h2", "refresh_bf16")]


@pytest.mark.parametrize("dtype", ["f16x2", "bf16", "f32x3", "f32"])
def test_training_loop_with_the_fused_step_refreshes_once_at_the_start_and_never_again(dtype):
    m = Model()
    m.world.dtype = dtype
    m.forward()
    first = len(_refreshes(m.handle.calls))
    assert first == (1 if dtype in REFRESH else 0)
    for _ in range(3):
        m.fused_step()
        n = len(m.handle.calls)
        m.forward()
        assert m.handle.calls[n:] == [], "the forward after a fused step issues no library call of the chain"
        h = m.handle
        assert h.prepared == (m.world.content, h.flavour())                  # ... and prepares again: the statics were void
        assert h.bf16_from == (m.world.content if h.bf16_on else None) and h.h2_from == (m.world.content if h.h2_on else None)
    assert len(_refreshes(m.handle.calls)) == first
    assert m.handle.saved                        # a step keeps the saved forwards, as a refresh does


@pytest.mark.parametrize("dtype", ["f16x2", "bf16"])
def test_the_cache_is_dropped_and_the_statics_are_void_after_a_fused_step(dtype):
    m = Model()
    m.world.dtype, m.world.training = dtype, False
    m.forward(graph=False)                       # eval mode: builds the cache, prepares
    assert m.derived.cache is not None and m.handle.cache is not None and not m.derived.statics_void
    m.fused_step()
    assert m.derived.cache is None and m.handle.cache is None, "both sides agree: no cache"
    assert m.derived.statics_void and m.handle.prepared is None and m.prep_key is None
    n = len(m.handle.calls)
    m.forward(graph=False)                       # eval after the step: no refresh (the product is current), the cache rebuilt
    assert m.handle.calls[n:] == [("build_cache",)]
    assert m.handle.cache == (m.world.content, m.handle.flavour()) and m.handle.prepared == (m.world.content, m.handle.flavour())


@pytest.mark.parametrize("dtype", ["f16x2", "bf16"])
@pytest.mark.parametrize("foreign", [c for n in (1, 2) for c in itertools.product(FOREIGN, repeat=n)])
def test_every_foreign_write_between_step_and_forward_restores_todays_calls(dtype, foreign):
    """today's sequence: the same events with the step of an optimizer nobody tells the books about (the version moves, the product is
    stale) in place of the fused one"""
    def run(fused):
        m = Model()
        m.world.dtype = dtype
        m.forward()
        if fused:
            m.fused_step()
        else:
            m.inplace_op()                       # (any optimizer, as the version sees it)
        n = len(m.handle.calls)
        for f in foreign:
            getattr(m, f)()
        m.forward()
        return m, m.handle.calls[n:]
    new, calls = run(True)
    _, today = run(False)
    assert calls == today and len(_refreshes(calls)) == 1, (foreign, calls, today)
    h = new.handle
    assert h.bf16_from == (new.world.content if h.bf16_on else None) and h.h2_from == (new.world.content if h.h2_on else None)
    # and the shortcut is back for the step after
    new.fused_step()
    n = len(h.calls)
    new.forward()
    assert h.calls[n:] == []


def test_a_flavour_switch_between_step_and_forward_goes_through_the_chain():
    m = Model()
    m.forward()
    m.fused_step()
    n = len(m.handle.calls)
    m.set_compute_dtype("bf16")
    m.forward()
    assert m.handle.calls[n:] == [("refresh_bf16", True), ("set_gemm_mode", False), ("refresh_h2", False)]
    m.fused_step()                               # now the bf16 copies are the product the step rebuilds
    n = len(m.handle.calls)
    m.forward()
    assert m.handle.calls[n:] == [] and m.handle.bf16_from == m.world.content


def test_a_second_forward_without_a_step_refreshes_as_today():
    m = Model()
    m.forward()
    m.fused_step()
    m.forward()
    n = len(m.handle.calls)
    m.forward()                                  # gradient accumulation: nobody stepped, the forward still expects that somebody did
    assert m.handle.calls[n:] == [("refresh_h2", True)]


def test_first_step_before_any_forward_binds_and_then_steps():
    m = Model()
    m.fused_step()
    assert m.handle.calls == [("bind", ("A",)), ("refresh_h2", True), ("adam_step",)]
    n = len(m.handle.calls)
    m.forward()
    assert m.handle.calls[n:] == []


# ------------------------------------------------------------------------------------------------ the model's counters (CPU)
def _cpu_model():
    from models import ControllableCaptioningModel
    return ControllableCaptioningModel(6, 20, 2, det_feat_size=16, input_encoding_size=8, rnn_size=8, att_size=8, verb_2_vob_all={})


def test_own_steps_are_neutral_for_the_model_and_counted_for_every_other():
    a, b = _cpu_model(), _cpu_model()

    class Own(torch.optim.SGD):
        rebuilds_derived_state = True
    dummy = torch.nn.Parameter(torch.zeros(3))
    dummy.grad = torch.ones(3)
    own = Own([dummy], lr=0.1)
    own.model = a
    va, vb = a._weights_version(), b._weights_version()
    own.step()
    assert a._weights_version() == va, "the step of the model's own optimizer is announced by the step itself, not by the count"
    assert b._weights_version() != vb, "every other model is voided as by any optimizer"
    va = a._weights_version()
    torch.optim.SGD([dummy], lr=0.1).step()
    assert a._weights_version() != va


def test_set_compute_dtype_forgets_the_step():
    m = _cpu_model()
    m._stepped_at = m._weights_version()
    m.set_compute_dtype("f32x3")
    assert m._stepped_at is None


# ------------------------------------------------------------------------------------------------ constructor refusals
@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)])
def test_constructor_refuses_what_the_kernel_does_not_implement(kw):
    from vsrcap.optim import Adam
    with pytest.raises(ValueError, match=next(iter(kw))):
        Adam(_cpu_model(), **kw)


def test_constructor_refuses_cpu_parameters_parameter_lists_and_bad_values():
    from vsrcap.optim import Adam
    m = _cpu_model()
    with pytest.raises(RuntimeError, match="GPU only"):
        Adam(m)
    with pytest.raises(TypeError, match="ControllableCaptioningModel"):
        Adam(list(m.parameters()))
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-0.1), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            Adam(m, **kw)


def test_torch_optimizers_are_told_nothing_new():
    from vsrcap.optim import Adam
    assert Adam.rebuilds_derived_state is True
    assert not hasattr(torch.optim.Adam, "rebuilds_derived_state") and not hasattr(torch.optim.SGD, "rebuilds_derived_state")


# ------------------------------------------------------------------------------------------------ the fp64 reference
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fp64_reference_is_torchs_adam_in_float64(wd):
    g = torch.Generator().manual_seed(5)
    params = {"a": torch.randn(7, 5, generator=g), "b": torch.randn(50, generator=g) * 1e-3, "c": torch.zeros(3)}
    grads = [{"a": torch.randn(7, 5, generator=g) * 1e-2, "b": torch.randn(50, generator=g), "c": None if i == 1 else torch.randn(3, generator=g)}
             for i in range(4)]
    lrs = [5e-4 * 0.5 ** i for i in range(4)]                       # StepLR(step_size=1, gamma=0.5)
    ref = optim_ref.run_fp64(params, grads, lrs, weight_decay=wd)
    tp = {k: torch.nn.Parameter(p.double()) for k, p in params.items()}
    opt = torch.optim.Adam(list(tp.values()), lr=5e-4, weight_decay=wd)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for i, gr in enumerate(grads):
        for k, p in tp.items():
            p.grad = None if gr[k] is None else gr[k].double()
        opt.step()
        sched.step()
        for k, p in tp.items():
            rp, rm, rv = ref[i][k]
            torch.testing.assert_close(p.detach(), rp, rtol=1e-13, atol=1e-300)
            torch.testing.assert_close(opt.state[p]["exp_avg"], rm, rtol=1e-13, atol=1e-300)
            torch.testing.assert_close(opt.state[p]["exp_avg_sq"], rv, rtol=1e-13, atol=1e-300)
    assert float(opt.state[tp["c"]]["step"]) == 3 and float(opt.state[tp["a"]]["step"]) == 4
