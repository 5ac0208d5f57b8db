"""The bookkeeping of the state derived from the weights (vsrcap/derived.py) against a fake handle that records the library calls and
follows the handle's voiding rules (include/vsrcap.h: a flavour transition voids the decode cache, the saved forwards and the
prepared statics; a refresh while on voids the cache and the statics and keeps the forwards).  Every sequence of up to four events
is enumerated.  No library, no GPU: the GPU side is tests/test_gpu_weight_generation.py."""
import itertools

import pytest

from vsrcap.derived import Derived

DTYPES = ("f32", "f32x3", "f16x2", "bf16")
# (bf16 copies, x3 switch, fp16-pair images) of a compute dtype, written out here a second time on purpose
SWITCHES = {"f32": (False, False, False), "f32x3": (False, True, False), "f16x2": (False, True, True), "bf16": (True, False, False)}


class World:
    """what is true outside the handle: the parameters' storage, the version the model reports, and the CONTENT of the weights (which
    moves with every version bump, and also behind the version's back: the p.data edit that invalidate() is for)"""

    def __init__(self):
        self.ptrs, self.version, self.content = ("A",), 0, 0
        self.dtype, self.training = "f16x2", False

    def target(self):
        return (self.ptrs, self.version, self.dtype, True, self.training)


class FakeHandle:
    """the library's side: the switches, what each product was built from (the world's content at the time), the calls it received"""

    def __init__(self, world):
        self.world = world
        self.calls = []
        self.bf16_on, self.x3_on, self.h2_on = False, True, False
        self.bf16_from = self.h2_from = None
        self.cache = None                # (content, flavour) the decode cache was built from
        self.prepared = None             # ... and the hoisted statics
        self.saved = False               # a training forward is saved

    def flavour(self):
        return (self.bf16_on, self.x3_on, self.h2_on)

    def _void(self, flavour_changed):
        self.cache = self.prepared = None
        if flavour_changed:
            self.saved = False

    def bind(self, ptrs):
        self.calls.append(("bind", ptrs))
        self._void(True)
        self.bf16_on = self.h2_on = False
        self.bf16_from = self.h2_from = None

    def refresh_bf16(self, on):
        self.calls.append(("refresh_bf16", on))
        if on or self.bf16_on:
            self._void(on != self.bf16_on)
        self.bf16_on, self.bf16_from = on, self.world.content if on else None

    def set_gemm_mode(self, x3):
        self.calls.append(("set_gemm_mode", x3))
        if x3 != self.x3_on:
            self._void(True)
        self.x3_on = x3

    def refresh_h2(self, on):
        self.calls.append(("refresh_h2", on))
        if on or self.h2_on:
            self._void(on != self.h2_on)
        self.h2_on, self.h2_from = on, self.world.content if on else None

    def build_cache(self):
        self.calls.append(("build_cache",))
        self.cache = (self.world.content, self.flavour())

    def drop_cache(self):
        self.calls.append(("drop_cache",))
        self.cache = None

    def prepare(self):
        self.prepared = (self.world.content, self.flavour())

    def state(self):
        return (self.flavour(), self.bf16_from, self.h2_from, self.cache, self.prepared)

    def cache_is_stale(self):
        return self.cache is not None and (self.world.training or self.cache != (self.world.content, self.flavour()))

    def trace(self):
        return [c for c in self.calls if c != ("drop_cache",)]


class NewEngine:
    """what vsrcap.engine.Engine does with a Derived: sync, void the prepare key when told, prepare when the key differs"""

    def __init__(self, world):
        self.world, self.handle, self.derived = world, FakeHandle(world), Derived()
        self.prep_key = None

    def invalidate(self):
        self.derived.invalidate(self.handle)

    def decode(self):
        w = self.world
        if self.derived.sync(w.target(), self.handle):
            self.prep_key = None
        if self.prep_key != (w.ptrs, w.version):
            self.handle.prepare()
            self.prep_key = (w.ptrs, w.version)
        if w.training:
            self.handle.saved = True


class ParentEngine:
    """The five Engine methods and invalidate() of the commit before vsrcap/derived.py, transcribed literally: a ctypes call became the
    backend call of the same meaning, the buffers are left out.  decode() is ControllableCaptioningModel._engine()'s five calls."""

    def __init__(self, world):
        self.world, self.handle = world, FakeHandle(world)
        self._bound_ptrs = None
        self._prep_key = None

    def bind(self, ptrs):
        if ptrs != self._bound_ptrs:
            self.handle.bind(ptrs)
            self._bound_ptrs = ptrs
            self._prep_key = None
            self._cache_key = None

    def invalidate(self):
        self._prep_key = None
        self._cache_key = None
        if getattr(self, "_bf16_key", None) is not None:
            self._bf16_key = ("stale",)
        if getattr(self, "_h2_key", None) is not None:
            self._h2_key = ("stale",)

    def set_gemm_mode(self, x3):
        x3 = bool(x3)
        if x3 != getattr(self, "_x3", True):
            self.handle.set_gemm_mode(x3)
            self._x3 = x3
            self._cache_key = None
            self._prep_key = None

    def set_h2(self, weights_version, enable):
        key = (self._bound_ptrs, weights_version) if enable else None
        if key == getattr(self, "_h2_key", None):
            return
        self.handle.refresh_h2(bool(enable))
        self._cache_key = None
        self._prep_key = None
        self._h2_key = key

    def set_bf16(self, weights_version, enable):
        key = (self._bound_ptrs, weights_version) if enable else None
        if key == getattr(self, "_bf16_key", None):
            return
        self.handle.refresh_bf16(bool(enable))
        if (key is None) != (getattr(self, "_bf16_key", None) is None):
            self._cache_key = None
            self._prep_key = None
        self._bf16_key = key

    def decode_cache(self, weights_version, enable=True):
        key = (self._bound_ptrs, weights_version) if enable else None
        if key == getattr(self, "_cache_key", None):
            return
        if not enable:
            self.handle.drop_cache()
            self._cache_key = None
            return
        self.handle.build_cache()
        self._cache_key = key

    def decode(self):
        w = self.world
        self.bind(w.ptrs)
        self.set_bf16(w.version, w.dtype == "bf16")
        self.set_gemm_mode(w.dtype in ("f32x3", "f16x2"))
        self.set_h2(w.version, w.dtype == "f16x2")
        self.decode_cache(w.version, enable=not w.training)


EVENTS = [("dtype", d) for d in DTYPES] + [("training", False), ("training", True), ("bump",), ("invalidate",), ("rebind",), ("decode",)]


def _apply(world, engines, event):
    kind = event[0]
    if kind == "dtype":
        world.dtype = event[1]
    elif kind == "training":
        world.training = event[1]
    elif kind == "bump":                 # an optimizer step, a graph-building forward, train() / eval(): the version says so
        world.version += 1
        world.content += 1
    elif kind == "invalidate":           # a p.data edit nothing sees, then the documented call
        world.content += 1
        for e in engines:
            e.invalidate()
    elif kind == "rebind":               # the parameters moved to new storage
        world.ptrs = (world.ptrs[0] + "'",)
        world.content += 1
    else:
        for e in engines:
            e.decode()


def _sequences(max_len=4):
    for n in range(max_len + 1):
        yield from itertools.product(EVENTS, repeat=n)


def _run(seq):
    """the sequence followed by a final decode, on the new and the parent bookkeeping side by side; returns (world, new, parent, whether
    each ever decoded with a stale cache in the handle)"""
    world = World()
    new, parent = NewEngine(world), ParentEngine(world)
    stale = [False, False]
    for event in seq + (("decode",),):
        _apply(world, (new, parent), event)
        if event == ("decode",):
            stale[0] |= new.handle.cache_is_stale()
            stale[1] |= parent.handle.cache_is_stale()
    return world, new, parent, stale


def test_every_sequence_converges_never_decodes_from_a_stale_cache_and_keeps_the_parents_calls():
    parent_stale = 0
    for seq in _sequences():
        world, new, parent, stale = _run(seq)
        # converges to fresh: the handle is where a new handle synced straight into the final target is
        fresh = NewEngine(world)
        fresh.decode()
        assert new.handle.state() == fresh.handle.state(), seq
        # ... which is: every product present is built from the current weights in the current flavour
        h = new.handle
        assert h.flavour() == SWITCHES[world.dtype], seq
        assert h.bf16_from == (world.content if h.bf16_on else None) and h.h2_from == (world.content if h.h2_on else None), seq
        assert h.prepared == (world.content, h.flavour()), seq
        assert (h.cache is None) == world.training, seq
        # the stale case
        assert not stale[0], seq
        # behaviour preserved: the parent's calls, plus drops of the decode cache and nothing else
        assert new.handle.trace() == parent.handle.trace(), seq
        parent_stale += stale[1]
    assert parent_stale > 0, "the enumeration does not reach the parent's hole"


def test_python_and_handle_agree_on_the_cache_at_every_point():
    """there is no moment at which the Python side believes 'no cache' while the handle holds one (or the reverse)"""
    for seq in _sequences(3):
        world = World()
        new = NewEngine(world)
        for event in seq + (("decode",),):
            _apply(world, (new,), event)
            assert (new.derived.cache is None) == (new.handle.cache is None), (seq, event)


def _calls(events):
    world = World()
    new = NewEngine(world)
    for event in events:
        _apply(world, (new,), event)
    return new.handle.calls, new.handle


def test_training_loop_refreshes_once_per_forward_and_keeps_the_saved_forward():
    loop = (("training", True), ("decode",), ("bump",), ("decode",), ("bump",), ("decode",))
    calls, h = _calls(loop)
    assert calls == [("bind", ("A",)), ("refresh_h2", True), ("refresh_h2", True), ("refresh_h2", True)]
    assert h.saved                                   # a refresh while on keeps the forward a backward is still owed for
    calls, _ = _calls((("dtype", "bf16"),) + loop)
    assert calls == [("bind", ("A",)), ("refresh_bf16", True), ("set_gemm_mode", False), ("refresh_bf16", True), ("refresh_bf16", True)]
    calls, _ = _calls((("dtype", "f32"),) + loop)
    assert calls == [("bind", ("A",)), ("set_gemm_mode", False)]


def test_eval_train_eval():
    seq = (("decode",), ("training", True), ("bump",), ("decode",), ("training", False), ("bump",), ("decode",))
    calls, _ = _calls(seq)              # f16x2: the refresh itself voids the handle's cache, no drop needed
    assert calls == [("bind", ("A",)), ("refresh_h2", True), ("build_cache",),
                     ("refresh_h2", True),
                     ("refresh_h2", True), ("build_cache",)]
    calls, _ = _calls((("dtype", "bf16"),) + seq)
    assert calls == [("bind", ("A",)), ("refresh_bf16", True), ("set_gemm_mode", False), ("build_cache",),
                     ("refresh_bf16", True),
                     ("refresh_bf16", True), ("build_cache",)]
    calls, _ = _calls((("dtype", "f32x3"),) + seq)      # no refresh call to void it: the drop is explicit
    assert calls == [("bind", ("A",)), ("build_cache",),
                     ("drop_cache",),
                     ("build_cache",)]


@pytest.mark.parametrize("a,b", [(a, b) for a in DTYPES for b in DTYPES if a != b])
def test_dtype_switch_goes_bf16_then_mode_then_h2_then_cache(a, b):
    def moves(frm, to):
        (b0, x0, h0), (b1, x1, h1) = frm, to
        return ([("refresh_bf16", b1)] if b0 != b1 else []) + ([("set_gemm_mode", x1)] if x0 != x1 else []) + \
               ([("refresh_h2", h1)] if h0 != h1 else [])
    calls, _ = _calls((("dtype", a), ("decode",), ("dtype", b), ("decode",)))
    default = (False, True, False)
    assert calls == ([("bind", ("A",))] + moves(default, SWITCHES[a]) + [("build_cache",)] +
                     moves(SWITCHES[a], SWITCHES[b]) + [("build_cache",)])


def test_sizes_that_are_no_multiple_of_8_run_f16x2_as_plain_f32x3():
    h = FakeHandle(World())
    d = Derived()
    assert d.sync((("A",), 0, "f16x2", False, False), h) is True
    assert h.calls == [("bind", ("A",)), ("build_cache",)] and not h.h2_on
    assert d.sync((("A",), 0, "f16x2", False, False), h) is False and len(h.calls) == 2


def test_a_call_that_raises_leaves_the_product_not_built():
    class Failing(FakeHandle):
        def refresh_h2(self, on):
            raise RuntimeError("buffer too small")
    h = Failing(World())
    d = Derived()
    with pytest.raises(RuntimeError):
        d.sync((("A",), 0, "f16x2", True, False), h)
    assert d.h2 is None and not d.h2_on and d.cache is None and d.statics_void
