"""The bookkeeping of the live training forwards (vsrcap/forwards.py) against a fake library that follows the saved-forward rules of
include/vsrcap.h (at vsr_train_select): forwards filed under a strictly increasing generation in the two buffers they were given, dropped
when a later call is handed one of those buffers or the flavour changes.  Every sequence of up to five events is enumerated, on the new
bookkeeping and on a literal transcription of the slot code it replaced.  No library, no GPU: the GPU side is
tests/test_gpu_live_forwards.py."""
import weakref

import pytest

from vsrcap.forwards import MAX_LIVE_FORWARDS, ForwardToken, Forwards

SIZES = {"small": 1, "large": 2}
MAX_FORWARDS, MAX_EVENTS, TAPE_STEPS = 3, 5, 2


class FakeLibraryError(AssertionError):
    pass


class Buf:
    """a caller buffer: an opaque object that is allocated until the backend replaces it"""
    __slots__ = ("name", "size", "allocated")

    def __init__(self, name, size):
        self.name, self.size, self.allocated = name, size, True


class FakeLibrary:
    """The library's side.  trace: the list its calls are recorded in (the engine's own, so decisions and calls interleave).
    truly_live(): the generations somebody can still ask the first gradient of - what is true outside, whatever the host side believes."""

    def __init__(self, trace, truly_live):
        self.trace, self.truly_live = trace, truly_live
        self.counter = 0
        self.saved = {}                  # generation -> (prepare workspace, training workspace)
        self.filed_in = {}               # ... and the same for every generation ever filed
        self.current = 0                 # the handle's current forward (0: none)
        self.ws = None                   # the workspace of the last prepare / select

    def _handed(self, buf, who):
        if not buf.allocated:
            raise FakeLibraryError("%s was handed the freed buffer %s" % (who, buf.name))
        for g in self.truly_live():
            if buf in self.filed_in[g]:
                raise FakeLibraryError("%s was handed %s, which the live forward %d is saved in" % (who, buf.name, g))
        for g in [g for g, bufs in self.saved.items() if buf in bufs]:
            del self.saved[g]

    def _intact(self, g, who):
        for buf in self.saved[g]:
            if not buf.allocated:
                raise FakeLibraryError("%s of generation %d reads the freed buffer %s" % (who, g, buf.name))

    def prepare(self, ws):
        self.trace.append(("prepare", ws.name))
        self._handed(ws, "prepare")
        self.current, self.ws = 0, ws

    def file(self, tws, what):
        """vsr_train_forward* / vsr_train_tape_begin"""
        assert self.ws is not None, "prepare first"
        self._handed(tws, what)
        self.counter += 1
        self.current = self.counter
        self.saved[self.current] = self.filed_in[self.current] = (self.ws, tws)
        self.trace.append((what, tws.name, self.current))

    def generation(self):
        return self.current

    def select(self, g):
        ok = g > 0 and (g == self.current or g in self.saved)
        self.trace.append(("select", g, ok))
        if ok:
            self.current, self.ws = g, self.saved[g][0]
        return ok

    def backward(self):
        """vsr_train_backward differentiates the handle's CURRENT forward"""
        assert self.current, "no current forward"
        self.trace.append(("backward", self.current))
        self._intact(self.current, "backward")

    def tape_step(self, g):
        assert self.select(g), "the engine selects first"
        self._intact(g, "tape step")

    tape_seal = tape_step

    def flavour_change(self):
        self.trace.append(("flavour",))
        self.saved.clear()
        self.current, self.ws = 0, None


class Gone(Exception):
    pass


class FakeBackend:
    """what both engines share: the fake library, buffers that grow like engine._grown, and the records of the forwards taken"""

    def __init__(self):
        self.trace = []
        self.taken = []                  # per forward / tape: [generation, token, differentiated by the library]
        self.lib = FakeLibrary(self.trace, lambda: [g for g, tok, done in self.taken if tok is not None and not done])
        self.names = 0

    def grown(self, buf, size):
        if buf is None or buf.size < size:
            if buf is not None:
                buf.allocated = False    # nobody else holds the tensor: back to the allocator
            self.names += 1
            return Buf("b%d" % self.names, size)
        return buf

    def guarded(self, call, *args):
        """the documented errors become trace entries; anything else (the fake library's assertions) propagates"""
        try:
            return call(*args)
        except RuntimeError as e:
            kind = "gone" if "saved activations are gone" in str(e) else "limit" if "alive and not yet differentiated" in str(e) else None
            if kind is None:
                raise
            self.trace.append(("raise", kind))
            if kind == "gone":
                raise Gone()
            raise

    # the events, as models/controllable_captioning.py and vsrcap/train.py compose them from Engine's methods
    def forward(self, size):
        self.guarded(self.prepare, size, size, True)
        g = self.train_forward(size)
        self.taken.append([g, self.note_forward(), False])

    def tape(self, size):
        self.guarded(self.prepare, size, size, True)
        g, token = self.tape_begin(size)
        self.taken.append([g, token, False])

    def step(self, i):
        self.guarded(self.tape_step, self.taken[i][0])

    def backward(self, i, tape):
        g = self.taken[i][0]
        if tape:
            self.guarded(self.tape_seal, g)
        self.guarded(self.train_backward, g)
        assert self.lib.trace[-1] == ("backward", g), "the backward ran on another forward than the one it names"
        self.taken[i][2] = True

    def drop(self, i):
        self.taken[i][1] = None

    def decode(self, size):
        self.prepare(size, size, False)


class NewEngine(FakeBackend):
    """what vsrcap.engine.Engine does with a Forwards"""

    def __init__(self):
        super().__init__()
        self.forwards = Forwards()
        self.orphan = False              # the last make_current found no slot that knows the generation

    def _where(self):
        return self.forwards.slots.index(self.forwards.current)

    def flavour(self):
        self.lib.flavour_change()        # (Derived.sync issues the call and says the statics are void)
        self.forwards.void_key()

    def prepare(self, key, size, for_training):
        slot = self.forwards.begin_prepare(key, for_training)
        if slot is None:
            self.trace.append(("served", self._where()))
            return
        self.trace.append(("slot", self._where()))
        slot.ws = self.grown(slot.ws, size)
        self.lib.prepare(slot.ws)
        self.forwards.prepared(key, None)

    def train_forward(self, size):
        slot = self.forwards.filing_slot("training forward")
        slot.tws = self.grown(slot.tws, size)
        self.lib.file(slot.tws, "forward")
        self.forwards.filed(self.lib.generation())
        return self.lib.generation()

    def note_forward(self):
        return self.forwards.note_forward()

    def _make_current(self, generation, who, differentiate=False):
        calls = len(self.trace)
        try:
            self.forwards.make_current(generation, who, lambda g: None if self.lib.select(g) else "the library's words", differentiate)
        finally:
            self.orphan = len(self.trace) == calls
        self.trace.append(("current", self._where()))

    def train_backward(self, generation):
        self._make_current(generation, "backward of a forward pass", differentiate=True)
        self.lib.backward()

    def tape_begin(self, size):
        slot = self.forwards.filing_slot("tape")
        slot.tws = self.grown(slot.tws, size)
        self.lib.file(slot.tws, "tape")
        self.forwards.filed(self.lib.generation())
        return slot.generation, self.note_forward()

    def tape_step(self, generation):
        self._make_current(generation, "step of a manual loop")
        self.lib.tape_step(generation)

    def tape_seal(self, generation):
        self._make_current(generation, "backward of a manual loop")
        self.lib.tape_seal(generation)

    def n_slots(self):
        return len(self.forwards.slots)


class _ParentSlot:
    __slots__ = ("ws", "tws", "keep", "token", "generation", "differentiated")

    def __init__(self):
        self.ws = self.tws = self.keep = self.token = None
        self.generation = 0
        self.differentiated = True

    def live(self):
        return self.token is not None and self.token() is not None and not self.differentiated


class ParentEngine(FakeBackend):
    """The slot code of the commit before vsrcap/forwards.py, transcribed literally from its engine.py: _Slot and the _ws / _tws / _keep
    properties, _claim_slot, the cache test of _prepare_in_slot, the flag assignments of train_forward, note_forward, train_backward's
    differentiated = True, _make_current with its else-less loop, tape_begin.  A ctypes call became the fake library's call of the same
    meaning, _grown the backend's grown."""

    def __init__(self):
        super().__init__()
        self._slots = [_ParentSlot()]
        self._slot = self._slots[0]
        self._prep_key = None
        self.orphan = False

    _ws = property(lambda self: self._slot.ws, lambda self, v: setattr(self._slot, "ws", v))
    _tws = property(lambda self: self._slot.tws, lambda self, v: setattr(self._slot, "tws", v))
    _keep = property(lambda self: self._slot.keep, lambda self, v: setattr(self._slot, "keep", v))

    def _where(self):
        return self._slots.index(self._slot)

    def flavour(self):
        self.lib.flavour_change()
        self._prep_key = None

    def _claim_slot(self):
        if not self._slot.live():
            return
        for sl in self._slots:
            if not sl.live():
                self._slot = sl
                return
        if len(self._slots) >= MAX_LIVE_FORWARDS:
            raise RuntimeError("%d training forwards of this model are alive and not yet differentiated: each holds its own workspaces "
                               "(~GBs at batch 100). Call backward() on some of them (or drop their outputs) before the next forward."
                               % len(self._slots))
        self._slot = _ParentSlot()
        self._slots.append(self._slot)

    def prepare(self, key, size, for_training):
        if key == self._prep_key and not (for_training and self._slot.live()):
            self.trace.append(("served", self._where()))
            return
        self._prep_key = None
        self._claim_slot()
        self.trace.append(("slot", self._where()))
        self._ws = self.grown(self._ws, size)
        self.lib.prepare(self._ws)
        self._keep = None
        self._prep_key = key

    def train_forward(self, size):
        self._tws = self.grown(self._tws, size)
        if self._slot.live():
            raise RuntimeError("internal: training forward into a slot that holds a live forward (prepare(for_training=True) first)")
        self.lib.file(self._tws, "forward")
        self._slot.generation = self.lib.generation()
        self._slot.token = None
        self._slot.differentiated = True
        return self.lib.generation()

    def note_forward(self):
        tok = ForwardToken(self._slot.generation)
        self._slot.token = weakref.ref(tok)
        self._slot.differentiated = False
        return tok

    def train_backward(self, generation):
        self._make_current(generation, "backward of a forward pass")
        self._slot.differentiated = True
        self.lib.backward()

    def _make_current(self, generation, who):
        if not self.lib.select(generation):
            raise RuntimeError("%s whose saved activations are gone (%s)." % (who, "the library's words"))
        if self._slot.generation != generation:
            for sl in self._slots:
                if sl.generation == generation:
                    self._slot = sl
                    self._prep_key = None
                    break
        self.trace.append(("current", self._where()))

    def tape_begin(self, size):
        if self._slot.live():
            raise RuntimeError("internal: tape into a slot that holds a live forward (prepare(for_training=True) first)")
        self._tws = self.grown(self._tws, size)
        self.lib.file(self._tws, "tape")
        self._slot.generation = self.lib.generation()
        return self._slot.generation, self.note_forward()

    def tape_step(self, generation):
        self._make_current(generation, "step of a manual loop")
        self.lib.tape_step(generation)

    def tape_seal(self, generation):
        self._make_current(generation, "backward of a manual loop")
        self.lib.tape_seal(generation)

    def n_slots(self):
        return len(self._slots)


# ---------------------------------------------------------------------------------------------------- the enumeration
def _next_events(taken):
    """taken: per forward so far [is a tape, steps, differentiated at least once, graph consumed, outputs dropped] - which events autograd
    and the tape's lineage (vsrcap/steptape.py) let through to the engine at all"""
    ev = []
    if len(taken) < MAX_FORWARDS:
        ev += [("forward", s) for s in SIZES] + [("tape", "small")]      # (a tape files like a forward: one size of it keeps the count down)
    for i, (tape, steps, closed, consumed, dropped) in enumerate(taken):
        if dropped:
            continue
        if tape and not closed and steps < TAPE_STEPS:
            ev.append(("step", i))
        if not consumed:                 # (a second backward without retain_graph fails in autograd, before the engine is asked)
            ev += [("backward", i, True), ("backward", i, False)]
        ev.append(("drop", i))
    return ev + [("decode", s) for s in SIZES] + [("flavour",)]


def _advance(taken, event):
    taken = [list(t) for t in taken]
    if event[0] in ("forward", "tape"):
        taken.append([event[0] == "tape", 0, False, False, False])
    elif event[0] == "step":
        taken[event[1]][1] += 1
    elif event[0] == "backward":
        taken[event[1]][2] = True
        taken[event[1]][3] = not event[2]
    elif event[0] == "drop":
        taken[event[1]][4] = True
    return taken


def _sequences(max_len=MAX_EVENTS, seq=(), taken=()):
    yield seq, taken
    if len(seq) < max_len:
        for event in _next_events(taken):
            yield from _sequences(max_len, seq + (event,), _advance(taken, event))


def _apply(engine, event, taken):
    """one event on one engine -> None, 'gone' (the documented error) or 'tripped' (an assertion of the fake library)"""
    kind = event[0]
    try:
        if kind in ("forward", "tape", "decode"):
            getattr(engine, kind)(SIZES[event[1]])
        elif kind == "step":
            engine.step(event[1])
        elif kind == "backward":
            engine.backward(event[1], taken[event[1]][0])
        elif kind == "drop":
            engine.drop(event[1])
        else:
            engine.flavour()
    except Gone:
        return "gone"
    except FakeLibraryError:
        return "tripped"
    return None


ADVISOR = (("forward", "small"), ("backward", 0, True), ("forward", "large"), ("backward", 0, False))


def _run(seq):
    """the sequence on the new bookkeeping and on the parent's, side by side -> (new engine, the parent's outcome at every event where
    the new one was asked for a generation no slot holds)"""
    new, parent = NewEngine(), ParentEngine()
    taken, orphans, raised = (), [], False
    for event in seq:
        at = len(new.trace)
        got = _apply(new, event, taken)
        assert got != "tripped", (seq, event, new.trace)
        assert new.n_slots() <= MAX_LIVE_FORWARDS
        raised |= got is not None
        if parent is not None:
            their_at = len(parent.trace)
            was = _apply(parent, event, taken)
            mine, theirs = new.trace[at:], parent.trace[their_at:]
            if got == "gone" and new.orphan:
                # the one exception: the parent asks the library, which refuses - or does not, and then a freed buffer is read
                orphans.append(was)
                assert was in ("gone", "tripped"), (seq, event, theirs)
                assert mine[-1] == ("raise", "gone") and mine[:-1] == theirs[:len(mine) - 1], (seq, event, mine, theirs)
                if was == "gone":
                    assert theirs[len(mine) - 1:] == [("select", theirs[-2][1], False), ("raise", "gone")], (seq, event, theirs)
                else:
                    parent = None        # its state is not worth following any further
            else:
                assert (got, mine) == (was, theirs), (seq, event, mine, theirs)
        taken = _advance(taken, event)
    if raised:                           # the owner's state is still consistent: the next forward and its backward go through
        for event in (("forward", "small"), ("backward", len(taken), False)):
            assert _apply(new, event, [[False]] * (len(taken) + 1)) is None, (seq, new.trace)
    return new, orphans


def test_every_sequence_is_safe_on_the_new_bookkeeping_and_decides_as_the_parent_did():
    holes, refused, n = [], 0, 0
    for seq, taken in _sequences():
        new, orphans = _run(seq)
        n += 1
        refused += orphans.count("gone")
        if "tripped" in orphans:
            holes.append(seq)
    assert n > 10000 and refused > 0
    # the sequences in which the parent differentiates (or steps, or seals) a forward whose buffers went back to the allocator:
    # all of them ask for a generation after a LARGER prepare / forward replaced a buffer of its slot
    assert ADVISOR in holes
    for seq in holes:
        assert any(e[0] in ("forward", "decode") and e[1] == "large" for e in seq[1:]), seq


def test_the_advisors_sequence_on_both():
    new, orphans = _run(ADVISOR)
    assert orphans == ["tripped"]
    assert new.trace[new.trace.index(("raise", "gone")) - 1] == ("forward", "b4", 2)     # no library call after the larger forward
    assert new.forwards.live_count() == 1                                                # the larger forward is still owed its backward
    parent = ParentEngine()
    for event in ADVISOR[:-1]:
        assert _apply(parent, event, [[False]] * 2) is None
    with pytest.raises(FakeLibraryError, match="backward of generation 1 reads the freed buffer"):
        parent.backward(0, False)
    assert parent._slot.differentiated and parent._slot.generation == 2                  # ... and the live forward's slot was marked


@pytest.mark.parametrize("retain", [False, True])
def test_forward_backward_pairs_of_any_sizes_stay_in_one_slot(retain):
    import itertools
    for sizes in itertools.product(SIZES, repeat=4):
        new = NewEngine()
        for i, s in enumerate(sizes):
            new.forward(SIZES[s])
            new.backward(i, False)
            if retain:
                new.backward(i, False)
        assert new.n_slots() == 1, sizes


def test_a_ninth_live_forward_raises_and_the_next_one_goes_through_once_one_is_gone():
    for free in ("drop", "backward"):
        new, parent = NewEngine(), ParentEngine()
        for e in (new, parent):
            for _ in range(MAX_LIVE_FORWARDS):
                e.forward(SIZES["small"])
            assert e.n_slots() == MAX_LIVE_FORWARDS
            with pytest.raises(RuntimeError, match="%d training forwards of this model are alive and not yet differentiated" % MAX_LIVE_FORWARDS):
                e.forward(SIZES["small"])
            assert len(e.taken) == MAX_LIVE_FORWARDS
            if free == "drop":
                e.drop(3)
            else:
                e.backward(3, False)
            e.forward(SIZES["large"])
            e.backward(MAX_LIVE_FORWARDS, False)
            e.backward(0, False)                     # the others are still differentiable
            assert e.n_slots() == MAX_LIVE_FORWARDS
        assert new.trace == parent.trace
        assert new.forwards.live_count() == MAX_LIVE_FORWARDS - 2


def test_a_prepare_that_raises_leaves_no_key_and_no_generation_behind():
    new = NewEngine()
    new.forward(SIZES["small"])
    new.backward(0, True)
    fw = new.forwards
    assert fw.prep_key == SIZES["small"] and fw.current.generation == 1
    assert fw.begin_prepare("other", False) is fw.current       # the library call that would follow raises: nothing else happens
    assert fw.prep_key is None and fw.current.generation == 0
    with pytest.raises(Gone):
        new.backward(0, False)
    assert new.trace[-1] == ("raise", "gone") and new.trace[-2][0] == "backward"         # (the first one's): the library was not asked
