"""Lineage of a manual decode loop under autograd: which tape a step() call belongs to.

The reference's step() (controllable_captioning.py:117-190) is plain autograd, and CaptioningModel.forward (:22-36) is a loop over it
from init_state.  Here a grad-enabled step() appends to a TAPE - a training forward saved one step at a time (include/vsrcap.h,
vsr_train_tape_begin) - and one hand-written backward differentiates the whole tape.  That only describes a loop the library can replay:
a chain of steps from the zero state, every step fed the state the step before returned.  This module decides, from the state
tensors alone, whether a call continues such a chain, opens one, or is something the tape cannot express - and then says so.

  init_state() records the state it returned                        -> Lineage.note_init
  a step whose state is one init_state returned opens a tape        -> Lineage.resolve returns None
  a step whose state is the one a tape's last step returned appends -> Lineage.resolve returns that tape
  anything else raises TapeError: a branch (a state an EARLIER step of a tape returned), an edited state (tensor._version moved), a
  mix of two states, a state from nowhere, more steps than the tape was opened for, a tape that has already been differentiated.

"Same state" = the same tensor objects with unmodified _version.  States are held by weak reference: a tape lives exactly as long as
the autograd graph of its steps (the caller's outputs), never because of this registry.

No dependency on the library or on a GPU: the rules are tested on CPU tensors (tests/test_step_tape_logic.py)."""
import weakref

ALTERNATIVE = ("A differentiable manual loop is a chain of step() calls from init_state(), each fed the state the call before returned, at most "
               "seq_len steps, without gradients to the state and without verb forcing; for anything else use forward() / sample_rl(), "
               "which are differentiable as a whole, or call step() under torch.no_grad().")


class TapeError(RuntimeError):
    def __init__(self, what):
        super().__init__("step() under autograd: %s. %s" % (what, ALTERNATIVE))


def state_tensors(state):
    """((h1, c1), (h2, c2), slot) -> the five tensors"""
    (h1, c1), (h2, c2), slot = state
    return (h1, c1, h2, c2, slot)


class StateRef:
    """identity and write counters of a state's tensors, without keeping them alive"""
    __slots__ = ("refs", "versions")

    def __init__(self, state):
        ts = state_tensors(state)
        self.refs = [weakref.ref(t) for t in ts]
        self.versions = [t._version for t in ts]

    def alive(self):
        return all(r() is not None for r in self.refs)

    def shared(self, state):
        """how many of the state's tensors are this record's"""
        return sum(1 for r, t in zip(self.refs, state_tensors(state)) if r() is t)

    def same_tensors(self, state):
        return self.shared(state) == len(self.refs)

    def unmodified(self, state):
        return all(v == t._version for v, t in zip(self.versions, state_tensors(state)))


class Tape:
    """The lineage side of one tape: the steps taken, the state its last step returned and those the earlier steps returned.  The owner
    (vsrcap/train.py) subclasses it with what the library needs; autograd nodes hold it, the Lineage only a weak reference."""

    def __init__(self, max_steps):
        self.max_steps = int(max_steps)
        self.steps = 0
        self.last = None                 # StateRef of the newest state (None until the first step has returned)
        self.earlier = []                # StateRefs of the states before it: feeding one of them again is a branch
        self.closed = False              # differentiated: no further step

    def advance(self, state_out):
        if self.last is not None:
            self.earlier.append(self.last)
        self.last = StateRef(state_out)
        self.steps += 1


class Lineage:
    MAX_INITS = 64                       # init_state() records kept (dead ones are dropped first)

    def __init__(self):
        self._inits = []
        self._tapes = []                 # weak references

    def __getstate__(self):              # (a pickled / copied model starts without records: they are weak references to live tensors)
        return {}

    def __setstate__(self, state):
        self._inits, self._tapes = [], []

    def note_init(self, state):
        self._inits = [r for r in self._inits if r.alive()][-(self.MAX_INITS - 1):]
        self._inits.append(StateRef(state))
        return state

    def tapes(self):
        live = [(r, r()) for r in self._tapes]
        self._tapes = [r for r, t in live if t is not None]
        return [t for _, t in live if t is not None]

    def register(self, tape):
        """a tape just opened (resolve() returned None for its first state)"""
        self._tapes.append(weakref.ref(tape))
        return tape

    def resolve(self, state):
        """None: the state is one init_state() returned - open a tape.  A Tape: the state is the one its last step returned - append.
        Raises TapeError for everything else."""
        tapes = self.tapes()
        for tape in tapes:
            if tape.last is not None and tape.last.same_tensors(state):
                if not tape.last.unmodified(state):
                    raise TapeError("the state was modified in place after the step that returned it (the saved forward holds the "
                                    "unmodified one; gradients to an edited state are out of scope)")
                if tape.closed:
                    raise TapeError("this loop has already been differentiated: its saved forward is sealed, a further step needs a new "
                                    "loop from init_state()")
                if tape.steps >= tape.max_steps:
                    raise TapeError("this would be step %d of a loop whose limit is %d steps (seq_len, or the slots of the region "
                                    "sequence in teacher-forcing mode)" % (tape.steps + 1, tape.max_steps))
                return tape
        for rec in self._inits:
            if rec.same_tensors(state):
                if not rec.unmodified(state):
                    raise TapeError("the initial state was modified in place after init_state() returned it (a loop starts from the "
                                    "zero state; a non-zero initial state is out of scope)")
                return None
        for tape in tapes:
            if any(e.same_tensors(state) for e in tape.earlier):
                raise TapeError("the state was returned by an earlier step of a loop that has moved on: branching a loop is not "
                                "supported (one saved forward holds one chain of steps)")
        known = [t.last for t in tapes if t.last is not None] + [e for t in tapes for e in t.earlier] + self._inits
        if any(r.shared(state) for r in known):
            raise TapeError("the state mixes tensors of different steps, loops or init_state() calls")
        raise TapeError("the state was returned neither by init_state() nor by the last step of a loop (a detached copy, a state built "
                        "by hand, or one whose loop is gone)")
