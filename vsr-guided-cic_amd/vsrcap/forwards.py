"""The training forwards one handle keeps alive at once, and the caller buffers they are saved in.

A forward's saved state lives in a SLOT: the pair of buffers it was given (the vsr_prepare*() workspace `ws` and the training workspace
`tws`) plus the inputs the library borrows (`keep`).  The library files every forward (and every tape of a manual step() loop) under a
strictly increasing generation and drops it when a later call is handed memory that overlaps its buffers (include/vsrcap.h at
vsr_train_select).  Forwards mirrors that on the host: the slots, which one is current (the one the handle's pointers are in), each
slot's generation / token / differentiated flag, and the key of the statics the handle has prepared.  The calls go through a backend
(vsrcap/engine.py: allocation, ctypes, device and stream); buffers are opaque objects here.  The rules:

  Generations.  A generation is known to at most one slot, and a slot knows at most the last forward or tape filed in its buffers
  (generations only grow, so filing cannot collide).  A slot forgets its generation when either of its buffer objects is replaced
  (Slot.ws / Slot.tws), when a prepare writes into its workspace (begin_prepare) and when a new forward or tape is about to be filed
  in it (filing_slot) - each time before the library is called, so a call that raises leaves nothing behind.
  Live.  A slot is live while its forward's token (ForwardToken, held by the autograd node) is alive and the forward has not been
  differentiated.  A live slot's buffers are never given to a prepare-for-training, a training forward or a tape.
  Claiming.  A prepare that would overwrite a live current slot moves to the first slot that is not live, or opens one; a slot beyond
  MAX_LIVE_FORWARDS raises.  An ordinary forward / backward loop therefore stays in one slot.
  Serving a prepare from the cache.  Served when the key matches, except for_training into a live slot.  The key is void from the moment
  a prepare starts until it has succeeded (prepared), whenever the current slot changes, and when the owner of the weights' derived
  state says so (void_key: Derived.sync, adam_step).
  Making a forward current (backward, tape step, tape seal).  The slot that knows the generation is looked up FIRST; if none does the
  "saved activations are gone" error is raised and the library is not called (it may still hold an entry whose buffers went back to the
  allocator).  Only then the library selects; its refusal (a flavour change dropped every saved forward) raises the same error with its
  message.  After success that slot is current, and only that slot is ever marked differentiated.

No torch, no ctypes: tests/test_forwards_logic.py enumerates event sequences against a fake library."""
import weakref

MAX_LIVE_FORWARDS = 8


class ForwardToken:
    """Lives in the autograd node of one training forward (train._DecoderFn): while it is alive and its forward has not been
    differentiated, the buffers that forward was saved in are not handed to anyone else."""
    __slots__ = ("generation", "__weakref__")

    def __init__(self, generation):
        self.generation = generation


class Slot:
    """One pair of caller buffers of the C ABI - the vsr_prepare*() workspace and the training workspace - plus the inputs they borrow.
    A saved training forward lives in exactly one slot (include/vsrcap.h, vsr_train_select)."""
    __slots__ = ("_ws", "_tws", "keep", "token", "generation", "differentiated")

    def __init__(self):
        self._ws = self._tws = self.keep = None
        self.forget()

    def forget(self):
        self.token = None
        self.generation = 0
        self.differentiated = True

    def live(self):
        """holds a forward somebody can still ask the gradient of for the FIRST time"""
        return self.token is not None and self.token() is not None and not self.differentiated

    def _replace(self, name, buf):
        if buf is not getattr(self, name):           # the old object goes back to the allocator: what was saved in it is gone
            setattr(self, name, buf)
            self.forget()

    ws = property(lambda self: self._ws, lambda self, buf: self._replace("_ws", buf))
    tws = property(lambda self: self._tws, lambda self, buf: self._replace("_tws", buf))


def gone(who, why):
    return RuntimeError(
        "%s whose saved activations are gone (%s). A forward stays differentiable until its "
        "buffers are reused: that happens once it HAS been differentiated (a second backward needs a new forward - "
        "retain_graph=True is not supported across a later forward), when more than %d forwards are alive, or when "
        "the compute dtype / the parameters' storage changed in between." % (who, why, MAX_LIVE_FORWARDS))


class Forwards:
    def __init__(self):
        self.slots = [Slot()]                # more than one only while several training forwards are alive
        self.current = self.slots[0]
        self.prep_key = None                 # whose hoisted statics the handle holds; None: nobody's

    def live_count(self):
        return sum(1 for sl in self.slots if sl.live())

    def void_key(self):
        self.prep_key = None

    def begin_prepare(self, key, for_training):
        """None: served from the cache.  Else the slot whose workspace the prepare writes; the key is void until prepared(key)."""
        if key == self.prep_key and not (for_training and self.current.live()):
            return None
        self.prep_key = None
        if self.current.live():
            self.current = next((sl for sl in self.slots if not sl.live()), None) or self._open()
        self.current.forget()
        return self.current

    def _open(self):
        """The reference has no limit at all (eager autograd); MAX_LIVE_FORWARDS pairs of buffers is where this build stops."""
        if len(self.slots) >= MAX_LIVE_FORWARDS:
            raise RuntimeError("%d training forwards of this model are alive and not yet differentiated: each holds its own workspaces "
                               "(~GBs at batch 100). Call backward() on some of them (or drop their outputs) before the next forward."
                               % len(self.slots))
        self.slots.append(Slot())
        return self.slots[-1]

    def prepared(self, key, keep):
        self.current.keep = keep
        self.prep_key = key

    def filing_slot(self, what):
        """the current slot, for a training forward or a tape about to be filed in it"""
        if self.current.live():
            raise RuntimeError("internal: %s into a slot that holds a live forward (prepare(for_training=True) first)" % what)
        self.current.forget()
        return self.current

    def filed(self, generation):
        """the library filed a forward in the current slot; nobody can ask for its gradient until note_forward() hands out its token"""
        self.current.generation = generation

    def note_forward(self):
        """the autograd node of the forward just filed: returns the token that keeps its buffers reserved"""
        tok = ForwardToken(self.current.generation)
        self.current.token = weakref.ref(tok)
        self.current.differentiated = False
        return tok

    def make_current(self, generation, who, select, differentiate=False):
        """select(generation): the library call, returns None or the library's words for its refusal"""
        slot = next((sl for sl in self.slots if generation and sl.generation == generation), None)
        why = "no buffers of this model hold them any more" if slot is None else select(generation)
        if why is not None:
            raise gone(who, why)
        if slot is not self.current:
            self.current = slot
            self.prep_key = None             # the handle's hoisted state is this slot's now
        if differentiate:
            slot.differentiated = True
