"""The lineage rules of a manual step() loop under autograd (vsrcap/steptape.py) on plain CPU tensors: which call opens a tape,
which appends, and what is refused - a branch, an edited state, a mix, a state from nowhere, a step past the limit, a step after the
backward.  No library, no GPU: the GPU side is tests/test_gpu_step_grad.py."""
import gc

import pytest
import torch

from vsrcap import steptape
from vsrcap.steptape import Lineage, Tape, TapeError


def _state(fill=0.0):
    z = lambda: torch.full((3, 4), fill)
    return (z(), z()), (z(), z()), torch.zeros(3, dtype=torch.long)


def _step(lin, state, max_steps=3, share_slot=False):
    """what ControllableCaptioningModel._step_taped does with the lineage: resolve, open or append, advance"""
    tape = lin.resolve(state)
    if tape is None:
        tape = lin.register(Tape(max_steps))
    new = _state(1.0)
    if share_slot:                       # teacher forcing hands the slot tensor through
        new = (new[0], new[1], state[2])
    tape.advance(new)
    return tape, new


def test_open_then_append():
    lin = Lineage()
    s0 = lin.note_init(_state())
    assert lin.resolve(s0) is None
    tape, s1 = _step(lin, s0)
    assert tape.steps == 1
    assert lin.resolve(s1) is tape
    t2, s2 = _step(lin, s1)
    assert t2 is tape and tape.steps == 2 and lin.resolve(s2) is tape


def test_slot_tensor_handed_through_does_not_confuse_the_states():
    lin = Lineage()
    s0 = lin.note_init(_state())
    tape, s1 = _step(lin, s0, share_slot=True)
    _, s2 = _step(lin, s1, share_slot=True)
    assert s2[2] is s0[2]
    assert lin.resolve(s2) is tape
    with pytest.raises(TapeError, match="branching"):
        lin.resolve(s1)


def test_branch_raises_and_names_the_alternative():
    lin = Lineage()
    s0 = lin.note_init(_state())
    tape, s1 = _step(lin, s0)
    _step(lin, s1)
    with pytest.raises(TapeError, match="branching") as e:
        lin.resolve(s1)
    assert "forward()" in str(e.value) and "sample_rl()" in str(e.value)
    assert isinstance(e.value, RuntimeError)
    assert tape.steps == 2               # the refused call left the tape as it was


def test_the_initial_state_may_open_several_tapes():
    lin = Lineage()
    s0 = lin.note_init(_state())
    a, sa = _step(lin, s0)
    b, sb = _step(lin, s0)
    assert a is not b
    assert lin.resolve(sa) is a and lin.resolve(sb) is b


def test_edited_state_raises():
    lin = Lineage()
    s0 = lin.note_init(_state())
    tape, s1 = _step(lin, s0)
    s1[0][0].mul_(0.5)                   # bumps _version
    with pytest.raises(TapeError, match="modified in place"):
        lin.resolve(s1)


def test_edited_initial_state_raises():
    lin = Lineage()
    s0 = lin.note_init(_state())
    s0[1][1].add_(1.0)
    with pytest.raises(TapeError, match="initial state was modified"):
        lin.resolve(s0)


def test_state_from_another_tape():
    lin = Lineage()
    a, sa = _step(lin, lin.note_init(_state()))
    b, sb = _step(lin, lin.note_init(_state()))
    assert lin.resolve(sb) is b and lin.resolve(sa) is a        # each state continues ITS tape
    mixed = (sa[0], sb[1], sa[2])
    with pytest.raises(TapeError, match="mixes tensors"):
        lin.resolve(mixed)
    other = Lineage()                                            # another model's registry knows neither
    with pytest.raises(TapeError, match="neither by init_state"):
        other.resolve(sa)


def test_state_from_nowhere_raises():
    lin = Lineage()
    lin.note_init(_state())
    with pytest.raises(TapeError, match="neither by init_state"):
        lin.resolve(_state())
    s0 = lin.note_init(_state())
    _, s1 = _step(lin, s0)
    detached = ((s1[0][0].detach(), s1[0][1].detach()), (s1[1][0].detach(), s1[1][1].detach()), s1[2].clone())
    with pytest.raises(TapeError):
        lin.resolve(detached)


def test_step_count_limit():
    lin = Lineage()
    s = lin.note_init(_state())
    for _ in range(3):
        tape, s = _step(lin, s, max_steps=3)
    assert tape.steps == 3
    with pytest.raises(TapeError, match="step 4 of a loop whose limit is 3"):
        lin.resolve(s)


def test_no_step_after_the_backward():
    lin = Lineage()
    tape, s1 = _step(lin, lin.note_init(_state()))
    tape.closed = True
    with pytest.raises(TapeError, match="already been differentiated"):
        lin.resolve(s1)


def test_registry_keeps_nothing_alive():
    lin = Lineage()
    s0 = lin.note_init(_state())
    tape, s1 = _step(lin, s0)
    assert lin.tapes() == [tape]
    del tape
    gc.collect()
    assert lin.tapes() == []
    with pytest.raises(TapeError, match="neither by init_state"):
        lin.resolve(s1)                  # its loop is gone
    for _ in range(3 * Lineage.MAX_INITS):
        lin.note_init(_state())
    assert len(lin._inits) <= Lineage.MAX_INITS
    assert "no_grad" in steptape.ALTERNATIVE
