"""The beam selection inside the LSTM1 kernel with TWO hidden units per lane (csrc/kernels.h: k_select_lstm1_x2, slices of 128 units per
workgroup, 8-byte loads and stores) against the same decode with VSR_FUSE_SELECT=0, which takes k_select_beam + k_lstm1 (one unit per
thread, 4-byte accesses).  Same expressions in the same order: words, gates and both log-prob tensors must agree BIT FOR BIT.
H = 64: half a slice; H = 72: a slice that is neither full nor a multiple of the wave; H = 136: one full slice plus a partial one.
That kernel needs 8-byte aligned bases.  vsr_create admits only rnn_size % 4 == 0 and the workspace is carved at 256 bytes: the one
pointer that can miss is a decode cache a C-ABI caller built at an address that is only 4-byte aligned.  vsr_beam then does not fuse
the selection (there is no one-unit-per-lane fused kernel any more); the second test builds such a cache and decodes over it.
Reference ops: models/CaptioningModel.py:136-180 (selection), controllable_captioning.py:151-154 (LSTM1 + gates)."""
import ctypes as C
import os

import pytest
import torch

import helpers
from vsrcap import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAVOURS = ("f16x2", "f32x3", "f32")


def _model(cfg, w, flavour, fuse):
    old = os.environ.get("VSR_FUSE_SELECT")
    os.environ["VSR_FUSE_SELECT"] = fuse
    try:
        m = helpers.build_model(cfg, w, DEV).set_compute_dtype(flavour)
        m._engine(torch.device(DEV))          # the handle reads VSR_FUSE_SELECT when it is created
    finally:
        if old is None:
            os.environ.pop("VSR_FUSE_SELECT", None)
        else:
            os.environ["VSR_FUSE_SELECT"] = old
    return m


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("H", [64, 72, 136])
@pytest.mark.parametrize("beam", [2, 5])
def test_two_units_per_lane_equals_the_separate_launches(beam, H, flavour):
    cfg = dict(V=50, B=3, R0=7, R=5, D=64, L=4, T=4, E=64, H=H, A=32)
    w = helpers.weights_for(cfg)
    det, ctrl = (x.to(DEV) for x in helpers.decode_inputs(cfg, 77))
    outs = []
    for fuse in ("3", "0"):
        m = _model(cfg, w, flavour, fuse)
        with torch.no_grad():
            (words, gates), (lp_w, lp_g) = m.beam_search((det, ctrl), [3, -1], beam, beam)
        outs.append((words.cpu(), gates.cpu(), lp_w.cpu(), lp_g.cpu()))
    assert outs[0][0].shape == (3, beam, 4)
    for name, a, b in zip(("words", "gates", "word log-probs", "gate log-probs"), *outs):
        assert torch.equal(a, b), "%s differ between the fused and the separate selection: %d of %d entries" % (name, int((a != b).sum()), a.numel())


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("beam", [2, 5])
def test_decode_cache_at_a_4_byte_aligned_address_decodes_the_same(beam, flavour):
    cfg = dict(V=50, B=3, R0=7, R=5, D=64, L=4, T=4, E=64, H=72, A=32)
    w = helpers.weights_for(cfg)
    det, ctrl = (x.to(DEV) for x in helpers.decode_inputs(cfg, 77))
    m = _model(cfg, w, flavour, "3")

    def decode():
        with torch.no_grad():
            (words, gates), (lp_w, lp_g) = m.beam_search((det, ctrl), [3, -1], beam, beam)
        return words.cpu(), gates.cpu(), lp_w.cpu(), lp_g.cpu()

    first = decode()                                      # over the engine's own cache (512-byte aligned): the fused kernel
    eng = m._engine(torch.device(DEV))
    n = eng.lib.vsr_decode_cache_floats(eng.h)
    buf = torch.empty(n + 1, dtype=torch.float32, device=DEV)       # (stays alive over the second decode)
    assert buf.data_ptr() % 8 == 0
    _lib.check(eng.lib.vsr_build_decode_cache(eng.h, C.c_void_p(buf.data_ptr() + 4), n, eng._stream(buf.device)))
    # the cache itself (V, 6H) came out the same through the GEMMs' element-by-element stores ...
    own, nc = eng._wbuf["cache"], cfg["V"] * 6 * cfg["H"]
    assert torch.equal(buf[1:1 + nc], own[:nc]), "the cache built at the 4-byte aligned address differs from the aligned one"
    # ... and the second decode reads THAT one: the engine's own buffer is poisoned, and must still be poison afterwards (the weights
    # have not moved, so the engine rebuilds nothing; a rebuild would write it, a decode that read it would return NaN log-probs)
    own.fill_(float("nan"))
    second = decode()
    assert bool(torch.isnan(own).all()), "the engine rebuilt its own decode cache: the second decode did not run over the caller's"
    assert first[0].shape == (3, beam, 4)
    for name, a, b in zip(("words", "gates", "word log-probs", "gate log-probs"), first, second):
        assert torch.equal(a, b), "%s differ over the 4-byte aligned decode cache: %d of %d entries" % (name, int((a != b).sum()), a.numel())
    del buf
