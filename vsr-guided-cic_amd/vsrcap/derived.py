"""The state one handle derives from the borrowed weights, and the one order in which it is brought up to date:

  bound pointers -> flavour (bf16 copies | x3 switch | fp16-pair images) -> decode cache -> prepared statics

A product is void when anything to its left moved.  Derived mirrors what the library holds (include/vsrcap.h: a flavour transition
voids the decode cache, the saved forwards and the prepared statics; a refresh while on voids the cache and the statics) and sync()
issues the calls that bring a handle to a target in the chain's order - the decode cache last, in the final flavour.  The calls go
through a backend (vsrcap/engine.py: buffers, ctypes, device and stream) with one method per library call: bind(ptrs),
refresh_bf16(on), set_gemm_mode(x3), refresh_h2(on), build_cache(), drop_cache().
One event comes from outside the chain: stepped(), after the optimizer of vsrcap/optim.py has rewritten the weights AND their flavour
product in one library call - the product is current, everything to its right is void.
No torch, no ctypes: tests/test_derived_logic.py enumerates event sequences against a fake handle."""

# compute dtype -> (bf16 copies, x3 switch, fp16-pair images); f16x2 needs sizes that are multiples of 8 and is plain f32x3 otherwise
FLAVOURS = {'f32': (False, False, False), 'f32x3': (False, True, False), 'f16x2': (False, True, True), 'bf16': (True, False, False)}


class Derived:
    def __init__(self):
        self.ptrs = None                     # the 28 bound pointers
        self.x3 = True                       # the library's default
        self.bf16_on = self.h2_on = False    # what the library was last told
        self.bf16 = self.h2 = None           # (ptrs, weights_version) the copies / images were built from; None: not built
        self.cache = None                    # ... and the decode cache; not None <=> the handle holds a cache pointer
        self.statics_void = True

    def _drop_cache(self, backend):          # forgetting the key and dropping the library's pointer are one operation
        if self.cache is not None:
            backend.drop_cache()
            self.cache = None

    def _library_voided(self):               # every call above the cache makes the library drop its cache pointer and its statics
        self.cache = None
        self.statics_void = True

    def invalidate(self, backend):
        """the weights were rewritten behind every counter: everything downstream of the pointers is not built"""
        self.bf16 = self.h2 = None
        self._drop_cache(backend)
        self.statics_void = True

    def stepped(self, ptrs, version):
        """the library's own optimizer step (vsr_adam_step) wrote the bound weights and, in the same call, rebuilt the flavour product
        that is on from them: that product is of (ptrs, version) - the weights as they are now - and, as after any refresh, the
        library dropped its cache pointer and the statics are void.  The caller vouches for ptrs == self.ptrs (the call fails otherwise)."""
        key = (ptrs, version)
        if self.bf16_on:
            self.bf16 = key
        if self.h2_on:
            self.h2 = key
        self._library_voided()

    def sync(self, target, backend):
        """target: (bound_ptrs, weights_version, compute_dtype, dims_multiple_of_8, training).  Returns whether the prepared statics are
        void (the library dropped them, or invalidate() was called, since the last sync)."""
        ptrs, version, dtype, dims8, training = target
        want_bf16, want_x3, want_h2 = FLAVOURS[dtype]
        want_h2 = want_h2 and dims8
        key = (ptrs, version)
        if ptrs != self.ptrs:
            backend.bind(ptrs)               # (the library also switches bf16 / f16x2 off: the keys below no longer match)
            self.ptrs = ptrs
            self._library_voided()
        if self.bf16_on != want_bf16 or (want_bf16 and self.bf16 != key):
            backend.refresh_bf16(want_bf16)
            self.bf16_on, self.bf16 = want_bf16, key if want_bf16 else None
            self._library_voided()
        if self.x3 != want_x3:
            backend.set_gemm_mode(want_x3)
            self.x3 = want_x3
            self._library_voided()
        if self.h2_on != want_h2 or (want_h2 and self.h2 != key):
            backend.refresh_h2(want_h2)
            self.h2_on, self.h2 = want_h2, key if want_h2 else None
            self._library_voided()
        if training:                         # the weights move every step: no weight-only cache
            self._drop_cache(backend)
        elif self.cache != key:
            backend.build_cache()
            self.cache = key
        void, self.statics_void = self.statics_void, False
        return void
