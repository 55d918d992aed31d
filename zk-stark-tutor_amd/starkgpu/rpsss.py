"""RPSSS, the Rescue-Prime STARK signature scheme (rpsss.rs), over libstarkgpu's sg_rpsss_* entry
points: one object that owns the hash, the Stark and the transition constraints (built once).

The reference draws from `thread_rng` in keygen and sign; here those draws are explicit arguments
(the 17 seed bytes, the trace randomizers and the randomizer polynomial's coefficients), as they
are for `Stark.prove`.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import sg_fe
from .api import (Context, IndependentProofStream, SignatureProofStream, _ctx, _fe, _int, _ptr, _u8, fe_array,
                  to_ints)

SEED_BYTES = 17  # rpsss.rs:62-66


class RPSSS:
    """rpsss.rs:16-79 RPSSS::{new, keygen, sign, verify} (needs a GPU context)."""

    def __init__(self, expansion_factor: int, num_colinearity_checks: int, security_level: int,
                 transition_constraints_degree: int, ctx: Optional[Context] = None):
        self.ctx = _ctx(ctx)
        h = ctypes.c_void_p()
        self.handle = None
        self.ctx.check(self.ctx._lib.sg_rpsss_create(self.ctx.handle, expansion_factor, num_colinearity_checks,
                                                     security_level, transition_constraints_degree,
                                                     ctypes.byref(h)))
        self.handle = h

    def params(self) -> Tuple[int, int]:
        """(trace randomizer elements, randomizer coefficients) one sign() takes."""
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        self.ctx.check(self.ctx._lib.sg_rpsss_params(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def keygen(self, seed: bytes) -> Tuple[int, int]:
        """rpsss.rs:61-68: (sk, pk) = (Field::sample(seed), hash(sk)) from thread_rng's 17 bytes."""
        if len(seed) != SEED_BYTES:
            raise ValueError("keygen takes 17 seed bytes")
        sk, pk = sg_fe(), sg_fe()
        self.ctx.check(self.ctx._lib.sg_rpsss_keygen(self.ctx.handle, self.handle, _u8(seed), ctypes.byref(sk),
                                                     ctypes.byref(pk)))
        return _int(sk), _int(pk)

    def keygen_batch(self, seeds: Sequence[bytes]) -> Tuple[List[int], List[int]]:
        """keygen() for every seed: sampled on the host, hashed as one batch (the device kernel from
        the context option "rescue_device_min" on)."""
        if any(len(s) != SEED_BYTES for s in seeds):
            raise ValueError("keygen takes 17 seed bytes")
        n = len(seeds)
        sk = np.empty((max(n, 1), 2), dtype=np.uint64)
        pk = np.empty((max(n, 1), 2), dtype=np.uint64)
        self.ctx.check(self.ctx._lib.sg_rpsss_keygen_batch(self.ctx.handle, self.handle, _u8(b"".join(seeds)), n,
                                                           _ptr(sk), _ptr(pk)))
        return to_ints(sk[:n]), to_ints(pk[:n])

    def sign_stream(self, sk: int, document: bytes, trace_randomizers, randomizer_coefficients):
        """sign(), returning the SignatureProofStream that holds the signature's objects."""
        tr = fe_array(trace_randomizers) if isinstance(trace_randomizers, np.ndarray) \
            else fe_array([v for row in trace_randomizers for v in row])
        rc = fe_array(randomizer_coefficients)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx._lib.sg_rpsss_sign(self.ctx.handle, self.handle, _fe(sk), _u8(document),
                                                   len(document), _ptr(tr), _ptr(rc), len(rc), ctypes.byref(h)))
        s = SignatureProofStream.__new__(SignatureProofStream)  # adopt the library's stream
        IndependentProofStream.__init__(s, h.value)
        return s

    def sign(self, sk: int, document: bytes, trace_randomizers, randomizer_coefficients) -> bytes:
        """rpsss.rs:70-73: the signature bytes.  trace_randomizers: num_randomizers rows of m values
        (or an (n, 2) array), randomizer_coefficients: params()[1] values."""
        return self.sign_stream(sk, document, trace_randomizers, randomizer_coefficients).digest()

    def verify(self, pk: int, document: bytes, signature: bytes) -> Tuple[bool, str]:
        """rpsss.rs:75-79: (ok, error text of the reference's Err); a signature that does not
        deserialize raises StarkGpuError."""
        rc = self.ctx._lib.sg_rpsss_verify(self.ctx.handle, self.handle, _fe(pk), _u8(document), len(document),
                                           _u8(signature), len(signature))
        if rc < 0:
            self.ctx.check(rc)
        if rc == 1:
            return True, ""
        return False, self.ctx._lib.sg_last_error(self.ctx.handle).decode(errors="replace")

    def free(self) -> None:
        if self.handle:
            self.ctx._lib.sg_rpsss_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
