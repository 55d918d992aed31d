"""CPU-side checks of the verifier's C ABI (no GPU compute): every new entry point is declared in
include/stark_gpu.h and registered in starkgpu/_lib.py with the same number of arguments, the
kernel-shape constants the bindings export are the library's, and the verifier's view of a native
proof stream (sg_stream_verifier_callbacks: pull + fiat_shamir_verifier, proof_stream.rs:6-12)
returns the objects in order with the oracle's Fiat-Shamir bytes after every pull."""
import ctypes
import os
import re

import pytest

import stark_oracle as o
import starkgpu as sg
from starkgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["sg_poly_evaluate_points", "sg_zerofier_geometric_at", "sg_merkle_verify_batch",
               "sg_stream_verifier_callbacks", "sg_fri_verify", "sg_stark_verify", "sg_verify_kernel_shape"]


def _header():
    text = open(os.path.join(ROOT, "include", "stark_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _declared_arity(text, name):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, "%s is not declared in include/stark_gpu.h" % name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbol_declared_registered_and_exported(name):
    assert name in _lib.PROTOTYPES, name + " is not registered in starkgpu/_lib.py"
    assert len(_lib.PROTOTYPES[name][1]) == _declared_arity(_header(), name)
    assert hasattr(sg.lib(), name), "libstarkgpu.so does not export " + name


def test_verifier_stream_struct_and_option_documented():
    text = open(os.path.join(ROOT, "include", "stark_gpu.h")).read()
    assert re.search(r"\}\s*sg_verifier_stream\s*;", text)
    assert [f[0] for f in _lib.sg_verifier_stream._fields_] == ["user", "pull", "fiat_shamir_verifier"]
    assert '"verify_device"' in text
    # sg_proof_stream is unchanged: push + fiat_shamir_prover
    assert [f[0] for f in _lib.sg_proof_stream._fields_] == ["user", "push", "fiat_shamir_prover"]


def test_kernel_shape_constants_are_the_librarys():
    b, c = ctypes.c_size_t(), ctypes.c_size_t()
    sg.lib().sg_verify_kernel_shape(ctypes.byref(b), ctypes.byref(c))
    assert (b.value, c.value) == (sg.EVAL_BLOCK, sg.EVAL_CHUNK)
    assert c.value % b.value == 0 and c.value > b.value


OBJECTS = [(o.ROOT, bytes(range(64))), (o.ROOT, bytes(64)), (o.CODEWORD, [3, o.P - 1, 0, 5]),
           (o.LEAFS, (7, 8, o.P - 1)), (o.PATH, [bytes([1] * 64), bytes([2] * 64)]), (o.VALUE, 11),
           (o.PATH, [bytes([9] * 64)])]


def _pull(vs):
    code, p, n = ctypes.c_uint8(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    rc = vs.pull(vs.user, ctypes.byref(code), ctypes.byref(p), ctypes.byref(n))
    if rc != 0:
        return rc, None
    return 0, sg.decode_object(code.value, ctypes.string_at(p, n.value) if n.value else b"")


def _fs(vs, nbytes):
    buf = (ctypes.c_uint8 * nbytes)()
    assert vs.fiat_shamir_verifier(vs.user, nbytes, buf) == 0
    return bytes(buf)


@pytest.mark.parametrize("document", [None, b"Hello, World!"])
def test_native_stream_verifier_callbacks_match_oracle(document):
    if document is None:
        gs, os_ = sg.IndependentProofStream(), o.IndependentProofStream()
    else:
        gs, os_ = sg.SignatureProofStream(document), o.SignatureProofStream(document)
    for ob in OBJECTS:
        gs.push(ob)
        os_.push(ob)
    vs = gs.verifier_callbacks()
    assert _fs(vs, 32) == os_.fiat_shamir_verifier(32)  # nothing pulled yet
    for ob in OBJECTS:
        rc, got = _pull(vs)
        assert rc == 0 and got == ob == os_.pull()
        assert _fs(vs, 32) == os_.fiat_shamir_verifier(32)
        assert _fs(vs, 7) == os_.fiat_shamir_verifier(7)
    rc, _ = _pull(vs)
    assert rc == _lib.SG_ERR_INVALID  # "Cannot pull, queue is empty"


def test_callback_stream_pull_side_over_an_oracle_stream():
    """CallbackProofStream's pull side hands the oracle stream's objects to the library's callbacks."""
    os_ = o.IndependentProofStream(list(OBJECTS))
    mirror = o.IndependentProofStream(list(OBJECTS))
    ad = sg.CallbackProofStream(os_)
    vs = ad.verifier_callbacks()
    for ob in OBJECTS:
        rc, got = _pull(vs)
        assert rc == 0 and got == ob == mirror.pull()
        assert _fs(vs, 32) == mirror.fiat_shamir_verifier(32)
    rc, _ = _pull(vs)
    assert rc != 0 and ad.error is not None
