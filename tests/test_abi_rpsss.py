"""CPU-side checks of the batched Rescue-Prime entry points and the RPSSS object (no GPU): on a
host context the batch forms run the host loop, which shares its rounds and its alpha_inv addition
chain (csrc/rescue_pow.hpp) with the device kernel; the device forms and the RPSSS object ask for a
GPU context; null arguments are rejected."""
import ctypes

import numpy as np
import pytest

import rescue_batch_case as B
import starkgpu as sg
from starkgpu import _lib
from starkgpu.api import _ptr, fe_array

SHAPES = [(2, 1, 128, 27), (3, 1, 2, 7)]
N_INPUTS = 12  # the nine edge inputs and three seeded ones


@pytest.fixture(scope="module")
def host():
    return sg.HostContext()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_host_hash_batch_equals_oracle(host, shape):
    rp = sg.RescuePrime(*shape, ctx=host)
    got = rp.hash_batch(B.inputs(N_INPUTS))
    assert got == B.oracle_hashes(shape, N_INPUTS)
    if shape == B.KAT_SHAPE:
        assert got[B.KAT_HASH_AT] == B.KAT_HASH_OUT, "rescue_prime.rs:323-331"
    # the single-input entry point (square-and-multiply) agrees with the batch loop (addition chain)
    assert got[:4] == [rp.hash(x) for x in B.inputs(4)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_host_trace_batch_equals_oracle(host, shape):
    rp = sg.RescuePrime(*shape, ctx=host)
    got = rp.trace_batch(B.inputs(N_INPUTS))
    assert got == B.oracle_traces(shape, N_INPUTS)
    if shape == B.KAT_SHAPE:
        t = got[B.KAT_TRACE_AT]
        assert t[0][0] == B.KAT_TRACE_FIRST and t[-1][0] == B.KAT_TRACE_LAST, "rescue_prime.rs:333-342"


def test_host_batch_m1_and_m5_take_the_generic_loop(host):
    for shape in [(1, 1, 2, 3), (5, 1, 2, 2)]:
        rp = sg.RescuePrime(*shape, ctx=host)
        assert rp.hash_batch(B.inputs(9)) == B.oracle_hashes(shape, 9)
        assert rp.trace_batch(B.inputs(9)) == B.oracle_traces(shape, 9)


def test_host_batch_empty_and_noncanonical(host):
    rp = sg.RescuePrime(2, 1, 2, 3, ctx=host)
    assert rp.hash_batch([]) == [] and rp.trace_batch([]) == []
    xs = fe_array([5, 6, 7, B.P, 8, B.P + 1])
    out = np.full((6, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = host._lib.sg_rescue_hash_batch(None, rp.handle, _ptr(xs), 6, _ptr(out))
    assert rc == _lib.SG_ERR_NONCANONICAL
    assert b"input 3" in host._lib.sg_last_error(None)
    assert (out == 0xA5A5A5A5A5A5A5A5).all(), "a rejected batch writes nothing"


def test_capacity_other_than_one_is_rejected_like_hash(host):
    rp = sg.RescuePrime(3, 2, 2, 3, ctx=host)
    with pytest.raises(sg.StarkGpuError, match="Received wrong number of input elements") as ei:
        rp.hash_batch([1, 2])
    assert ei.value.code == _lib.SG_ERR_INVALID


def test_device_forms_and_rpsss_need_a_gpu_context(host):
    rp = sg.RescuePrime(2, 1, 2, 3, ctx=host)
    for call in (lambda: rp.hash_batch_dev(0, 1, 0), lambda: rp.trace_batch_dev(0, 1, 0),
                 lambda: sg.RPSSS(4, 64, 128, 3, ctx=host)):
        with pytest.raises(sg.StarkGpuError, match="a GPU context is required") as ei:
            call()
        assert ei.value.code == _lib.SG_ERR_INVALID


def test_null_arguments_are_invalid(host):
    L = host._lib
    rp = sg.RescuePrime(2, 1, 2, 3, ctx=host)
    xs, out = fe_array([1, 2]), np.zeros((8, 2), dtype=np.uint64)
    assert L.sg_rescue_hash_batch(None, None, _ptr(xs), 2, _ptr(out)) == _lib.SG_ERR_INVALID
    assert L.sg_rescue_hash_batch(None, rp.handle, None, 2, _ptr(out)) == _lib.SG_ERR_INVALID
    assert L.sg_rescue_trace_batch(None, rp.handle, _ptr(xs), 2, None) == _lib.SG_ERR_INVALID
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.sg_rpsss_params(None, ctypes.byref(a), ctypes.byref(b)) == _lib.SG_ERR_INVALID
    sk, pk = _lib.sg_fe(), _lib.sg_fe()
    seed = (ctypes.c_uint8 * 17)()
    assert L.sg_rpsss_keygen(None, None, seed, ctypes.byref(sk), ctypes.byref(pk)) == _lib.SG_ERR_INVALID
    assert L.sg_rpsss_keygen_batch(None, None, seed, 1, ctypes.byref(sk), ctypes.byref(pk)) == _lib.SG_ERR_INVALID
    h = ctypes.c_void_p()
    assert L.sg_rpsss_create(None, 4, 64, 128, 3, None) == _lib.SG_ERR_INVALID
    assert L.sg_rpsss_sign(None, None, sk, None, 0, None, None, 0, ctypes.byref(h)) == _lib.SG_ERR_INVALID
    assert L.sg_rpsss_verify(None, None, pk, None, 0, None, 0) == _lib.SG_ERR_INVALID
    L.sg_rpsss_free(None)
