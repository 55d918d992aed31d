"""Batched Rescue-Prime on the GPU (csrc/rescue_kernels.hip: one lane per input) against the
oracle: every kernel instantiation (m = 2, 3, 4), batch sizes around the 64-lane block, the
fallbacks, the error paths, and a trace block handed straight to sg_stark_prove_dev.  Every test
that sets a context option does so on its own context."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import rescue_batch_case as B
import stark_oracle as o
import stark_prove_oracle as e
import starkgpu as sg
from starkgpu import _lib
from starkgpu.api import _ptr, fe_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 128, 27), (3, 1, 2, 9), (4, 1, 2, 3), (2, 1, 2, 1)]
# a single lane, a partial wave, a full wave, a wave plus one, several blocks with a ragged tail
SIZES = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def dctx():
    """A context of this module's own on which every batch runs the kernel."""
    c = sg.Context()
    c.set_option("rescue_device_min", 0)
    yield c
    c.close()


def _dev(values):
    return torch.from_numpy(fe_array(values).view(np.int64).reshape(-1).copy()).to("cuda:0")


def _empty(count):
    return torch.full((2 * max(count, 1),), -1, dtype=torch.int64, device="cuda:0")


def _ints(t, count):
    return sg.to_ints(t.cpu().numpy().view(np.uint64).reshape(-1, 2)[:count])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hash_batch_equals_oracle(dctx, shape):
    rp = sg.RescuePrime(*shape, ctx=dctx)
    want = B.oracle_hashes(shape, max(SIZES))
    for n in SIZES:
        assert rp.hash_batch(B.inputs(n)) == want[:n], n
    if shape == B.KAT_SHAPE:
        assert rp.hash_batch(B.inputs(max(SIZES)))[B.KAT_HASH_AT] == B.KAT_HASH_OUT, "rescue_prime.rs:323-331"
    # the device-pointer form, with a guard element behind the output
    n = 65
    d_in, d_out = _dev(B.inputs(n)), _empty(n + 1)
    rp.hash_batch_dev(d_in.data_ptr(), n, d_out.data_ptr())
    assert _ints(d_out, n) == want[:n]
    assert d_out[2 * n:].tolist() == [-1, -1], "wrote past the n outputs"


@pytest.mark.parametrize("shape", [(2, 1, 128, 27), (3, 1, 2, 9)], ids=str)
def test_trace_batch_equals_oracle(dctx, shape):
    rp = sg.RescuePrime(*shape, ctx=dctx)
    n = 65
    got, want = rp.trace_batch(B.inputs(n)), B.oracle_traces(shape, n)
    for i in range(n):
        assert got[i] == want[i], f"trace of input {i}"
    if shape == B.KAT_SHAPE:
        t = got[B.KAT_TRACE_AT]
        assert t[0][0] == B.KAT_TRACE_FIRST and t[-1][0] == B.KAT_TRACE_LAST, "rescue_prime.rs:333-342"
    per = (rp.N + 1) * rp.m
    d_in, d_out = _dev(B.inputs(n)), _empty(n * per + 1)
    rp.trace_batch_dev(d_in.data_ptr(), n, d_out.data_ptr())
    assert _ints(d_out, n * per) == [v for t in want for row in t for v in row]
    assert d_out[2 * n * per:].tolist() == [-1, -1], "wrote past the n traces"


def test_m5_host_forms_fall_back_and_dev_forms_refuse(dctx):
    shape = (5, 1, 2, 2)
    rp = sg.RescuePrime(*shape, ctx=dctx)
    assert rp.hash_batch(B.inputs(9)) == B.oracle_hashes(shape, 9)
    assert rp.trace_batch(B.inputs(9)) == B.oracle_traces(shape, 9)
    d_in, d_out = _dev(B.inputs(9)), _empty(9 * 15)
    for call in (rp.hash_batch_dev, rp.trace_batch_dev):
        with pytest.raises(sg.StarkGpuError, match="m = 2, 3, 4") as ei:
            call(d_in.data_ptr(), 9, d_out.data_ptr())
        assert ei.value.code == _lib.SG_ERR_INVALID


def test_noncanonical_input_names_its_index_and_writes_nothing(dctx):
    rp = sg.RescuePrime(2, 1, 2, 3, ctx=dctx)
    xs = fe_array(B.inputs(3) + [B.P] + B.inputs(4))
    for fn, per in ((dctx._lib.sg_rescue_hash_batch, 1), (dctx._lib.sg_rescue_trace_batch, 8)):
        out = np.full((len(xs) * per, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        assert fn(dctx.handle, rp.handle, _ptr(xs), len(xs), _ptr(out)) == _lib.SG_ERR_NONCANONICAL
        assert b"input 3" in dctx._lib.sg_last_error(dctx.handle)
        assert (out == 0xA5A5A5A5A5A5A5A5).all(), "a rejected batch writes nothing"


def test_host_and_device_paths_return_the_same_values():
    shape, n = (2, 1, 128, 27), 65
    outs = []
    for minimum in (2 ** 62, 0):
        c = sg.Context()
        c.set_option("rescue_device_min", minimum)
        rp = sg.RescuePrime(*shape, ctx=c)
        c.profile(True)
        outs.append((rp.hash_batch(B.inputs(n)), rp.trace_batch(B.inputs(n))))
        launched = sum(v["launches"] for k, v in c.profile_report().items() if k.startswith("rescue_"))
        assert launched == (0 if minimum else 2), "the option decides which path runs"
        c.profile(False)
        c.close()
    assert outs[0] == outs[1]
    assert outs[0][0] == B.oracle_hashes(shape, n)


def test_empty_batch_is_ok(dctx):
    rp = sg.RescuePrime(2, 1, 2, 3, ctx=dctx)
    assert rp.hash_batch([]) == [] and rp.trace_batch([]) == []
    rp.hash_batch_dev(0, 0, 0)
    rp.trace_batch_dev(0, 0, 0)


def test_dev_forms_honour_async():
    c = sg.Context()
    shape, n = (2, 1, 128, 27), 257
    rp = sg.RescuePrime(*shape, ctx=c)
    d_in, d_out = _dev(B.inputs(n)), _empty(n)
    c.set_async(True)
    rp.hash_batch_dev(d_in.data_ptr(), n, d_out.data_ptr())
    c.synchronize()
    c.set_async(False)
    assert _ints(d_out, n) == B.oracle_hashes(shape, n)
    c.close()


def test_trace_block_feeds_stark_prove_dev(dctx):
    """trace_batch_dev on [sk, sk + 1]; block 0's device pointer is sg_stark_prove_dev's d_trace at
    the published RPSSS configuration: the signature has the committed length and SHA-256."""
    import rpsss_case as R
    with open(os.path.join(ROOT, "tests", "golden", "rpsss_published.json")) as f:
        g = json.load(f)
    sk, pk = int(g["sk"]), int(g["pk"])
    rp = sg.RescuePrime(*R.RESCUE, ctx=dctx)
    st = sg.Stark(R.EXPANSION, R.CHECKS, R.SECURITY, rp.m, rp.N + 1, R.TCD, ctx=dctx)
    air = rp.transition_constraints(st.omicron, st.omicron_domain_length)
    per = (rp.N + 1) * rp.m
    d_in, d_tr = _dev([sk, sk + 1]), _empty(2 * per)
    rp.trace_batch_dev(d_in.data_ptr(), 2, d_tr.data_ptr())
    assert _ints(d_tr, 2 * per)[(rp.N) * rp.m] == pk, "block 0 ends in hash(sk)"
    nrc = st.num_randomizer_coefficients(air)
    r = e.randomness_from_seed(g["seed"].encode(), rp.m * st.num_randomizers + nrc)
    d_r, d_c = _dev(r[:rp.m * st.num_randomizers]), _dev(r[rp.m * st.num_randomizers:])
    ps = sg.SignatureProofStream(g["document"].encode())
    st.prove_dev(d_tr.data_ptr(), rp.N + 1, air, rp.boundary_constraints(pk), ps, d_r.data_ptr(), d_c.data_ptr(), nrc)
    sig = ps.digest()
    assert len(sig) == g["proof_len"] == R.PROOF_LEN
    assert hashlib.sha256(sig).hexdigest() == g["proof_sha256"]
