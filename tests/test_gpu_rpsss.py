"""The RPSSS object (rpsss.rs; sg_rpsss_*) at the reference's published configuration
RPSSS::new(field, 4, 64, 128, 3) (rpsss.rs:103) against the committed known answers
(tests/golden/rpsss_published.json) and the oracle's field / hash functions."""
import hashlib
import json
import os

import pytest

import rescue_batch_case as B
import rpsss_case as R
import stark_oracle as o
import stark_prove_oracle as e
import starkgpu as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "rpsss_published.json")) as _f:
    G = json.load(_f)
SEED = G["seed"].encode()
SK, PK = int(G["sk"]), int(G["pk"])
DOCUMENT, FORGED = G["document"].encode(), G["forged_document"].encode()


@pytest.fixture(scope="module")
def ctx():
    c = sg.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def rpsss(ctx):
    return sg.RPSSS(R.EXPANSION, R.CHECKS, R.SECURITY, R.TCD, ctx=ctx)


@pytest.fixture(scope="module")
def randomizers(rpsss):
    n_tr, n_rc = rpsss.params()
    r = e.randomness_from_seed(SEED, n_tr + n_rc)
    return [r[2 * i:2 * i + 2] for i in range(n_tr // 2)], r[n_tr:]


@pytest.fixture(scope="module")
def signature(rpsss, randomizers):
    return rpsss.sign(SK, DOCUMENT, *randomizers)


def test_keygen_returns_the_golden_key_pair(rpsss):
    assert rpsss.keygen(o.shake256(b"rpsss-keygen" + SEED, 17)) == (SK, PK)


def test_params_count_the_draws_of_one_sign(rpsss):
    # stark.rs:285-301: 4 c = 256 randomizer rows of m = 2; stark.rs:425-433: max_degree + 1
    n_tr, n_rc = rpsss.params()
    assert n_tr == 4 * R.CHECKS * 2
    st = e.Stark(R.EXPANSION, R.CHECKS, R.SECURITY, 2, 28, R.TCD)
    air = B.oracle(R.RESCUE).transition_constraints(st.omicron, st.omicron_domain_length)
    assert n_rc == st.num_randomizer_coefficients(air), "stark.rs:171-186 max_degree + 1"


def test_sign_gives_the_published_signature_and_rebuilds_nothing(ctx, rpsss, randomizers, signature):
    assert len(signature) == G["proof_len"] == R.PROOF_LEN, "rpsss.rs:89"
    assert hashlib.sha256(signature).hexdigest() == G["proof_sha256"]
    before = ctx.cached_tables()
    assert rpsss.sign(SK, DOCUMENT, *randomizers) == signature
    assert ctx.cached_tables() == before, "a sign after the first adds no table to the context"


def test_verify_accepts_rejects_and_survives_bad_signatures(ctx, rpsss, signature):
    good = lambda: rpsss.verify(PK, DOCUMENT, signature)  # noqa: E731
    assert good() == (True, "")
    assert rpsss.verify(PK, FORGED, signature) == (False, G["forged_error"]), "rpsss.rs:127-131"
    assert good() == (True, "")
    ok, err = rpsss.verify(PK + 1, DOCUMENT, signature)
    assert not ok and err
    assert good() == (True, "")
    # cut to half its length: it does not deserialize (stark.rs:30-67)
    L = ctx._lib
    sig_half = signature[:len(signature) // 2]
    from starkgpu.api import _fe, _u8
    rc = L.sg_rpsss_verify(ctx.handle, rpsss.handle, _fe(PK), _u8(DOCUMENT), len(DOCUMENT), _u8(sig_half),
                           len(sig_half))
    assert rc == sg._lib.SG_ERR_INVALID
    assert L.sg_rpsss_verify(ctx.handle, rpsss.handle, _fe(PK), _u8(DOCUMENT), len(DOCUMENT), _u8(b""), 0) \
        == sg._lib.SG_ERR_INVALID, "a zero-length signature"
    assert good() == (True, "")
    # one flipped byte in the middle: rejected or an error, never accepted
    mid = len(signature) // 2
    bad = signature[:mid] + bytes([signature[mid] ^ 0x01]) + signature[mid + 1:]
    rc = L.sg_rpsss_verify(ctx.handle, rpsss.handle, _fe(PK), _u8(DOCUMENT), len(DOCUMENT), _u8(bad), len(bad))
    assert rc <= 0
    assert good() == (True, "")
    before = ctx.cached_tables()
    assert good() == (True, "")
    assert ctx.cached_tables() == before, "a verify after the first adds no table to the context"


def test_keygen_batch_equals_oracle_and_single_calls():
    c = sg.Context()
    c.set_option("rescue_device_min", 0)
    rp = sg.RPSSS(R.EXPANSION, R.CHECKS, R.SECURITY, R.TCD, ctx=c)
    seeds = [o.shake256(b"rpsss-keygen-batch" + bytes([i]), 17) for i in range(65)]
    c.profile(True)
    sk, pk = rp.keygen_batch(seeds)
    assert c.profile_report()["rescue_hash_batch"]["launches"] == 1, "the batch ran the kernel"
    c.profile(False)
    assert sk == [o.sample(s) for s in seeds]
    oracle = B.oracle(R.RESCUE)
    assert pk == [oracle.hash(x) for x in sk]
    assert (sk, pk) == tuple(map(list, zip(*[rp.keygen(s) for s in seeds])))
    rp.free()
    c.close()


def test_signature_stream_feeds_the_existing_verifier(ctx, rpsss, randomizers, signature):
    """sign's SignatureProofStream through its verifier callbacks into sg_stark_verify, with a
    RescuePrime, Stark and constraints built by the existing entry points."""
    stream = rpsss.sign_stream(SK, DOCUMENT, *randomizers)
    assert isinstance(stream, sg.SignatureProofStream) and stream.digest() == signature
    rp = sg.RescuePrime(*R.RESCUE, ctx=ctx)
    st = sg.Stark(R.EXPANSION, R.CHECKS, R.SECURITY, rp.m, rp.N + 1, R.TCD, ctx=ctx)
    air = rp.transition_constraints(st.omicron, st.omicron_domain_length)
    assert st.verify(air, rp.boundary_constraints(PK), stream) == (True, "")
