"""Inputs and oracle values shared by the batched Rescue-Prime tests (test_abi_rpsss.py,
test_gpu_rescue_batch.py).  TEST INFRASTRUCTURE: expected values come from the oracle
(`stark_prove_oracle.RescuePrime`) and the reference's known answers only, computed once per shape."""
import functools
import json
import os

import stark_oracle as o
import stark_prove_oracle as e

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = o.P

with open(os.path.join(ROOT, "tests", "golden", "reference_kats_e2e.json")) as _f:
    KATS = json.load(_f)
KAT_HASH_IN, KAT_HASH_OUT = int(KATS["rescue_hash"]["input"]), int(KATS["rescue_hash"]["output"])
KAT_TRACE_IN = int(KATS["rescue_trace"]["input"])
KAT_TRACE_FIRST, KAT_TRACE_LAST = int(KATS["rescue_trace"]["first_rate"]), int(KATS["rescue_trace"]["last_rate"])
KAT_SHAPE = (2, 1, 128, 27)  # rescue_prime.rs:323-342: the shape both known answers are for

# carry and reduction edges of the 128-bit arithmetic, then the reference's two test inputs
EDGES = [0, 1, P - 1, P - 2, (1 << 64) - 1, 1 << 64, 1 << 127, KAT_HASH_IN, KAT_TRACE_IN]
KAT_HASH_AT, KAT_TRACE_AT = EDGES.index(KAT_HASH_IN), EDGES.index(KAT_TRACE_IN)


def inputs(n: int, tag: bytes = b"rescue-batch"):
    """The first n of: the edge values, then seeded elements (a batch of n is a prefix of a longer one)."""
    return (EDGES + o.synthetic_elements(7, tag, max(n - len(EDGES), 0)))[:n]


@functools.lru_cache(maxsize=None)
def oracle(shape):
    return e.RescuePrime(*shape)


@functools.lru_cache(maxsize=None)
def oracle_hashes(shape, n: int):
    rp = oracle(shape)
    return [rp.hash(x) for x in inputs(n)]


@functools.lru_cache(maxsize=None)
def oracle_traces(shape, n: int):
    rp = oracle(shape)
    return [rp.trace(x) for x in inputs(n)]
