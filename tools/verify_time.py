#!/usr/bin/env python3
"""Time Stark::verify (stark.rs:565-770) on the GPU against the same orchestration with plain host
loops (context option verify_device = 0), beside the prove of the same statement.

One JSON line per size: a Rescue-Prime trace of 2^log_rows - 1 randomized rows, expansion 8,
c = 64, security 128, transition degree 3 (C4: log_rows = 16; the headline statement: 20), set up
as tests/test_gpu_fullsize.py's _prove_gpu_and_checker.  Verify times are host wall clock around
the call with a context synchronize inside, median of `--reps` after `--warmup` calls; the host
loop is O(coefficients x points) on one core, so its repetitions are set apart (--host-reps,
--host-warmup; 0 skips it).  The verdicts must be 1 for the proof and 0 for a false claim.

usage: verify_time.py [--log-rows 16 20] [--reps 5] [--warmup 2] [--host-reps 5] [--host-warmup 2]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zk-stark-tutor_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import starkgpu as sg  # noqa: E402

P = sg.FIELD_PRIME


def synthetic(tag: bytes, n: int) -> np.ndarray:
    """n field elements from SHAKE256(b"sg-bench" || 0 || tag): 16-byte BE chunks mod p, as limbs."""
    raw = hashlib.shake_256(b"sg-bench" + (0).to_bytes(8, "big") + tag).digest(16 * n)
    be = np.frombuffer(raw, dtype=">u8").reshape(n, 2)
    hi, lo = be[:, 0].astype(np.uint64), be[:, 1].astype(np.uint64)
    p_hi, p_lo = np.uint64(P >> 64), np.uint64(P & (2**64 - 1))
    ge = (hi > p_hi) | ((hi == p_hi) & (lo >= p_lo))  # p > 2^127: one subtraction reduces
    borrow = (lo < p_lo) & ge
    lo = np.where(ge, lo - p_lo, lo)
    hi = np.where(ge, hi - p_hi - borrow.astype(np.uint64), hi)
    return np.ascontiguousarray(np.stack([lo, hi], axis=1))


def timed(ctx, fn, warmup, reps, setup=lambda: None):
    """median of `reps` timed fn(setup()) calls after `warmup` untimed ones; setup is not timed"""
    out = None
    for _ in range(warmup):
        out = fn(setup())
    ts = []
    for _ in range(reps):
        arg = setup()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn(arg)
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, (statistics.median(ts) if ts else None), ts


def run(log_rows, args):
    ctx = sg.Context(0)
    N = (1 << log_rows) - 2 - 256
    rp = sg.RescuePrime(2, 1, 128, N, ctx=ctx)
    st = sg.Stark(8, 64, 128, 2, N + 1, 3, ctx=ctx)
    air = rp.transition_constraints(st.omicron, st.omicron_domain_length)
    tag = b"verify-time-%d" % log_rows
    trace = rp.trace_array(sg.sample(tag))
    out = sg.to_ints(trace[-2:-1])[0]
    bnd = rp.boundary_constraints(out)
    false_bnd = rp.boundary_constraints((out + 1) % P)
    tr = synthetic(tag + b"trace-rand", 2 * st.num_randomizers)
    rc = synthetic(tag + b"rand-poly", st.num_randomizer_coefficients(air))

    def prove(_):
        ps = sg.IndependentProofStream()
        st.prove(trace, air, bnd, ps, tr, rc)
        return ps

    ps, prove_ms, _ = timed(ctx, prove, 1, 3)
    proof = ps.digest()

    def stream():  # a verify consumes its stream: a fresh one per call, parsed outside the timing
        return sg.IndependentProofStream.deserialize(proof)

    def verify(b, s=None):
        return st.verify(air, b, s if s is not None else stream())

    res = {"tool": "verify_time", "log_rows": log_rows, "fri_domain_log": log_rows + 5, "c": 64,
           "proof_bytes": len(proof), "prove_ms": round(prove_ms, 3)}
    ctx.set_option("verify_device", 1)
    (ok, err), dev_ms, dev_all = timed(ctx, lambda s: verify(bnd, s), args.warmup, args.reps, stream)
    assert ok, "verify_device=1 rejected the proof: " + err
    ok_false, err_false = verify(false_bnd)
    assert not ok_false, "verify_device=1 accepted a false claim"
    res.update(verdict=int(ok), verdict_false_claim=int(ok_false), false_claim_error=err_false,
               verify_device_ms=round(dev_ms, 3), verify_device_all_ms=[round(t, 3) for t in dev_all])
    # per-kernel times of one more device verify (HIP events; a run of its own)
    ctx.profile(True)
    verify(bnd)
    ctx.synchronize()
    rep = ctx.profile_report()
    ctx.profile(False)
    names = ("point_powers", "eval_points", "eval_points_finish", "geo_zerofier_at", "geo_zerofier_finish",
             "merkle_verify_batch")
    res["kernels"] = {k: rep[k] for k in names if k in rep}
    res["other_kernels_ms"] = round(sum(v["ms"] for k, v in rep.items() if k not in names), 3)
    if args.host_reps > 0:
        ctx.set_option("verify_device", 0)
        (ok, err), host_ms, host_all = timed(ctx, lambda s: verify(bnd, s), args.host_warmup, args.host_reps, stream)
        assert ok, "verify_device=0 rejected the proof: " + err
        res.update(verify_host_ms=round(host_ms, 3), verify_host_all_ms=[round(t, 3) for t in host_all],
                   host_reps=args.host_reps, host_warmup=args.host_warmup,
                   host_over_device=round(host_ms / dev_ms, 2))
        ctx.set_option("verify_device", 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--host-warmup", type=int, default=2)
    args = ap.parse_args()
    for lr in args.log_rows:
        run(lr, args)


if __name__ == "__main__":
    main()
