#!/usr/bin/env python3
"""Time the RPSSS object (rpsss.rs; sg_rpsss_*) and the batched Rescue-Prime kernel behind its
key generation, at the reference's published configuration RPSSS::new(field, 4, 64, 128, 3).

One JSON line (also written to --out, a file under profiles/):
  keygen_batch   device time of the rescue_hash_batch kernel (sg_ctx_profile, HIP events), median
                 of --reps after --warmup, at every --batch-log size; hashes per second
  host loop      hashes per second of the host loop on one core (option rescue_device_min above n)
  crossover      wall time of sg_rescue_hash_batch (upload, launch, download included) against the
                 host loop at n = 1, 2, 4, ...: the first n from which the device form stays faster
  roof           --field-rate (G products/s, tools/microbench_field's figure measured on the same
                 box) / products per hash counted from the code; the kernel's fraction of it
  sign / verify  wall time of sg_rpsss_sign (median of --sign-reps after --sign-warmup) beside the
                 hand-assembled composition that rebuilds the constraints per signature (bench.py's
                 side.rpsss_sign_ms), same process, and sg_rpsss_verify

usage: rpsss_time.py [--batch-log 10 16 20] [--reps 5] [--warmup 2] [--field-rate 462] [--out FILE]
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
from starkgpu.api import _ptr  # noqa: E402

P = sg.FIELD_PRIME
M, N = 2, 27
# csrc/rescue_kernels.hip: N m (143 + 2m) + 2 products per hash
PRODUCTS_PER_HASH = N * M * (143 + 2 * M) + 2
HOST_FOREVER = 1 << 62


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


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def hash_batch(ctx, rp, xs, out):
    ctx.check(ctx._lib.sg_rescue_hash_batch(ctx.handle, rp.handle, _ptr(xs), len(xs), _ptr(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-log", type=int, nargs="+", default=[10, 16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sign-reps", type=int, default=20)
    ap.add_argument("--sign-warmup", type=int, default=3)
    ap.add_argument("--field-rate", type=float, default=462.0,
                    help="G products/s of tools/microbench_field on this box (DESIGN.md 8.1)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ctx = sg.Context(0)
    rp = sg.RescuePrime(M, 1, 128, N, ctx=ctx)
    res = {"tool": "rpsss_time", "m": M, "N": N, "products_per_hash": PRODUCTS_PER_HASH,
           "field_rate_gproducts_s": args.field_rate}

    # ---- the kernel alone (HIP events), and the whole host-pointer call beside it
    ctx.set_option("rescue_device_min", 0)
    kernel = {}
    for lg in args.batch_log:
        n = 1 << lg
        xs, out = synthetic(b"rpsss-time-%d" % lg, n), np.empty((n, 2), dtype=np.uint64)
        for _ in range(args.warmup):
            hash_batch(ctx, rp, xs, out)
        ms = []
        for _ in range(args.reps):
            ctx.profile(True)
            hash_batch(ctx, rp, xs, out)
            ms.append(ctx.profile_report()["rescue_hash_batch"]["ms"])
            ctx.profile(False)
        call_ms, _ = wall_ms(lambda: hash_batch(ctx, rp, xs, out), 0, args.reps)
        med = statistics.median(ms)
        kernel[str(n)] = {"kernel_ms": round(med, 4), "kernel_all_ms": [round(t, 4) for t in ms],
                          "hashes_per_s": round(n / (med * 1e-3)), "call_ms": round(call_ms, 4),
                          "gproducts_per_s": round(n * PRODUCTS_PER_HASH / (med * 1e-3) / 1e9, 2)}
    res["keygen_batch"] = kernel
    roof = args.field_rate * 1e9 / PRODUCTS_PER_HASH
    res["roof_hashes_per_s"] = round(roof)
    top = kernel[str(1 << max(args.batch_log))]
    res["fraction_of_roof_at_largest"] = round(top["hashes_per_s"] / roof, 3)

    # ---- the host loop on one core
    n = 1 << 10
    xs, out = synthetic(b"rpsss-time-host", n), np.empty((n, 2), dtype=np.uint64)
    ctx.set_option("rescue_device_min", HOST_FOREVER)
    host_ms, _ = wall_ms(lambda: hash_batch(ctx, rp, xs, out), 1, 3)
    res["host_loop"] = {"n": n, "ms": round(host_ms, 3), "hashes_per_s": round(n / (host_ms * 1e-3))}

    # ---- crossover: the whole call, device against host, n = 1, 2, 4, ...
    cross, first = [], None
    for lg in range(0, 11):
        k = 1 << lg
        ctx.set_option("rescue_device_min", 0)
        dev_ms, _ = wall_ms(lambda: hash_batch(ctx, rp, xs[:k], out), 2, 7)
        ctx.set_option("rescue_device_min", HOST_FOREVER)
        hst_ms, _ = wall_ms(lambda: hash_batch(ctx, rp, xs[:k], out), 1, 5)
        cross.append({"n": k, "device_call_ms": round(dev_ms, 4), "host_ms": round(hst_ms, 4)})
        if dev_ms < hst_ms:
            first = k if first is None else first
        else:
            first = None
    res["crossover"] = {"table": cross, "device_wins_from_n": first}

    # ---- sign / verify beside the hand-assembled composition (constraints rebuilt per signature)
    rpsss = sg.RPSSS(4, 64, 128, 3, ctx=ctx)
    n_tr, n_rc = rpsss.params()
    tr, rc = synthetic(b"rpsss-trace-rand", n_tr), synthetic(b"rpsss-rand-poly", n_rc)
    sk = int.from_bytes(hashlib.shake_256(b"sg-bench-rpsss").digest(17), "big") % P
    doc = b"Hello, World!"
    st = sg.Stark(4, 64, 128, M, N + 1, 3, ctx=ctx)

    def composed():
        pk = rp.hash(sk)
        trace = rp.trace_array(sk)
        tcs = rp.transition_constraints(st.omicron, st.omicron_domain_length)
        return st.prove(trace, tcs, rp.boundary_constraints(pk), sg.SignatureProofStream(doc), tr, rc)

    sig = rpsss.sign(sk, doc, tr, rc)
    assert sig == composed() and len(sig) == 1156888
    pk = rp.hash(sk)
    sign_ms, sign_all = wall_ms(lambda: rpsss.sign(sk, doc, tr, rc), args.sign_warmup, args.sign_reps)
    comp_ms, comp_all = wall_ms(composed, args.sign_warmup, args.sign_reps)
    ver_ms, _ = wall_ms(lambda: rpsss.verify(pk, doc, sig), args.sign_warmup, args.sign_reps)
    assert rpsss.verify(pk, doc, sig) == (True, "") and not rpsss.verify(pk, b"Malicious document", sig)[0]
    res["sign"] = {"sg_rpsss_sign_ms": round(sign_ms, 3), "composed_sign_ms": round(comp_ms, 3),
                   "difference_ms": round(sign_ms - comp_ms, 3), "sg_rpsss_verify_ms": round(ver_ms, 3),
                   "reps": args.sign_reps, "warmup": args.sign_warmup, "signature_bytes": len(sig),
                   "sg_rpsss_sign_all_ms": [round(t, 3) for t in sign_all],
                   "composed_sign_all_ms": [round(t, 3) for t in comp_all]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
