"""GPU: the device build of the 128-bit field arithmetic on the directed carry-edge cases.

The device mul_wide is not the code the host runs: it goes through the inline-asm mac3 /
mac3_first pair (v_mad_u64_u32 plus a carry into a third word).  The rest of the GPU suite feeds
it uniformly random elements, which never take the paths tests/fe128_cases.py is built for (and
tests/test_fe128_edges.py proves it reaches).  Here those cases go through the existing ABI, one
entry per primitive:

* sg_scale_dev            -- mont_mul(data[i], constant);
* sg_fri_fold_runs_dev    -- fe_add, fe_halve, fe_sub and a product (alpha = 0: exactly (x+y)/2);
* sg_ntt_rows_dev, sg_ntt -- the lazy butterflies (fe_add_lazy, fe_sub_lazy, fe_canon);
* FRI::prove              -- the same fold fused into the Merkle leaf kernels;
* sg_mul_pow_dev and sg_fri_fold_runs_dev at exponents up to 2^36 - 1 / 2^29, where the
  2^12 and 2^24 power tables are read at non-zero indices.

Every comparison is exact equality against big-int arithmetic or the oracle.
"""
import pytest

import fe128_cases as C
import stark_oracle as o
import starkgpu as sg

pytestmark = pytest.mark.gpu

P = o.P
R = 1 << 128
R_INV = pow(R, -1, P)
HALF = pow(2, -1, P)
BLOCK = 256


@pytest.fixture(scope="module")
def be():
    import dist_model as M
    return M.GpuRows()


def _out(be, count):
    import torch
    return torch.empty(2 * count, dtype=torch.int64, device=be.device)


def _fold_expect(x, y, alpha, offset, omega, i):
    """fri.rs:150-159 at global index i: 2^-1 ((1 + a/(o w^i)) x + (1 - a/(o w^i)) y)."""
    abo = alpha * pow(offset * pow(omega, i, P) % P, -1, P) % P
    return ((1 + abo) * x + (1 - abo) * y) * HALF % P


# ------------------------------------------------------------------ 1. mont_mul through sg_scale_dev

def test_device_mont_mul_on_directed_pairs(be):
    """k_scale_const computes mont_mul(data[i], to_mont(c)); with c = b R^-1 that is mont_mul(a, b)
    for every directed pair, one launch per distinct b.  Some buffers hold values in [p, 2^128):
    that is mont_mul's own contract (a < 2^128), which the lazy NTT values exercise in production
    -- the buffers are no canonical field data.  Expected: a b R^-1 mod p, elementwise."""
    assert len(C.MONT_GROUPS) <= C.MAX_B_GROUPS
    bad = []
    for b, vals in C.MONT_GROUPS:
        vals = list(vals)
        if len(vals) % BLOCK == 0:  # the last block must be a partial one
            vals.append(1)
        assert len(vals) % BLOCK != 0
        buf = be.from_ints(vals)
        be.scale(buf, len(vals), b * R_INV % P)
        got = be.to_ints(buf)
        bad += [(hex(a), hex(b), hex(g)) for a, g in zip(vals, got) if g != a * b * R_INV % P]
    assert not bad, (len(bad), bad[:5])


# ------------------------------------------------------------------ 2. add / halve / sub through the fold

@pytest.mark.parametrize("scalars", ["alpha0", "one", "random"])
def test_device_add_halve_sub_through_fold(be, scalars):
    """The whole-codeword layout (n_local = n_global = 2N, one run of N): the directed (x, y) sit
    at (l, l + N).  alpha = 0 leaves exactly (x + y) / 2 (fe_add, fe_halve; the product's second
    factor is 0); alpha = offset = 1 and a random alpha / offset give the full fold."""
    pairs = C.ADDSUB_PAIRS
    N = 1 << 8
    assert N < len(pairs) <= 2 * N
    omega = o.primitive_nth_root(2 * N)
    alpha, offset = {"alpha0": (0, o.GENERATOR), "one": (1, 1),
                     "random": tuple(o.synthetic_elements(5, b"fold-edges", 2))}[scalars]
    for start in (0, len(pairs) - N):  # two codewords cover every pair
        chunk = pairs[start:start + N]
        cw = [x for x, _ in chunk] + [y for _, y in chunk]
        dst = _out(be, N)
        be.fold_runs(omega, offset, alpha, be.from_ints(cw), 2 * N, N, N, 0, 2 * N, dst)
        got = be.to_ints(dst)
        assert got == o.FRI.fold(cw, alpha, omega, offset)
        if alpha == 0:
            assert got == [(x + y) * HALF % P for x, y in chunk]


# ------------------------------------------------------------------ 3. the lazy butterflies

@pytest.mark.parametrize("n", C.NTT_SIZES)
def test_device_lazy_butterflies_on_directed_rows(be, n):
    """sg_ntt_rows_dev on rows whose stage-1 partners are the directed pairs (sums of exactly
    2^128, 2^128 - 1, p; differences of 0 and -1; ripples through every limb) and, at n = 4 and 8,
    rows solved so that stage 2 takes a non-canonical sum and adds up to exactly 2^128."""
    rows = C.ntt_rows(n)
    flat = [v for row in rows for v in row]
    src = be.from_ints(flat)
    for root in C.ntt_roots(n, o.primitive_nth_root(n)):
        dst = _out(be, len(flat))
        be.ntt_rows(root, src, n, len(rows), dst, n)
        got = be.to_ints(dst)
        for r, row in enumerate(rows):
            assert got[r * n:(r + 1) * n] == o.ntt(root, row), (n, hex(root), r)


def test_device_multi_pass_ntt_round_trip_on_directed_pairs():
    """One single-transform sg.ntt / sg.intt round at 2^12 (the multi-pass path) whose stage-1
    partners come from the directed pairs."""
    n = 1 << 12
    root = o.primitive_nth_root(n)
    x = C.pair_codeword(n)
    y = sg.to_ints(sg.ntt(root, x))
    assert y == o.ntt(root, x)
    assert sg.to_ints(sg.intt(root, x)) == o.intt(root, x)
    assert sg.to_ints(sg.intt(root, y)) == x


# ------------------------------------------------------------------ 4. the fold fused into the leaf kernels

@pytest.mark.parametrize("n,exp,c", [(1 << 10, 4, 8), (1 << 14, 8, 16)])
def test_device_fused_fold_in_fri_prove(n, exp, c):
    """FRI::prove on a codeword whose fold partners (cw[i], cw[i + n/2]) cycle through the directed
    pairs (the prover does not require a low degree): top indices and proof-stream bytes equal the
    oracle's, as in test_fri_prove_stream_bytes_match_oracle."""
    omega = o.primitive_nth_root(n)
    cw = C.pair_codeword(n)
    ops = o.IndependentProofStream()
    otop = o.FRI(o.GENERATOR, omega, n, exp, c).prove(cw, ops)
    gps = sg.IndependentProofStream()
    gtop = sg.FRI(o.GENERATOR, omega, n, exp, c).prove(cw, gps)
    assert gtop == otop
    assert gps.digest() == ops.digest()


# ------------------------------------------------------------------ 5. large exponents

def test_device_mul_pow_large_exponents(be):
    """k_mul_pow's three power tables at non-zero indices: b0 just below and above 2^12 and 2^24,
    a row term (a1, b1 != 0) that crosses a table boundary, the largest exponent 2^36 - 1; every
    element against pow(base, e, p).  A largest exponent of exactly 2^36 is refused."""
    rows, cols = 5, 7
    base = o.synthetic_elements(1, b"pow-edges", 1)[0]
    x = o.synthetic_elements(2, b"pow-edges", rows * cols - 4) + [0, 1, P - 1, P - 2]

    def emax(a0, a1, b0, b1):
        return (a0 + a1 * (rows - 1)) * (cols - 1) + b0 + b1 * (rows - 1)

    a0, a1, b1 = 3, 1 << 10, 4095
    top = (1 << 36) - 1 - emax(a0, a1, 0, b1)
    cases = [(a0, a1, b0, b1) for b0 in ((1 << 12) - 2, (1 << 12) + 1, (1 << 24) - 2, (1 << 24) + 1, top)]
    cases += [(0, 0, (1 << 36) - 1, 0), (1 << 23, 1 << 11, 4095, (1 << 24) - 1)]
    assert emax(*cases[4]) == (1 << 36) - 1
    for (a0, a1, b0, b1) in cases:
        assert emax(a0, a1, b0, b1) < 1 << 36
        buf = be.from_ints(x)
        be.mul_pow(base, buf, rows, cols, a0, a1, b0, b1)
        got = be.to_ints(buf)
        seen = set()
        for r in range(rows):
            for c in range(cols):
                e = (a0 + a1 * r) * c + b0 + b1 * r
                seen.add((e >> 24, (e >> 12) & 4095))
                assert got[r * cols + c] == x[r * cols + c] * pow(base, e, P) % P, (a0, a1, b0, b1, r, c)
        assert len(seen) > 1 or b0 == (1 << 36) - 1  # the table indices move within one call
    buf = be.from_ints(x)
    with pytest.raises(sg.StarkGpuError):
        be.mul_pow(base, buf, rows, cols, cases[4][0], cases[4][1], top + 1, cases[4][3])
    assert be.to_ints(buf) == x


@pytest.mark.parametrize("run_off", [0, 4097, (1 << 23) - 1])
def test_device_fold_runs_large_exponents(be, run_off):
    """A 128-element shard of a 2^30-point codeword, runs of one element 2^23 apart: the fold's
    exponents reach 2^29, so its 2^12 and 2^24 tables are read at non-zero indices.  Every output
    against the big-int fold of its global index."""
    n_global, stride, n_local = 1 << 30, 1 << 23, 128
    half = n_local // 2
    omega = o.primitive_nth_root(n_global)
    alpha, offset = o.synthetic_elements(6, b"fold-big", 2)
    pairs = C.ADDSUB_PAIRS
    chunk = [pairs[(run_off + 3 * k) % len(pairs)] for k in range(half)]
    cw = [x for x, _ in chunk] + [y for _, y in chunk]
    dst = _out(be, half)
    be.fold_runs(omega, offset, alpha, be.from_ints(cw), n_local, 1, stride, run_off, n_global, dst)
    got = be.to_ints(dst)
    idx = [l * stride + run_off for l in range(half)]
    assert max(idx) >> 24 > 0 and any((i >> 12) & 4095 for i in idx)
    for l, i in enumerate(idx):
        assert got[l] == _fold_expect(chunk[l][0], chunk[l][1], alpha, offset, omega, i), (run_off, l)
