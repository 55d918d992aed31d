"""Carry-edge coverage of the 128-bit field arithmetic, on the CPU.

* the integer model (tests/fe128_model.py) equals big-int arithmetic on every directed case
  (tests/fe128_cases.py) and on 20 000 seeded random cases per function;
* the directed cases reach every event of the required list -- the carry paths uniformly random
  inputs never take -- and every named family lands what it was built for, so dropping a family
  fails here;
* the host build of mont_mul (the plain C++ mac3 fallback, through sg_fe_mul) is right on every
  directed pair.  The device build goes through the same cases in tests/test_gpu_field_edges.py.

Needs the built library (as tests/test_abi_host.py does), no GPU.
"""
import random

import pytest

import fe128_cases as C
import fe128_model as M
import stark_oracle as o
import starkgpu as sg
from starkgpu._lib import sg_fe

P, R = M.P, M.R
N_RANDOM = 20000


def _union(sets):
    out = set()
    for s in sets:
        out |= s
    return out


@pytest.fixture(scope="module")
def mont_events():
    """{(a, b): events} of the model over every directed mont_mul pair, results checked on the way."""
    ev = {}
    for a, b in C.mont_pairs():
        r, e = M.mont_mul(a, b)
        assert r == a * b * M.R_INV % P, (hex(a), hex(b))
        ev[(a, b)] = e
    return ev


@pytest.fixture(scope="module")
def ntt_events():
    """Events of ntt_lazy over the directed rows of every size, results checked against o.ntt."""
    ev = set()
    for n in C.NTT_SIZES:
        for root in C.ntt_roots(n, o.primitive_nth_root(n)):
            for row in C.ntt_rows(n):
                got, e = M.ntt_lazy(root, row, limb_products=n <= 64)
                assert got == o.ntt(root, row), (n, hex(root))
                ev |= e
    return ev


# ------------------------------------------------------------------ the model against big-int arithmetic

def test_model_constants():
    assert P == o.P and M.R_MOD_P == R - P and M.NEG_P == R - P
    assert M.limbs(P) == [1, 0, 0, 0xCB800000]
    assert len(C.MONT_GROUPS) <= C.MAX_B_GROUPS
    assert all(0 <= x < P and 0 <= y < P for x, y in C.ADDSUB_PAIRS)


def test_model_mont_mul_random():
    rng = random.Random(128)
    for _ in range(N_RANDOM):
        a, b = rng.randrange(R), rng.randrange(P)
        assert M.mont_mul(a, b)[0] == a * b * M.R_INV % P


def test_model_value_functions_directed_and_random():
    rng = random.Random(129)
    pairs = list(C.ADDSUB_PAIRS) + [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]
    half = pow(2, -1, P)
    for x, y in pairs:
        assert M.fe_add(x, y)[0] == (x + y) % P
        assert M.fe_sub(x, y)[0] == (x - y) % P
        s = (x + y) % P
        assert M.fe_halve(s)[0] == s * half % P
        assert M.fe_halve(x)[0] == x * half % P
    # lazy forms: any first operand below 2^128; the result is below 2^128 and in the right class
    lazy = pairs + [(x + P, y) for x, y in C.ADDSUB_PAIRS if x + P < R] + \
        [(rng.randrange(P, R), rng.randrange(P)) for _ in range(N_RANDOM)]
    for a, b in lazy:
        r = M.fe_add_lazy(a, b)[0]
        assert 0 <= r < R and r % P == (a + b) % P
        r = M.fe_sub_lazy(a, b)[0]
        assert 0 <= r < R and r % P == (a - b) % P
    for a in [P - 1, P, P + 1, R - 1, 0, 1] + [rng.randrange(R) for _ in range(N_RANDOM)]:
        assert M.fe_canon(a)[0] == a % P


def test_model_ntt_lazy_random():
    rng = random.Random(130)
    butterflies = 0
    for n, rows in ((1, 3), (2, 3), (16, 3), (128, 45)):
        root = o.primitive_nth_root(n)
        for _ in range(rows):
            row = [rng.randrange(P) for _ in range(n)]
            assert M.ntt_lazy(root, row)[0] == o.ntt(root, row)
            butterflies += (n // 2) * (n.bit_length() - 1)
    assert butterflies >= N_RANDOM


# ------------------------------------------------------------------ the coverage condition

def test_required_list_names_every_class():
    """The list the other tests check against holds what it must (nothing waived by editing it)."""
    req = set(C.REQUIRED_EVENTS)
    for e in ["s1:lo64=0", "s2:lo64=0", "s1+s2:lo64=0", "s1:w0=0,w1!=0", "s2:w0=0,w1!=0", "s1:carry0", "s2:carry0",
              "s1:carry_into_u5", "fin:r=p", "res:p-1", "col3:w2=3", "fin:c", "fin:g", "fin:none",
              "col1:w2=1", "col2:w2=2", "col4:w2=2", "col5:w2=1"]:
        assert e in req, e
    assert {"s1:carry%d" % i for i in range(5)} | {"s2:carry%d" % i for i in range(4)} <= req
    assert {"add:c", "add:g", "add:none", "sub:borrow", "sub:noborrow"} <= req
    assert {"halve:even", "halve:odd:bit128", "halve:odd:nobit128"} <= req
    assert {"ntt:addl:carry:noncanon", "ntt:addl:nocarry:noncanon", "ntt:subl:noborrow:noncanon",
            "ntt:subl:borrow:canon", "ntt:canon:p-1", "ntt:canon:p", "ntt:canon:2^128-1", "ntt:canon:keep"} <= req


def test_mont_pairs_reach_every_required_event(mont_events):
    seen = _union(mont_events.values())
    missing = [e for e in C.MONT_REQUIRED if e not in seen]
    assert not missing, missing
    # mac3_first never carries above column 1 (fe128_cases.py says why): the model agrees
    assert not any(e.startswith("col") and e.endswith("first_carry") and e[3] != "1" for e in seen)


def test_mont_families_land(mont_events):
    """Every family does what it was built for, on every one of its pairs."""
    fam = C.MONT_FAMILIES
    assert set(fam) == {"patterned", "constants", "zero_low64", "lazy_a", "target", "mult_2_32", "mult_2_64", "u_zero"}
    assert all(len(v) > 0 for v in fam.values())
    ev = mont_events
    # the patterned limbs alone reach every column count and every carry of the two chains
    pat = _union(ev[pr] for pr in fam["patterned"])
    assert not [e for e in C.MONT_REQUIRED if e not in pat and not e.startswith("res:")]
    assert {b for _, b in fam["constants"]} >= {1, 2, P - 1, P - 2, M.R_MOD_P, M.R2_MOD_P}
    assert {"fin:c", "fin:g", "fin:none"} <= _union(ev[pr] for pr in fam["constants"])
    for a, b in fam["zero_low64"]:
        assert a % (1 << 64) == 0 and "s1:lo64=0" in ev[(a, b)]
    for a, b in fam["mult_2_64"]:
        assert a % (1 << 64) == 0 and b % (1 << 64) == 0 and "s1+s2:lo64=0" in ev[(a, b)]
    for a, b in fam["mult_2_32"]:
        assert a % (1 << 32) == 0 and b % (1 << 32) == 0
        assert "s1:lo64=0" in ev[(a, b)] or "s1:w0=0,w1!=0" in ev[(a, b)]
    assert {a for a, _ in fam["lazy_a"]} == {P, P + 1, R - 1}
    for a, b in fam["lazy_a"]:
        if a == P and b != 0:
            assert {"fin:r=p", "res:0,nonzero_operands"} <= ev[(a, b)]
    got = {a * b * M.R_INV % P for a, b in fam["target"]}
    assert got == {0, 1, P - 1}
    assert any(a >= P for a, _ in fam["target"])
    assert "res:p-1" in _union(ev[pr] for pr in fam["target"])
    for a, b in fam["u_zero"]:
        assert "s2:lo64=0,T0!=0" in ev[(a, b)], (hex(a), hex(b))
    assert "s2:w0=0,w1!=0" in pat and "s1:w0=0,w1!=0" in _union(ev[pr] for pr in fam["u_zero"])


def test_addsub_pairs_reach_every_required_event():
    fam_ev = {}
    for name, pairs in C.ADDSUB_FAMILIES.items():
        e = set()
        for x, y in pairs:
            for f in (M.fe_add, M.fe_sub, M.fe_add_lazy, M.fe_sub_lazy):
                e |= f(x, y)[1]
            e |= M.fe_halve((x + y) % P)[1]
            e |= M.fe_canon(x)[1] | M.fe_canon(y)[1]
            if x + y < R:
                e |= M.fe_canon(x + y)[1]
        fam_ev[name] = e
    seen = _union(fam_ev.values())
    missing = [e for e in C.PAIRS_REQUIRED if e not in seen]
    assert not missing, missing
    assert set(fam_ev) == {"sum", "diff", "ripple", "halve"}
    assert {x + y for x, y in C.ADDSUB_FAMILIES["sum"]} == set(C.SUM_TARGETS)
    assert {x - y for x, y in C.ADDSUB_FAMILIES["diff"]} == set(C.DIFF_TARGETS)
    assert {"add:c", "add:g", "add:none", "addl:sum=2^128", "addl:sum=2^128-1", "addl:sum=p", "canon:p",
            "canon:2^128-1", "canon:p-1"} <= fam_ev["sum"]
    assert {"sub:borrow", "sub:noborrow", "subl:diff=0", "subl:diff=-1"} <= fam_ev["diff"]
    assert {"add:ripple", "sub:ripple", "addl:ripple", "subl:ripple"} <= fam_ev["ripple"]
    assert set(C.HALVE_REQUIRED) <= fam_ev["halve"]


def test_ntt_rows_reach_every_required_event(ntt_events):
    missing = [e for e in C.NTT_REQUIRED if e not in ntt_events]
    assert not missing, missing
    # the lazy subtraction cannot borrow from a non-canonical first operand (fe128_cases.py)
    assert "ntt:subl:borrow:noncanon" not in ntt_events
    # the solved rows: the first stage-2 butterfly takes e = x[0] + x[n/2] (lazy) and
    # o = (x[n/4] + x[3n/4]) mod p -- a stage-1 sum in [p, 2^128) and one of exactly 2^128 among
    # the e, and stage-2 sums of exactly 2^128 and 2^128 - 1 from a non-canonical e
    for n in (4, 8):
        solved = C._solved_rows(n)
        assert len(solved) >= 20 and all(row in C.ntt_rows(n) for row in solved)
        classes = set()
        for row in solved:
            s1 = row[0] + row[n // 2]
            e = M.fe_add_lazy(row[0], row[n // 2])[0]
            oo = (row[n // 4] + row[3 * n // 4]) % P
            classes.add((s1 == R, P <= s1 < R, e >= P, e + oo == R, e + oo == R - 1, e - oo in (0, -1)))
        assert any(c[0] for c in classes) and any(c[1] and c[2] for c in classes)
        assert any(c[2] and c[3] for c in classes) and any(c[2] and c[4] for c in classes)
        assert any(c[5] for c in classes)


# ------------------------------------------------------------------ the host build of mont_mul

def _fe(v):
    return sg_fe(v & M.M64, v >> 64)


def test_host_mont_mul_on_directed_pairs():
    """sg_fe_mul(a, b) = mont_mul(mont_mul(a, b), R^2): the host mont_mul (plain C++ mac3) sees
    every directed pair as its first step, values a in [p, 2^128) included (its contract)."""
    f = sg.lib().sg_fe_mul
    for b, vals in C.MONT_GROUPS:
        fb = _fe(b)
        for a in vals:
            r = f(_fe(a), fb)
            assert (int(r.hi) << 64) | int(r.lo) == a * b % P, (hex(a), hex(b))


def test_host_pow_and_inverse_at_the_constants():
    for x in (1, 2, P - 1, P - 2, M.R_MOD_P):
        assert sg.fe_inverse(x) == pow(x, -1, P)
        assert sg.fe_mul(x, sg.fe_inverse(x)) == 1
        for e in (0, 1, 2, 3, 1 << 32, 1 << 63, (1 << 64) - 1):  # the ABI's exponent is 64 bits
            assert sg.fe_pow(x, e) == pow(x, e, P), (hex(x), e)
