"""Deterministic directed inputs for the 128-bit field arithmetic (csrc/fe128.hpp, fe_halve), and
the list of model events (tests/fe128_model.py) they are required to reach.

Uniformly random field elements never take several carry paths of this arithmetic (a zero low
half of the product, a carry out of a saturated limb, a sum of exactly 2^128, ...).  The cases
here are built to take them; tests/test_fe128_edges.py asserts through the model that they do, and
tests/test_gpu_field_edges.py sends the same cases through the device code.

Nothing here is an expected value: expected values are big-int arithmetic in the tests.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Sequence, Tuple

from fe128_model import M64, NEG_P, P, R, R2_MOD_P, R_MOD_P

# ------------------------------------------------------------------ mont_mul pairs

LIMB_PATTERNS = [0, 1, 0x80000000, 0xCB7FFFFF, 0xCB800000, 0xFFFFFFFE, 0xFFFFFFFF]


def _val(l: Sequence[int]) -> int:
    return l[0] | (l[1] << 32) | (l[2] << 64) | (l[3] << 96)


# every a in [0, 2^128) whose four limbs are patterns (values >= p included): 7^4
A_PATTERNED = [_val(l) for l in itertools.product(LIMB_PATTERNS, repeat=4)]
# a short list for the constants that are not patterns themselves
A_SHORT = sorted(set([_val(l) for l in itertools.product([0, 1, 0xFFFFFFFF], repeat=4)] +
                     [P - 2, P - 1, P, P + 1, R - 2, R - 1, 1 << 127, (1 << 127) - 1, R_MOD_P, R2_MOD_P, NEG_P - 1]))
# a with a zero low 64 bits; a (and b below) multiples of 2^32 and of 2^64
A_ZERO_LOW64 = [k << 64 for k in (1, 2, M64, M64 - 1, 1 << 63, 0xCB80000000000000, 0xCB7FFFFFFFFFFFFF,
                                  0xFFFFFFFF00000000, 0x00000000FFFFFFFF, 0x8000000000000001)]
A_MULT_2_32 = [k << 32 for k in (1, (1 << 96) - 1, 0xCB7FFFFF_FFFFFFFF_FFFFFFFF, 0xFFFFFFFF_00000000_FFFFFFFF,
                                 0x80000000_00000000_00000001, 0xCB800000_00000000_00000000)]
A_LAZY = [P, P + 1, R - 1]  # mont_mul's own contract is a < 2^128: lazy NTT values reach it

# b whose limbs are patterns: the top limb at, just below and far below p's, the low limbs
# saturated or zero (so multiples of 2^32 and 2^64 are among them)
B_PATTERNED = [_val((w0, w1, w2, w3)) for w3 in (0, 0x80000000, 0xCB7FFFFF)
               for w2 in (0, 0xFFFFFFFF) for w1 in (0, 0xFFFFFFFF) for w0 in (0, 0xFFFFFFFF)]
B_PATTERNED += [_val((1, 1, 1, 1)), _val((0xFFFFFFFE, 0xFFFFFFFE, 0xFFFFFFFE, 0xCB7FFFFF)),
                _val((0x80000000, 0x80000000, 0x80000000, 0x80000000)), _val((0xCB800000, 0xCB7FFFFF, 1, 0x80000000))]
B_SPECIAL = [1, 2, P - 1, P - 2, R_MOD_P, R2_MOD_P]
# odd constants for the solved families (b must be invertible mod 2^128 there)
B_ODD = [3, 0x0123456789ABCDEF_FEDCBA9876543211, NEG_P, _val((0xFFFFFFFF, 0, 0xFFFFFFFF, 0xCB7FFFFF))]

MAX_B_GROUPS = 64  # the device probe (sg_scale_dev) takes one constant per launch

# low words T0 of the product for the family solved for (u0, u1) == 0 with T0 != 0
_T0_SOLVED = [1, 2, 1 << 63, M64, M64 - 1, 1 << 32, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF, 0xCB80000000000001]


def _solve_u_zero(b: int, t0: int) -> int:
    """a with a*b = T0 + T1 2^64 (mod 2^128) where step 1 of the reduction leaves (u0, u1) = 0:
    m = -T0, T + m p = T + m + (m * 0xCB8) << 116, so u = T1 + 1 + (m * 0xCB8 << 52) (mod 2^64)."""
    assert b & 1 and 0 < t0 <= M64
    m = (-t0) & M64
    t1 = (-(1 + ((m * 0xCB8) << 52))) & M64
    return (t0 + (t1 << 64)) * pow(b, -1, R) % R


def _solved_for_target(b: int) -> List[int]:
    """a = r R b^-1 mod p for r in {0, 1, p-1} (so mont_mul(a, b) = r), and a + p where it fits."""
    out = []
    if b == 0:
        return out
    binv = pow(b, -1, P)
    for r in (0, 1, P - 1):
        a = r * R * binv % P
        out.append(a)
        if a + P < R:
            out.append(a + P)
    return out


def _build_mont_families() -> Dict[str, List[Tuple[int, int]]]:
    """The directed families, by name: lists of (a, b).  tests/test_fe128_edges.py states what each
    must reach, so that dropping one fails there."""
    fam: Dict[str, List[Tuple[int, int]]] = {}
    fam["patterned"] = [(a, b) for b in B_PATTERNED for a in A_PATTERNED]
    fam["constants"] = [(a, b) for b in B_SPECIAL + B_ODD for a in A_SHORT]
    all_b = list(dict.fromkeys(B_PATTERNED + B_SPECIAL + B_ODD))
    fam["zero_low64"] = [(a, b) for b in all_b for a in A_ZERO_LOW64]
    fam["lazy_a"] = [(a, b) for b in all_b for a in A_LAZY]
    fam["target"] = [(a, b) for b in all_b for a in _solved_for_target(b)]
    fam["mult_2_32"] = [(a, b) for b in all_b if b % (1 << 32) == 0 for a in A_MULT_2_32]
    fam["mult_2_64"] = [(a, b) for b in all_b if b % (1 << 64) == 0 for a in A_ZERO_LOW64]
    fam["u_zero"] = [(_solve_u_zero(b, t0), b) for b in all_b if b & 1 for t0 in _T0_SOLVED]
    return fam


MONT_FAMILIES = _build_mont_families()


def _group(families: Dict[str, List[Tuple[int, int]]]) -> List[Tuple[int, List[int]]]:
    groups: Dict[int, Dict[int, None]] = {}
    for pairs in families.values():
        for a, b in pairs:
            assert 0 <= a < R and 0 <= b < P
            groups.setdefault(b, {})[a] = None
    assert len(groups) <= MAX_B_GROUPS
    return [(b, list(vals)) for b, vals in groups.items()]


# [(b, [a, ...])]: every pair is mont_mul(a, b) with a < 2^128, b < p; one group per distinct b
MONT_GROUPS = _group(MONT_FAMILIES)


def mont_pairs() -> List[Tuple[int, int]]:
    return [(a, b) for b, vals in MONT_GROUPS for a in vals]


# ------------------------------------------------------------------ add / sub / halve pairs (canonical)

_X_CANDIDATES = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, (1 << 96) - 1, 1 << 96, (1 << 127) - 1,
                 1 << 127, (P - 1) // 2, (P + 1) // 2, NEG_P - 1, NEG_P, NEG_P + 1, P - 2, P - 1,
                 _val((0xFFFFFFFF, 0, 0xFFFFFFFF, 0x80000000)), _val((1, 0xFFFFFFFF, 0, 0xCB7FFFFF)),
                 0x6487ED5110B4611A62633145C06E0E68]

SUM_TARGETS = [P - 1, P, P + 1, R - 1, R, R + 1, 2 * P - 2]
DIFF_TARGETS = [0, 1, -1, -(P - 1)]


def _build_addsub_families() -> Dict[str, List[Tuple[int, int]]]:
    fam: Dict[str, List[Tuple[int, int]]] = {"sum": [], "diff": [], "ripple": [], "halve": []}

    def add(name: str, x: int, y: int) -> None:
        if 0 <= x < P and 0 <= y < P:
            fam[name].append((x, y))

    for t in SUM_TARGETS:
        for x in _X_CANDIDATES:
            add("sum", x, t - x)
            add("sum", t - x, x)
    for d in DIFF_TARGETS:
        for x in _X_CANDIDATES:
            add("diff", x, x - d)
    # a carry / a borrow that ripples through all four limbs
    for k in (1, 2, 3):
        add("ripple", (1 << (32 * k)) - 1, 1)
        add("ripple", 1, (1 << (32 * k)) - 1)
        add("ripple", 1 << (32 * k), 1)
        add("ripple", 0, (1 << (32 * k)) - 1)
    add("ripple", (1 << 96) - 1 + (0x80000000 << 96), (0x4B7FFFFF << 96) + 1)   # ripple, then p <= sum < 2^128
    add("ripple", (1 << 127) - 1, (1 << 127) + 1)                                # out of bit 127: exactly 2^128
    add("ripple", 1 << 96, (1 << 96) + 1)                                        # borrow through every limb
    add("ripple", 0, 1)
    add("ripple", P - 1, P - 1)
    add("ripple", 0, 0)
    add("ripple", 0, P - 1)
    # halving: (x + y) mod p even / odd, an odd sum whose + p needs the 129th bit (sum >= 2^128 - p),
    # and an odd low word of all ones (the + 1 carries into the high word)
    for s in (0, 1, 2, 3, NEG_P - 2, NEG_P, NEG_P + 2, P - 2, P - 1, M64, M64 - 1, (1 << 127) + M64,
              (0xCB7FFFFF_FFFFFFFF << 64) + M64, (1 << 64) + 1, 1 << 127, (1 << 127) + 1):
        add("halve", s, 0)
        add("halve", s // 2, s - s // 2)
        add("halve", s + 5 - P if s + 5 >= P else s + 5, P - 5)                  # the same sum through a wrap
    return fam


ADDSUB_FAMILIES = _build_addsub_families()
# every (x, y), both canonical, once
ADDSUB_PAIRS = list(dict.fromkeys(pr for pairs in ADDSUB_FAMILIES.values() for pr in pairs))


# ------------------------------------------------------------------ NTT rows (lazy butterflies)

NTT_SIZES = [2, 4, 8, 64, 2048]
# an arbitrary value that is no root of unity of small order: the graph does not need one
NON_ROOT = 0x1B2E3D4C5F607182_93A4B5C6D7E8F901
assert NON_ROOT < P


def _pair_row(n: int, start: int) -> List[int]:
    """A row whose stage-1 partners (x[j], x[j + n/2]) are the directed pairs from `start` on."""
    row = [0] * n
    for j in range(n // 2):
        row[j], row[j + n // 2] = ADDSUB_PAIRS[(start + j) % len(ADDSUB_PAIRS)]
    return row


def _lazy(s: int) -> int:
    """The value fe_add_lazy leaves for an exact sum s < 2^128 + p."""
    return s - P if s >= R else s


def _solved_rows(n: int) -> List[List[int]]:
    """Rows whose first stage-2 butterfly takes chosen stage-1 outputs: e = x[0] + x[n/2] (lazily
    reduced, so possibly in [p, 2^128)), o = (x[n/4] + x[3n/4]) mod p.  The stage-1 sums are a value
    in [p, 2^128) and exactly 2^128; o is solved so that e + o is exactly 2^128, 2^128 - 1, p, or
    stays well below, and e - o is 0, -1 or positive."""
    rows = []
    k = 0
    split = 0x2545F4914F6CDD1D_0F1E2D3C4B5A6978 % P
    for s in (P, P + 1, R - 1, R, R + 1, P + (NEG_P >> 1), P - 1, 2 * P - 2):
        e = _lazy(s)
        for o in (R - e, R - 1 - e, P - e, 0, 1, e, e + 1, e - 1, 5):
            if not 0 <= o < P:
                continue
            row = _pair_row(n, 7 * k)
            k += 1
            x0 = s // 2
            row[0], row[n // 2] = x0, s - x0
            i3 = split if o >= split else o // 3
            row[n // 4], row[3 * n // 4] = o - i3, i3
            assert all(0 <= v < P for v in row)
            rows.append(row)
    return rows


def ntt_rows(n: int) -> List[List[int]]:
    """The rows for size n: pair rows that together walk the directed pairs, plus (n = 4, 8) the
    solved rows."""
    per = n // 2
    count = {2: len(ADDSUB_PAIRS), 4: (len(ADDSUB_PAIRS) + 1) // 2, 8: (len(ADDSUB_PAIRS) + 3) // 4,
             64: 8, 2048: 3}[n]
    rows = [_pair_row(n, r * per) for r in range(count)]
    if n in (4, 8):
        rows += _solved_rows(n)
    return rows


def ntt_roots(n: int, primitive_root: int) -> List[int]:
    return [primitive_root, NON_ROOT] if n in (4, 8) else [primitive_root]


def pair_codeword(n: int) -> List[int]:
    """A codeword whose FRI fold partners (cw[i], cw[i + n/2]) cycle through the directed pairs."""
    return _pair_row(n, 0)


# ------------------------------------------------------------------ required events

# mac3_first cannot carry in columns 2 to 5: the accumulator carried in from the column below is
# < 2^34 and the first product a.w[i] * b.w[j] <= (2^32 - 1)^2 = 2^64 - 2^33 + 1 -- and with b < p
# the first products of columns 3 to 5 take b.w[3] <= 0xCB800000, further below still.  So
# "colK:first_carry" is required for column 1 only, and a column's third word can reach at most
# the number of its later products.
MONT_REQUIRED = [
    "s1:lo64=0",             # the low 64 bits of a*b are zero: step 1 runs with br = 0
    "s2:lo64=0",             # (u0, u1) == 0 going into step 2
    "s1+s2:lo64=0",          # both
    "s2:lo64=0,T0!=0",       # (u0, u1) == 0 although step 1 had work to do
    "s1:w0=0,w1!=0",         # t[0] == 0, t[1] != 0: no borrow into the negation's second limb
    "s2:w0=0,w1!=0",
    "s1:carry0", "s1:carry1", "s1:carry2", "s1:carry3", "s1:carry4",   # out of every limb of the chain
    "s1:carry_into_u5",
    "s2:carry0", "s2:carry1", "s2:carry2", "s2:carry3",
    "fin:c", "fin:g", "fin:none",
    "fin:r=p",               # r == p exactly before the final subtraction
    "res:0,nonzero_operands",
    "res:p-1",
    "col1:first_carry", "col1:w2=1", "col2:w2=2", "col3:w2=3", "col4:w2=2", "col5:w2=1",
]

ADD_REQUIRED = ["add:c", "add:g", "add:none", "add:ripple"]
SUB_REQUIRED = ["sub:borrow", "sub:noborrow", "sub:ripple"]
HALVE_REQUIRED = ["halve:even", "halve:odd:bit128", "halve:odd:nobit128", "halve:odd:low_word_carry"]
# fe_sub_lazy cannot borrow from a non-canonical first operand: its second operand is canonical,
# so a >= p > b.  "subl:borrow:noncanon" is therefore no event of any input and is not listed.
LAZY_REQUIRED = [
    "addl:carry:canon", "addl:nocarry:canon", "addl:carry:noncanon", "addl:nocarry:noncanon",
    "addl:sum=2^128", "addl:sum=2^128-1", "addl:sum=p", "addl:ripple",
    "subl:borrow:canon", "subl:noborrow:canon", "subl:noborrow:noncanon",
    "subl:diff=0", "subl:diff=-1", "subl:ripple",
]
CANON_REQUIRED = ["canon:p-1", "canon:p", "canon:2^128-1", "canon:keep", "canon:take"]

# what the NTT rows must reach through ntt_lazy (its events carry the "ntt:" prefix)
NTT_REQUIRED = ["ntt:" + e for e in LAZY_REQUIRED + CANON_REQUIRED +
                ["addl:sum=2^128:noncanon", "addl:sum=2^128-1:noncanon"]]   # the solved stage-2 operands
# what the canonical (x, y) pairs reach when given to the value-level functions directly
PAIRS_REQUIRED = ADD_REQUIRED + SUB_REQUIRED + HALVE_REQUIRED + CANON_REQUIRED + \
    [e for e in LAZY_REQUIRED if "noncanon" not in e]

REQUIRED_EVENTS = MONT_REQUIRED + PAIRS_REQUIRED + NTT_REQUIRED
