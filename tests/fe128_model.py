"""TEST MODEL of csrc/fe128.hpp and fe_halve (csrc/dev_util.hpp): the integer steps restated on
Python ints, each function returning ``(result, events)``.

``events`` is a set of short strings naming the rare paths the inputs took: which carries and
borrows the C code branches on, which limbs were zero, how high a column's third word counted.
The model supplies NO expected values -- those come from big-int arithmetic (``a*b*R^-1 % p``,
``(x+y) % p``, the oracle's ntt / fold).  It exists so a test can assert that its directed inputs
(tests/fe128_cases.py) reach the paths uniformly random data never takes, and it is itself pinned
to big-int arithmetic by tests/test_fe128_edges.py.

* ``mont_mul`` is restated limb by limb: the Comba columns with their 96-bit accumulator
  (``mac3_first`` / ``mac3``), both 64-bit reduction steps with their add chains, the final
  ``(c, g)`` selection.
* ``fe_add`` / ``fe_sub`` / ``fe_add_lazy`` / ``fe_sub_lazy`` / ``fe_canon`` / ``fe_halve`` are
  restated on whole values, recording the carry / borrow bits the C code branches on.
* ``ntt_lazy`` is the reference's DIT graph (fft/ntt.rs:26-46) on the lazy butterfly of
  csrc/kernels.hip (``o = mont_mul(x, w)``, ``e + o`` and ``e - o`` lazily reduced, the last stage
  canonicalised), collecting every butterfly's events.
"""
from __future__ import annotations

from typing import List, Sequence, Set, Tuple

P = 1 + 407 * (1 << 119)
R = 1 << 128
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
M128 = R - 1
P3 = 0xCB800000          # p = 1 + (P3 << 96)
NEG_P = R - P            # 0x347FFFFF_FFFFFFFF_FFFFFFFF_FFFFFFFF
R_MOD_P = R % P
R2_MOD_P = R * R % P
R_INV = pow(R, -1, P)

assert P == 1 + (P3 << 96) and NEG_P >> 96 == 0x347FFFFF

Events = Set[str]


def limbs(x: int) -> List[int]:
    return [(x >> (32 * i)) & M32 for i in range(4)]


def _addc(a: int, b: int, c: int) -> Tuple[int, int]:
    s = a + b + c
    return s & M32, s >> 32


def _subc(a: int, b: int, br: int) -> Tuple[int, int]:
    d = a - b - br
    return d & M32, 1 if d < 0 else 0


# ------------------------------------------------------------------ mont_mul, limb level

def _mac3_first(a: int, b: int, acc: int) -> Tuple[int, int]:
    s = acc + a * b
    return s & M64, s >> 64


def _mac3(a: int, b: int, acc: int, acc2: int) -> Tuple[int, int]:
    s = acc + a * b
    return s & M64, acc2 + (s >> 64)


def mul_wide(a: int, b: int, ev: Events) -> List[int]:
    """fe128.hpp mul_wide: the 8 limbs of a*b; events ``colK:w2=N`` (the third word of column K
    ended at N > 0) and ``colK:first_carry`` (mac3_first itself carried)."""
    A, B = limbs(a), limbs(b)
    t = [0] * 8
    acc = A[0] * B[0]
    t[0] = acc & M32
    acc >>= 32
    acc += A[0] * B[1]
    assert acc <= M64  # "no carry"
    cols = {1: [(1, 0)], 2: [(0, 2), (1, 1), (2, 0)], 3: [(0, 3), (1, 2), (2, 1), (3, 0)],
            4: [(1, 3), (2, 2), (3, 1)], 5: [(2, 3), (3, 2)]}
    for k in range(1, 6):
        (i, j), rest = cols[k][0], cols[k][1:]
        acc, acc2 = _mac3_first(A[i], B[j], acc)
        if acc2:
            ev.add("col%d:first_carry" % k)
        for (i, j) in rest:
            acc, acc2 = _mac3(A[i], B[j], acc, acc2)
        assert acc2 <= M32
        if acc2:
            ev.add("col%d:w2=%d" % (k, acc2))
        t[k] = acc & M32
        acc = (acc >> 32) | (acc2 << 32)
    acc += A[3] * B[3]
    assert acc <= M64  # "the top column cannot overflow"
    t[6] = acc & M32
    t[7] = acc >> 32
    return t


def _reduce_step(tag: str, lo0: int, lo1: int, hi: Sequence[int], ev: Events) -> Tuple[List[int], int, bool]:
    """One 64-bit Montgomery step on (lo0, lo1 | hi...): returns the sums of the add chain over
    ``hi``, its last carry, and whether (lo0, lo1) was zero."""
    m0, br = _subc(0, lo0, 0)
    m1, br = _subc(0, lo1, br)
    zero = lo0 == 0 and lo1 == 0
    assert br == (0 if zero else 1)
    if zero:
        ev.add(tag + ":lo64=0")
    if lo0 == 0 and lo1 != 0:
        ev.add(tag + ":w0=0,w1!=0")
    q0 = m0 * P3
    q1 = m1 * P3 + (q0 >> 32)
    adds = [br, q0 & M32, q1 & M32, q1 >> 32]
    out = []
    c = 0
    for i, h in enumerate(hi):
        s, c = _addc(h, adds[i] if i < 4 else 0, c if i else 0)
        if c:
            ev.add("%s:carry%d" % (tag, i))
        out.append(s)
    return out, c, zero


def mont_mul(a: int, b: int) -> Tuple[int, Events]:
    """a*b*R^-1 mod p for a < 2^128, b < p (fe128.hpp mont_mul), limb by limb."""
    assert 0 <= a < R and 0 <= b < P
    ev: Events = set()
    t = mul_wide(a, b, ev)
    # step 1: eliminate (t0, t1); u0..u4 by the chain, u5 = t7 + c
    u, c, z1 = _reduce_step("s1", t[0], t[1], t[2:7], ev)
    u5 = t[7] + c
    assert u5 <= M32  # "U < 2^192"
    if c:
        ev.add("s1:carry_into_u5")
    # step 2: eliminate (u0, u1)
    r, c, z2 = _reduce_step("s2", u[0], u[1], [u[2], u[3], u[4], u5], ev)
    if z1 and z2:
        ev.add("s1+s2:lo64=0")
    if z2 and not z1:
        ev.add("s2:lo64=0,T0!=0")
    rv = r[0] | (r[1] << 32) | (r[2] << 64) | (r[3] << 96)
    d = rv + NEG_P
    g = d >> 128
    assert rv + (c << 128) < 2 * P
    if c:
        ev.add("fin:c")
    elif g:
        ev.add("fin:g")
    else:
        ev.add("fin:none")
    if not c and rv == P:
        ev.add("fin:r=p")
    res = d & M128 if (c | g) else rv
    if res == P - 1:
        ev.add("res:p-1")
    if res == 0 and a != 0 and b != 0:  # only the lazy value a = p
        ev.add("res:0,nonzero_operands")
    return res, ev


# ------------------------------------------------------------------ value level

def _ripple_add(x: int, y: int) -> bool:
    """A carry out of every one of the three low limbs of x + y."""
    return all(((x & ((1 << k) - 1)) + (y & ((1 << k) - 1))) >> k for k in (32, 64, 96))


def _ripple_sub(x: int, y: int) -> bool:
    """A borrow out of every one of the three low limbs of x - y."""
    return all((x & ((1 << k) - 1)) < (y & ((1 << k) - 1)) for k in (32, 64, 96))


def fe_add(x: int, y: int) -> Tuple[int, Events]:
    """(x + y) mod p, x and y canonical: taken by c (sum >= 2^128), by g only (p <= sum < 2^128), or not."""
    assert 0 <= x < P and 0 <= y < P
    ev: Events = set()
    s = x + y
    c, s = s >> 128, s & M128
    d = s + NEG_P
    g, d = d >> 128, d & M128
    ev.add("add:c" if c else ("add:g" if g else "add:none"))
    if _ripple_add(x, y):
        ev.add("add:ripple")
    return (d if (c | g) else s), ev


def fe_sub(x: int, y: int) -> Tuple[int, Events]:
    assert 0 <= x < P and 0 <= y < P
    ev: Events = set()
    d = x - y
    br = 1 if d < 0 else 0
    d &= M128
    ev.add("sub:borrow" if br else "sub:noborrow")
    if _ripple_sub(x, y):
        ev.add("sub:ripple")
    return ((d + P) & M128 if br else d), ev


def _canon_tag(a: int) -> str:
    return "noncanon" if a >= P else "canon"


def fe_add_lazy(a: int, b: int) -> Tuple[int, Events]:
    """a in [0, 2^128), b canonical: a + b, minus p on a carry out of bit 127."""
    assert 0 <= a < R and 0 <= b < P
    ev: Events = set()
    s = a + b
    c, lo = s >> 128, s & M128
    ev.add("addl:%s:%s" % ("carry" if c else "nocarry", _canon_tag(a)))
    for name, v in (("2^128", R), ("2^128-1", R - 1), ("p", P)):
        if s == v:
            ev.add("addl:sum=" + name)
            if a >= P:
                ev.add("addl:sum=%s:noncanon" % name)
    if _ripple_add(a, b):
        ev.add("addl:ripple")
    r = lo + NEG_P if c else lo
    assert r < R  # the second chain's carry is dropped: it never occurs
    return r, ev


def fe_sub_lazy(a: int, b: int) -> Tuple[int, Events]:
    """a in [0, 2^128), b canonical: a - b, plus p on a borrow."""
    assert 0 <= a < R and 0 <= b < P
    ev: Events = set()
    d = a - b
    br = 1 if d < 0 else 0
    ev.add("subl:%s:%s" % ("borrow" if br else "noborrow", _canon_tag(a)))
    for name, v in (("0", 0), ("-1", -1)):
        if d == v:
            ev.add("subl:diff=" + name)
    if _ripple_sub(a, b):
        ev.add("subl:ripple")
    r = (d & M128) + P if br else d
    assert (r >> 128) == br  # wraps back below 2^128 exactly when it borrowed
    return r & M128, ev


def fe_canon(a: int) -> Tuple[int, Events]:
    assert 0 <= a < R
    ev: Events = set()
    d = a + NEG_P
    g = d >> 128
    ev.add("canon:take" if g else "canon:keep")
    for name, v in (("p-1", P - 1), ("p", P), ("2^128-1", R - 1)):
        if a == v:
            ev.add("canon:" + name)
    return (d & M128 if g else a), ev


def fe_halve(a: int) -> Tuple[int, Events]:
    """a * 2^-1 mod p for canonical a, on 64-bit words as dev_util.hpp does it."""
    assert 0 <= a < P
    ev: Events = set()
    a0, a1 = a & M64, a >> 64
    odd = a0 & 1
    s0 = (a0 + odd) & M64
    c0 = 1 if s0 < odd else 0
    add1 = (P3 << 32) if odd else 0
    s1 = (a1 + add1) & M64
    c1 = 1 if s1 < add1 else 0
    s1b = (s1 + c0) & M64
    c1 += 1 if s1b < c0 else 0
    assert c1 <= 1
    if not odd:
        ev.add("halve:even")
    else:
        ev.add("halve:odd:bit128" if c1 else "halve:odd:nobit128")
        if c0:
            ev.add("halve:odd:low_word_carry")
    r0 = (s0 >> 1) | ((s1b << 63) & M64)
    r1 = (s1b >> 1) | (c1 << 63)
    return r0 | (r1 << 64), ev


# ------------------------------------------------------------------ the lazy DIT transform

def _bit_reverse(x: Sequence[int]) -> List[int]:
    n = len(x)
    logn = n.bit_length() - 1
    out = [0] * n
    for k, v in enumerate(x):
        out[int(format(k, "0%db" % logn)[::-1], 2) if logn else 0] = v
    return out


def ntt_lazy(root: int, row: Sequence[int], limb_products: bool = True) -> Tuple[List[int], Events]:
    """The reference's radix-2 DIT graph (bit_reverse_copy, stage `size`, twiddle root^(k n/size),
    (e + w o, e - w o)) on the lazy butterfly: o = mont_mul(x, Montgomery(w)) is canonical,
    e + o and e - o stay in [0, 2^128), and the last stage is canonicalised.  Events carry a
    ``ntt:`` prefix.  `limb_products` = False takes the product from big-int arithmetic (no
    mont_mul events), for long rows."""
    n = len(row)
    assert n >= 1 and n & (n - 1) == 0 and all(0 <= v < P for v in row)
    ev: Events = set()
    x = _bit_reverse(row)
    pw = [1]
    for _ in range(n // 2 - 1):
        pw.append(pw[-1] * root % P)
    size = 1
    while size < n:
        size <<= 1
        half, step = size // 2, n // size
        for i in range(0, n, size):
            for k, j in enumerate(range(i, i + half)):
                w = pw[k * step]
                if limb_products:
                    o, e1 = mont_mul(x[j + half], w * R % P)
                    ev.update("ntt:" + s for s in e1)
                else:
                    o = x[j + half] * w % P
                e = x[j]
                x[j], e2 = fe_add_lazy(e, o)
                x[j + half], e3 = fe_sub_lazy(e, o)
                ev.update("ntt:" + s for s in e2)
                ev.update("ntt:" + s for s in e3)
    out = []
    for v in x:
        r, e4 = fe_canon(v)
        ev.update("ntt:" + s for s in e4)
        out.append(r)
    return out, ev
