"""GPU verifier (fri.rs:250-416 FRI::verify, stark.rs:565-770 Stark::verify) and its three device
evaluations against the CPU oracle: exact equality of every field value, flag, verdict and point
list; rejection texts are the reference's, of which the oracle's are prefixes."""
import pytest

import stark_oracle as o
import stark_prove_oracle as e
import starkgpu as sg

pytestmark = pytest.mark.gpu
P = o.P
B, C = sg.EVAL_BLOCK, sg.EVAL_CHUNK


@pytest.fixture(scope="module")
def fc():
    import fast_cpu
    fast_cpu.lib()
    return fast_cpu


# ------------------------------------------------------------------ evaluate_points

# 65 points: 0, 1, p - 1 and a duplicate first, so that every prefix the tests take is fixed
XS = [0, 1, P - 1, 12345, 12345] + o.synthetic_elements(7, b"verify-points", 60)
LENGTHS = [0, 1, 2, B - 1, B, B + 1, C - 1, C, C + 1, 2 * C + 3, (1 << 17) + 1]


def _coeffs(n):
    v = o.synthetic_elements(n, b"verify-coeffs", n)
    if n >= 1:
        v[-1] = P - 1
    if n >= 2:
        v[n // 2] = 0
    return v


@pytest.fixture(scope="module")
def eval_reference(fc):
    """{length: (coefficients, values at XS)} from the CPU checker's Horner (fast_cpu.eval_points)."""
    ref = {}
    for n in LENGTHS:
        c = _coeffs(n)
        ref[n] = (c, fc.ints(fc.eval_points(c, XS)) if n else [0] * len(XS))
    return ref


def test_eval_reference_agrees_with_python_oracle(eval_reference):
    for n in (0, 1, 2, B - 1, B, B + 1):
        c, want = eval_reference[n]
        assert want == [o.evaluate(c, x) for x in XS]


@pytest.mark.parametrize("nx", [1, 2, 64, 65])
def test_evaluate_points_every_length(eval_reference, nx):
    """Polynomial::evaluate of every length around the block (B) and chunk (C) sizes, all in one
    batch, at nx points (1, 2: below the points a lane holds; 64, 65: a whole and a ragged group)."""
    polys = [sg.Polynomial.new(eval_reference[n][0]) if n else sg.Polynomial.new([]) for n in LENGTHS]
    got = sg.evaluate_points(polys, XS[:nx])
    for n, g in zip(LENGTHS, got):
        assert g == eval_reference[n][1][:nx], "length %d at %d points" % (n, nx)


def test_evaluate_points_batch_of_three_from_lists(eval_reference):
    ns = (B + 1, 2 * C + 3, 2)
    got = sg.evaluate_points([eval_reference[n][0] for n in ns], XS)
    assert got == [eval_reference[n][1] for n in ns]


# ------------------------------------------------------------------ zerofier_geometric_at

@pytest.mark.parametrize("n", [0, 1, 2, B - 1, B, B + 1, C, C + 1, 65537])
def test_zerofier_geometric_at(fc, n):
    """prod_{r<n} (x - q^r), q of order 2^17; one x on the domain (q^5) gives 0 once n > 5."""
    q = o.primitive_nth_root(1 << 17)
    xs = XS[:40] + [o.fpow(q, 5)] + XS[40:64]
    got = sg.zerofier_geometric_at(q, n, xs)
    assert got == fc.geometric_prod(q, n, xs)
    assert (got[40] == 0) == (n > 5)
    if n <= 300:
        want = []
        for x in xs:
            acc, cur = 1, 1
            for _ in range(n):
                acc = acc * (x - cur) % P
                cur = cur * q % P
            want.append(acc)
        assert got == want


# ------------------------------------------------------------------ MerkleRoot.verify_batch

@pytest.fixture(scope="module")
def merkle_items():
    """257 honest (root, index, leaf, path) items over trees of 2, 4, 8 and 2^13 leaves (leaves
    include 0 and p - 1: 1 and 39 decimal digits): every index of the 8-leaf tree first, then the
    other trees in turn, so any slice of the list mixes depths."""
    trees = []
    for n in (2, 4, 8, 1 << 13):
        leaves = o.synthetic_elements(n, b"verify-leaves", n)
        leaves[0], leaves[-1] = 0, P - 1
        levels = o.merkle_levels(leaves)
        trees.append((leaves, levels, levels[-1][0]))
    items = []
    leaves, levels, root = trees[2]
    for i in range(8):
        items.append((root, i, leaves[i], o.merkle_open_levels(i, levels)))
    k = 0
    while len(items) < 257:
        leaves, levels, root = trees[k % 4]
        i = (k * 2654435761) % len(leaves) if k % 8 else (0 if k % 16 else len(leaves) - 1)
        items.append((root, i, leaves[i], o.merkle_open_levels(i, levels)))
        k += 1
    assert {len(it[3]) for it in items[:63]} == {1, 2, 3, 13}
    return items


def _batch(items):
    return sg.MerkleRoot.verify_batch([it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                                      [it[3] for it in items])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_merkle_verify_batch_honest(merkle_items, n):
    items = merkle_items[:n]
    assert _batch(items) == [True] * n
    assert all(o.merkle_verify(*[it[0], it[1], it[3], it[2]]) for it in items[:16])


def test_merkle_verify_batch_tampered_items(merkle_items):
    """A changed leaf, path node, root and a wrong index: exactly those items report 0, as
    MerkleRoot::verify (oracle and the library's host sg_merkle_verify) does item by item."""
    items = list(merkle_items[:65])

    def flip(b, at=0):
        return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]

    r, i, leaf, path = items[3]
    items[3] = (r, i, (leaf + 1) % P, path)
    r, i, leaf, path = items[20]
    items[20] = (r, i, leaf, path[:-1] + [flip(path[-1], 63)])
    r, i, leaf, path = items[41]
    items[41] = (flip(r, 17), i, leaf, path)
    r, i, leaf, path = items[64]
    items[64] = (r, i ^ 1, leaf, path)
    got = _batch(items)
    assert [k for k, ok in enumerate(got) if not ok] == [3, 20, 41, 64]
    assert got == [o.merkle_verify(r, i, path, leaf) for (r, i, leaf, path) in items]
    assert got == [sg.MerkleRoot.verify(r, i, path, leaf) for (r, i, leaf, path) in items]


def test_merkle_verify_batch_invalid_input_raises(merkle_items):
    r, i, leaf, path = merkle_items[0]
    with pytest.raises(sg.StarkGpuError):
        _batch([merkle_items[1], (r, i, leaf, [])])              # depth 0
    with pytest.raises(sg.StarkGpuError):
        _batch([(r, 1 << len(path), leaf, path), merkle_items[1]])  # index >= 2^depth


# ------------------------------------------------------------------ FRI.verify

def _native(objs, document=None):
    s = sg.IndependentProofStream() if document is None else sg.SignatureProofStream(document)
    for ob in objs:
        s.push(ob)
    return s


def _fri_setup(n, exp, c, seed, zero_third=False):
    omega = o.primitive_nth_root(n)
    coeffs = o.synthetic_elements(seed, b"verify-fri", n // exp)
    cw = o.fast_coset_evaluate(omega, n, o.GENERATOR, coeffs)
    if zero_third:  # fri.rs:514-528 (tests/test_gpu_parity.py test_fri_tampered_codeword_rejected)
        for i in range((n // exp - 1) // 3):
            cw[i] = 0
    gps = sg.IndependentProofStream()
    sg.FRI(o.GENERATOR, omega, n, exp, c).prove(cw, gps)
    return omega, gps.objects()


def _first(objs, code, k=0):
    return [i for i, ob in enumerate(objs) if ob[0] == code][k]


def _flip(b, at=5):
    return b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]


def _fri_tampers(objs):
    """name -> tampered object list."""
    out = {}
    i = _first(objs, o.CODEWORD)
    cwd = list(objs[i][1])
    cwd[1] = (cwd[1] + 1) % P
    out["last codeword element"] = objs[:i] + [(o.CODEWORD, cwd)] + objs[i + 1:]
    out["last root"] = objs[:i - 1] + [(o.ROOT, _flip(objs[i - 1][1]))] + objs[i:]
    i = _first(objs, o.LEAFS)
    ay, by, cy = objs[i][1]
    out["ay"] = objs[:i] + [(o.LEAFS, ((ay + 1) % P, by, cy))] + objs[i + 1:]
    out["cy"] = objs[:i] + [(o.LEAFS, (ay, by, (cy + 1) % P))] + objs[i + 1:]
    for k, name in enumerate(("aa", "bb", "cc")):
        i = _first(objs, o.PATH, k)
        path = list(objs[i][1])
        path[len(path) // 2] = _flip(path[len(path) // 2])
        out["path " + name] = objs[:i] + [(o.PATH, path)] + objs[i + 1:]
    return out


FRI_SHAPES = [(256, 4, 17), (1 << 13, 8, 16)]  # fri.rs:450-531 (degree 63); __graft_entry__.smoke()'s


@pytest.fixture(scope="module")
def fri_cases():
    """[(name, oracle (ok, err, points), GPU (ok, err, points))] over both shapes: the honest proof,
    the stream tampers and the low-degree violation."""
    rows = []
    for (n, exp, c) in FRI_SHAPES:
        omega, objs = _fri_setup(n, exp, c, n)
        cases = {"honest": objs}
        cases.update(_fri_tampers(objs))
        cases["low-degree violation"] = _fri_setup(n, exp, c, n, zero_third=True)[1]
        for name, ob in cases.items():
            want = o.FRI(o.GENERATOR, omega, n, exp, c).verify(o.IndependentProofStream(ob))
            got = sg.FRI(o.GENERATOR, omega, n, exp, c).verify(_native(ob))
            rows.append(("%d/%s" % (n, name), want, got))
    return rows


def test_fri_verify_honest_equals_oracle(fri_cases):
    for name, want, got in fri_cases:
        if name.endswith("honest"):
            assert want[0] and got == want, name
            assert len(got[2]) == 2 * dict((n, c) for n, _, c in FRI_SHAPES)[int(name.split("/")[0])]


def test_fri_verify_tampers_equal_oracle(fri_cases):
    seen = 0
    for name, want, got in fri_cases:
        if not name.endswith("honest"):
            assert not want[0], name + ": the tamper no longer bites the oracle"
            assert got[0] == want[0] and got[1].startswith(want[1]) and want[1], (name, want[1], got[1])
            assert got[2] == want[2], name  # the points read before the rejection
            seen += 1
    assert seen == 2 * 8


def test_fri_verify_path_messages_name_the_opening(fri_cases):
    got = {name.split("/")[1]: g[1] for name, _, g in fri_cases if name.startswith("256/path")}
    assert got == {"path " + k: "Merkle auth path verification failed for " + k for k in ("aa", "bb", "cc")}


def test_fri_verify_truncated_stream():
    """A changed cy with the stream cut after the first round's objects still reports the
    colinearity failure (the reference never reads further); the honest stream cut there raises."""
    n, exp, c = FRI_SHAPES[1]
    omega, objs = _fri_setup(n, exp, c, n)
    fri_o, fri_g = o.FRI(o.GENERATOR, omega, n, exp, c), sg.FRI(o.GENERATOR, omega, n, exp, c)
    rounds = fri_o.num_rounds()
    assert rounds > 2
    cut = rounds + 1 + 4 * c
    assert objs[cut][0] == o.LEAFS and objs[cut - 1][0] == o.PATH and len(objs) > cut
    bad = _fri_tampers(objs)["cy"][:cut]
    want = fri_o.verify(o.IndependentProofStream(bad))
    got = fri_g.verify(_native(bad))
    assert want[:2] == (False, "colinearity check failure") and got == want
    with pytest.raises(sg.StarkGpuError, match="Cannot pull"):
        fri_g.verify(_native(objs[:cut]))
    with pytest.raises(AssertionError):
        fri_o.verify(o.IndependentProofStream(objs[:cut]))
    # a failing path before the cut wins over running out of objects after it
    bad = _fri_tampers(objs)["path bb"][:cut]
    assert fri_g.verify(_native(bad))[:2] == (False, "Merkle auth path verification failed for bb")


def test_fri_verify_wrong_kind_raises():
    n, exp, c = FRI_SHAPES[0]
    omega, objs = _fri_setup(n, exp, c, n)
    with pytest.raises(sg.StarkGpuError, match="expected StarkProofStreamEnum to be Root"):
        sg.FRI(o.GENERATOR, omega, n, exp, c).verify(_native([(o.VALUE, 3)] + objs))
    i = _first(objs, o.CODEWORD)
    with pytest.raises(sg.StarkGpuError) as ei:
        sg.FRI(o.GENERATOR, omega, n, exp, c).verify(_native(objs[:i] + [(o.CODEWORD, [P] + objs[i][1][1:])] + objs[i + 1:]))
    assert ei.value.code == -3  # SG_ERR_NONCANONICAL


# ------------------------------------------------------------------ Stark.verify

STARK_SHAPES = [(27, 4, 2, 2, 2), (27, 8, 4, 8, 3), (40, 4, 3, 4, 2), (9, 16, 2, 4, 4)]


def _stark_case(N, exp, c, sec, tcd, ctx=None, m=2):
    """As tests/test_gpu_stark.py's _case: oracle and GPU objects of one Rescue-Prime statement and
    the GPU's proof objects."""
    seed = b"case-%d" % N
    rp_o, rp_g = e.RescuePrime(m, 1, sec, N), sg.RescuePrime(m, 1, sec, N, ctx=ctx)
    st_o, st_g = e.Stark(exp, c, sec, m, N + 1, tcd), sg.Stark(exp, c, sec, m, N + 1, tcd, ctx=ctx)
    air_o = rp_o.transition_constraints(st_o.omicron, st_o.omicron_domain_length)
    air_g = rp_g.transition_constraints(st_g.omicron, st_g.omicron_domain_length)
    inp = o.sample(seed)
    out = rp_o.hash(inp)
    r = e.randomness_from_seed(seed, m * st_o.num_randomizers + st_o.num_randomizer_coefficients(air_o))
    tr = [r[m * i:m * i + m] for i in range(st_o.num_randomizers)]
    gps = sg.IndependentProofStream()
    st_g.prove(rp_o.trace(inp), air_g, rp_o.boundary_constraints(out), gps, tr, r[m * st_o.num_randomizers:])
    return rp_o, st_o, st_g, air_o, air_g, out, gps.objects()


def _both(st_o, st_g, air_o, air_g, bnd, objs):
    return st_o.verify(air_o, bnd, o.IndependentProofStream(objs)), st_g.verify(air_g, bnd, _native(objs))


def _same_verdict(want, got):
    return got[0] == want[0] and (got[1] == want[1] if want[0] else bool(want[1]) and got[1].startswith(want[1]))


@pytest.mark.parametrize("shape", STARK_SHAPES)
def test_stark_verify_honest_equals_oracle(shape):
    """The verdict on the GPU's own proof equals the oracle's -- also where the transition degree is
    too small for alpha = 3 (max_degree >= the omicron order: the reference's products wrap) and
    the reference rejects the honest prover's bytes."""
    rp_o, st_o, st_g, air_o, air_g, out, objs = _stark_case(*shape)
    want, got = _both(st_o, st_g, air_o, air_g, rp_o.boundary_constraints(out), objs)
    assert want[0] == (st_o.max_degree(air_o) < st_o.omicron_domain_length)
    assert _same_verdict(want, got), (want, got)


@pytest.fixture(scope="module")
def stark_cases():
    """[(name, oracle (ok, err), GPU (ok, err))] on (27, 8, 4, 8, 3): the false claim and the tail
    tampers.  After the FRI part each of the m + 1 trees contributes 4c (Value, Path) pairs; the
    positions are found by walking the kinds."""
    rp_o, st_o, st_g, air_o, air_g, out, objs = _stark_case(*STARK_SHAPES[1])
    m, c = 2, STARK_SHAPES[1][2]
    bnd = rp_o.boundary_constraints(out)
    values = [i for i, ob in enumerate(objs) if ob[0] == o.VALUE]
    assert len(values) == (m + 1) * 4 * c and values[0] > 0
    assert all(objs[i + 1][0] == o.PATH for i in values) and values[-1] == len(objs) - 2

    def with_value(i):
        return objs[:i] + [(o.VALUE, (objs[i][1] + 1) % P)] + objs[i + 1:]

    def with_path(i):
        path = list(objs[i][1])
        path[0] = _flip(path[0])
        return objs[:i] + [(o.PATH, path)] + objs[i + 1:]

    cases = {
        "honest": (bnd, objs),
        "false claim": (rp_o.boundary_constraints(o.add_mod(out, 1)), objs),
        "bq value": (bnd, with_value(values[0])),
        "bq path": (bnd, with_path(values[0] + 1)),
        "randomizer value": (bnd, with_value(values[m * 4 * c])),
        "randomizer path": (bnd, with_path(values[m * 4 * c] + 1)),
        "bq root": (bnd, [(o.ROOT, _flip(objs[0][1]))] + objs[1:]),
        # a tamper inside the FRI part comes back with the reference's prefix
        "fri tamper inside stark": (bnd, objs[:m + 1] + _fri_tampers(objs[m + 1:values[0]])["cy"] + objs[values[0]:]),
    }
    rows = []
    for name, (b, ob) in cases.items():
        want, got = _both(st_o, st_g, air_o, air_g, b, ob)
        rows.append((name, want, got))
    return rows


def test_stark_verify_tampers_equal_oracle(stark_cases):
    for name, want, got in stark_cases:
        assert want[0] == (name == "honest"), name + ": " + want[1]
        assert _same_verdict(want, got), (name, want, got)
    got = {name: g[1] for name, _, g in stark_cases}
    assert got["fri tamper inside stark"] == "FRI verification failed: colinearity check failure"
    assert got["bq value"].startswith("Boundary quotient root ") and got["bq value"].endswith(" is not verified")
    assert got["randomizer path"].startswith("Randomizer leaf ") and got["randomizer path"].endswith(" not verified")


def test_oracle_messages_cover_every_check(fri_cases, stark_cases):
    """Asserted about the ORACLE's outputs, so that a tamper that stops biting is noticed."""
    msgs = [w[1] for _, w, _ in fri_cases] + [w[1] for _, w, _ in stark_cases]
    for text in ("last codeword is not well formed", "colinearity check failure",
                 "Merkle auth path verification failed", "Boundary quotient root", "Randomizer leaf",
                 "Combination doesn't match"):
        assert any(text in msg for msg in msgs), text


def test_stark_verify_structural_problems():
    rp_o, st_o, st_g, air_o, air_g, out, objs = _stark_case(*STARK_SHAPES[0])
    bnd = rp_o.boundary_constraints(out)
    assert st_g.verify(air_g, bnd, _native(objs)) == (True, "")
    with pytest.raises(sg.StarkGpuError, match="boundary is empty"):
        st_g.verify(air_g, [], _native(objs))
    with pytest.raises(sg.StarkGpuError, match="Cannot pull"):
        st_g.verify(air_g, bnd, _native(objs[:-1]))
    with pytest.raises(sg.StarkGpuError, match="to be Root"):
        st_g.verify(air_g, bnd, _native(objs[3:]))
    # a rejection that comes first in the reference's order is not turned into an error by a
    # structural problem after it: a bad first opening, and the stream's end missing
    first = _first(objs, o.VALUE)
    bad = objs[:first] + [(o.VALUE, (objs[first][1] + 1) % P)] + objs[first + 1:-1]
    ok, err = st_g.verify(air_g, bnd, _native(bad))
    assert not ok and err.startswith("Boundary quotient root ")


# ------------------------------------------------------------------ larger and cross-path cases

def test_stark_verify_midsize(fc):
    """tests/midsize_case.py (T = 1257, FRI 2^15, c = 64) with sg-built constraints: the GPU's proof
    is accepted and the false claim rejected, as by the oracle's verifier over the AIR's structure
    (fast_cpu.verifier_stark + rescue_air_at_point, as tests/test_gpu_fullsize.py)."""
    import midsize_case as M
    rp_o, st_o, trace, bnd, tr, rc = M.light_inputs()
    rp_g = sg.RescuePrime(*M.RESCUE)
    st_g = sg.Stark(M.EXPANSION, M.CHECKS, M.SECURITY, rp_g.m, M.RESCUE[3] + 1, M.TCD)
    air_g = rp_g.transition_constraints(st_g.omicron, st_g.omicron_domain_length)
    gps = sg.IndependentProofStream()
    st_g.prove(trace, air_g, bnd, gps, tr, rc)
    objs = gps.objects()
    false_bnd = list(bnd[:-1]) + [(bnd[-1][0], bnd[-1][1], o.add_mod(bnd[-1][2], 1))]
    vst = fc.verifier_stark(M.EXPANSION, M.CHECKS, M.SECURITY, rp_o.m, M.RESCUE[3] + 1, M.TCD)
    sair = fc.rescue_air_at_point(rp_o, vst.omicron)
    for b, accepted in ((bnd, True), (false_bnd, False)):
        want = vst.verify(sair, b, o.IndependentProofStream(objs))
        got = st_g.verify(air_g, b, _native(objs))
        assert want[0] == accepted and _same_verdict(want, got), (want, got)


def test_stark_verify_rpsss_signature():
    """The reference's published RPSSS configuration (tests/rpsss_case.py, rpsss.rs:103-131): the
    GPU's signature verifies for its document through a SignatureProofStream and is rejected for
    the forged document -- the verdicts of the oracle's RPSSS::verify."""
    import rpsss_case as R
    c = R.Case()
    rp_g = sg.RescuePrime(*R.RESCUE)
    st_g = sg.Stark(R.EXPANSION, R.CHECKS, R.SECURITY, rp_g.m, R.RESCUE[3] + 1, R.TCD)
    air_g = rp_g.transition_constraints(st_g.omicron, st_g.omicron_domain_length)
    sps = sg.SignatureProofStream(R.DOCUMENT)
    sig = st_g.prove(c.trace, air_g, c.boundary, sps, c.trace_randomizers, c.randomizer_coefficients)
    assert len(sig) == R.PROOF_LEN
    objs = sps.objects()
    for doc, accepted in ((R.DOCUMENT, True), (R.FORGED, False)):
        want = c.oracle_verify(doc, sig)
        got = st_g.verify(air_g, c.boundary, _native(objs, document=doc))
        assert want[0] == accepted and _same_verdict(want, got), (doc, want, got)


def test_verify_device_option_gives_identical_results():
    """Context option verify_device = 0 (plain host loops for the three evaluations) against 1, on
    a fresh context: identical (ok, err, points) for an honest and a tampered FRI proof, identical
    (ok, err) for a STARK proof and a false claim."""
    ctx = sg.Context(0)
    n, exp, c = FRI_SHAPES[1]
    omega, objs = _fri_setup(n, exp, c, n)
    fri = sg.FRI(o.GENERATOR, omega, n, exp, c, ctx=ctx)
    rp_o, st_o, st_g, air_o, air_g, out, sobjs = _stark_case(*STARK_SHAPES[1], ctx=ctx)
    bnd = rp_o.boundary_constraints(out)
    results = {}
    for dev in (1, 0):
        ctx.set_option("verify_device", dev)
        results[dev] = [fri.verify(_native(objs)), fri.verify(_native(_fri_tampers(objs)["path cc"])),
                        fri.verify(_native(_fri_tampers(objs)["ay"])),
                        st_g.verify(air_g, bnd, _native(sobjs)),
                        st_g.verify(air_g, rp_o.boundary_constraints(o.add_mod(out, 1)), _native(sobjs))]
        xs = XS[:5]
        results[dev].append(sg.evaluate_points([_coeffs(B + 1), _coeffs(3)], xs, ctx=ctx))
        results[dev].append(sg.zerofier_geometric_at(o.primitive_nth_root(1 << 10), B + 1, xs, ctx=ctx))
    assert results[0] == results[1]
    assert [r[0] for r in results[1][:5]] == [True, False, False, True, False]
    assert results[1][0] == o.FRI(o.GENERATOR, omega, n, exp, c).verify(o.IndependentProofStream(objs))


def test_verify_through_callback_stream_equals_native():
    """Verifying an oracle IndependentProofStream through CallbackProofStream's pull side equals
    verifying the native stream, for FRI and for the STARK."""
    n, exp, c = FRI_SHAPES[0]
    omega, objs = _fri_setup(n, exp, c, n)
    fri = sg.FRI(o.GENERATOR, omega, n, exp, c)
    for ob in (objs, _fri_tampers(objs)["path aa"]):
        assert fri.verify(o.IndependentProofStream(ob)) == fri.verify(_native(ob))
    rp_o, st_o, st_g, air_o, air_g, out, sobjs = _stark_case(*STARK_SHAPES[3])
    bnd = rp_o.boundary_constraints(out)
    assert st_g.verify(air_g, bnd, o.IndependentProofStream(sobjs)) == st_g.verify(air_g, bnd, _native(sobjs)) == (True, "")
    # an exhausted Python stream raises the stream's own error
    with pytest.raises(AssertionError, match="Cannot pull"):
        fri.verify(o.IndependentProofStream(objs[:-1]))
