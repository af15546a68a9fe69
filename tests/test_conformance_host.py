"""CPU leg of the device conformance suite (tests/device_conformance.py).

(a) tests/device/conformance.hip cross-compiles for gfx950 with the product's flags, so a break of the device form shows
    here, without a GPU.
(b) The same op bodies, built by g++ with -DTC_BOUND_CHECK (the host Fq2 form), run THE SAME case tables as the GPU leg
    against the same big-integer references and output contracts, with every input slot's declared interval loaded into
    the interval bookkeeping: this proves that the operands lie inside the input contract and that the encoder and the
    references are right before any GPU time is spent.  Each op runs in a child process: a bound violation aborts it.
"""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import device_conformance as dc  # noqa: E402


def test_conformance_kernels_cross_compile_for_gfx950():
    lib = dc.build_device()
    assert os.path.getsize(lib) > 0


@pytest.fixture(scope="module")
def host_lib():
    return dc.build_host()


@pytest.mark.parametrize("op", sorted(dc.SPECS, key=lambda k: dc.OPS[k]))
def test_case_table_under_the_bound_analysis(host_lib, op):
    r = subprocess.run([sys.executable, os.path.join(HERE, "device_conformance.py"), "host", op], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])


def test_every_op_has_a_case_table():
    """Every op of conformance.h has a table, and every table holds its directed edges plus random cases."""
    import re
    with open(os.path.join(HERE, "device", "conformance.h")) as f:
        src = f.read()
    enum = re.search(r"enum Op \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r"\b([A-Z][A-Z0-9_]+)\b(?:\s*=\s*(\d+))?", re.sub(r"//[^\n]*", "", enum))
    ids, nxt = {}, 0
    for name, val in names:
        nxt = int(val) if val else nxt
        ids[name] = nxt
        nxt += 1
    assert ids == dc.OPS
    assert set(dc.SPECS) == set(dc.OPS)


def test_encoder_hits_the_declared_limits():
    """encode() returns v R + k p with limbs at the interval ends it was asked for, and refuses what breaks the contract."""
    import random
    rnd = random.Random(3)
    for k in (-300, -1, 0, 1, 299):
        for push, iv in (("hi", (-7.9, 7.9)), ("lo", (-7.9, 7.9)), ("alt", (-2.85, 2.85)), (None, (0.0, 1.0))):
            if push is None and k:
                continue
            v = rnd.randrange(dc.P)
            op = dc.encode(v, k, iv, push)
            assert dc.value(op.limbs) == dc.mont(v) + k * dc.P and dc.residue(op.limbs) == v
            if push == "hi":
                assert max(op.limbs[:13]) > (iv[1] - 1) * 2 ** 28
            if push == "lo":
                assert min(op.limbs[:13]) < (iv[0] + 1) * 2 ** 28
    with pytest.raises(AssertionError):
        dc.encode(5, 300, (-7.9, 7.9))  # value above 300 p
    with pytest.raises(AssertionError):
        dc.encode(5, 0, (-8.5, 8.5))  # limb interval beyond 7.9 * 2^28
    with pytest.raises(AssertionError):
        dc.check_product_operands(dc.encode(1, 0, (-3.0, 3.0)), dc.encode(1, 0, (-3.0, 3.0)))


def test_div_by_x_abs_table_takes_both_outcomes():
    """DIV_BY_X_ABS: a Python model of div_by_x_abs classifies the table's divisions.  Both reachable outcomes occur (no
    correction; the first correction, r > q0), and the model agrees with divmod on each.  The second correction
    (r >= |x|) cannot fire for this |x|: U / |x| exceeds the reciprocal's estimate q / 2^64 by less than 1 (exact bound)."""
    seen = {}
    for c in dc.table("DIV_BY_X_ABS"):
        q, r, c1, c2 = dc.div_by_x_abs_model(c.u1, c.u0)
        assert (q, r) == divmod((c.u1 << 64) | c.u0, dc.X), c.tag
        seen[(c1, c2)] = seen.get((c1, c2), 0) + 1
    assert seen.get((False, False), 0) > 0 and seen.get((True, False), 0) > 0, seen
    assert dc.div_second_correction_bound() < 1
    assert not any(c2 for c1, c2 in seen)


@pytest.mark.parametrize("op", sorted(dc.LAYOUTS, key=lambda k: dc.OPS[k]))
def test_wave_layout_of_per_wave_decisions(op):
    """Ops whose device form decides once per wave: the table opens with one full wave per path (every lane takes it),
    and later waves mix the paths.  n = 1, a partial wave and one wave still run (sizes).  A wave holds 64 jobs of a
    one-lane op and 32 of a lane-pair op."""
    path_of, makers = dc.LAYOUTS[op]
    cases = dc.table(op)
    wave = 64 // dc.lanes(op)
    waves = [cases[k:k + wave] for k in range(0, len(cases), wave)]
    for w, p in zip(waves, makers):
        assert len(w) == wave and all(path_of(c) == p for c in w), (op, p)
    mixed = [w for w in waves[len(makers):] if len({path_of(c) for c in w}) > 1]
    assert len(mixed) >= 2, op
    assert {path_of(c) for w in mixed for c in w} >= set(makers)
    assert len(cases) % wave and dc.sizes(op, len(cases))[:3] == [1, wave // 2 + 3, wave]
    assert [1, wave // 2 + 3, wave] == ([1, 35, 64] if dc.lanes(op) == 1 else [1, 19, 32])


def test_point_multiplication_models_agree_with_the_oracle():
    """The path models of the point-multiplication block walk the ladders on the oracle's group law.  Their results equal
    E.mul / E.add (so the walk is the ladder the routine runs), psi on the whole curve is [x] on G2, and the models see
    the special cases they are there to see: a generic case is not special, a case built on an exception is."""
    import random
    o = dc.o
    rnd = random.Random(11)
    p, q = dc.g2_point(rnd), dc.curve_point(dc.G2F, rnd)
    assert dc.psi(p) == dc._psi_ref(p) and dc.psi(q) != dc._psi_ref(q) and o.E2.on_curve(dc.psi(q))
    for E, fld in ((o.E1, dc.G1F), (o.E2, dc.G2F)):
        a = dc._pt(fld, rnd)
        assert dc.ladder_uniform_model(E, a, dc.X, 63) == (E.mul(a, dc.X), False)
        for s in dc.small_points(fld):
            assert dc.ladder_uniform_model(E, s, dc.X, 63)[0] == E.mul(s, dc.X)
        assert dc.ladder_uniform_model(E, None, dc.X, 63) == (None, True)
    assert dc.ladder_uniform_model(o.E1, (0, 2), dc.X, 63)[1]  # order 3: 2 P = -P, the first addition is P = -Q
    for k in (0, 1, 2, dc.R - 1, rnd.randrange(dc.R), 2 * rnd.randrange(dc.R // 2)):
        r, special = dc.mul_gls_model(p, k)
        assert r == o.E2.mul(p, k) and special == (k == 0), hex(k)  # (k = 0 runs as r: the last addition is P = -Q)
    bases = [dc.g2_point(rnd) for _ in range(4)]
    for d in ([5, 7, 9, 11], [4, 7, 0, 11], [rnd.getrandbits(64) for _ in range(4)]):
        want = None
        for b, x in zip(bases, d):
            want = o.E2.add(want, o.E2.mul(b, x))
        assert dc.joint_mul4_model(bases, d)[0] == want and dc.joint_mul4_model(bases, d)[2] == (d[0] % 2 == 0)
    assert dc.joint_mul4_model([bases[0], o.E2.neg(bases[0])] + bases[2:], [3, 1, 0, 0])[1]
    for fix in (True, False):
        assert dc.clear_cofactor_model(q, fix) == (o.E2.mul(q, dc.H2 if fix else dc.CLEAR_NOFIX), False)
        assert dc.clear_cofactor_model(dc.small_points(dc.G2F)[0], fix) == (None, True)
    pts = [dc.g1_point(rnd) for _ in range(3)]
    cs = [rnd.getrandbits(40), 3, 1 << 62]
    want = None
    for b, x in zip(pts, cs):
        want = o.E1.add(want, o.E1.mul(b, x))
    assert dc.straus_model(o.E1, pts, cs, 64) == (want, False)
    assert dc.straus_model(o.E1, [pts[0], o.E1.neg(pts[0])], [3, 3], 64) == (None, True)
    assert dc.straus_model(o.E1, pts, [0, 0, 0], 64) == (None, False)


def test_point_multiplication_tables_hold_every_path():
    """Every op of the point-multiplication block with a per-wave decision: the Python model finds cases of every path it
    knows among the DIRECTED cases or the table, and the block's tables hold the edges the routines turn on."""
    new = [op for op in dc.LAYOUTS if dc.OPS["G1_ADD_AFFINE"] <= dc.OPS[op] < dc.BYTE_OPS_FROM]
    assert len(new) == 13
    for op in new:
        path_of, makers = dc.LAYOUTS[op]
        cases = dc.table(op)
        seen = {}
        for c in cases:
            seen[path_of(c)] = seen.get(path_of(c), 0) + 1
        assert set(seen) == set(makers) and min(seen.values()) >= 64 // dc.lanes(op), (op, seen)
    assert set(dc.NEEDS_TABLE) <= set(dc.OPS) and all(dc.lanes(op) == (1 if op.startswith("G1") else 2) for op in dc.OPS if 140 <= dc.OPS[op] < dc.BYTE_OPS_FROM)
    # combine_divide: D = 1, every 2^a (a = 1 .. 16), 2^17, odd, >= 2^32, near 2^62, each with both signs, and Q = O
    for op in ("G1_COMBINE_DIVIDE", "G1_COMBINE_DIVIDE_ARENA", "G2_COMBINE_DIVIDE"):
        ds = {(c.d, c.neg) for c in dc.table(op)}
        for d in [1, 3, 1 << 17, (1 << 32) + 15, (1 << 62) - 1] + [1 << a for a in range(1, 17)]:
            assert (d, False) in ds and (d, True) in ds, (op, d)
        assert any(c.p is None for c in dc.table(op))
    # g2_joint_mul4 / g2_mul_gls: even and odd d0 / k, zero digits, the largest digits
    ds = [c.d for c in dc.table("G2_JOINT_MUL4")]
    assert any(d[0] % 2 for d in ds) and any(d[0] % 2 == 0 for d in ds) and any(d[1:] == [0, 0, 0] for d in ds)
    ks = {c.k for c in dc.table("G2_MUL_GLS")}
    assert ks >= set(dc.MUL_SCALARS) and any(max(dc.gls_digits(k)[:3]) == dc.X - 1 for k in ks)
    # straus_small: all zero, a single one, a 63-bit coefficient beside tiny ones, for K = 2, 3, 4
    for K in (2, 3, 4):
        cs = [c.cs for c in dc.table("G2_STRAUS_SMALL") if len(c.cs) == K]
        assert [0] * K in cs and [1] + [0] * (K - 1) in cs and any(max(c) >> 62 and min(c) < 16 for c in cs)
    xs = {dc.words_value(c.slots[3]) & dc.M64 for c in dc.table("G1_MUL_U64")}
    assert xs >= {0, 1, 1 << 63, dc.M64}


def test_combine_quotient_decompose_table_takes_both_branches():
    """COMBINE_QUOTIENT_DECOMPOSE: a Python model of the routine classifies the table's denominators.  The bit-by-bit 128-bit
    path of udiv_u128_u64 and the plain 64-bit divide both occur, and so do both signs of the rounding's numerator; the
    model keeps the routine's promise on each D it takes.  The directed list holds what the issue names: every generic
    ten-signer denominator (28 of the 4-subsets, the largest 189; 18 of the 3-subsets; 5 of the 2-subsets), every power of
    two, the ends of the range and the denominators around |x|."""
    assert [len(dc.ten_signer_denominators(K)) for K in (2, 3, 4)] == [5, 18, 28] and max(dc.ten_signer_denominators(4)) == 189
    ds = {c.v for c in dc.table("COMBINE_QUOTIENT_DECOMPOSE")}
    assert ds >= set(dc.TEN_DS) | set(range(8)) | {1 << a for a in range(63)} | {dc.X - 1, dc.X, dc.X + 1, (1 << 62) - 1, (1 << 62) + 1}
    assert ds >= set(dc.QUOTIENT_DS) <= {c.v for c in dc.table("COMBINE_DIVIDE_CHOICE")}
    seen = {}
    for d in sorted(ds):
        m = dc.quotient_decompose_model(d)
        assert (m is not None) == (3 <= d < 1 << 62 and d & (d - 1) != 0), d
        if m is None:
            continue
        q, T, E, wide, negative = m
        assert q == dc.X // d >= 3 and all(2 * abs(t) <= d for t in T) and all(2 * abs(e) <= d + 4 for e in E), d
        assert d * dc.quotient_scalar(q, T, E) % dc.R == 1, d
        seen[(wide, negative)] = seen.get((wide, negative), 0) + 1
    assert {w for w, _ in seen} == {False, True} and {n for _, n in seen} == {False, True}, seen
    # the choice: small denominators take the quotient form, long ones keep the 4-dimensional ladder
    assert dc.takes_quotient_model(35) and not dc.takes_quotient_model(81000000) and not dc.takes_quotient_model(1 << 20)


def _blocks(cases):
    return [cases[k:k + dc.WAVE_JOBS] for k in range(0, len(cases), dc.WAVE_JOBS)]


@pytest.mark.parametrize("op", sorted(dc.UNIFORM, key=lambda k: dc.OPS[k]))
def test_wave_layout_of_uniform_ops(op):
    """Ops whose routine reads its parameters from the wave's first lane: every aligned block of 32 jobs shares the key, the
    table ends in a ragged block (so the prefixes sizes() launches stay uniform: lanes past the end copy the last job), one
    block is special on all 32 jobs, one on none, at least two mix them, and a special case stands at lane-pair position 0
    and at position 31 of a mixed block."""
    key_of, special_of = dc.UNIFORM[op]
    cases = dc.table(op)
    blocks = _blocks(cases)
    assert len(cases) % dc.WAVE_JOBS != 0 and dc.sizes(op, len(cases)) == [1, 19, 32, len(cases)]
    assert op in dc.NEEDS_TABLE and dc.lanes(op) == 2
    for b in blocks:
        assert len({key_of(c) for c in b}) == 1, (op, b[0].tag)
    sp = [[bool(special_of(c)) for c in b] for b in blocks if len(b) == dc.WAVE_JOBS]
    assert any(all(s) for s in sp) and any(not any(s) for s in sp), op
    mixed = [s for s in sp if any(s) and not all(s)]
    assert len(mixed) >= 2 and any(s[0] for s in mixed) and any(s[31] for s in mixed) and any(any(s[1:31]) for s in mixed), op
    assert any(not s[0] for s in mixed) and any(not s[31] for s in mixed), op


def test_wave_layout_of_the_combine_job():
    """JOB_COMBINE_SMALL_G2 and the parameters of its neighbours: the waves (a) to (e) of the job body are what they are meant to
    be, and the uniform ops run the classes, denominators and coefficient tuples the issue names."""
    blocks = _blocks(dc.table("JOB_COMBINE_SMALL_G2"))
    assert len(blocks[-1]) < dc.WAVE_JOBS
    by = {b[0].wave: b for b in blocks}
    assert all(len({c.wave for c in b}) == 1 for b in blocks)
    for K in (2, 3, 4):  # (a) one tuple, every job on the fast path
        b = by["a%d" % K]
        assert len({tuple(c.ids) for c in b}) == 1 and len(b[0].ids) == K and not any(dc.combine_leaves_early(c) for c in b)
    assert len({tuple(c.ids) for c in by["b"]}) == dc.WAVE_JOBS and not any(dc.combine_leaves_early(c) for c in by["b"])
    ids = [tuple(c.ids) for c in by["c"]]
    assert len(set(ids)) == 2 and sorted(ids.count(t) for t in set(ids)) == [1, 31] and not any(dc.combine_leaves_early(c) for c in by["c"])
    kinds = set()
    for k in range(3):  # (d) the leaver is job 0: the first lane still there is job 1
        b = by["d first %d" % k]
        assert [dc.combine_leaves_early(c) for c in b] == [True] + [False] * 31
        kinds.add(b[0].kind)
    assert kinds == {"index 65535", "undecodable share", "duplicate index"}
    assert [dc.combine_leaves_early(c) for c in by["d last"]] == [False] * 30 + [True, True]
    assert [dc.combine_leaves_early(c) for c in by["d every other"]] == [True, False] * 16
    assert {c.kind for c in by["d every other"]} >= kinds
    for b in (by["d last"], by["d every other"]):  # the jobs that stay hold one tuple
        assert len({tuple(c.ids) for c in b if not dc.combine_leaves_early(c)}) == 1
    e = by["e"]
    assert {e[0].kind, e[31].kind} == {"share at infinity"} and "two equal shares" in {c.kind for c in e} and "ordinary" in {c.kind for c in e}
    assert len({tuple(c.ids) for c in e}) == 1
    # combine_uniform_wave: D = 1, a power of two, a D that takes the quotient form and one that does not, both signs
    cs = dc.table("G2_COMBINE_UNIFORM_WAVE")
    classes = {(dc.combine_class(c.d) if dc.combine_class(c.d) != "generic" else "quotient" if dc.takes_quotient_model(c.d) else "ladder", c.neg)
               for c in cs}
    assert classes == {(k, n) for k in ("one", "pow2", "quotient", "ladder") for n in (False, True)}
    assert any(c.d == 81000000 for c in cs) and {len(c.cs) for c in cs} == {2, 3, 4}
    # both [1 / D] forms run every ten-signer denominator and the long ones; the quotient form also the D it refuses
    for op in ("G2_COMBINE_DIVIDE_UNIFORM", "G2_COMBINE_DIVIDE_QUOTIENT"):
        assert {c.d for c in dc.table(op)} >= set(dc.DIVIDE_UNIFORM_DS) >= set(dc.TEN_DS) | {5720, (1 << 62) - 57}
    assert {c.d for c in dc.table("G2_COMBINE_DIVIDE_QUOTIENT")} >= {1, 2, 4, 1 << 20}
    # straus_small_uniform: the coefficient tuples per K, and the related points of the mid-ladder exceptions
    for K in (2, 3, 4):
        keys = {tuple(c.cs) for c in dc.table("G2_STRAUS_SMALL_UNIFORM") if len(c.cs) == K}
        big = (1 << 63) - 1
        assert keys >= {(0,) * K, (1,) + (0,) * (K - 1), (0,) * (K - 1) + (1,), (1,) * K, (3, 1) + (0,) * (K - 2), (big,) * K}
        assert any(max(k) == 1 << 62 and min(k) < 4 for k in keys) and tuple(dc.ten_signer_tuples(K)[0][1]) in keys
    assert [max(dc.ten_signer_tuples(K)[0][1]).bit_length() for K in (2, 3, 4)] == [4, 7, 9]  # (the 9-bit coefficients: K = 4)
    # g2_quotient_mul: what no denominator reaches
    qk = {c.key for c in dc.table("G2_QUOTIENT_MUL")}
    assert any(not any(T) for _, T, _ in qk) and any(not any(E) for _, _, E in qk) and {q for q, _, _ in qk} >= {3, (1 << 63) + 1, dc.M64}
    assert {T for _, T, _ in qk} >= {tuple(s if j == k else 0 for j in range(4)) for k in range(4) for s in (1, -1)}
    assert any(min(T) == -(1 << 61) and min(E) == -(1 << 61) for _, T, E in qk)
    assert any(dc.wnaf_model(q, dc.QUOT_WIDTH)[64] and max(E) >> 62 for q, _, E in qk)  # a digit in column 64, E bits in column 63
    assert any(max(abs(e) for e in E).bit_length() > q.bit_length() for q, _, E in qk)  # E longer than q
    # g2_wnaf_table: E'(Fq2) has no point of order 3, 5 or 7, so the operand of order three lies on another curve of j = 0
    assert all(dc.H2 % l for l in (3, 5, 7))
    tags = {c.tag for c in dc.table("G2_WNAF_TABLE")}
    assert {"P = O", "order two", "order three", "order seven", "order 13", "outside G2", "ordinary"} <= tags
    p7 = dc.order_seven_point()
    assert p7 is not None and dc.o.E2.mul(p7, 7) is None and not any(n % 5 == 0 for n in dc.j0_curve_orders())


def test_uniform_models_agree_with_the_oracle():
    """The three ladder models of the uniform ops return E.mul or the sum on generic input and flag nothing there; they flag the
    constructed exceptions; and quotient_mul_model fed with a Python decomposition of D is [1 / D] Q for every ten-signer D."""
    import random
    o = dc.o
    E = o.E2
    rnd = random.Random(17)
    p, q, r = dc.g2_pool()[:3]
    # straus_uniform_model
    cs = [rnd.getrandbits(40), 3, (1 << 63) - 1]
    want = None
    for b, x in zip((p, q, r), cs):
        want = E.add(want, E.mul(b, x))
    assert dc.straus_uniform_model(E, [p, q, r], cs) == (want, False)
    assert dc.straus_uniform_model(E, [p, q], [0, 0]) == (None, False)
    assert dc.straus_uniform_model(E, [None, q], [0, 5]) == (E.mul(q, 5), False)  # (a base that is never taken)
    assert dc.straus_uniform_model(E, [None, q], [1, 5])[1] and dc.straus_uniform_model(E, [q, None], [8, 1])[1]
    p3, p2 = E.mul(p, 3), E.dbl(p)
    for pts, c in (([p, p3], [3, 1]), ([p, E.neg(p3)], [3, 1]), ([p, p2], [2, 1]), ([p, E.neg(p2)], [2, 1]), ([p, p2], [4, 2]),
                   ([p, E.neg(p2)], [4, 2]), ([p, p], [1, 1]), ([p, E.neg(p)], [1, 1])):
        assert dc.straus_uniform_model(E, pts, c)[1], c
        assert not dc.straus_uniform_model(E, [p, q], c)[1], c
    assert not dc.straus_uniform_model(E, [p, p3], [2, 1])[1] and not dc.straus_uniform_model(E, [p, p2], [3, 1])[1]
    # wnaf_ladder_model and quotient_mul_model: [1 / D] Q on G2, for every ten-signer denominator
    for d in dc.TEN_DS + [65521, (1 << 62) - 57]:
        want = E.mul(q, pow(d, -1, dc.R))
        qq, T, Ec = dc.quotient_decompose_model(d)[:3]
        assert dc.quotient_mul_model(q, qq, T, Ec) == (want, False), d
        if d in dc.TEN_DS[::5] + [65521]:
            assert dc.wnaf_ladder_model(q, d) == (want, False), d
    assert dc.wnaf_ladder_model(None, 35) == (None, True) and dc.quotient_mul_model(None, 3, [1, 0, 0, 0], [0, 1, 0, 0])[1]
    assert dc.quotient_mul_model(q, 9, [0, 0, 0, 0], [1, 0, 0, 0])[1]  # T = 0: no first ladder
    assert dc.quotient_mul_model(q, 9, [1, 0, 0, 0], [0, 0, 0, 0]) == (E.mul(q, 9), False)
    assert dc.quotient_mul_model(q, 9, [1, 0, 0, 0], [9, 0, 0, 0])[1]  # the top digit of q starts acc = P1 = P, and E adds P in that column
    # outside G2 the two forms are different maps: psi is not [x] there
    c = dc.curve_pool()[0]
    qq, T, Ec = dc.quotient_decompose_model(35)[:3]
    assert dc.wnaf_ladder_model(c, 35)[0] != dc.quotient_mul_model(c, qq, T, Ec)[0]
    # the recodings
    for v in (0, 1, 7, dc.X, dc.M64, rnd.getrandbits(64)):
        for W in (3, 4):
            assert sum(m << i for i, m in enumerate(dc.wnaf_model(v, W))) == v
        pos, neg = dc.naf_model(v >> 1)
        assert pos - neg == v >> 1 and not pos & neg


def test_miller_reference_model_agrees_with_the_oracle():
    """dev_miller_loop -- the product's step formulas on residues, the exact reference of MILLER_LOOP2, MILLER_LINES and
    Q_MILLER_LOOP -- differs from the oracle's Miller loop by a factor in Fq2 (and with a conjugation dropped it would
    not), gives the same pairing after the final exponentiation, and is 1 for an empty product.  Its lines are Fq2
    multiples of the oracle's, step by step."""
    import random
    o = dc.o
    rnd = random.Random(5)
    p0, q0, p1, q1 = dc.g1_point(rnd), dc.g2_point(rnd), dc.g1_point(rnd), dc.g2_point(rnd)
    f = dc.dev_miller_loop([(p0, q0), (p1, q1)])
    g = o.miller_loop([(p0, q0), (p1, q1)])
    assert dc.f12_is_fq2(o.f12_mul(f, o.f12_inv(g))) and not dc.f12_is_fq2(f)
    assert not dc.f12_is_fq2(o.f12_mul(o.f12_conj(f), o.f12_inv(g)))
    assert o.final_exponentiation_chain(f) == o.final_exponentiation_chain(g)
    assert dc.dev_miller_loop([(None, q0), (p1, None)]) == o.F12_ONE
    assert all(dc.f2_multiple(a, b) for a, b in zip(dc.dev_scaled_lines(p0, q0), dc.oracle_scaled_lines(p0, q0)))


def test_pairing_tables_mix_skip_patterns_and_quad_sizes():
    """The Miller-loop tables hold every skip pattern (pair 0, pair 1, both, none), and the first wave already mixes all
    four (skip is per-lane data that miller_apply_lines branches on).  Quad ops run four lanes per job: 16 per wave."""
    for op in ("MILLER_LOOP2", "MILLER_LINES", "Q_MILLER_LOOP"):
        cases = dc.table(op)
        wave = 64 // dc.lanes(op)
        assert {dc._skip_of(c.pts) for c in cases[:wave]} == {(a, b) for a in (False, True) for b in (False, True)}, op
    assert [dc.lanes(op) for op in ("MILLER_LOOP2", "FINAL_EXP", "Q_MILLER_LOOP", "Q_PAIRING_CHECK")] == [2, 2, 4, 4]
    n = len(dc.table("Q_FINAL_EXP"))
    assert n % 16 and dc.sizes("Q_FINAL_EXP", n)[:3] == [1, 11, 16]
