"""GPU parity of the DKG resharing: tc_g1_weighted_sum_batch, tc_fr_weighted_sum_batch and tc_dkg_reshare_batch (`Poly * Fr`
src/poly.rs:210-254, Commitment::add_assign :462-471, the finalisation :870-876 and :895-898 with the Lagrange coefficients of
src/lib.rs:719-767) vs Oracle A.  Byte-exact, no tolerance anywhere.

Shapes: 70 outputs are more than one wave and no multiple of 64; n = 5 leaves most lanes of a 64-lane output with nothing, n = 67
gives most of them one term.  The test points are [a] g1 for known scalars a (tc_g1_commitment_batch; tests/test_gpu_dkg.py checks
it against the oracle), so what a weighted sum should be is ONE oracle multiplication per output: (sum_k w_k a_kj mod r) g1.  Every
sum runs with the default choice of lanes per output, with TC_SUM_PARTS = 1, 4 and 64, and with forced slices per output of the
weighted G1 sum (TC_WSUM_SLICES = 3 at 4 lanes, 5 at 64 lanes, 64 at one lane): the bytes must not depend on any of it."""
import contextlib
import random

import numpy as np
import pytest

import tc_oracle as o
from threshold_crypto_amd import _native, api
from threshold_crypto_amd.poly import BivarCommitment, BivarPoly, Commitment, Poly, ShareMismatch, dkg_generate, dkg_reshare

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
IDENT = bytes([0x40]) + bytes(95)
OK, NOT_ENOUGH, DUPLICATE, INVALID, MISMATCH = 0, 1, 2, 3, 4


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def fr(v):
    return u8(int(v).to_bytes(32, "little"))


def frs(vals):
    return np.stack([fr(v) for v in vals])


def ints(a):
    return [int.from_bytes(bytes(r), "little") for r in a]


def gen_mul(k):
    k %= o.R
    return IDENT if k == 0 else o.g1_uncompressed(o.E1.mul(o.G1_GEN, k))


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.copy()).to(torch.device("cuda:0"))


def off_curve_g1(rnd):
    while True:
        x, y = rnd.randrange(o.Q), rnd.randrange(o.Q)
        if (y * y - x * x * x - 4) % o.Q:
            return x.to_bytes(48, "big") + y.to_bytes(48, "big")


def non_member_g1(rnd):
    """an on-curve point of E(Fq) outside the order-r subgroup"""
    while True:
        x = rnd.randrange(o.Q)
        y2 = (x * x * x + 4) % o.Q
        y = pow(y2, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == y2 and o.E1.mul((x, y), o.R) is not None:
            return o.g1_uncompressed((x, y))


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0x5E5B)


@pytest.fixture(scope="module")
def engines(engine):
    """the session context (the default rule for the lanes per output), one context per forced TC_SUM_PARTS, and three that
    also force the slices per output of the weighted G1 sum (TC_WSUM_SLICES): 3 slices of 4 lanes (uneven slices, and empty
    lanes at n = 5), 5 slices of 64 lanes, and one lane per slice with as many slices as the context takes.  tc_ctx_create reads
    TC_WSUM_SLICES = 1 .. 64 and leaves anything else to the default rule, so 1000 is the default rule (one slice at one lane per
    output) and 64 is the largest forced value: g1_wsum_slices clamps it to n, one term per slice at n = 5"""
    from conftest import engine_with_env
    forced = [dict(TC_SUM_PARTS=p) for p in (1, 4, 64)]
    forced += [dict(TC_SUM_PARTS=4, TC_WSUM_SLICES=3), dict(TC_SUM_PARTS=64, TC_WSUM_SLICES=5), dict(TC_SUM_PARTS=1, TC_WSUM_SLICES=1000),
               dict(TC_SUM_PARTS=1, TC_WSUM_SLICES=64)]
    with contextlib.ExitStack() as stack:
        yield [engine] + [stack.enter_context(engine_with_env(**env)) for env in forced]


@pytest.fixture(scope="module")
def unchecked(engines):
    """input checks off on every context (the test points are the library's own outputs), whatever an earlier test left"""
    was = [e.input_checks() for e in engines]
    for e in engines:
        e.set_input_checks(False)
    yield engines
    for e, w in zip(engines, was):
        e.set_input_checks(w)


def known_points(engine, rnd, n, B):
    """scalars a (n x B lists) and the points [a_kj] g1 as an (n, B, 96) array"""
    a = [[rnd.randrange(o.R) for _ in range(B)] for _ in range(n)]
    out, st = engine.g1_commitment(frs([v for row in a for v in row]))
    assert not st.any()
    return a, out.reshape(n, B, 96)


def wsums(engines, pts, weights, mask=None):
    """the call on every context: the outputs must be the same bytes; returns them once"""
    res = [e.g1_weighted_sum(pts, weights, mask) for e in engines]
    for out, st in res[1:]:
        assert (out == res[0][0]).all() and (st == res[0][1]).all()
    return [bytes(p) for p in res[0][0]], res[0][1].tolist()


# ---- 1. the primitives -------------------------------------------------------------------------------------------------------
def test_weighted_sum_small_against_the_oracle(unchecked, rnd):
    """3 outputs x 5 terms, every product and every addition by the oracle's E1.mul / E1.add"""
    n, B = 5, 3
    a, pts = known_points(unchecked[0], rnd, n, B)
    w = [rnd.randrange(o.R) for _ in range(n)]
    w[1], w[3] = 0, o.R - 1
    want = []
    for j in range(B):
        acc = None
        for k in range(n):
            P = o.g1_from_uncompressed(bytes(pts[k, j]), check=False)
            acc = o.E1.add(acc, o.E1.mul(P, w[k]) if w[k] else None)
        want.append(IDENT if acc is None else o.g1_uncompressed(acc))
    got, st = wsums(unchecked, pts, frs(w))
    assert st == [OK] * B and got == want


@pytest.mark.parametrize("n", [5, 67])
def test_weighted_sum_seventy_outputs(unchecked, rnd, n):
    B = 70
    a, pts = known_points(unchecked[0], rnd, n, B)
    w = [rnd.randrange(o.R) for _ in range(n)]
    want = [gen_mul(sum(w[k] * a[k][j] for k in range(n))) for j in range(B)]
    got, st = wsums(unchecked, pts, frs(w))
    assert st == [OK] * B and got == want
    # a mask; an excluded term may be garbage with a garbage weight
    mask = np.ones(n, dtype=np.uint8)
    mask[[1, n - 1]] = 0
    spoiled, w2 = pts.copy(), frs(w)
    spoiled[1, 3] = u8(off_curve_g1(rnd))
    spoiled[n - 1] = 0xA5
    w2[1] = fr(2 ** 256 - 1)
    want_m = [gen_mul(sum(w[k] * a[k][j] for k in range(n) if mask[k])) for j in range(B)]
    got, st = wsums(unchecked, spoiled, w2, mask)
    assert st == [OK] * B and got == want_m
    # the same bad term included fails its own output; the non-canonical weight included fails every output
    mask[1] = 1
    got, st = wsums(unchecked, spoiled, frs(w), mask)
    assert st == [INVALID if j == 3 else OK for j in range(B)] and got[3] == IDENT and got[4] != IDENT
    got, st = wsums(unchecked, pts, w2, mask)
    assert st == [INVALID] * B and got == [IDENT] * B
    # the Fr twin over the same scalars, host and device I/O
    e = unchecked[0]
    vals = np.stack([frs(row) for row in a])
    mask[1] = 0
    want_fr = [sum(w[k] * a[k][j] for k in range(n) if mask[k]) % o.R for j in range(B)]
    out, st = e.fr_weighted_sum(vals, frs(w), mask)
    assert not st.any() and ints(out) == want_fr
    out, st = e.fr_weighted_sum(to_dev(vals), to_dev(frs(w)), to_dev(mask))
    e.sync()
    assert not st.cpu().numpy().any() and ints(out.cpu().numpy()) == want_fr
    out, st = e.fr_weighted_sum(vals, w2, mask)                          # the bad weight is masked out ...
    assert not st.any() and ints(out) == want_fr
    out, st = e.fr_weighted_sum(vals, w2)                                # ... and included
    assert st.tolist() == [INVALID] * B and not out.any()
    # device I/O of the G1 sum
    import torch
    t_pts, t_w, t_mask = to_dev(pts), to_dev(frs(w)), to_dev(mask)
    torch.cuda.synchronize()
    for e in unchecked:
        out, st = e.g1_weighted_sum(t_pts, t_w, t_mask)
        e.sync()
        assert not st.cpu().numpy().any() and [bytes(p) for p in out.cpu().numpy()] == want_m
    out, st = unchecked[0].g1_weighted_sum(pts, frs(w), mask)            # and back in host-I/O mode
    assert not st.any() and [bytes(p) for p in out] == want_m


def test_weighted_sum_equal_and_opposite_products(unchecked, rnd):
    """w_a P_a = +-w_b P_b for different points: the complete addition inside a lane and in the tree"""
    n, B = 6, 4
    a, pts = known_points(unchecked[0], rnd, n, B)
    w = [rnd.randrange(1, o.R) for _ in range(n)]
    for j in range(B):                                                   # per output the products of terms 0/1 and 2/5 collide
        a[1][j] = (1 if j % 2 == 0 else -1) * w[0] * a[0][j] * pow(w[1], -1, o.R) % o.R
        a[5][j] = (-1 if j % 2 == 0 else 1) * w[2] * a[2][j] * pow(w[5], -1, o.R) % o.R
    out, st = unchecked[0].g1_commitment(frs([v for row in a for v in row]))
    assert not st.any()
    pts = out.reshape(n, B, 96)
    got, st = wsums(unchecked, pts, frs(w))
    assert st == [OK] * B and got == [gen_mul(sum(w[k] * a[k][j] for k in range(n))) for j in range(B)]
    got, st = wsums(unchecked, pts[[0, 1]], frs(w[:2]))
    assert got[1] == IDENT and got[3] == IDENT and got[0] == gen_mul(2 * w[0] * a[0][0])


def test_weighted_sum_checked_mode_and_empty(engines, rnd):
    n, B = 5, 70
    a, pts = known_points(engines[0], rnd, n, B)
    w = [rnd.randrange(o.R) for _ in range(n)]
    spoiled = pts.copy()
    spoiled[2, 9] = u8(non_member_g1(rnd))
    without = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    want = [gen_mul(sum(w[k] * a[k][j] for k in range(n))) for j in range(B)]
    want_wo = [gen_mul(sum(w[k] * a[k][j] for k in range(n) if without[k])) for j in range(B)]
    was = [e.input_checks() for e in engines]
    try:
        for e in engines:
            e.set_input_checks(True)
        got, st = wsums(engines, spoiled, frs(w))                        # an included non-member fails only its own output
        assert st == [INVALID if j == 9 else OK for j in range(B)]
        assert got == [IDENT if j == 9 else want[j] for j in range(B)]
        got, st = wsums(engines, spoiled, frs(w), without)               # the same point masked out fails nothing
        assert st == [OK] * B and got == want_wo
    finally:
        for e, x in zip(engines, was):
            e.set_input_checks(x)
    e = engines[0]
    out, st = e.g1_weighted_sum(np.zeros((0, B, 96), dtype=np.uint8), np.zeros((0, 32), dtype=np.uint8))      # n = 0
    assert not st.any() and [bytes(p) for p in out] == [IDENT] * B
    out, st = e.g1_weighted_sum(pts, frs(w), np.zeros(n, dtype=np.uint8))
    assert not st.any() and [bytes(p) for p in out] == [IDENT] * B
    out, st = e.g1_weighted_sum(pts, frs([0] * n))
    assert not st.any() and [bytes(p) for p in out] == [IDENT] * B


def test_weighted_sum_is_the_lincomb_composition(unchecked, rnd):
    """what the library offered before: tc_g1_lincomb_batch on gathered points with the weights replicated per output, 68 x 68"""
    n = B = 68
    a, pts = known_points(unchecked[0], rnd, n, B)
    w = frs([rnd.randrange(o.R) for _ in range(n)])
    got, st = wsums(unchecked, pts, w)
    assert st == [OK] * B
    out, st = unchecked[0].lincomb_g1(np.ascontiguousarray(np.broadcast_to(w[None], (B, n, 32))), np.ascontiguousarray(pts.transpose(1, 0, 2)))
    assert not st.any() and [bytes(p) for p in out] == got


# ---- 2. tc_dkg_reshare_batch ---------------------------------------------------------------------------------------------------
def lagrange_at_zero(idx):
    xs = [(i + 1) % o.R for i in idx]
    lam = []
    for a, xa in enumerate(xs):
        num = den = 1
        for b, xb in enumerate(xs):
            if b != a:
                num = num * xb % o.R
                den = den * (xb - xa) % o.R
        lam.append(num * pow(den, -1, o.R) % o.R)
    return lam


class Scene:
    """an old key set of degree t_old, P dealers (old nodes dealer_idx) dealing polynomials of the new degree, and what node `node`
    of the new set received: n_v samples of every dealer's row"""

    def __init__(self, engine, rnd, t_old, dealer_idx, degree, node=3, n_v=None):
        self.t_old, self.degree, self.idx, self.node = t_old, degree, list(dealer_idx), node
        self.P = len(self.idx)
        self.f = [rnd.randrange(o.R) for _ in range(t_old + 1)]
        nco = (degree + 1) * (degree + 2) // 2
        self.coeffs = [[o.poly_evaluate(self.f, i + 1)] + [rnd.randrange(o.R) for _ in range(nco - 1)] for i in self.idx]
        out, st = engine.g1_commitment(frs(self.f + [c for cs in self.coeffs for c in cs]))
        assert not st.any()
        self.old_commit = out[:t_old + 1].copy()
        self.commits = out[t_old + 1:].reshape(self.P, nco, 96).copy()
        self.dealer_idx = np.array(self.idx, dtype=np.uint64)
        n_v = degree + 1 if n_v is None else n_v
        self.xs = np.array([rnd.sample(range(1, 200), n_v) for _ in range(self.P)], dtype=np.uint64)
        self.vals = self.samples_of(node)

    def samples_of(self, m):
        return np.stack([frs([o.bivar_poly_evaluate(self.degree, cs, m, int(x)) for x in self.xs[p]]) for p, cs in enumerate(self.coeffs)])

    def expect(self, accept, m=None):
        """(used, the new commitment's scalars, node m's share) by the rule of the issue"""
        m = self.node if m is None else m
        S = [p for p in range(self.P) if accept is None or accept[p]][:self.t_old + 1]
        lam = lagrange_at_zero([self.idx[p] for p in S])
        col = [sum(l * self.coeffs[p][o.coeff_pos(i, 0)] for l, p in zip(lam, S)) % o.R for i in range(self.degree + 1)]
        share = sum(l * o.bivar_poly_evaluate(self.degree, self.coeffs[p], m, 0) for l, p in zip(lam, S)) % o.R
        return [1 if p in S else 0 for p in range(self.P)], col, share

    def run(self, e, accept=None, **over):
        a = dict(old_commit=self.old_commit, dealer_idx=self.dealer_idx, commits=self.commits, xs=self.xs, vals=self.vals)
        a.update(over)
        out, share, used, st, status = e.dkg_reshare(a["old_commit"], a["dealer_idx"], a["commits"], self.degree, accept, a["xs"], a["vals"])
        return [bytes(p) for p in out], (None if share is None else int.from_bytes(bytes(share), "little")), used.tolist(), st.tolist(), int(status[0])

    def guarded(self, res, code, part_status):
        out, share, used, st, status = res
        assert status == code and st == part_status and used == [0] * self.P
        assert out == [IDENT] * (self.degree + 1) and share in (0, None)


@pytest.mark.parametrize("degree,nodes", [(3, 7), (1, 4)])
def test_reshare_grow_and_shrink(engines, rnd, degree, nodes):
    """t_old = 2, five dealers of which one is rejected and holds garbage, to degree 3 with 7 new nodes and to degree 1 with 4"""
    s = Scene(engines[0], rnd, 2, [4, 0, 6, 2, 1], degree)
    accept = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
    commits = s.commits.copy()
    commits[1] = 0xA5
    used, col, _ = s.expect(accept)
    assert used == [1, 0, 1, 1, 0]                                        # exactly the first three accepted parts
    want_commit = [gen_mul(c) for c in col]
    assert col[0] == s.f[0] and want_commit[0] == bytes(s.old_commit[0])  # the master key does not move
    shares = {}
    was = engines[0].input_checks()
    try:
        for m in range(1, nodes + 1):
            vals = s.samples_of(m)
            for checks in ((False, True) if m == 1 else (False,)):
                engines[0].set_input_checks(checks)
                for e in (engines if m == 1 else engines[:1]):
                    out, share, u, st, status = s.run(e, accept, commits=commits, vals=vals)
                    assert (status, st, u) == (OK, [OK] * 5, used) and out == want_commit
                    assert share == s.expect(accept, m)[2]
            shares[m] = share
    finally:
        engines[0].set_input_checks(was)
    e = engines[0]
    new_commit = np.stack([u8(c) for c in want_commit])
    pks, st = e.public_key_shares(new_commit, np.array([m - 1 for m in shares], dtype=np.uint64))
    assert not st.any() and [bytes(p) for p in pks] == [gen_mul(v) for v in shares.values()]      # share * g1 == out_commit.evaluate(m)
    for pick in ([1, 2, 3, 4, 5, 6, 7][:degree + 1], list(range(nodes, 0, -1))[:degree + 1]):     # any degree+1 new shares give f(0)
        assert o.poly_interpolate([(m, shares[m]) for m in pick])[0] == s.f[0]


def test_reshare_smallest_and_seventy_dealers(engines, rnd):
    s = Scene(engines[0], rnd, 0, [5], 0)                                 # t_old = 0, degree = 0: one dealer hands the key on as it is
    out, share, used, st, status = s.run(engines[0])
    assert (status, st, used) == (OK, [OK], [1]) and out == [bytes(s.old_commit[0])] and share == s.f[0]
    idx = list(range(70))
    rnd.shuffle(idx)
    s = Scene(engines[0], rnd, 66, idx, 2)                                # 70 dealers, 67 of them used
    accept = np.ones(70, dtype=np.uint8)
    accept[[3, 65]] = 0
    used, col, share_w = s.expect(accept)
    assert sum(used) == 67 and col[0] == s.f[0]
    for e in engines:
        out, share, u, st, status = s.run(e, accept)
        assert (status, u, share) == (OK, used, share_w) and not any(st) and out == [gen_mul(c) for c in col]


def test_reshare_too_few_accepted_parts(engine, rnd):
    s = Scene(engine, rnd, 2, [4, 0, 6, 2], 1)
    s.guarded(s.run(engine, np.array([1, 0, 1, 0], dtype=np.uint8)), NOT_ENOUGH, [OK] * 4)
    assert s.run(engine, np.array([1, 0, 1, 1], dtype=np.uint8))[4] == OK


@pytest.mark.parametrize("where", [1, 4])
def test_reshare_wrong_constant_inside_and_outside_the_selection(engine, rnd, where):
    """part 1 is in S, part 4 is not: the blame and the guarded outputs are the same"""
    s = Scene(engine, rnd, 2, [4, 0, 6, 2, 1], 2)
    commits = s.commits.copy()
    commits[where, 0] = u8(gen_mul(s.coeffs[where][0] + 1))
    s.guarded(s.run(engine, commits=commits), MISMATCH, [MISMATCH if p == where else OK for p in range(5)])
    accept = np.ones(5, dtype=np.uint8)
    accept[where] = 0                                                     # the same part rejected: never read
    assert s.run(engine, accept, commits=commits)[3:] == ([OK] * 5, OK)


def test_reshare_claimed_and_repeated_dealer_indices(engine, rnd):
    s = Scene(engine, rnd, 2, [4, 0, 6, 2, 1], 2)
    idx = s.dealer_idx.copy()
    idx[2] = 3                                                            # old node 6 claims to be node 3: its constant is node 6's
    s.guarded(s.run(engine, dealer_idx=idx), MISMATCH, [OK, OK, MISMATCH, OK, OK])
    idx = s.dealer_idx.copy()
    idx[3] = 4                                                            # ... claims an index an earlier part holds
    s.guarded(s.run(engine, dealer_idx=idx), DUPLICATE, [OK, OK, OK, DUPLICATE, OK])
    # the honest repeat: the same old node deals twice, both parts consistent
    s2 = Scene(engine, rnd, 1, [4, 0, 4], 1)
    s2.guarded(s2.run(engine), DUPLICATE, [OK, OK, DUPLICATE])
    assert s2.run(engine, np.array([1, 1, 0], dtype=np.uint8))[4] == OK   # a rejected part's index is nobody's duplicate
    assert s2.run(engine, np.array([0, 1, 1], dtype=np.uint8))[4] == OK


def test_reshare_bad_points_values_and_abscissae(engine, rnd):
    s = Scene(engine, rnd, 1, [4, 0, 6, 2], 2)
    was = engine.input_checks()
    try:
        for checks in (False, True):
            engine.set_input_checks(checks)
            commits = s.commits.copy()
            commits[3, o.coeff_pos(2, 0)] = u8(off_curve_g1(rnd))         # an undecodable first-column point, outside S
            s.guarded(s.run(engine, commits=commits), INVALID, [OK, OK, OK, INVALID])
            commits = s.commits.copy()
            commits[0, 0] = u8(off_curve_g1(rnd))                         # ... and the constant itself
            s.guarded(s.run(engine, commits=commits), INVALID, [INVALID, OK, OK, OK])
            other = s.commits.copy()
            other[3, o.coeff_pos(1, 2)] = u8(off_curve_g1(rnd))           # a point OUTSIDE the first column is not this entry's business
            assert s.run(engine, commits=other)[3:] == ([OK] * 4, OK)
            vals = s.vals.copy()
            vals[2, 1] = fr(o.R)                                          # a non-canonical value
            s.guarded(s.run(engine, vals=vals), INVALID, [OK, OK, INVALID, OK])
            xs = s.xs.copy()
            xs[1, 2] = xs[1, 0]                                           # a repeated abscissa
            s.guarded(s.run(engine, xs=xs), DUPLICATE, [OK, DUPLICATE, OK, OK])
            member = s.commits.copy()
            member[2, o.coeff_pos(1, 0)] = u8(non_member_g1(rnd))         # on the curve, outside G1
            res = s.run(engine, commits=member)
            if checks:
                s.guarded(res, INVALID, [OK, OK, INVALID, OK])
            else:
                assert INVALID not in res[3] and res[4] != INVALID        # checks off: the same call runs, nothing is INVALID_ENCODING
    finally:
        engine.set_input_checks(was)


def test_reshare_bad_old_commitment(engine, rnd):
    s = Scene(engine, rnd, 2, [4, 0, 6, 2], 1)
    was = engine.input_checks()
    try:
        for checks in (False, True):
            engine.set_input_checks(checks)
            old = s.old_commit.copy()
            old[1] = u8(off_curve_g1(rnd))
            s.guarded(s.run(engine, old_commit=old), INVALID, [OK] * 4)
            commits = s.commits.copy()
            commits[1, 0] = u8(off_curve_g1(rnd))                         # ... whatever else is wrong: every part stays OK
            s.guarded(s.run(engine, old_commit=old, commits=commits), INVALID, [OK] * 4)
            s.guarded(s.run(engine, np.zeros(4, dtype=np.uint8), old_commit=old), INVALID, [OK] * 4)
            old = s.old_commit.copy()
            old[2] = u8(non_member_g1(rnd))
            res = s.run(engine, old_commit=old)
            if checks:
                s.guarded(res, INVALID, [OK] * 4)
            else:
                assert res[4] != INVALID
    finally:
        engine.set_input_checks(was)


def test_reshare_precedence_when_two_faults_meet(engine, rnd):
    s = Scene(engine, rnd, 1, [4, 0, 4, 2], 2)                            # part 2 repeats part 0's index
    s.guarded(s.run(engine), DUPLICATE, [OK, OK, DUPLICATE, OK])
    commits = s.commits.copy()
    commits[2, 0] = u8(gen_mul(5))                                        # a repeated index AND a wrong constant: DUPLICATE_ENTRY
    s.guarded(s.run(engine, commits=commits), DUPLICATE, [OK, OK, DUPLICATE, OK])
    commits[2, o.coeff_pos(1, 0)] = u8(off_curve_g1(rnd))                 # ... AND a bad point: INVALID_ENCODING
    s.guarded(s.run(engine, commits=commits), INVALID, [OK, OK, INVALID, OK])
    xs, commits = s.xs.copy(), s.commits.copy()
    xs[3, 1] = xs[3, 0]
    commits[3, 0] = u8(gen_mul(5))                                        # a repeated abscissa AND a wrong constant
    commits[1, 0] = u8(gen_mul(6))                                        # the call's status is the FIRST failed part's code
    s.guarded(s.run(engine, xs=xs, commits=commits), MISMATCH, [OK, MISMATCH, DUPLICATE, DUPLICATE])
    vals = s.vals.copy()
    vals[3, 0] = fr(2 ** 256 - 1)                                         # a non-canonical value beats the repeated abscissa
    s.guarded(s.run(engine, xs=xs, vals=vals), DUPLICATE, [OK, OK, DUPLICATE, INVALID])


def test_reshare_modes(engine, rnd):
    s = Scene(engine, rnd, 2, [4, 0, 6, 2, 1], 3)
    accept = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    used, col, share_w = s.expect(accept)
    want = [gen_mul(c) for c in col]
    host = s.run(engine, accept)
    assert host == (want, share_w, used, [OK] * 5, OK)
    out, share, u, st, status = engine.dkg_reshare(s.old_commit, s.dealer_idx, s.commits, s.degree, accept)        # an observer
    assert share is None and [bytes(p) for p in out] == want and u.tolist() == used and int(status[0]) == OK
    out, share, u, st, status = engine.dkg_reshare(to_dev(s.old_commit), to_dev(s.dealer_idx), to_dev(s.commits), s.degree, to_dev(accept),
                                                   to_dev(s.xs), to_dev(s.vals))                                 # device I/O
    engine.sync()
    assert [bytes(p) for p in out.cpu().numpy()] == want and int.from_bytes(bytes(share.cpu().numpy()), "little") == share_w
    assert u.cpu().tolist() == used and st.cpu().tolist() == [OK] * 5 and status.cpu().tolist() == [OK]
    commits = s.commits.copy()
    commits[4, 0] = u8(gen_mul(7))
    out, share, u, st, status = engine.dkg_reshare(to_dev(s.old_commit), to_dev(s.dealer_idx), to_dev(commits), s.degree, to_dev(accept),
                                                   to_dev(s.xs), to_dev(s.vals))                                 # the guard, device I/O
    engine.sync()
    assert [bytes(p) for p in out.cpu().numpy()] == [IDENT] * 4 and not share.cpu().numpy().any() and not u.cpu().numpy().any()
    assert st.cpu().tolist() == [OK, OK, OK, OK, MISMATCH] and status.cpu().tolist() == [MISMATCH]
    assert s.run(engine, accept) == host                                                                         # and back in host-I/O mode


def test_reshare_null_arguments_and_zero_sizes(engine):
    lib, ctx = engine._lib, engine._ctx
    buf = np.zeros(8192, dtype=np.uint8)
    p = buf.ctypes.data
    engine._mode(buf)                                                    # host-I/O mode
    bad, ok = _native.TC_ERR_INVALID_ARG, _native.TC_OK
    assert lib.tc_g1_weighted_sum_batch(ctx, None, 96, 2, p, None, 1, p, p) == bad
    assert lib.tc_g1_weighted_sum_batch(ctx, p, 96, 2, None, None, 1, p, p) == bad
    assert lib.tc_g1_weighted_sum_batch(ctx, p, 96, 2, p, None, 1, None, p) == bad
    assert lib.tc_g1_weighted_sum_batch(ctx, p, 95, 2, p, None, 1, p, p) == bad
    assert lib.tc_g1_weighted_sum_batch(ctx, p, 96, 2, p, None, 2, p, p) == bad
    assert lib.tc_fr_weighted_sum_batch(ctx, None, 32, 2, p, None, 1, p, p) == bad
    assert lib.tc_fr_weighted_sum_batch(ctx, p, 32, 2, None, None, 1, p, p) == bad
    assert lib.tc_fr_weighted_sum_batch(ctx, p, 32, 2, p, None, 1, None, p) == bad
    assert lib.tc_fr_weighted_sum_batch(ctx, p, 48, 2, p, None, 1, p, p) == bad
    reshare = lib.tc_dkg_reshare_batch
    assert reshare(ctx, None, 0, p, p, 96, 0, 1, None, None, None, 0, p, None, p, p, p) == bad
    assert reshare(ctx, p, 0, None, p, 96, 0, 1, None, None, None, 0, p, None, p, p, p) == bad
    assert reshare(ctx, p, 0, p, None, 96, 0, 1, None, None, None, 0, p, None, p, p, p) == bad
    assert reshare(ctx, p, 0, p, p, 0, 0, 1, None, None, None, 0, p, None, p, p, p) == bad
    assert reshare(ctx, p, 0, p, p, 96, 0, 1, None, None, p, 2, p, p, p, p, p) == bad          # a share needs its samples
    assert reshare(ctx, p, 0, p, p, 96, 0, 1, None, p, None, 2, p, p, p, p, p) == bad
    buf[:] = 0x77
    assert lib.tc_g1_weighted_sum_batch(ctx, None, 0, 0, None, None, 0, None, None) == ok       # B = 0 / P = 0: nothing is written
    assert lib.tc_fr_weighted_sum_batch(ctx, None, 0, 0, None, None, 0, None, None) == ok
    assert reshare(ctx, None, 0, None, None, 0, 0, 0, None, None, None, 0, p, p, p, p, p) == ok
    assert (buf == 0x77).all()
    assert lib.tc_g1_weighted_sum_batch(ctx, None, 0, 0, None, None, 2, p, None) == ok          # n = 0: identities; status is optional
    assert bytes(buf[:192]) == IDENT * 2 and buf[192] == 0x77
    assert lib.tc_fr_weighted_sum_batch(ctx, None, 0, 0, None, None, 2, p, p + 64) == ok
    assert not buf[:66].any()


# ---- 3. poly.dkg_reshare --------------------------------------------------------------------------------------------------------
def test_reshare_after_distributed_key_generation(engine, rnd):
    """the shape of the reference's `distributed_key_generation` test (src/poly.rs:866-899: 3 dealers, 5 nodes, degree 2), then four of
    the five nodes hand the key to a new set of 4 nodes with threshold 1: a signature combined from the NEW shares verifies under
    the OLD master key"""
    api.set_default_engine(engine)
    dealer_num, node_num, faulty_num = 3, 5, 2
    ncoef = (faulty_num + 1) * (faulty_num + 2) // 2
    bi_polys = [BivarPoly(faulty_num, [rnd.randrange(o.R) for _ in range(ncoef)]) for _ in range(dealer_num)]
    bi_commits = [bp.commitment() for bp in bi_polys]
    old_commit, old_shares = None, {}
    for m in range(1, node_num + 1):
        old_commit, old_shares[m - 1] = dkg_generate(bi_commits, None, [{i: bp.evaluate(m, i) for i in (1, 2, 4)} for bp in bi_polys])
    old_pk = api.PublicKeySet(old_commit.coeff, _trusted=True).public_key()
    # old nodes 4, 0, 2 and 1 deal; the first three are combined
    dealers, new_t, new_nodes = [4, 0, 2, 1], 1, 4
    parts = [BivarPoly.random_with_constant(new_t, old_shares[i], rnd) for i in dealers]
    assert all(bp.evaluate(0, 0) == old_shares[i] for bp, i in zip(parts, dealers))
    commits = [bp.commitment() for bp in parts]
    new_commit, none, used = dkg_reshare(old_commit, dealers, commits, None)       # an observer
    assert none is None and used == [True, True, True, False] and new_commit.degree() == new_t
    assert new_commit.coeff[0] == old_commit.coeff[0]
    lam = lagrange_at_zero(dealers[:3])
    assert new_commit == Commitment.weighted_sum([c.row(0) for c in commits[:3]], lam)
    new_shares = {}
    for m in range(1, new_nodes + 1):
        commit, share, _ = dkg_reshare(old_commit, dealers, commits, [1, 1, 1, 1], [{i: bp.evaluate(m, i) for i in (1, 2)} for bp in parts])
        assert commit == new_commit
        assert Poly([share]) == Poly.weighted_sum([Poly([bp.evaluate(m, 0)]) for bp in parts[:3]], lam)
        new_shares[m - 1] = share
    msg = b"the key outlives the validators"
    new_pks = api.PublicKeySet(new_commit.coeff, _trusted=True)
    sig = new_pks.combine_signatures({i: api.SecretKeyShare(new_shares[i]).sign(msg) for i in (3, 1)})
    assert old_pk.verify(sig, msg) and new_pks.public_key().verify(sig, msg)
    assert not old_pk.verify(sig, b"another message")
    # failures raise, as in dkg_generate
    wrong = [commits[0], BivarPoly.random_with_constant(new_t, old_shares[0] + 1, rnd).commitment()] + commits[2:]
    with pytest.raises(ShareMismatch):
        dkg_reshare(old_commit, dealers, wrong, None)
    with pytest.raises(api.NotEnoughShares):
        dkg_reshare(old_commit, dealers, commits, [1, 0, 0, 1])
    with pytest.raises(api.DuplicateEntry):
        dkg_reshare(old_commit, [4, 0, 4, 1], commits, None)
    junk = BivarCommitment(new_t, [b"\xa5" * 96] * 3, _trusted=True)
    assert dkg_reshare(old_commit, dealers, [commits[0], junk] + commits[2:], [1, 0, 1, 1])[2] == [True, False, True, True]
    with pytest.raises(api.FromBytesError):
        dkg_reshare(old_commit, dealers, [commits[0], junk] + commits[2:], None)
