"""GPU parity of the DKG finalisation: tc_g1_sum_batch, tc_bivar_commitment_row0_sum_batch, tc_fr_sum_batch and
tc_dkg_generate_batch (src/poly.rs:870-876, 895-898, Commitment::add_assign :462-471, Poly::add_assign :68-80) vs Oracle A.

Shapes: 70 outputs are more than one wave and no multiple of 64, and 70 x parts is no multiple of 64 for parts < 32; n = 5 and
n = 67 terms (n = 5 leaves most lanes of a 64-lane output with nothing); one 68 x 200 run, the library's large shape.  Every sum
runs with the default choice of lanes per output and with TC_SUM_PARTS = 1, 4 and 64: the bytes must not depend on it.  The test
points are made by tc_g1_commitment_batch (tests/test_gpu_dkg.py checks it against the oracle); what the sums should be comes
from the oracle's affine E1.add."""
import contextlib
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import tc_oracle as o
from threshold_crypto_amd import _native, api
from threshold_crypto_amd.poly import BivarCommitment, BivarPoly, Commitment, Poly, dkg_generate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2 ** 64 - 1
B = 70
IDENT = bytes([0x40]) + bytes(95)
OK, DUPLICATE, INVALID = 0, 2, 3


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def fr(v):
    return u8(int(v).to_bytes(32, "little"))


def frs(vals):
    return np.stack([fr(v) for v in vals])


def enc(P):
    return IDENT if P is None else o.g1_uncompressed(P)


def dec(b):
    return o.g1_from_uncompressed(bytes(b), check=False)


def fold(points):
    acc = None
    for P in points:
        acc = o.E1.add(acc, P)
    return acc


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.copy()).to(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xD1CA)


@pytest.fixture(scope="module")
def engines(engine):
    """the session context (the default rule for the lanes per output) and one context per forced TC_SUM_PARTS"""
    from conftest import engine_with_env
    with contextlib.ExitStack() as stack:
        yield [engine] + [stack.enter_context(engine_with_env(TC_SUM_PARTS=p)) for p in (1, 4, 64)]


@pytest.fixture(scope="module")
def unchecked(engines):
    """input checks off on every context (the test points are the library's own outputs), whatever an earlier test left"""
    was = [e.input_checks() for e in engines]
    for e in engines:
        e.set_input_checks(False)
    yield engines
    for e, w in zip(engines, was):
        e.set_input_checks(w)


@pytest.fixture(scope="module")
def pool(engine, rnd):
    """1 024 random points of G1 as (oracle point, 96 bytes), made once by the fixed-base kernel"""
    out, st = engine.g1_commitment(frs([rnd.randrange(1, o.R) for _ in range(1024)]))
    assert not st.any()
    return [(dec(p), bytes(p)) for p in out]


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


class Cases:
    """(n, B, 96) terms whose columns walk through the case list of the issue, with the oracle's point for every term"""

    def __init__(self, pool, rnd, n, width=B):
        self.n, self.width = n, width
        neg = o.E1.neg
        pick = lambda: rnd.choice(pool)[0]
        self.cols = []
        for j in range(width):
            kind = j % 6
            if kind == 0 or kind == 5:                                  # random terms
                col = [pick() for _ in range(n)]
            elif kind == 1:                                             # n copies of one point: [n] P
                col = [pick()] * n
            elif kind == 2:                                             # P, -P side by side (an odd n ends with the identity)
                col = []
                for _ in range(n // 2):
                    P = pick()
                    col += [P, neg(P)]
                col += [None] * (n - len(col))
            elif kind == 3:                                             # P_i in the first half, -P_i mirrored in the second
                half = [pick() for _ in range(n // 2)]
                col = half + [None] * (n - 2 * len(half)) + [neg(P) for P in reversed(half)]
            else:                                                       # identities between random terms
                col = [None if k % 2 == 0 else pick() for k in range(n)]
            self.cols.append(col)
        self.pts = np.stack([np.stack([u8(enc(self.cols[j][k])) for j in range(width)]) for k in range(n)])

    def want(self, mask=None):
        return [enc(fold(P for k, P in enumerate(col) if mask is None or mask[k])) for col in self.cols]


@pytest.fixture(scope="module", params=[5, 67])
def cases(request, pool, rnd):
    return Cases(pool, rnd, request.param)


def sums(engines, pts, mask=None):
    """the call on every context: the outputs must be the same bytes; returns them once"""
    res = [e.g1_sum(pts, mask) for e in engines]
    for out, st in res[1:]:
        assert (out == res[0][0]).all() and (st == res[0][1]).all()
    return [bytes(p) for p in res[0][0]], res[0][1].tolist()


# ---- 1. tc_g1_sum_batch ----------------------------------------------------------------------------------------------------
def test_g1_sum_case_list(unchecked, cases):
    c = cases
    got, st = sums(unchecked, c.pts)
    assert st == [OK] * B and got == c.want()
    for j in range(B):
        if j % 6 == 1:
            assert got[j] == enc(o.E1.mul(c.cols[j][0], c.n))
        if j % 6 in (2, 3):
            assert got[j] == IDENT


def test_g1_sum_mask_and_bad_terms(unchecked, cases, rnd):
    c = cases
    mask = np.ones(c.n, dtype=np.uint8)
    mask[1] = 0
    mask[c.n - 1] = 0
    got, st = sums(unchecked, c.pts, mask)
    assert st == [OK] * B and got == c.want(mask)
    got, st = sums(unchecked, c.pts, np.zeros(c.n, dtype=np.uint8))     # everything masked out
    assert st == [OK] * B and got == [IDENT] * B
    spoiled = c.pts.copy()
    spoiled[1, 3] = u8(off_curve_g1(rnd))
    spoiled[1, 64] = u8(bytes([0xE0]) + bytes(95))
    got, st = sums(unchecked, spoiled, mask)                            # masked out: ignored, however malformed
    assert st == [OK] * B and got == c.want(mask)
    mask[1] = 1
    got, st = sums(unchecked, spoiled, mask)                            # included: its own output fails, nothing else
    want = c.want(mask)
    assert st == [INVALID if j in (3, 64) else OK for j in range(B)]
    assert got == [IDENT if j in (3, 64) else want[j] for j in range(B)]


def test_g1_sum_large_shape_strided_and_empty(unchecked, pool, rnd):
    c = Cases(pool, rnd, 200, width=68)                                # the library's large shape: degree 67, 200 parts
    got, st = sums(unchecked, c.pts)
    assert st == [OK] * 68 and got == c.want()
    small = Cases(pool, rnd, 5)
    wide = np.zeros((5, B + 3, 96), dtype=np.uint8)                    # term_stride > B * 96: three points of padding per term
    wide[:, :B] = small.pts
    wide[:, B:] = 0xFF
    for e in unchecked:
        out, st = e.g1_sum_strided(wide, B)
        assert not st.any() and [bytes(p) for p in out] == small.want()
    out, st = unchecked[0].g1_sum(np.zeros((0, B, 96), dtype=np.uint8))  # n = 0: the empty sum
    assert not st.any() and [bytes(p) for p in out] == [IDENT] * B


def test_g1_sum_device_io(unchecked, cases):
    c = cases
    mask = np.ones(c.n, dtype=np.uint8)
    mask[2] = 0
    t_pts, t_mask = to_dev(c.pts), to_dev(mask)
    import torch
    torch.cuda.synchronize()
    for e in unchecked:
        out, st = e.g1_sum(t_pts, t_mask)
        e.sync()
        assert not st.cpu().numpy().any() and [bytes(p) for p in out.cpu().numpy()] == c.want(mask)
    out, st = unchecked[0].g1_sum(c.pts, mask)                          # and back in host-I/O mode
    assert not st.any() and [bytes(p) for p in out] == c.want(mask)


# ---- 2. checked-input mode --------------------------------------------------------------------------------------------------
def test_g1_sum_checked_mode(engines, pool, rnd):
    c = Cases(pool, rnd, 5)
    spoiled = c.pts.copy()
    spoiled[2, 9] = u8(non_member_g1(rnd))
    all_in, without = np.ones(5, dtype=np.uint8), np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    was = [e.input_checks() for e in engines]
    try:
        for e in engines:
            e.set_input_checks(True)
        got, st = sums(engines, spoiled, all_in)                        # an included non-member fails only its own output
        want = c.want()
        assert st == [INVALID if j == 9 else OK for j in range(B)]
        assert got == [IDENT if j == 9 else want[j] for j in range(B)]
        got, st = sums(engines, spoiled, without)                       # the same point masked out fails nothing
        assert st == [OK] * B and got == c.want(without)
        for e in engines:
            e.set_input_checks(False)
        got, st = sums(engines, spoiled, all_in)                        # checks off: it is on the curve, nothing is flagged
        assert st == [OK] * B and [g for j, g in enumerate(got) if j != 9] == [w for j, w in enumerate(want) if j != 9]
        got, st = sums(engines, spoiled, without)
        assert st == [OK] * B and got == c.want(without)
    finally:
        for e, w in zip(engines, was):
            e.set_input_checks(w)


# ---- 3. tc_bivar_commitment_row0_sum_batch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [2, 7])
def test_row0_sum(engines, pool, rnd, degree):
    P, nco = 5, (degree + 1) * (degree + 2) // 2
    parts = [rnd.sample(pool, nco) for _ in range(P)]
    commits = np.stack([np.stack([u8(b) for _, b in part]) for part in parts])
    mask = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    want = []
    for i in range(degree + 1):
        acc = None
        for p in range(P):
            if mask[p]:
                acc = o.E1.add(acc, o.bivar_commitment_row(degree, [pt for pt, _ in parts[p]], 0)[i])
        want.append(enc(acc))
    garbage = commits.copy()
    garbage[2] = 0xA5                                                   # the masked part may hold anything
    for e in engines:
        was = e.input_checks()
        for checks in (False, True):
            e.set_input_checks(checks)
            for blob in (commits, garbage):
                out, st = e.bivar_row0_sum(blob, degree, mask)
                assert not st.any() and [bytes(p) for p in out] == want, (checks, degree)
        e.set_input_checks(was)
    # ... and it is tc_g1_sum_batch over the rows tc_bivar_commitment_row_batch returns for x = 0
    e = engines[0]
    rows = np.stack([e.bivar_commitment_rows(commits[p], degree, np.array([0], dtype=np.uint64))[0][0] for p in range(P)])
    out, st = e.g1_sum(rows, mask)
    assert not st.any() and [bytes(p) for p in out] == want
    # an included bad point fails its own coefficient only
    bad = commits.copy()
    bad[4, o.coeff_pos(1, 0)] = u8(off_curve_g1(rnd))
    out, st = e.bivar_row0_sum(bad, degree, mask)
    assert st.tolist() == [INVALID if i == 1 else OK for i in range(degree + 1)]
    assert [bytes(p) for p in out] == [IDENT if i == 1 else want[i] for i in range(degree + 1)]


# ---- 4. tc_fr_sum_batch ------------------------------------------------------------------------------------------------------
def test_fr_sum(engine, rnd):
    n = 5
    vals = [[rnd.randrange(o.R) for _ in range(B)] for _ in range(n)]
    vals[0][1], vals[1][1], vals[2][1], vals[3][1], vals[4][1] = o.R - 1, o.R - 1, 2, 0, 0
    blob = np.stack([frs(v) for v in vals])
    ints = lambda a: [int.from_bytes(bytes(r), "little") for r in a]
    out, st = engine.fr_sum(blob)
    assert not st.any() and ints(out) == [sum(vals[k][j] for k in range(n)) % o.R for j in range(B)]
    mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    want = [sum(vals[k][j] for k in range(n) if mask[k]) % o.R for j in range(B)]
    out, st = engine.fr_sum(blob, mask)
    assert not st.any() and ints(out) == want
    out, st = engine.fr_sum(to_dev(blob), to_dev(mask))
    engine.sync()
    assert not st.cpu().numpy().any() and ints(out.cpu().numpy()) == want
    spoiled = blob.copy()
    spoiled[1, 7] = fr(o.R)                                              # masked out: ignored
    spoiled[4, 66] = fr(2 ** 256 - 1)
    out, st = engine.fr_sum(spoiled, mask)
    assert not st.any() and ints(out) == want
    out, st = engine.fr_sum(spoiled)                                    # included: zero and INVALID_ENCODING for that output
    full = [sum(vals[k][j] for k in range(n)) % o.R for j in range(B)]
    assert st.tolist() == [INVALID if j in (7, 66) else OK for j in range(B)]
    assert ints(out) == [0 if j in (7, 66) else full[j] for j in range(B)]
    out, st = engine.fr_sum(blob, np.zeros(n, dtype=np.uint8))
    assert not st.any() and not out.any()


# ---- 5. tc_dkg_generate_batch --------------------------------------------------------------------------------------------------
def test_ref_distributed_key_generation_tail(engine, rnd):
    """src/poly.rs:866-899 through poly.py: 3 dealers, 5 nodes, degree 2, every node interpolating from nodes 1, 2 and 4"""
    api.set_default_engine(engine)
    dealer_num, node_num, faulty_num = 3, 5, 2
    ncoef = (faulty_num + 1) * (faulty_num + 2) // 2
    bi_polys = [BivarPoly(faulty_num, [rnd.randrange(o.R) for _ in range(ncoef)]) for _ in range(dealer_num)]
    bi_commits = [bp.commitment() for bp in bi_polys]
    sec_key_set = Poly.sum([bp.row(0) for bp in bi_polys])
    assert sec_key_set == bi_polys[0].row(0) + bi_polys[1].row(0) + bi_polys[2].row(0)
    want_commit = sec_key_set.commitment()
    sum_commit, none = dkg_generate(bi_commits, None)                    # an observer: out_share_fr = NULL
    assert none is None and sum_commit == want_commit                    # :899
    assert sum_commit == BivarCommitment.row0_sum(bi_commits) == Commitment.sum([bc.row(0) for bc in bi_commits])
    assert sum_commit == bi_commits[0].row(0) + bi_commits[1].row(0) + bi_commits[2].row(0)
    for m in range(1, node_num + 1):
        samples = [{i: bp.evaluate(m, i) for i in (1, 2, 4)} for bp in bi_polys]     # :866-869
        commit, share = dkg_generate(bi_commits, [True] * dealer_num, samples)
        assert commit == want_commit and share == sec_key_set.evaluate(m)              # :890
        assert Poly([share]).commitment() == Commitment([sum_commit.evaluate(m)], _trusted=True)     # g1 * share
    # one rejected dealer whose commitment bytes are garbage changes nothing but the sums
    m = 3
    junk = BivarCommitment(faulty_num, [b"\xa5" * 96] * ncoef, _trusted=True)
    kept = [bi_polys[0], bi_polys[2]]
    samples = [{i: bi_polys[0].evaluate(m, i) for i in (1, 2, 4)}, None, {i: bi_polys[2].evaluate(m, i) for i in (1, 2, 4)}]
    was = engine.input_checks()
    for checks in (False, True):
        engine.set_input_checks(checks)
        commit, share = dkg_generate([bi_commits[0], junk, bi_commits[2]], [1, 0, 1], samples)
        assert commit == Poly.sum([bp.row(0) for bp in kept]).commitment()
        assert share == sum(bp.evaluate(m, 0) for bp in kept) % o.R
    engine.set_input_checks(was)
    with pytest.raises(api.FromBytesError):
        dkg_generate([bi_commits[0], junk, bi_commits[2]], None, None)   # the same garbage accepted: the part fails
    with pytest.raises(ValueError):
        dkg_generate(bi_commits, None, [{1: 5, 2: 6, 4: 7}, [(1, 5), (1, 6), (4, 7)], {1: 5, 2: 6, 4: 7}])   # a repeated abscissa


def _parts(engine, rnd, degree, P, n_v):
    nco = (degree + 1) * (degree + 2) // 2
    coeffs = [[rnd.randrange(o.R) for _ in range(nco)] for _ in range(P)]
    commits, st = engine.g1_commitment(frs([c for cs in coeffs for c in cs]))
    assert not st.any()
    commits = commits.reshape(P, nco, 96)
    node = 9
    xs = np.array([rnd.sample(range(1, 200), n_v) for _ in range(P)], dtype=np.uint64)
    xs[0, :3] = [0, U64, 1]
    vals = np.stack([frs([o.bivar_poly_evaluate(degree, cs, node, int(x)) for x in xs[p]]) for p, cs in enumerate(coeffs)])
    share0 = [o.bivar_poly_evaluate(degree, cs, node, 0) for cs in coeffs]
    return coeffs, commits, xs, vals, share0


def test_dkg_generate_statuses_and_never_a_partial_key(engine, rnd):
    degree, P, n_v = 2, 5, 3
    coeffs, commits, xs, vals, share0 = _parts(engine, rnd, degree, P, n_v)
    accept = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    want_commit = [enc(fold(dec(commits[p, o.coeff_pos(i, 0)]) for p in range(P) if accept[p])) for i in range(degree + 1)]
    want_share = sum(s for s, a in zip(share0, accept) if a) % o.R
    ints = lambda a: int.from_bytes(bytes(a), "little")
    was = engine.input_checks()
    try:
        for checks in (False, True):
            engine.set_input_checks(checks)
            out, share, st = engine.dkg_generate(commits, degree, accept, xs, vals)
            assert st.tolist() == [OK] * P and [bytes(p) for p in out] == want_commit and ints(share) == want_share
            out, share, st = engine.dkg_generate(to_dev(commits), degree, to_dev(accept), to_dev(xs), to_dev(vals))    # device-I/O mode
            engine.sync()
            assert st.cpu().tolist() == [OK] * P and [bytes(p) for p in out.cpu().numpy()] == want_commit and ints(share.cpu().numpy()) == want_share
            out, share, st = engine.dkg_generate(commits, degree, accept)              # out_share_fr = NULL
            assert share is None and st.tolist() == [OK] * P and [bytes(p) for p in out] == want_commit
            spoiled = [(commits.copy(), xs, vals, INVALID), (commits, xs.copy(), vals, DUPLICATE), (commits, xs, vals.copy(), INVALID)]
            spoiled[0][0][3, o.coeff_pos(2, 0)] = u8(off_curve_g1(rnd))                 # a wrong-encoding first-column point
            spoiled[1][1][3, 2] = spoiled[1][1][3, 0]                                    # a repeated abscissa
            spoiled[2][2][3, 1] = fr(o.R)                                                # a non-canonical value
            if checks:
                member = commits.copy()
                member[3, o.coeff_pos(1, 0)] = u8(non_member_g1(rnd))                    # on the curve, outside G1
                spoiled.append((member, xs, vals, INVALID))
            for c, x, v, code in spoiled:
                out, share, st = engine.dkg_generate(c, degree, accept, x, v)           # TC_OK: the call itself succeeds
                assert st.tolist() == [OK, OK, OK, code, OK]
                assert [bytes(p) for p in out] == [IDENT] * (degree + 1) and ints(share) == 0
                rejected = accept.copy()
                rejected[3] = 0                                                          # the same part rejected: never read
                out, share, st = engine.dkg_generate(c, degree, rejected, x, v)
                assert st.tolist() == [OK] * P and ints(share) == (want_share - share0[3]) % o.R
            # a column point OUTSIDE the first column is not this entry's business
            other = commits.copy()
            other[3, o.coeff_pos(1, 2)] = u8(off_curve_g1(rnd))
            out, share, st = engine.dkg_generate(other, degree, accept, xs, vals)
            assert st.tolist() == [OK] * P and [bytes(p) for p in out] == want_commit
    finally:
        engine.set_input_checks(was)


def test_dkg_generate_seventy_parts_degree_seven(engines, rnd):
    degree, P, n_v = 7, 70, 8
    coeffs, commits, xs, vals, share0 = _parts(engines[0], rnd, degree, P, n_v)
    accept = np.ones(P, dtype=np.uint8)
    accept[[5, 64]] = 0
    want_commit = [enc(fold(dec(commits[p, o.coeff_pos(i, 0)]) for p in range(P) if accept[p])) for i in range(degree + 1)]
    want_share = sum(s for s, a in zip(share0, accept) if a) % o.R
    for e in engines:
        out, share, st = e.dkg_generate(commits, degree, accept, xs, vals)
        assert not st.any() and [bytes(p) for p in out] == want_commit and int.from_bytes(bytes(share), "little") == want_share
    # the secret key set of these dealers, committed to: the oracle's commitment of the summed first rows
    row0 = [sum(cs[o.coeff_pos(i, 0)] for cs, a in zip(coeffs, accept) if a) % o.R for i in range(degree + 1)]
    assert want_commit == [enc(P_) for P_ in o.commitment(row0)]


def test_null_arguments_and_zero_sizes(engine):
    lib, ctx = engine._lib, engine._ctx
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data
    engine._mode(buf)                                                    # host-I/O mode
    bad = _native.TC_ERR_INVALID_ARG
    assert lib.tc_g1_sum_batch(ctx, None, 96, 2, None, 1, p, p) == bad
    assert lib.tc_g1_sum_batch(ctx, p, 96, 2, None, 1, None, p) == bad
    assert lib.tc_g1_sum_batch(ctx, p, 95, 2, None, 1, p, p) == bad        # the stride: a multiple of 96 ...
    assert lib.tc_g1_sum_batch(ctx, p, 96, 2, None, 2, p, p) == bad        # ... and at least B points
    assert lib.tc_bivar_commitment_row0_sum_batch(ctx, None, 96, 0, 1, None, p, p) == bad
    assert lib.tc_bivar_commitment_row0_sum_batch(ctx, p, 96, 0, 1, None, None, p) == bad
    assert lib.tc_bivar_commitment_row0_sum_batch(ctx, p, 0, 0, 1, None, p, p) == bad
    assert lib.tc_bivar_commitment_row0_sum_batch(ctx, p, 2 * 96, 1, 1, None, p, p) == bad     # degree 1: three points per part
    assert lib.tc_fr_sum_batch(ctx, None, 32, 2, None, 1, p, p) == bad
    assert lib.tc_fr_sum_batch(ctx, p, 32, 2, None, 1, None, p) == bad
    assert lib.tc_fr_sum_batch(ctx, p, 48, 2, None, 1, p, p) == bad
    assert lib.tc_dkg_generate_batch(ctx, None, 96, 0, 1, None, None, None, 0, p, None, p) == bad
    assert lib.tc_dkg_generate_batch(ctx, p, 96, 0, 1, None, None, p, 2, p, p, p) == bad          # a share needs its samples
    assert lib.tc_dkg_generate_batch(ctx, p, 96, 0, 1, None, p, None, 2, p, p, p) == bad
    assert lib.tc_dkg_generate_batch(ctx, p, 0, 0, 1, None, None, None, 0, p, None, p) == bad
    buf[:] = 0x77
    ok = _native.TC_OK
    assert lib.tc_g1_sum_batch(ctx, None, 0, 0, None, 0, None, None) == ok           # B = 0 / P = 0: nothing is written
    assert lib.tc_bivar_commitment_row0_sum_batch(ctx, None, 0, 0, 0, None, None, None) == ok
    assert lib.tc_fr_sum_batch(ctx, None, 0, 0, None, 0, None, None) == ok
    assert lib.tc_dkg_generate_batch(ctx, None, 0, 0, 0, None, None, None, 0, p, p, p) == ok
    assert (buf == 0x77).all()
    assert lib.tc_g1_sum_batch(ctx, None, 0, 0, None, 2, p, None) == ok               # n = 0: identities; status is optional
    assert bytes(buf[:192]) == IDENT * 2 and buf[192] == 0x77
    assert lib.tc_fr_sum_batch(ctx, None, 0, 0, None, 2, p, p + 64) == ok
    assert not buf[:66].any()


# ---- 6. the C++ mirror -----------------------------------------------------------------------------------------------------
def test_cpp_mirror(engine, rnd, tmp_path):
    """include/threshold_crypto.hpp commitment_sum and dkg_generate, from a stand-alone program (tests/cpp/test_dkg_generate.cpp)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_dkg_generate.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_dkg_generate")
    libdir = os.path.join(ROOT, "threshold_crypto_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir, "-ltc_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    degree, P, n_v = 2, 4, 3
    coeffs, commits, xs, vals, share0 = _parts(engine, rnd, degree, P, n_v)
    accept = [1, 0, 1, 1]
    nco = commits.shape[1]
    want_commit = [enc(fold(dec(commits[p, o.coeff_pos(i, 0)]) for p in range(P) if accept[p])) for i in range(degree + 1)]
    want_share = sum(s for s, a in zip(share0, accept) if a) % o.R
    rows = [[bytes(commits[p, o.coeff_pos(i, 0)]) for i in range(degree + 1 - (p == 1))] for p in range(P)]   # one shorter commitment
    want_sum = [enc(fold(dec(r[i]) for p, r in enumerate(rows) if accept[p] and i < len(r))) for i in range(degree + 1)]
    fx = struct.pack("<III", degree, P, n_v) + bytes(accept) + commits.tobytes() + xs.tobytes() + vals.tobytes()
    fx += b"".join(want_commit) + want_share.to_bytes(32, "little")
    fx += b"".join(struct.pack("<I", len(r)) + b"".join(r) for r in rows) + b"".join(want_sum)
    assert nco == 6
    path = tmp_path / "fixture.bin"
    path.write_bytes(fx)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-DKG-OK" in r.stdout, r.stdout + r.stderr
