"""GPU parity of the DKG verification entries: the secret side in Fr (Poly::evaluate, BivarPoly::row), the rows check
`row_poly.commitment() == bi_commit.row(m)` and the values check `bi_commit.evaluate(m, s) == g1 * val` of
`distributed_key_generation` (src/poly.rs:838-878) -- exact, and by one random linear combination per part -- vs Oracle A.

Shapes: degree 2 is the reference's own (4 points: the small linear-combination kernel), degree 6 gives exactly
kMsmMinPoints = 8 points, degree 7 takes the two-stage kernels; 70 jobs are more than one wave and no multiple of 64; n = 5
values per part, one case n = 70.  The commitments of the test polynomials are made by tc_g1_commitment_batch
(tests/test_gpu_dkg.py checks it against the oracle); what the checks should answer comes from the oracle's Fr and G1
arithmetic."""
import random

import numpy as np
import pytest

import tc_oracle as o
from threshold_crypto_amd import api
from threshold_crypto_amd.poly import BivarPoly, Commitment, Poly

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
B, N = 70, 5
IDENT = bytes([0x40]) + bytes(95)


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def fr(v):
    return u8(int(v).to_bytes(32, "little"))


def frs(vals):
    return np.stack([fr(v) for v in vals])


def ints(a):
    return [int.from_bytes(bytes(r), "little") for r in a.reshape(-1, 32)]


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xD1C8)


@pytest.fixture(scope="module")
def checked(engine):
    """checked-input mode (the default of a context) for the tests below, whatever an earlier test left"""
    was = engine.input_checks()
    engine.set_input_checks(True)
    yield engine
    engine.set_input_checks(was)


def off_curve_g1(rnd):
    """96 bytes in range that are no point of the curve"""
    while True:
        x, y = rnd.randrange(o.Q), rnd.randrange(o.Q)
        if (y * y - x * x * x - 4) % o.Q:
            return u8(x.to_bytes(48, "big") + y.to_bytes(48, "big"))


def non_member_g1(rnd):
    """an on-curve point of E(Fq) outside the order-r subgroup"""
    while True:
        x = rnd.randrange(o.Q)
        y2 = (x * x * x + 4) % o.Q
        y = pow(y2, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == y2 and o.E1.mul((x, y), o.R) is not None:
            return u8(o.g1_uncompressed((x, y)))


# ---- the secret side -----------------------------------------------------------------------------------------------
def test_fr_poly_evaluate_matches_oracle(engine, rnd):
    """300 polynomials x 5 abscissae (more than one workgroup of outputs per launch and no multiple of 64), degree 7, edge
    coefficients and abscissae; then status bytes for a non-canonical coefficient (its polynomial's row) and a non-canonical
    abscissa (its column), and the zero polynomial (n = 0)."""
    n = 8
    polys = [[rnd.randrange(o.R) for _ in range(n)] for _ in range(300)]
    polys[1] = [0] * n
    polys[2] = [o.R - 1] * n
    polys[3] = [rnd.choice([0, o.R - 1]) for _ in range(n)]
    xs = [0, 1, U64, o.R - 1, rnd.randrange(o.R)]
    coeff = np.stack([frs(p) for p in polys])
    out, st = engine.fr_poly_evaluate(coeff, frs(xs))
    assert not st.any()
    assert ints(out) == [o.poly_evaluate(p, x) for p in polys for x in xs]
    bad = coeff[:4].copy()
    bad[2, 5] = fr(o.R)
    out, st = engine.fr_poly_evaluate(bad, frs(xs + [o.R + 2]))
    want_st = [[3 if (j == 2 or m == 5) else 0 for m in range(6)] for j in range(4)]
    assert st.tolist() == want_st
    got = np.array(ints(out), dtype=object).reshape(4, 6)
    for j in range(4):
        for m in range(6):
            assert got[j, m] == (0 if want_st[j][m] else o.poly_evaluate(polys[j], xs[m]))
    out, st = engine.fr_poly_evaluate(np.zeros((3, 0, 32), dtype=np.uint8), frs(xs))
    assert not st.any() and not out.any() and out.shape == (3, 5, 32)


def test_bivar_poly_rows_match_oracle(engine, rnd):
    for d, xs in ((7, [0, 1, 2, 200, U64] + list(range(3, 68))), (2, [0, 1, U64]), (0, [5, 0])):
        coeff = [rnd.randrange(o.R) for _ in range((d + 1) * (d + 2) // 2)]
        if d == 2:
            coeff[1], coeff[4] = 0, o.R - 1
        out, st = engine.bivar_poly_rows(frs(coeff), d, np.array(xs, dtype=np.uint64))
        assert not st.any() and out.shape == (len(xs), d + 1, 32)
        assert ints(out) == [c for x in xs for c in o.bivar_poly_row(d, coeff, x)]
    # a coefficient >= r fails exactly the rows that depend on it: (0, 2) = (2, 0) -> rows 0 and 2 of every abscissa
    d, coeff = 2, [rnd.randrange(o.R) for _ in range(6)]
    blob = frs(coeff)
    blob[o.coeff_pos(0, 2)] = fr(o.R)
    out, st = engine.bivar_poly_rows(blob, d, np.array([7, 9], dtype=np.uint64))
    assert st.tolist() == [[3, 0, 3], [3, 0, 3]]
    for m, x in enumerate((7, 9)):
        assert ints(out[m]) == [0, o.bivar_poly_row(d, coeff, x)[1], 0]


# ---- the rows check ------------------------------------------------------------------------------------------------
def _row_bytes(d, commit_pts, x):
    return [o.g1_uncompressed(p) for p in o.bivar_commitment_row(d, commit_pts, x)]


def test_verify_rows_per_job_commitments(checked, rnd):
    """70 dealers' commitments, every node asks for row 3: honest rows pass and out_rows is BivarCommitment::row; a row coefficient
    off by one, a row coefficient >= r, an off-curve commitment point and (checked-input mode) an on-curve point outside G1 each
    fail their own job only."""
    engine, d, x = checked, 2, 3
    nco = (d + 1) * (d + 2) // 2
    coeffs = [[rnd.randrange(o.R) for _ in range(nco)] for _ in range(B)]
    commits, st = engine.g1_commitment(frs([c for cs in coeffs for c in cs]))
    assert not st.any()
    commits = commits.reshape(B, nco, 96)
    rows_fr = np.stack([frs(o.bivar_poly_row(d, cs, x)) for cs in coeffs])
    xs = np.full(B, x, dtype=np.uint64)
    out, ok = engine.dkg_verify_rows(commits, d, xs, rows_fr)
    assert ok.tolist() == [1] * B
    want = [_row_bytes(d, [o.g1_from_uncompressed(bytes(p), check=False) for p in commits[j]], x) for j in range(B)]
    assert [[bytes(p) for p in out[j]] for j in range(B)] == want
    bad_rows, bad_commits = rows_fr.copy(), commits.copy()
    bad_rows[9, 1] = fr((o.bivar_poly_row(d, coeffs[9], x)[1] + 1) % o.R)
    bad_rows[11, 2] = fr(o.R)
    bad_commits[13, 4] = off_curve_g1(rnd)
    bad_commits[15, 0] = non_member_g1(rnd)
    out, ok = engine.dkg_verify_rows(bad_commits, d, xs, bad_rows)
    assert ok.tolist() == [0 if j in (9, 11, 13, 15) else 1 for j in range(B)]
    for j in range(B):
        assert [bytes(p) for p in out[j]] == ([IDENT] * (d + 1) if j in (13, 15) else want[j]), j


def test_verify_rows_one_commitment_many_abscissae(checked, rnd):
    """stride 0: one dealer's commitment, 70 nodes with their own abscissae -- 0 and 2^64 - 1 among them"""
    engine, d = checked, 2
    coeff = [rnd.randrange(o.R) for _ in range(6)]
    commit, st = engine.g1_commitment(frs(coeff))
    assert not st.any()
    pts = [o.g1_from_uncompressed(bytes(p), check=False) for p in commit]
    xl = [0, U64] + list(range(1, B - 1))
    rows_fr = np.stack([frs(o.bivar_poly_row(d, coeff, x)) for x in xl])
    out, ok = engine.dkg_verify_rows(commit, d, np.array(xl, dtype=np.uint64), rows_fr)
    assert ok.tolist() == [1] * B
    for j, x in enumerate(xl):
        assert [bytes(p) for p in out[j]] == _row_bytes(d, pts, x), x
    rows_fr[1, 0] = fr((int.from_bytes(bytes(rows_fr[1, 0]), "little") + 1) % o.R)
    _, ok = engine.dkg_verify_rows(commit, d, np.array(xl, dtype=np.uint64), rows_fr)
    assert ok.tolist() == [1, 0] + [1] * (B - 2)


# ---- the values checks -----------------------------------------------------------------------------------------------
class Parts:
    """70 parts of degree d: row polynomials, their commitments, 5 abscissae and honest values each"""

    def __init__(self, engine, rnd, d, B=B, n=N):
        self.d, self.B, self.n = d, B, n
        self.polys = [[rnd.randrange(o.R) for _ in range(d + 1)] for _ in range(B)]
        rows, st = engine.g1_commitment(frs([c for p in self.polys for c in p]))
        assert not st.any()
        self.rows = rows.reshape(B, d + 1, 96)
        self.xs = np.array([[rnd.randrange(1, 201) for _ in range(n)] for _ in range(B)], dtype=np.uint64)
        self.xs[0, :5] = [0, U64, 3, 3, 1]                              # 0, 2^64 - 1 and a repeated abscissa
        self.vals = np.stack([frs([o.poly_evaluate(p, int(x)) for x in self.xs[j]]) for j, p in enumerate(self.polys)])

    def value(self, j, k):
        return o.poly_evaluate(self.polys[j], int(self.xs[j, k]))


@pytest.fixture(scope="module", params=[2, 6, 7])
def parts(request, engine, rnd):
    return Parts(engine, rnd, request.param)


def _spoil(p, rnd):
    """the wrong operands of the issue; returns (rows, xs, vals, expected ok)"""
    rows, xs, vals = p.rows.copy(), p.xs.copy(), p.vals.copy()
    want = np.ones((p.B, p.n), dtype=np.uint8)
    vals[9, 2] = fr((p.value(9, 2) + 1) % o.R)                          # one wrong value
    want[9, 2] = 0
    vals[20, 1], vals[20, 3] = fr((p.value(20, 1) + 9) % o.R), fr((p.value(20, 3) - 9) % o.R)   # cancels in the unweighted sum
    want[20, 1] = want[20, 3] = 0
    vals[11, 4] = fr(o.R + 1)                                           # a value >= r
    want[11, 4] = 0
    rows[13, p.d] = off_curve_g1(rnd)                                   # an undecodable row point: the whole job
    want[13] = 0
    for j in (30, 31):                                                  # the same wrong data in two jobs
        rows[j], xs[j], vals[j] = p.rows[30], p.xs[30], p.vals[30]
        vals[j, 0] = fr((p.value(30, 0) + 5) % o.R)
        want[j, 0] = 0
    rows[40, 0] = non_member_g1(rnd)                                    # checked-input mode: not a member of G1
    want[40] = 0
    return rows, xs, vals, want


def test_verify_values_exact(checked, rnd, parts):
    engine, p = checked, parts
    ok = engine.dkg_verify_values(p.rows, p.xs, p.vals)
    assert ok.shape == (p.B, p.n) and ok.all()
    # Commitment::evaluate itself, in the oracle's G1, for the edge abscissae of job 0
    pts = [o.g1_from_uncompressed(bytes(c), check=False) for c in p.rows[0]]
    for k in range(p.n):
        assert o.commitment_evaluate(pts, int(p.xs[0, k])) == o.E1.mul(o.G1_GEN, p.value(0, k))
    rows, xs, vals, want = _spoil(p, rnd)
    ok = engine.dkg_verify_values(rows, xs, vals)
    assert ok.tolist() == want.tolist()


def test_verify_values_rlc_equals_exact(checked, rnd, parts):
    engine, p = checked, parts
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    ok, nfb = engine.dkg_verify_values_rlc(p.rows, p.xs, p.vals, seed)
    assert ok.all() and nfb == 0
    vals = p.vals.copy()
    vals[9, 2] = fr((p.value(9, 2) + 1) % o.R)
    ok, nfb = engine.dkg_verify_values_rlc(p.rows, p.xs, vals, seed)
    want = np.ones((p.B, p.n), dtype=np.uint8)
    want[9, 2] = 0
    assert nfb == 1 and ok.tolist() == want.tolist()
    assert ok.tolist() == engine.dkg_verify_values(p.rows, p.xs, vals).tolist()
    rows, xs, vals, want = _spoil(p, rnd)
    ok, nfb = engine.dkg_verify_values_rlc(rows, xs, vals, seed)
    assert nfb == 7 and ok.tolist() == want.tolist()
    assert ok.tolist() == engine.dkg_verify_values(rows, xs, vals).tolist()


def test_verify_values_seventy_values_per_part(checked, rnd):
    """n = 70 values per part (more than one wave of value lanes per job)"""
    engine = checked
    p = Parts(engine, rnd, 2, B=3, n=70)
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    assert engine.dkg_verify_values(p.rows, p.xs, p.vals).all()
    ok, nfb = engine.dkg_verify_values_rlc(p.rows, p.xs, p.vals, seed)
    assert ok.all() and nfb == 0
    vals = p.vals.copy()
    vals[1, 66] = fr((p.value(1, 66) + 1) % o.R)
    want = np.ones((3, 70), dtype=np.uint8)
    want[1, 66] = 0
    assert engine.dkg_verify_values(p.rows, p.xs, vals).tolist() == want.tolist()
    ok, nfb = engine.dkg_verify_values_rlc(p.rows, p.xs, vals, seed)
    assert nfb == 1 and ok.tolist() == want.tolist()


def test_device_io_mode_gives_the_same_outputs(checked, rnd):
    import torch
    engine, d = checked, 2
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.copy()).to(dev)
    p = Parts(engine, rnd, d)
    rows, xs, vals, want = _spoil(p, rnd)
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    coeff = np.stack([frs(q) for q in p.polys])
    xs_fr = frs([0, 1, U64, o.R - 1, 77])
    bi = [rnd.randrange(o.R) for _ in range(6)]
    bxs = np.array([0, 1, 5, U64], dtype=np.uint64)
    commit, _ = engine.g1_commitment(frs(bi))
    brow = np.stack([frs(o.bivar_poly_row(d, bi, int(x))) for x in bxs])
    brow[2, 1] = fr(5)
    host = [engine.fr_poly_evaluate(coeff, xs_fr), engine.bivar_poly_rows(frs(bi), d, bxs), engine.dkg_verify_rows(commit, d, bxs, brow),
            (engine.dkg_verify_values(rows, xs, vals),), engine.dkg_verify_values_rlc(rows, xs, vals, seed)]
    assert host[2][1].tolist() == [1, 1, 0, 1]
    ops = [to(a) for a in (coeff, xs_fr, frs(bi), bxs, commit, brow, rows, xs, vals)]
    torch.cuda.synchronize()
    t_coeff, t_xs_fr, t_bi, t_bxs, t_commit, t_brow, t_rows, t_xs, t_vals = ops
    devr = [engine.fr_poly_evaluate(t_coeff, t_xs_fr), engine.bivar_poly_rows(t_bi, d, t_bxs), engine.dkg_verify_rows(t_commit, d, t_bxs, t_brow),
            (engine.dkg_verify_values(t_rows, t_xs, t_vals),), engine.dkg_verify_values_rlc(t_rows, t_xs, t_vals, seed)]
    engine.sync()
    for h, g in zip(host, devr):
        for a, b in zip(h, g):
            if isinstance(a, int):
                assert a == b == 7
            else:
                assert (a == b.cpu().numpy()).all()
    assert engine.dkg_verify_values(rows, xs, vals).tolist() == want.tolist()      # and back in host-I/O mode


# ---- distributed_key_generation (src/poly.rs:818-900) through the new methods of poly.py -------------------------------
def test_ref_distributed_key_generation_on_the_device(checked, rnd):
    """3 dealers, 5 nodes, degree 2: rows, values and both checks through BivarPoly.row_batch, Poly.evaluate_batch,
    BivarCommitment.verify_rows and Commitment.verify_values (exact and combined); the cheating dealer (row + 5 x^2, :858-861) is
    caught by verify_rows."""
    engine = checked
    api.set_default_engine(engine)
    dealer_num, node_num, faulty_num = 3, 5, 2
    nodes = list(range(1, node_num + 1))
    ncoef = (faulty_num + 1) * (faulty_num + 2) // 2
    bi_polys = [BivarPoly(faulty_num, [rnd.randrange(o.R) for _ in range(ncoef)]) for _ in range(dealer_num)]
    sec_keys = [0] * node_num
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    for bi_poly in bi_polys:
        bi_commit = bi_poly.commitment()
        row_polys = bi_poly.row_batch(nodes)
        assert row_polys == [bi_poly.row(m) for m in nodes]
        assert [r.coeff for r in row_polys] == [o.bivar_poly_row(faulty_num, bi_poly.coeff, m) for m in nodes]
        row_commits, ok = bi_commit.verify_rows(nodes, row_polys)                       # :841-843
        assert ok == [True] * node_num
        assert row_commits == bi_commit.row_batch(nodes)
        vals = Poly.evaluate_batch(row_polys, nodes)
        assert vals == [[r.evaluate(s) for s in nodes] for r in row_polys]
        assert vals == [[bi_poly.evaluate(m, s) for s in nodes] for m in nodes]          # :854
        xs = [nodes] * node_num
        assert Commitment.verify_values_batch(row_commits, xs, vals) == [[True] * node_num] * node_num      # :846-848
        assert Commitment.verify_values_batch(row_commits, xs, vals, seed=seed) == [[True] * node_num] * node_num
        assert row_commits[0].verify_values(nodes, vals[0]) == [True] * node_num
        # a cheating dealer is detected (:858-861)
        wrong = list(row_polys)
        wrong[3] = row_polys[3] + Poly([0, 0, 5])
        assert bi_commit.verify_rows(nodes, wrong)[1] == [True, True, True, False, True]
        lied = [list(v) for v in vals]
        lied[2][4] = (lied[2][4] + 1) % o.R
        for s in (None, seed):
            got = Commitment.verify_values_batch(row_commits, xs, lied, seed=s)
            assert got == [[not (m == 2 and k == 4) for k in range(node_num)] for m in range(node_num)]
        for m in nodes:
            my_row = Poly.interpolate({i: vals[m - 1][i - 1] for i in (1, 2, 4)})
            assert my_row == row_polys[m - 1]                                              # :876-877
            sec_keys[m - 1] = (sec_keys[m - 1] + my_row.evaluate(0)) % o.R
    sec_key_set = Poly([])
    for bp in bi_polys:
        sec_key_set = sec_key_set + bp.row(0)
    assert Poly.evaluate_batch([sec_key_set], nodes)[0] == sec_keys                        # :891
