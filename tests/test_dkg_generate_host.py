"""The routines of the DKG finalisation on the CPU: the device headers compiled by g++ (tests/dkg/dkg_generate_host.cpp, a test
harness -- not a product path).  The harness runs one output of k_g1_sum the way the kernel does -- the partial sums of the
lanes g = 0 .. parts-1, then the xor tree of complete additions -- so the cases below meet P + P and P + (-P) inside a lane
(jac_add_mixed) and across lanes (jac_add).  Everything is compared with Oracle A: E1.add folds, Python integers mod r and
poly_interpolate(samples)[0]."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tc_oracle as o  # noqa: E402

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "dkg", "dkg_generate_host.cpp")
U64 = 2 ** 64 - 1
IDENT = bytes([0x40]) + bytes(95)
PARTS = [1, 2, 4, 64]
OK, DUPLICATE, INVALID = 0, 2, 3


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)) \
        or os.path.getmtime(path) < os.path.getmtime(SRC)


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "dkg", "libdkg_generate_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, p = ctypes.c_size_t, ctypes.c_char_p
    lib.dg_sum_part.argtypes = [sz, sz, sz, ctypes.POINTER(sz)]
    lib.dg_sum_part.restype = None
    lib.dg_g1_sum.argtypes = [p, sz, sz, p, p, sz, p, p]
    lib.dg_fr_sum.argtypes = [p, sz, sz, p, p]
    lib.dg_fr_interpolate_at_zero.argtypes = [sz, ctypes.c_void_p, p, p]
    return lib


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xD1C9)


@pytest.fixture(scope="module")
def pool(rnd):
    """70 random points of G1, made once"""
    return [o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R)) for _ in range(70)]


def enc(P):
    return IDENT if P is None else o.g1_uncompressed(P)


def fold(points):
    acc = None
    for P in points:
        acc = o.E1.add(acc, P)
    return acc


def off_curve(rnd):
    while True:
        x, y = rnd.randrange(o.Q), rnd.randrange(o.Q)
        if (y * y - x * x * x - 4) % o.Q:
            return x.to_bytes(48, "big") + y.to_bytes(48, "big")


def g1_sum(L, terms, parts, mask=None, member=None):
    """terms: encodings; returns (status, 96 bytes, term_bad)"""
    n = len(terms)
    out, bad = ctypes.create_string_buffer(96), ctypes.create_string_buffer(max(n, 1))
    st = L.dg_g1_sum(b"".join(terms), 96, n, None if mask is None else bytes(mask), None if member is None else bytes(member), parts, out, bad)
    return st, out.raw, list(bad.raw[:n])


def same_for_every_parts(L, terms, want, mask=None):
    for parts in PARTS:
        st, got, bad = g1_sum(L, terms, parts, mask)
        assert (st, got) == (OK, enc(want)), parts
        assert not any(bad)


# ---- 1. sum_part ---------------------------------------------------------------------------------------------------------
def test_sum_part_covers_every_term_exactly_once(L):
    out = (ctypes.c_size_t * 2)()
    for n in range(71):
        for parts in (1, 2, 4, 8, 16, 32, 64):
            owned = []
            for g in range(parts):
                L.dg_sum_part(n, g, parts, out)
                assert out[0] <= out[1] <= n
                owned += list(range(out[0], out[1]))
            assert owned == list(range(n)), (n, parts)


# ---- 2. the G1 sum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 67])
def test_g1_sum_of_random_terms(L, pool, n):
    pts = pool[:n]
    same_for_every_parts(L, [enc(P) for P in pts], fold(pts))


@pytest.mark.parametrize("n", [1, 2, 3, 6, 8, 65])
def test_g1_sum_of_n_copies_is_n_times_the_point(L, pool, n):
    """every addition inside a lane and every round of the tree meets equal operands"""
    P = pool[7]
    same_for_every_parts(L, [enc(P)] * n, o.E1.mul(P, n))


def test_g1_sum_of_opposite_pairs_is_the_identity(L, pool):
    P, Q = pool[3], pool[4]
    neg = o.E1.neg
    # adjacent pairs (one lane for parts <= 2 of four terms), pairs split between lanes, and a pair around other terms
    for terms in ([P, neg(P)], [P, neg(P), Q, neg(Q)], [P, Q, neg(P), neg(Q)], [P, Q, neg(Q), neg(P)], [P, Q, Q, neg(P), neg(Q), neg(Q)],
                  [P] * 4 + [neg(P)] * 4):
        same_for_every_parts(L, [enc(T) for T in terms], None)
    same_for_every_parts(L, [enc(T) for T in [P, neg(P), Q]], Q)


def test_g1_sum_with_identities_interleaved(L, pool):
    pts = [None, pool[0], None, None, pool[1], pool[2], None]
    same_for_every_parts(L, [enc(P) for P in pts], fold(pts))
    same_for_every_parts(L, [IDENT] * 5, None)
    same_for_every_parts(L, [], None)                                    # n = 0


def test_g1_sum_mask(L, pool, rnd):
    pts = pool[10:17]
    terms = [enc(P) for P in pts]
    mask = [1, 0, 1, 1, 0, 0, 1]
    same_for_every_parts(L, terms, fold(P for P, m in zip(pts, mask) if m), mask)
    same_for_every_parts(L, terms, None, [0] * 7)                       # everything masked out
    # a masked-out off-curve term (and other garbage: bad flag bits, all ones) is ignored ...
    for junk in (off_curve(rnd), bytes([0xE0]) + bytes(95), b"\xff" * 96):
        spoiled = list(terms)
        spoiled[1] = junk
        same_for_every_parts(L, spoiled, fold(P for P, m in zip(pts, mask) if m), mask)
        # ... and the same term unmasked fails the output: INVALID_ENCODING, the identity, and only that term marked
        mask2 = list(mask)
        mask2[1] = 1
        for parts in PARTS:
            assert g1_sum(L, spoiled, parts, mask2) == (INVALID, IDENT, [0, 1, 0, 0, 0, 0, 0]), parts


def test_g1_sum_membership_bytes_follow_the_mask(L, pool):
    """checked-input mode hands the kernel one verdict per term: an included term marked as no member fails the output, an
    excluded one does not"""
    pts = pool[20:25]
    terms = [enc(P) for P in pts]
    member = [1, 1, 0, 1, 1]
    for parts in PARTS:
        assert g1_sum(L, terms, parts, None, member) == (INVALID, IDENT, [0, 0, 1, 0, 0])
        st, got, bad = g1_sum(L, terms, parts, [1, 1, 0, 1, 1], member)
        assert (st, got) == (OK, enc(fold(pts[:2] + pts[3:]))) and not any(bad)


# ---- 3. the Fr sum -------------------------------------------------------------------------------------------------------
def fr_sum(L, vals, mask=None, stride=32):
    out = ctypes.create_string_buffer(32)
    blob = b"".join(int(v).to_bytes(32, "little") + bytes(stride - 32) for v in vals)
    st = L.dg_fr_sum(blob, stride, len(vals), None if mask is None else bytes(mask), out)
    return st, int.from_bytes(out.raw, "little")


def test_fr_sum(L, rnd):
    for n in (0, 1, 2, 5, 67):
        vals = [rnd.randrange(o.R) for _ in range(n)]
        assert fr_sum(L, vals) == (OK, sum(vals) % o.R)
        assert fr_sum(L, vals, stride=96) == (OK, sum(vals) % o.R)
    assert fr_sum(L, [o.R - 1, o.R - 1, 2]) == (OK, 0)
    assert fr_sum(L, [o.R - 1, o.R - 1]) == (OK, o.R - 2)
    vals = [rnd.randrange(o.R) for _ in range(6)]
    mask = [1, 1, 0, 1, 0, 1]
    assert fr_sum(L, vals, mask) == (OK, sum(v for v, m in zip(vals, mask) if m) % o.R)
    assert fr_sum(L, vals, [0] * 6) == (OK, 0)
    for bad in (o.R, o.R + 1, 2 ** 256 - 1):
        spoiled = list(vals)
        spoiled[2] = bad
        assert fr_sum(L, spoiled, mask) == (OK, sum(v for v, m in zip(vals, mask) if m) % o.R)     # masked out: ignored
        assert fr_sum(L, spoiled) == (INVALID, 0)                                                  # included: rejected


# ---- 4. interpolation at zero ----------------------------------------------------------------------------------------------
def at_zero(L, samples):
    n = len(samples)
    out = ctypes.create_string_buffer(32)
    xs = (ctypes.c_uint64 * max(n, 1))(*[x for x, _ in samples])
    st = L.dg_fr_interpolate_at_zero(n, xs, b"".join(int(y).to_bytes(32, "little") for _, y in samples), out)
    return st, int.from_bytes(out.raw, "little")


def test_interpolate_at_zero_is_coefficient_zero(L, rnd):
    assert at_zero(L, []) == (OK, 0)
    for xs in ([5], [1, 2, 4], [4, 1, 2], [0, 7, U64], [1, 2, 4, 0, U64, 3, 200, 9]):
        for ys in ([rnd.randrange(o.R) for _ in xs], [0] * len(xs), [o.R - 1] * len(xs)):
            samples = list(zip(xs, ys))
            assert at_zero(L, samples) == (OK, o.poly_interpolate(samples)[0]), xs
    # the row of a symmetric bivariate polynomial from its values at 1, 2, 4, as in the reference's test (src/poly.rs:866-871)
    row = [rnd.randrange(o.R) for _ in range(3)]
    assert at_zero(L, [(x, o.poly_evaluate(row, x)) for x in (1, 2, 4)]) == (OK, row[0])


def test_interpolate_at_zero_statuses(L, rnd):
    y = [rnd.randrange(o.R) for _ in range(4)]
    assert at_zero(L, [(3, y[0]), (8, y[1]), (3, y[2])]) == (DUPLICATE, 0)
    assert at_zero(L, [(0, y[0]), (0, y[1])]) == (DUPLICATE, 0)
    assert at_zero(L, [(U64, y[0]), (1, y[1]), (2, y[2]), (U64, y[3])]) == (DUPLICATE, 0)
    for bad in (o.R, 2 ** 256 - 1):
        assert at_zero(L, [(1, y[0]), (2, bad), (4, y[2])]) == (INVALID, 0)
        assert at_zero(L, [(1, y[0]), (1, bad)]) == (INVALID, 0)          # as job_fr_interpolate: the encoding comes first
