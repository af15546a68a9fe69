"""The Fr routines of the DKG verification entries on the CPU: the device headers compiled by g++
(tests/dkg/dkg_verify_host.cpp, a test harness -- not a product path).  Poly::evaluate and BivarPoly::row against Oracle A,
the random scalars of the combined values check against a Python ChaCha20, its d+2 scalars against Python sums, and the
identity  sum_i c_i R_i + c_g g1 == 0  in Oracle A's G1: it holds for honest values and fails for one wrong value and for a
+delta / -delta pair (which cancels in the UNWEIGHTED sum, so the weights are seen to be applied)."""
import ctypes
import os
import random
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tc_oracle as o  # noqa: E402

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "dkg", "dkg_verify_host.cpp")
U64 = 2 ** 64 - 1
ABSCISSAE = [0, 1, 2, 5, U64]


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)) \
        or os.path.getmtime(path) < os.path.getmtime(SRC)


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "dkg", "libdkg_verify_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    lib.dv_rlc_rho.restype = ctypes.c_uint64
    lib.dv_rlc_rho.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    lib.dv_fr_poly_evaluate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    lib.dv_bivar_poly_row.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p]
    lib.dv_rlc_scalars.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p,
                                   ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xD1C7)


def le32(v):
    return int(v).to_bytes(32, "little")


def evaluate(L, coeffs, x):
    out = ctypes.create_string_buffer(32)
    st = L.dv_fr_poly_evaluate(b"".join(le32(c) for c in coeffs), len(coeffs), le32(x), out)
    return st, int.from_bytes(out.raw, "little")


def row(L, degree, coeff, x):
    out, st = ctypes.create_string_buffer(32 * (degree + 1)), ctypes.create_string_buffer(degree + 1)
    L.dv_bivar_poly_row(b"".join(le32(c) for c in coeff), degree, x, out, st)
    return list(st.raw), [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(degree + 1)]


def rho(seed, counter):
    w = o.chacha20_block(struct.unpack("<8I", seed), counter)
    return (w[0] | 1) | (w[1] << 32)


def scalars(L, seed, j, degree, xs, vals):
    n = len(xs)
    out = ctypes.create_string_buffer(32 * (degree + 2))
    ok = L.dv_rlc_scalars(seed, j, n, degree, (ctypes.c_uint64 * n)(*xs), b"".join(le32(v) for v in vals), out)
    return ok, [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(degree + 2)]


# ---- Poly::evaluate and BivarPoly::row ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 2, 7])
def test_fr_poly_evaluate_matches_oracle(L, rnd, degree):
    polys = [[rnd.randrange(o.R) for _ in range(degree + 1)], [0] * (degree + 1), [o.R - 1] * (degree + 1),
             [rnd.choice([0, o.R - 1, rnd.randrange(o.R)]) for _ in range(degree + 1)]]
    for coeffs in polys:
        for x in [0, 1, U64, o.R - 1, rnd.randrange(o.R)]:
            assert evaluate(L, coeffs, x) == (0, o.poly_evaluate(coeffs, x)), (coeffs, x)


def test_fr_poly_evaluate_zero_polynomial_and_rejections(L, rnd):
    assert evaluate(L, [], 5) == (0, 0)                                  # n = 0: the zero polynomial
    coeffs = [rnd.randrange(o.R) for _ in range(3)]
    for bad in (o.R, o.R + 1, 2 ** 256 - 1):
        assert evaluate(L, coeffs[:1] + [bad] + coeffs[2:], 3) == (3, 0)   # a coefficient >= r: TC_JOB_INVALID_ENCODING, zero
        assert evaluate(L, coeffs, bad) == (3, 0)                          # ... and an abscissa


@pytest.mark.parametrize("degree", [0, 2, 7])
def test_bivar_poly_row_matches_oracle(L, rnd, degree):
    ncoeff = (degree + 1) * (degree + 2) // 2
    sets = [[rnd.randrange(o.R) for _ in range(ncoeff)], [0] * ncoeff, [o.R - 1] * ncoeff]
    for coeff in sets:
        for x in [0, 1, U64, 200]:
            assert row(L, degree, coeff, x) == ([0] * (degree + 1), o.bivar_poly_row(degree, coeff, x)), x


def test_bivar_poly_row_rejects_only_the_rows_that_depend_on_a_bad_coefficient(L, rnd):
    degree = 2
    coeff = [rnd.randrange(o.R) for _ in range(6)]
    want = o.bivar_poly_row(degree, coeff, 7)
    bad = list(coeff)
    bad[o.coeff_pos(0, 2)] = o.R                                             # coefficient (0, 2) = (2, 0): rows 0 and 2
    st, got = row(L, degree, bad, 7)
    assert st == [3, 0, 3] and got == [0, want[1], 0]


# ---- the scalars of the combined values check --------------------------------------------------------------------
def test_rho_is_the_chacha20_block_of_its_counter(L, rnd):
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    for counter in [0, 1, 2, 69, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5]:
        got = L.dv_rlc_rho(seed, counter)
        assert got == rho(seed, counter) and got & 1 and got < 2 ** 64


def _case(rnd, degree):
    poly = [rnd.randrange(o.R) for _ in range(degree + 1)]
    commit = o.commitment(poly)
    vals = [o.poly_evaluate(poly, x) for x in ABSCISSAE]
    return poly, commit, vals


def _combination(commit, sc):
    acc = None
    for c, p in zip(sc, commit + [o.G1_GEN]):
        acc = o.E1.add(acc, o.E1.mul(p, c))
    return acc


@pytest.mark.parametrize("degree", [2, 7])
def test_scalars_equal_the_python_sums_and_the_identity_holds(L, rnd, degree):
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    _, commit, vals = _case(rnd, degree)
    n, j = len(ABSCISSAE), 3
    ok, sc = scalars(L, seed, j, degree, ABSCISSAE, vals)
    rhos = [rho(seed, j * n + k) for k in range(n)]
    want = [sum(r * pow(x, i, o.R) for r, x in zip(rhos, ABSCISSAE)) % o.R for i in range(degree + 1)]      # pow(0, 0) == 1
    want.append(-sum(r * v for r, v in zip(rhos, vals)) % o.R)
    assert ok == 1 and sc == want
    assert _combination(commit, sc) is None                                  # honest values: the identity
    # one wrong value
    wrong = list(vals)
    wrong[2] = (wrong[2] + 1) % o.R
    ok, sc = scalars(L, seed, j, degree, ABSCISSAE, wrong)
    assert ok == 1 and _combination(commit, sc) is not None
    # +9 and -9: the unweighted sum of the values is unchanged, the weighted one is not
    pair = list(vals)
    pair[1], pair[3] = (pair[1] + 9) % o.R, (pair[3] - 9) % o.R
    assert sum(pair) % o.R == sum(vals) % o.R
    ok, sc = scalars(L, seed, j, degree, ABSCISSAE, pair)
    assert ok == 1 and _combination(commit, sc) is not None


def test_two_jobs_with_equal_inputs_get_different_rho(L, rnd):
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    _, _, vals = _case(rnd, 2)
    a = scalars(L, seed, 0, 2, ABSCISSAE, vals)
    b = scalars(L, seed, 1, 2, ABSCISSAE, vals)
    assert a[0] == b[0] == 1 and a[1] != b[1]
    n = len(ABSCISSAE)
    assert len({rho(seed, c) for c in range(2 * n)}) == 2 * n and L.dv_rlc_rho(seed, 0) != L.dv_rlc_rho(seed, n)


def test_a_non_canonical_value_is_flagged(L, rnd):
    seed = bytes(rnd.getrandbits(8) for _ in range(32))
    _, _, vals = _case(rnd, 2)
    vals[4] = o.R
    ok, sc = scalars(L, seed, 0, 2, ABSCISSAE, vals)
    assert ok == 0 and sc[-1] == 0
