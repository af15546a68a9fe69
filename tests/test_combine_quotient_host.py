"""The quotient form of the [1 / D] step of the subset-grouped G2 combination on the CPU: the device headers compiled by
g++ (tests/uniform/combine_quotient_host.cpp, a test harness -- not a product path).  The decomposition is checked against
Python integers, both divide forms (forced by g_tc_force_divide_form) against Oracle B byte for byte, and the choice
between them against the multiply-adds the forms execute under -DTC_COUNT_OPS."""
import ctypes
import itertools
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import c_oracle  # noqa: E402
import tc_oracle as o  # noqa: E402

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "uniform", "combine_quotient_host.cpp")
X_ABS = 0xd201000000010000
R = X_ABS**4 - X_ABS**2 + 1
CURRENT, QUOTIENT = 1, 2


def _build(name, flags):
    lib = os.path.join(ROOT, "tests", "uniform", name)
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)) \
            or os.path.getmtime(lib) < os.path.getmtime(SRC):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w"] + flags + ["-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def L():
    assert R == o.R
    c_oracle.build()
    return _build("libcombine_quotient.so", [])


@pytest.fixture(scope="module")
def Lc():
    return _build("libcombine_quotient_cnt.so", ["-DTC_COUNT_OPS"])


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xD1F1DE)


def idx_arr(ids):
    return (ctypes.c_uint64 * len(ids))(*ids)


def small_D(L, t, ids):
    c_abs, d_abs = (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    return d_abs.value if L.cq_small_coeffs(t, idx_arr(ids), c_abs, ctypes.byref(d_abs)) else None


@pytest.fixture(scope="module")
def ten_signer_D(L):
    """the generic denominators of the 4-subsets of ten signers"""
    Ds = {small_D(L, 3, ids) for ids in itertools.combinations(range(10), 4)}
    Ds = sorted(D for D in Ds if D & (D - 1))
    assert len(Ds) == 28 and Ds[0] == 3 and Ds[-1] == 189
    return Ds


def combine(L, t, ids, shares, form):
    out = ctypes.create_string_buffer(192)
    st = L.cq_combine_g2(t, idx_arr(ids), b"".join(shares), out, form)
    return st, out.raw


def decompose(L, D):
    q, T, E = ctypes.c_uint64(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    if not L.cq_decompose(ctypes.c_uint64(D), ctypes.byref(q), T, E):
        return None
    return q.value, list(T), list(E)


# ---- the decomposition -----------------------------------------------------------------------------------
def test_decomposition_against_integers(L, rnd, ten_signer_D):
    Ds = list(range(3, 4097)) + ten_signer_D + [rnd.getrandbits(bits) | (1 << (bits - 1)) for bits in range(13, 64) for _ in range(6)]
    assert sum(1 for D in Ds if D >= 1 << 13) >= 300
    for D in Ds:
        got = decompose(L, D)
        if D & (D - 1) == 0 or D >> 62:         # the documented preconditions: not a power of two, below 2^62
            assert got is None, D
            continue
        assert got is not None, D
        q, T, E = got
        assert q == X_ABS // D and q >= 3
        assert D * sum((T[j] * q + E[j]) * (-X_ABS) ** j for j in range(4)) % R == 1, D
        assert all(2 * abs(v) <= D for v in T), (D, T)
        assert all(abs(v) <= D // 2 + 2 for v in E), (D, E)
    for D in (0, 1, 2) + tuple(1 << a for a in range(2, 64)):
        assert decompose(L, D) is None, D
    # the forms the issue quotes, as polynomials in psi
    assert decompose(L, 3)[1:] == ([0, 0, 1, 1], [0, 0, 1, 1])
    assert decompose(L, 5)[1:] == ([-2, 1, 1, 2], [-1, 0, 1, 1])
    assert decompose(L, 189)[1:] == ([-15, 75, -50, -2], [-13, 65, -43, -2])


# ---- both divide forms and the oracle ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def key_shares():
    rnd = random.Random(0x5EED2)
    out = {}
    for t in (1, 2, 3):
        P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
        poly = [rnd.randrange(o.R) for _ in range(t + 1)]
        out[t] = (P, poly, {i: o.g2_uncompressed(o.E2.mul(P, o.secret_key_share(poly, i))) for i in range(10)})
    return out


@pytest.mark.parametrize("t", [3, 2, 1])
def test_every_signer_subset_of_ten_in_both_forms(L, key_shares, t):
    P, poly, sh = key_shares[t]
    want = o.g2_uncompressed(o.E2.mul(P, poly[0]))
    generic = 0
    for ids in itertools.combinations(range(10), t + 1):
        D = small_D(L, t, ids)
        generic += D & (D - 1) != 0
        shares = [sh[i] for i in ids]
        rc, ref = c_oracle.combine_g2(t, list(ids), shares)
        assert rc == 0 and ref == want
        for form in (CURRENT, QUOTIENT, 0):
            assert combine(L, t, ids, shares, form) == (0, want), (ids, form)
    assert generic > 0 and (t != 3 or generic == 138)


def test_random_tuples_up_to_the_largest_index(L, rnd):
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    tuples = [(t, sorted(rnd.sample(range(hi), t + 1))) for t in (1, 2, 3) for hi in (40, 300, 4000, 65535) for _ in range(2)]
    tuples += [(3, [65534, 0, 65533, 1]), (1, [65534, 65533]), (2, [7, 3, 5]), (3, [65534, 65531, 65532, 65528]), (2, [65534, 1, 30000])]
    done, large = 0, 0
    for t, ids in tuples:
        poly = [rnd.randrange(o.R) for _ in range(t + 1)]
        shares = [o.g2_uncompressed(o.E2.mul(P, o.secret_key_share(poly, i))) for i in ids]
        rc, ref = c_oracle.combine_g2(t, ids, shares)
        assert rc == 0 and ref == o.g2_uncompressed(o.E2.mul(P, poly[0]))
        D = small_D(L, t, ids)
        if D is None:                                  # a product left 63 bits: the general path's job
            assert combine(L, t, ids, shares, QUOTIENT)[0] == -1
            continue
        for form in (CURRENT, QUOTIENT, 0):
            assert combine(L, t, ids, shares, form) == (0, ref), (ids, form)
        done += 1
        large += D >> 32 != 0 and D & (D - 1) != 0
    assert done >= 14 and large >= 2                   # (the quotient form with T and E of more than 31 bits among them)


def test_exceptional_shares_in_both_forms(L, rnd):
    """inputs that walk the special cases of the additions: the lanes' exception flags send them to the complete forms"""
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    S = [o.E2.mul(P, rnd.randrange(1, o.R)) for _ in range(4)]
    enc = o.g2_uncompressed
    cases = []
    for t in (1, 2, 3):
        for ids in ([0, 1, 2, 3], [2, 5, 7, 9], [1, 2, 4, 8], [0, 3, 6, 9]):
            ids = ids[:t + 1]
            base = [enc(s) for s in S[:t + 1]]
            cases.append((t, ids, [base[0]] * 2 + base[2:]))                                       # two equal shares
            cases.append((t, ids, [base[0], enc(o.E2.neg(S[0]))] + base[2:]))                      # a share and its negative
            cases.append((t, ids, [enc(None)] + base[1:]))                                         # a share at infinity
            cases.append((t, ids, base[:-1] + [enc(None)]))
            cases.append((t, ids, [enc(None)] * (t + 1)))                                          # nothing but infinity
            cases.append((t, ids, [base[0]] * (t + 1)))                                            # one point throughout
    for t, ids, shares in cases:
        rc, ref = c_oracle.combine_g2(t, ids, shares)
        assert rc == 0
        for form in (CURRENT, QUOTIENT):
            assert combine(L, t, ids, shares, form) == (0, ref), (t, ids, form)


def test_division_of_the_identity_raises_the_flag(L):
    """Q at infinity: both forms flag the lane (combine_uniform_wave then recomputes it by the complete form)"""
    for D in (3, 5, 189):
        for form in (CURRENT, QUOTIENT):
            out = ctypes.create_string_buffer(192)
            assert L.cq_divide(form, ctypes.c_uint64(D), o.g2_uncompressed(None), out) == 1


# ---- the choice --------------------------------------------------------------------------------------------
def _macs(c, lanes=2):
    """tests/count_ops.py macs(): limb multiply-adds of a G2 job body (two lanes per job)"""
    mul2, smul, ssqr, mul, sqr = c
    return mul2 * 588 + smul * 392 + ssqr * 301 + lanes * ((mul - smul) * 392 + (sqr - ssqr) * 301)


def test_choice_is_the_form_that_executes_fewer_multiply_adds(Lc, rnd, ten_signer_D):
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    pt = o.g2_uncompressed(P)

    def executed(form, D):
        out = ctypes.create_string_buffer(192)
        assert Lc.cq_divide(form, ctypes.c_uint64(D), pt, out) == 0
        a = (ctypes.c_uint64 * 5)()
        Lc.cq_divide_counts5(a)
        return _macs(tuple(a)), out.raw

    tried = ten_signer_D + [6 * 35 * 11, 4095, 12345] + [rnd.getrandbits(bits) | (1 << (bits - 1)) | 1 for bits in (10, 12, 13, 14, 15, 16, 17, 18, 24, 33, 48, 61)]
    tried += [(1 << 20) + 1, (1 << 21) + 7, 3 << 30]
    chose_quotient = {}
    for D in tried:
        cur, quo = ctypes.c_uint32(), ctypes.c_uint32()
        choice = Lc.cq_choice(ctypes.c_uint64(D), ctypes.byref(cur), ctypes.byref(quo))
        want = o.g2_uncompressed(o.E2.mul(P, 6 * pow(D, -1, o.R) % o.R))      # (the harness divides [6] P)
        m_cur, got_cur = executed(CURRENT, D)
        m_quo, got_quo = executed(QUOTIENT, D)
        assert got_cur == want and got_quo == want, D
        assert (cur.value, quo.value) == (m_cur, m_quo), D                    # the prediction is the count
        assert choice == (1 if m_quo < m_cur else 0), (D, m_cur, m_quo)
        chose_quotient[D] = choice
    assert all(chose_quotient[D] for D in ten_signer_D)
    assert not any(chose_quotient[D] for D in tried if D >> 20)
    # a power of two, a D of 2^62 or more: no decomposition, the current form
    cur, quo = ctypes.c_uint32(), ctypes.c_uint32()
    for D in (1 << 17, (1 << 62) + 3):
        assert Lc.cq_choice(ctypes.c_uint64(D), ctypes.byref(cur), ctypes.byref(quo)) == 0 and quo.value == 0


def test_unit_costs_of_the_prediction(Lc, rnd):
    """what the prediction charges per doubling and per mixed addition is what they execute"""
    pt = o.g2_uncompressed(o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R)))
    got = []
    for which in (0, 1):
        Lc.cq_one_step(which, pt)
        a = (ctypes.c_uint64 * 5)()
        Lc.cq_op_counts5(a, 1)
        got.append(_macs(tuple(a)))
    assert got == [Lc.cq_macs_dbl(), Lc.cq_macs_add()]
    assert 1.7 < got[1] / got[0] < 1.9          # "one mixed addition is 1.75 doublings"
