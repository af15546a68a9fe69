"""The planned quotient form of the [1 / D] step of the subset-grouped G2 combination on the CPU: the device headers compiled
by g++ (tests/uniform/combine_plan_host.cpp, a test harness -- not a product path).  tc_jobs.h combine_quotient_plan picks, per
denominator, the shift m of the ladder scalar q + m and the NAF width that execute the fewest multiply-adds.  Checked here: the
identity the shifted digits must satisfy (Python integers), the prediction against the -DTC_COUNT_OPS count of the executed
division, "never dearer than m = 0, width 3", and the canonical bytes of Oracle B for every signer subset of ten."""
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
SRC = os.path.join(ROOT, "tests", "uniform", "combine_plan_host.cpp")
X_ABS = 0xd201000000010000
R = X_ABS**4 - X_ABS**2 + 1
WIDTHS = (2, 3, 4)


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
    return _build("libcombine_plan.so", [])


@pytest.fixture(scope="module")
def Lc():
    return _build("libcombine_plan_cnt.so", ["-DTC_COUNT_OPS"])


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0x91A7)


def idx_arr(ids):
    return (ctypes.c_uint64 * len(ids))(*ids)


def small_D(L, t, ids):
    c_abs, d_abs = (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    return d_abs.value if L.cp_small_coeffs(t, idx_arr(ids), c_abs, ctypes.byref(d_abs)) else None


def generic(D):
    return D >= 3 and D & (D - 1) != 0


@pytest.fixture(scope="module")
def ten_signer_D(L):
    """the generic ones of the 35 denominators of the 2-, 3- and 4-subsets of ten signers (the other seven are 1 .. 64: no division,
    or the form of the powers of two)"""
    Ds = {small_D(L, t, ids) for t in (1, 2, 3) for ids in itertools.combinations(range(10), t + 1)}
    assert len(Ds) == 35 and Ds == {small_D(L, 3, ids) for ids in itertools.combinations(range(10), 4)}
    Ds = sorted(D for D in Ds if generic(D))
    assert len(Ds) == 28 and Ds[0] == 3 and Ds[-1] == 189
    return Ds


def decompose(L, D):
    q, T, E = ctypes.c_uint64(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    if not L.cp_decompose(ctypes.c_uint64(D), ctypes.byref(q), T, E):
        return None
    return q.value, list(T), list(E)


def force_of(m, width):
    return 16 * (m + 8) + width


def plan(L, D, force=0):
    """(m, width, its multiply-adds, those of m = 0 and width 3, those of the 4-dimensional ladder), None without a decomposition"""
    out = (ctypes.c_int64 * 5)()
    return tuple(out) if L.cp_plan(ctypes.c_uint64(D), force, out) else None


# ---- the identity -------------------------------------------------------------------------------------------
def test_planned_digits_against_integers(L, rnd, ten_signer_D):
    lo, hi = L.cp_shift_lo(), L.cp_shift_hi()
    assert lo <= 0 < hi
    Ds = list(range(3, 4097)) + ten_signer_D + [rnd.getrandbits(bits) | (1 << (bits - 1)) for bits in range(13, 62) for _ in range(6)]
    Ds += [(1 << 61) + 1, (1 << 62) - 1, X_ABS // 3, X_ABS // 4 + 1, X_ABS // 5]      # (q = 3, 4 and 5: q + m >= 3 binds)
    moved, widths = 0, set()
    for D in Ds:
        got = plan(L, D)
        if not generic(D) or D >> 62:
            assert got is None, D
            continue
        m, width, macs, parent, _ = got
        q, T, E = decompose(L, D)
        Ep = [E[j] - m * T[j] for j in range(4)]
        assert lo <= m <= hi and width in WIDTHS and q + m >= 3, (D, m, width)
        assert D * sum((T[j] * (q + m) + Ep[j]) * (-X_ABS) ** j for j in range(4)) % R == 1, D
        assert all(abs(e) < 1 << 63 for e in Ep), (D, Ep)                                # what quot_naf and the column loop accept
        assert macs <= parent, (D, got)                                                   # never dearer than before the plan
        assert (macs < parent) == ((m, width) != (0, 3)), (D, got)                        # ties stay with m = 0, width 3
        moved += m != 0
        widths.add(width)
    assert moved > 100 and widths == set(WIDTHS)


def test_plan_is_the_cheapest_candidate(L, rnd, ten_signer_D):
    """the plan against every candidate's own prediction (each forced in turn)"""
    lo, hi = L.cp_shift_lo(), L.cp_shift_hi()
    for D in ten_signer_D + [rnd.getrandbits(bits) | (1 << (bits - 1)) | 1 for bits in (9, 12, 17, 24, 40, 61)]:
        q = decompose(L, D)[0]
        best = plan(L, D)
        cands = {(m, w): plan(L, D, force_of(m, w))[2] for m in range(lo, hi + 1) for w in WIDTHS if q + m >= 3}
        assert cands[(0, 3)] == best[3], D                          # combine_divide_quotient_macs is the candidate (0, 3)
        assert best[2] == min(cands.values()) and cands[(best[0], best[1])] == best[2], (D, best, cands)


# ---- the prediction is the count -------------------------------------------------------------------------------
def _macs(c, lanes=2):
    """tests/count_ops.py macs(): limb multiply-adds of a G2 job body (two lanes per job)"""
    mul2, smul, ssqr, mul, sqr = c
    return mul2 * 588 + smul * 392 + ssqr * 301 + lanes * ((mul - smul) * 392 + (sqr - ssqr) * 301)


def test_prediction_is_the_count_and_never_above_the_parent(Lc, rnd, ten_signer_D):
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    pt = o.g2_uncompressed(P)

    def executed(D, force):
        out = ctypes.create_string_buffer(192)
        assert Lc.cp_divide(ctypes.c_uint64(D), force, pt, out) == 0
        a = (ctypes.c_uint64 * 5)()
        Lc.cp_divide_counts5(a)
        return _macs(tuple(a)), out.raw

    others = [6 * 35 * 11, 4095, 12345, (1 << 20) + 1, (1 << 21) + 7, 3 << 30]
    others += [rnd.getrandbits(bits) | (1 << (bits - 1)) | 1 for bits in (10, 12, 13, 14, 15, 16, 17, 18, 24, 33, 48, 61)]
    assert len(others) >= 12
    widths = set()
    for D in ten_signer_D + others:
        want = o.g2_uncompressed(o.E2.mul(P, 6 * pow(D, -1, o.R) % o.R))      # (the harness divides [6] P)
        m, width, macs, parent, _ = plan(Lc, D)
        count, got = executed(D, 0)
        assert got == want, D
        assert macs == count, (D, m, width, macs, count)                      # the prediction is the count
        count3, got3 = executed(D, force_of(0, 3))
        assert got3 == want and count3 == parent and count <= count3, (D, count, count3)
        widths.add(width)
    assert widths == set(WIDTHS)
    # every candidate of a few denominators: its prediction is its count, its result the same point
    for D in (3, 7, 9, 35, 189, 12345):
        q = decompose(Lc, D)[0]
        want = o.g2_uncompressed(o.E2.mul(P, 6 * pow(D, -1, o.R) % o.R))
        for m in (-1, 0, 1):                                                  # (m = -1: a candidate only the tests force)
            for w in WIDTHS:
                if q + m < 3:
                    continue
                count, got = executed(D, force_of(m, w))
                assert got == want and plan(Lc, D, force_of(m, w))[:3] == (m, w, count), (D, m, w)


_BOUND_CHILD = """
import ctypes, sys
lib, pt = ctypes.CDLL(sys.argv[1]), bytes.fromhex(sys.argv[2])
for D in (3, 5, 7, 9, 35, 36, 84, 112, 189, 286, 12345, (1 << 20) + 1, (1 << 40) + 9):
    for m in (-1, 0, 1):
        for w in (2, 3, 4):
            out = ctypes.create_string_buffer(192)
            assert lib.cp_divide(ctypes.c_uint64(D), 16 * (m + 8) + w, pt, out) == 0, (D, m, w)
            print(D, m, w, out.raw.hex())
"""


def test_every_candidate_under_the_bound_analysis(rnd):
    """the -DTC_BOUND_CHECK build (interval bookkeeping of every limb and value, tc_field.h) runs every candidate of a few
    denominators: the table entries of width 2 and width 4 stay inside the entry contract.  In a child process: a violation
    aborts it."""
    lib = os.path.join(ROOT, "tests", "uniform", "libcombine_plan_bc.so")
    _build("libcombine_plan_bc.so", ["-DTC_BOUND_CHECK", "-pthread"])
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    r = subprocess.run([sys.executable, "-c", _BOUND_CHILD, lib, o.g2_uncompressed(P).hex()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == 13 * 9
    want = {}
    for D, m, w, got in lines:
        if D not in want:
            want[D] = o.g2_uncompressed(o.E2.mul(P, 6 * pow(int(D), -1, o.R) % o.R)).hex()     # (the harness divides [6] P)
        assert got == want[D], (D, m, w)


# ---- bytes ---------------------------------------------------------------------------------------------------
def combine(L, t, ids, shares, form, force=0):
    out = ctypes.create_string_buffer(192)
    st = L.cp_combine_g2(t, idx_arr(ids), b"".join(shares), out, form, force)
    return st, out.raw


@pytest.fixture(scope="module")
def key_shares():
    rnd = random.Random(0x5EED3)
    out = {}
    for t in (1, 2, 3):
        P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
        poly = [rnd.randrange(o.R) for _ in range(t + 1)]
        out[t] = (P, poly, {i: o.g2_uncompressed(o.E2.mul(P, o.secret_key_share(poly, i))) for i in range(10)})
    return out


def test_every_signer_subset_of_ten_gives_the_oracle_bytes(L, key_shares):
    reached = set()
    for t in (1, 2, 3):
        P, poly, sh = key_shares[t]
        want = o.g2_uncompressed(o.E2.mul(P, poly[0]))
        for ids in itertools.combinations(range(10), t + 1):
            shares = [sh[i] for i in ids]
            rc, ref = c_oracle.combine_g2(t, list(ids), shares)
            assert rc == 0 and ref == want
            D = small_D(L, t, ids)
            if generic(D):
                m, width, macs, _, ladder = plan(L, D)
                assert macs < ladder, D                                  # the wave's own choice IS the planned form
                reached.add((width, m != 0))
            for form in (0, 2):
                assert combine(L, t, ids, shares, form) == (0, want), (ids, form)
    assert {w for w, _ in reached} == set(WIDTHS) and any(moved for _, moved in reached), reached


def test_exceptional_shares(L, rnd, ten_signer_D):
    """inputs that walk the special cases of the additions: the lanes' exception flags send them to the complete forms.  The
    index tuples have denominators that plan width 4, width 2 and m = 1 among them."""
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    S = [o.E2.mul(P, rnd.randrange(1, o.R)) for _ in range(4)]
    enc = o.g2_uncompressed
    planned = set()
    for t in (1, 2, 3):
        for ids in ([0, 1, 2, 3], [2, 5, 7, 9], [0, 1, 4, 8], [0, 3, 6, 9], [0, 2, 5, 9], [1, 2, 3, 8]):
            ids = ids[:t + 1]
            D = small_D(L, t, ids)
            if generic(D):
                planned.add(plan(L, D)[:2])
            base = [enc(s) for s in S[:t + 1]]
            cases = [[base[0]] * 2 + base[2:],                                # two equal shares
                     [base[0], enc(o.E2.neg(S[0]))] + base[2:],               # a share and its negative
                     [enc(None)] + base[1:], base[:-1] + [enc(None)],         # a share at infinity
                     [enc(None)] * (t + 1),                                   # nothing but infinity
                     [base[0]] * (t + 1)]                                     # one point throughout
            for shares in cases:
                rc, ref = c_oracle.combine_g2(t, ids, shares)
                assert rc == 0
                for form in (0, 2):
                    assert combine(L, t, ids, shares, form) == (0, ref), (t, ids, form)
    assert {w for _, w in planned} == set(WIDTHS) and any(m for m, _ in planned), planned


def test_division_of_the_identity_raises_the_flag(L):
    """Q at infinity: the planned form flags the lane at every width (combine_uniform_wave then recomputes it)"""
    for D in (3, 5, 7, 9, 189):
        for force in (0, force_of(0, 2), force_of(1, 3), force_of(-1, 4)):
            out = ctypes.create_string_buffer(192)
            assert L.cp_divide(ctypes.c_uint64(D), force, o.g2_uncompressed(None), out) == 1, (D, force)


def test_device_probe_cross_compiles_for_gfx950():
    """tests/device/plan_probe.hip (what tests/test_gpu_combine_plan.py runs) builds with the product's flags, without a GPU"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import device_conformance as dc
    from threshold_crypto_amd import build as tcb
    src = os.path.join(dc.DEV, "plan_probe.hip")
    lib = dc._build("libtc_plan_probe", lambda out: [dc.hipcc()] + tcb.FLAGS + ["-w", "-shared", "-I" + dc.CSRC, src, "-o", out], {"plan_probe.hip"})
    assert os.path.getsize(lib) > 0
