"""The subset-grouped G2 combination on the CPU: the device headers compiled by g++ (tests/uniform, a test harness -- not a
product path).  On the host one job is a wave, so job_combine_small takes the wave-uniform forms (the table-free NAF
short ladder and the width-4 NAF [1 / D] ladder); g_tc_force_mixed_combine reaches the forms of a mixed wave.  Both are
compared with Oracle B byte for byte; the recodings, psi^2 at the look-up and the grouping plan are checked on their own."""
import ctypes
import itertools
import json
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
SRC = os.path.join(ROOT, "tests", "uniform", "combine_uniform_host.cpp")
MACS_JSON = os.path.join(ROOT, "profiles", "combine_uniform_macs.json")
X_ABS = 0xd201000000010000


def _build(name, flags):
    lib = os.path.join(ROOT, "tests", "uniform", name)
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)) \
            or os.path.getmtime(lib) < os.path.getmtime(SRC):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w"] + flags + ["-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def L():
    c_oracle.build()
    return _build("libcombine_uniform.so", [])


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xC0B1)


@pytest.fixture(scope="module")
def key_shares():
    """per threshold: the message point, the polynomial and the encoded shares of signers 0..9"""
    rnd = random.Random(0x5EED)
    out = {}
    for t in (1, 2, 3):
        P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
        poly = [rnd.randrange(o.R) for _ in range(t + 1)]
        out[t] = (P, poly, {i: o.g2_uncompressed(o.E2.mul(P, o.secret_key_share(poly, i))) for i in range(10)})
    return out


def buf(n):
    return ctypes.create_string_buffer(n)


def idx_arr(ids):
    return (ctypes.c_uint64 * len(ids))(*ids)


def combine(L, t, ids, shares, mixed):
    out = buf(192)
    st = L.cu_combine_g2(t, idx_arr(ids), b"".join(shares), out, mixed)
    return st, out.raw


# ---- recodings ----------------------------------------------------------------------------------------
def _values64(rnd):
    return [0, 1, 2, 3, 7, 8, 9, 15, 16, 2**63, 2**64 - 1, X_ABS - 1, X_ABS, 0xAAAAAAAAAAAAAAAA, 0x7777777777777777] + \
           [rnd.getrandbits(64) for _ in range(400)] + [rnd.getrandbits(rnd.randrange(1, 65)) for _ in range(200)]


def test_width4_naf_of_a_digit(L, rnd):
    cols = L.cu_wnaf_cols()
    assert cols == 65
    for d in _values64(rnd):
        dig = (ctypes.c_int8 * cols)()
        L.cu_wnaf4(ctypes.c_uint64(d), dig)
        dig = list(dig)
        assert sum(v << i for i, v in enumerate(dig)) == d
        nz = [i for i, v in enumerate(dig) if v]
        assert all(dig[i] % 2 == 1 and abs(dig[i]) <= 7 for i in nz)
        assert all(b - a >= 4 for a, b in zip(nz, nz[1:]))


def test_naf_of_a_short_coefficient(L, rnd):
    for c in [v >> 1 for v in _values64(rnd)]:       # the coefficients of the fast path stay below 2^63
        pos, neg = ctypes.c_uint64(), ctypes.c_uint64()
        L.cu_naf(ctypes.c_uint64(c), ctypes.byref(pos), ctypes.byref(neg))
        pos, neg = pos.value, neg.value
        assert pos - neg == c and pos & neg == 0
        nz = pos | neg
        assert nz & (nz >> 1) == 0                    # no two adjacent nonzero digits


def test_psi_squared_at_the_look_up(L, rnd):
    """psi^2(x, y) = (PSI2_CX x, -y): what g2_wnaf_ladder derives from the stored entries, against g2_psi o g2_psi"""
    for _ in range(4):
        P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
        a, b = buf(192), buf(192)
        assert L.cu_psi2(o.g2_uncompressed(P), a, b) == 0
        assert a.raw == b.raw
        assert a.raw == o.g2_uncompressed(o.E2.mul(P, X_ABS * X_ABS % o.R))   # psi = [x] on G2


# ---- the two forms and the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("t", [3, 2, 1])
def test_every_signer_subset_of_ten(L, key_shares, t):
    P, poly, sh = key_shares[t]
    want = o.g2_uncompressed(o.E2.mul(P, poly[0]))
    for ids in itertools.combinations(range(10), t + 1):
        shares = [sh[i] for i in ids]
        rc, ref = c_oracle.combine_g2(t, list(ids), shares)
        assert rc == 0 and ref == want
        assert combine(L, t, ids, shares, 0) == (0, want), ids
        assert combine(L, t, ids, shares, 1) == (0, want), ids


def test_random_tuples_up_to_the_largest_index(L, rnd):
    P = o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    done = 0
    tuples = [(t, sorted(rnd.sample(range(hi), t + 1))) for t in (1, 2, 3) for hi in (40, 300, 65535) for _ in range(2)]
    tuples += [(3, [65534, 0, 65533, 1]), (1, [65534, 65533]), (2, [7, 3, 5])]       # unsorted tuples are tuples too
    for t, ids in tuples:
        poly = [rnd.randrange(o.R) for _ in range(t + 1)]
        shares = [o.g2_uncompressed(o.E2.mul(P, o.secret_key_share(poly, i))) for i in ids]
        rc, ref = c_oracle.combine_g2(t, ids, shares)
        assert rc == 0 and ref == o.g2_uncompressed(o.E2.mul(P, poly[0]))
        st, got = combine(L, t, ids, shares, 0)
        if st == -1:                                  # a product left 63 bits: the general path's job
            assert combine(L, t, ids, shares, 1)[0] == -1
            continue
        assert (st, got) == (0, ref), ids
        assert combine(L, t, ids, shares, 1) == (0, ref), ids
        done += 1
    assert done >= 12


def test_exceptional_shares(L, rnd):
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
        assert combine(L, t, ids, shares, 0) == (0, ref), (t, ids)
        assert combine(L, t, ids, shares, 1) == (0, ref), (t, ids)


# ---- the grouping plan ------------------------------------------------------------------------------------
def _plan(L, t, idx_rows):
    B = len(idx_rows)
    n = t + 1
    flat = (ctypes.c_uint64 * (B * n))(*[v for row in idx_rows for v in row])
    L.cu_group_slots.restype = ctypes.c_uint32
    slots = L.cu_group_slots(ctypes.c_size_t(B))
    perm = (ctypes.c_uint32 * slots)()
    starts = (ctypes.c_uint32 * 512)()
    orders = (ctypes.c_uint8 * 512)()
    groups = ctypes.c_uint32()
    mode = L.cu_plan(t, flat, ctypes.c_size_t(n), ctypes.c_size_t(B), perm, starts, orders, ctypes.byref(groups))
    return mode, list(perm), list(starts), list(orders), groups.value


def _check_perm(t, idx_rows, mode, perm, pad):
    B = len(idx_rows)
    placed = [p for p in perm if p != 0xffffffff]
    assert sorted(placed) == list(range(B))                      # every job exactly once
    # whole waves of one group: a wave never holds two keys (subset mode) / two classes
    for w in range(0, len(perm), pad):
        jobs = [p for p in perm[w:w + pad] if p != 0xffffffff]
        if mode == 1:
            assert len({tuple(idx_rows[j]) for j in jobs}) <= 1
    first = {}
    for pos, j in enumerate(perm):
        if j != 0xffffffff and mode == 1:
            first.setdefault(tuple(idx_rows[j]), pos)
    assert all(pos % pad == 0 for pos in first.values())        # groups start on multiples of the wave


@pytest.mark.parametrize("B", [1, 31, 32, 33, 4096])
def test_plan_places_every_job_once(L, rnd, B):
    subsets = list(itertools.combinations(range(10), 4))
    limit = (B // 8) // 32                                        # 32 G <= B / 8
    for G in sorted({max(limit, 1), limit + 1, 1}):
        G = min(G, B)
        chosen = rnd.sample(subsets, G)
        rows = [list(chosen[i % G]) for i in range(B)]
        rnd.shuffle(rows)
        mode, perm, starts, orders, groups = _plan(L, 3, rows)
        assert groups == G
        assert mode == (1 if 32 * G <= B // 8 else 0), (B, G)
        _check_perm(3, rows, mode, perm, 32 if mode else 64)
        if mode:
            # generic, then 2^a, then 1: the order of the classes along the permutation never decreases
            seq = [orders[i] for i in sorted((i for i in range(512) if starts[i] != 0xffffffff), key=lambda i: starts[i])]
            assert seq == sorted(seq)


def test_plan_modes(L, rnd):
    subsets = list(itertools.combinations(range(10), 4))
    rows = [list(subsets[i % 210]) for i in range(65536)]
    assert _plan(L, 3, rows)[0] == 1                              # the benchmark's shape: 210 subsets of 65 536 jobs
    rows = [list(subsets[i % 210]) for i in range(4096)]
    mode, perm, *_ = _plan(L, 3, rows)
    assert mode == 0                                              # 210 groups would pad 4096 jobs by far more than an eighth
    _check_perm(3, rows, mode, perm, 64)
    many = rnd.sample(list(itertools.combinations(range(16), 4)), 300)
    rows = [list(many[i % 300]) for i in range(65536)]
    mode, perm, _, _, groups = _plan(L, 3, rows)
    assert mode == 0 and groups > 256                             # more tuples than the table admits
    _check_perm(3, rows, mode, perm, 64)
    # jobs the fast path leaves (an index of 65 535, a repeated index) share one group, the last
    rows = [[0, 1, 2, 3]] * 100 + [[0, 1, 2, 65535]] * 3 + [[4, 4, 5, 6]] * 2 + [[1, 2, 3, 4]] * 4000
    mode, perm, starts, orders, groups = _plan(L, 3, rows)
    assert mode == 1 and groups == 3
    _check_perm(3, [r if r[3] != 65535 and r[0] != r[1] else ["none"] for r in rows], mode, perm, 32)
    assert sorted(orders[i] for i in range(512) if starts[i] != 0xffffffff)[-1] == 3


# ---- executed multiply-adds ---------------------------------------------------------------------------------
def _macs(c, lanes=2):
    """tests/count_ops.py macs(): limb multiply-adds of a G2 job body (two lanes per job)"""
    mul2, smul, ssqr, mul, sqr = c
    return mul2 * 588 + smul * 392 + ssqr * 301 + lanes * ((mul - smul) * 392 + (sqr - ssqr) * 301)


def test_uniform_form_executes_fewer_multiply_adds(key_shares):
    Lc = _build("libcombine_uniform_cnt.so", ["-DTC_COUNT_OPS"])
    P, poly, sh = key_shares[3]

    def cnt():
        a = (ctypes.c_uint64 * 5)()
        Lc.cu_op_counts5(a, 1)
        return tuple(a)

    table, generic = {}, 0
    for ids in itertools.combinations(range(10), 4):
        c_abs, d_abs = (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
        assert Lc.cu_small_coeffs(3, idx_arr(ids), c_abs, ctypes.byref(d_abs))
        D = d_abs.value
        shares = [sh[i] for i in ids]
        cnt()
        assert combine(Lc, 3, ids, shares, 0)[0] == 0
        uni = _macs(cnt())
        assert combine(Lc, 3, ids, shares, 1)[0] == 0
        old = _macs(cnt())
        is_generic = D & (D - 1) != 0
        if is_generic:
            generic += 1
            assert uni < old, (ids, uni, old)
        else:
            assert uni <= old, (ids, uni, old)
        table[" ".join(map(str, ids))] = {"D": D, "uniform_v_mad": uni, "mixed_wave_v_mad": old}
    assert generic == 138
    g = [v for v in table.values() if v["D"] & (v["D"] - 1)]
    doc = {"_comment": "limb multiply-adds per job of the G2 fast combine at t = 3 over every 4-subset of 10 signers: the wave-uniform forms "
                       "(a wave of one subset) and the forms of a mixed wave; written by tests/test_combine_uniform_host.py",
           "generic_mean_uniform": sum(v["uniform_v_mad"] for v in g) // len(g),
           "generic_mean_mixed_wave": sum(v["mixed_wave_v_mad"] for v in g) // len(g),
           "all_mean_uniform": sum(v["uniform_v_mad"] for v in table.values()) // len(table),
           "all_mean_mixed_wave": sum(v["mixed_wave_v_mad"] for v in table.values()) // len(table),
           "subsets": table}
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if os.access(os.path.dirname(MACS_JSON), os.W_OK) and (not os.path.exists(MACS_JSON) or open(MACS_JSON).read() != text):
        try:
            with open(MACS_JSON, "w") as f:
                f.write(text)
        except OSError:
            pass
