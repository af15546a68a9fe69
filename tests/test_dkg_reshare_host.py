"""The routines of the DKG resharing on the CPU: the device headers compiled by g++ (tests/dkg/dkg_reshare_host.cpp, a test
harness -- not a product path).  The harness runs one output of k_g1_wsum the way the kernel does -- the weights recoded once per
term, the partial sums of the lanes g = 0 .. parts-1, then the xor tree of complete additions -- so the cases below meet
w_a P_a = +-w_b P_b inside a lane and across lanes.  Everything is compared with Oracle A: E1.mul / E1.add, Python integers mod r,
and a Python model of the selection rule."""
import ctypes
import itertools
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tc_oracle as o  # noqa: E402

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "dkg", "dkg_reshare_host.cpp")
U64 = 2 ** 64 - 1
IDENT = bytes([0x40]) + bytes(95)
PARTS = [1, 2, 4, 64]
OK, DUPLICATE, INVALID, MISMATCH = 0, 2, 3, 4


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)) \
        or os.path.getmtime(path) < os.path.getmtime(SRC)


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "dkg", "libdkg_reshare_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, p, v = ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p
    lib.dr_g1_wsum.argtypes = [p, sz, sz, p, p, p, sz, p, p]
    lib.dr_g1_wsum_sel.argtypes = [p, sz, sz, p, p, v, sz, sz, p]
    lib.dr_slice_part.argtypes = [sz, sz, sz, sz, sz, ctypes.POINTER(sz)]
    lib.dr_slice_part.restype = None
    lib.dr_fr_wsum.argtypes = [p, sz, sz, p, p, p]
    lib.dr_select.argtypes = [p, v, sz, sz, p, v, v, p]
    lib.dr_lagrange.argtypes = [v, sz, p]
    lib.dr_constant_check.argtypes = [p, sz, ctypes.c_uint64, p]
    return lib


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0x5E5A)


@pytest.fixture(scope="module")
def pool(rnd):
    """13 random points of G1 with their discrete logarithms, made once"""
    logs = [rnd.randrange(1, o.R) for _ in range(13)]
    return logs, [o.E1.mul(o.G1_GEN, a) for a in logs]


def enc(P):
    return IDENT if P is None else o.g1_uncompressed(P)


def fr(v):
    return int(v).to_bytes(32, "little")


def wfold(points, weights):
    acc = None
    for P, w in zip(points, weights):
        acc = o.E1.add(acc, None if P is None else o.E1.mul(P, w % o.R))
    return acc


def off_curve(rnd):
    while True:
        x, y = rnd.randrange(o.Q), rnd.randrange(o.Q)
        if (y * y - x * x * x - 4) % o.Q:
            return x.to_bytes(48, "big") + y.to_bytes(48, "big")


def g1_wsum(L, terms, weights, parts, mask=None, member=None):
    """terms: encodings, weights: integers below 2^256; returns (status, 96 bytes, term_bad)"""
    n = len(terms)
    out, bad = ctypes.create_string_buffer(96), ctypes.create_string_buffer(max(n, 1))
    st = L.dr_g1_wsum(b"".join(terms), 96, n, b"".join(fr(w) for w in weights), None if mask is None else bytes(mask),
                      None if member is None else bytes(member), parts, out, bad)
    return st, out.raw, list(bad.raw[:n])


def same_for_every_parts(L, terms, weights, want, mask=None):
    for parts in PARTS:
        st, got, bad = g1_wsum(L, terms, weights, parts, mask)
        assert (st, got) == (OK, enc(want)), parts
        assert not any(bad)


# ---- 1. the weighted G1 sum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 13])
def test_g1_wsum_of_random_terms_and_weights(L, pool, rnd, n):
    pts = pool[1][:n]
    ws = [rnd.randrange(o.R) for _ in range(n)]
    same_for_every_parts(L, [enc(P) for P in pts], ws, wfold(pts, ws))


@pytest.mark.parametrize("n", [1, 2, 5, 13])
def test_g1_wsum_weights_zero_one_and_r_minus_one(L, pool, n):
    pts = pool[1][:n]
    for ws in ([0] * n, [1] * n, [o.R - 1] * n, [(0, 1, o.R - 1)[k % 3] for k in range(n)]):
        same_for_every_parts(L, [enc(P) for P in pts], ws, wfold(pts, ws))


@pytest.mark.parametrize("n", [1, 2, 5, 13])
def test_g1_wsum_non_canonical_weight_fails_the_output(L, pool, rnd, n):
    pts = pool[1][:n]
    for bad_w in (o.R, 2 ** 256 - 1):
        for at in sorted({0, n - 1, n // 2}):
            ws = [rnd.randrange(o.R) for _ in range(n)]
            ws[at] = bad_w
            for parts in PARTS:
                st, got, bad = g1_wsum(L, [enc(P) for P in pts], ws, parts)
                assert (st, got) == (INVALID, IDENT) and not any(bad), (parts, at)      # the POINT is not at fault
            # ... and the weight of an excluded term is not looked at
            mask = [1] * n
            mask[at] = 0
            keep = [k for k in range(n) if k != at]
            same_for_every_parts(L, [enc(P) for P in pts], ws, wfold([pts[k] for k in keep], [ws[k] for k in keep]), mask)


@pytest.mark.parametrize("n", [1, 2, 5, 13])
def test_g1_wsum_identity_terms(L, pool, rnd, n):
    pts = [None if k % 2 == 0 else pool[1][k] for k in range(n)]
    ws = [rnd.randrange(o.R) for _ in range(n)]
    same_for_every_parts(L, [enc(P) for P in pts], ws, wfold(pts, ws))
    same_for_every_parts(L, [IDENT] * n, ws, None)
    same_for_every_parts(L, [], [], None)                                                 # n = 0


@pytest.mark.parametrize("n", [2, 5, 13])
def test_g1_wsum_equal_and_opposite_products(L, pool, rnd, n):
    """w_a P_a = w_b P_b and w_a P_a = -w_b P_b with P_a != +-P_b, a and b adjacent (one lane at parts = 1, 2 for n >= 4) and at
    the two ends (different lanes for every parts > 1): the public weights let a dealer arrange exactly this"""
    logs, pts = pool
    for a, b in ((0, 1), (0, n - 1)):
        for sign in (1, -1):
            ws = [rnd.randrange(1, o.R) for _ in range(n)]
            # w_b = sign * w_a * log_a / log_b: the two products are the same point, or opposite ones
            ws[b] = sign * ws[a] * logs[a] * pow(logs[b], -1, o.R) % o.R
            assert o.E1.mul(pts[a], ws[a]) == (o.E1.mul(pts[b], ws[b]) if sign == 1 else o.E1.neg(o.E1.mul(pts[b], ws[b])))
            same_for_every_parts(L, [enc(P) for P in pts[:n]], ws, wfold(pts[:n], ws))
    # nothing but such pairs: the sum is the identity (n even) -- every round of the tree meets P + (-P) or 0 + 0
    m = n - n % 2
    ws = []
    for k in range(0, m, 2):
        w = rnd.randrange(1, o.R)
        ws += [w, -w * logs[k] * pow(logs[k + 1], -1, o.R) % o.R]
    same_for_every_parts(L, [enc(P) for P in pts[:m]], ws, None)


@pytest.mark.parametrize("n", [2, 5, 13])
def test_g1_wsum_mask_and_bad_terms(L, pool, rnd, n):
    pts = pool[1][:n]
    ws = [rnd.randrange(o.R) for _ in range(n)]
    at = n // 2
    mask = [1] * n
    mask[at] = 0
    keep = [k for k in range(n) if k != at]
    want = wfold([pts[k] for k in keep], [ws[k] for k in keep])
    for junk in (off_curve(rnd), bytes([0xE0]) + bytes(95), b"\xff" * 96):
        spoiled = [enc(P) for P in pts]
        spoiled[at] = junk
        same_for_every_parts(L, spoiled, ws, want, mask)                                  # masked garbage: ignored
        for parts in PARTS:                                                               # included: the output fails, that term is marked
            assert g1_wsum(L, spoiled, ws, parts) == (INVALID, IDENT, [1 if k == at else 0 for k in range(n)]), parts
    same_for_every_parts(L, [enc(P) for P in pts], ws, None, [0] * n)                     # everything masked out
    # membership verdicts follow the mask
    member = [1] * n
    member[at] = 0
    for parts in PARTS:
        assert g1_wsum(L, [enc(P) for P in pts], ws, parts, None, member) == (INVALID, IDENT, [1 if k == at else 0 for k in range(n)])
        st, got, bad = g1_wsum(L, [enc(P) for P in pts], ws, parts, mask, member)
        assert (st, got) == (OK, enc(want)) and not any(bad)


def test_g1_wsum_over_selected_terms(L, pool, rnd):
    """the resharing sums the t_old + 1 selected parts of P: the lanes split the selection, the terms keep their numbers"""
    pts = pool[1]
    n = len(pts)
    ws = [rnd.randrange(o.R) for _ in range(n)]
    terms = [enc(P) for P in pts]
    terms[6] = off_curve(rnd)                                            # not selected: never decoded
    ws[7] = 2 ** 256 - 1                                                  # not selected: never looked at
    for sel in ([0], [12, 0, 5], [1, 2, 3, 4, 5], [11, 9, 10, 8, 4, 3, 2, 1, 0, 12, 5]):
        for mask in (None, [0 if k == sel[0] else 1 for k in range(n)]):
            keep = [k for k in sel if mask is None or mask[k]]
            want = enc(wfold([pts[k] for k in keep], [ws[k] for k in keep]))
            for parts in PARTS:
                out = ctypes.create_string_buffer(96)
                st = L.dr_g1_wsum_sel(b"".join(terms), 96, n, b"".join(fr(w) for w in ws), None if mask is None else bytes(mask),
                                      (ctypes.c_uint32 * len(sel))(*sel), len(sel), parts, out)
                assert (st, out.raw) == (OK, want), (sel, parts)
    out = ctypes.create_string_buffer(96)
    assert L.dr_g1_wsum_sel(b"".join(terms), 96, n, b"".join(fr(w) for w in ws), None, (ctypes.c_uint32 * 2)(3, 6), 2, 2, out) == INVALID


def test_slices_and_lanes_cover_every_term_exactly_once(L):
    out = (ctypes.c_size_t * 2)()
    for n in list(range(0, 20)) + [63, 64, 65, 67, 68, 129, 200]:
        for slices in (1, 2, 3, 4, 15):
            for parts in (1, 4, 64):
                owned = []
                for s in range(slices):
                    for g in range(parts):
                        L.dr_slice_part(n, s, slices, g, parts, out)
                        assert out[0] <= out[1] <= n
                        owned += list(range(out[0], out[1]))
                assert owned == list(range(n)), (n, slices, parts)
    for n, slices in ((68, 2), (200, 4)):                                # the DKG shapes: one term per lane at most
        for s in range(slices):
            for g in range(64):
                L.dr_slice_part(n, s, slices, g, 64, out)
                assert out[1] - out[0] <= 1


# ---- 2. the weighted Fr sum ------------------------------------------------------------------------------------------------
def fr_wsum(L, vals, ws, mask=None, stride=32):
    out = ctypes.create_string_buffer(32)
    blob = b"".join(fr(v) + bytes(stride - 32) for v in vals)
    st = L.dr_fr_wsum(blob, stride, len(vals), b"".join(fr(w) for w in ws), None if mask is None else bytes(mask), out)
    return st, int.from_bytes(out.raw, "little")


def test_fr_wsum(L, rnd):
    for n in (0, 1, 2, 5, 13):
        vals = [rnd.randrange(o.R) for _ in range(n)]
        ws = [rnd.randrange(o.R) for _ in range(n)]
        want = sum(v * w for v, w in zip(vals, ws)) % o.R
        assert fr_wsum(L, vals, ws) == (OK, want)
        assert fr_wsum(L, vals, ws, stride=96) == (OK, want)
    assert fr_wsum(L, [o.R - 1, o.R - 1], [o.R - 1, 1]) == (OK, 0)
    assert fr_wsum(L, [5, 7], [0, 0]) == (OK, 0)
    vals = [rnd.randrange(o.R) for _ in range(6)]
    ws = [rnd.randrange(o.R) for _ in range(6)]
    mask = [1, 1, 0, 1, 0, 1]
    want = sum(v * w for v, w, m in zip(vals, ws, mask) if m) % o.R
    assert fr_wsum(L, vals, ws, mask) == (OK, want)
    assert fr_wsum(L, vals, ws, [0] * 6) == (OK, 0)
    for bad in (o.R, o.R + 1, 2 ** 256 - 1):
        for spoil_weight in (False, True):
            v2, w2 = list(vals), list(ws)
            (w2 if spoil_weight else v2)[2] = bad
            assert fr_wsum(L, v2, w2, mask) == (OK, want)                                 # masked out: ignored
            assert fr_wsum(L, v2, w2) == (INVALID, 0)                                     # included: rejected


# ---- 3. who deals ----------------------------------------------------------------------------------------------------------
GUARD = 0xA5


def select(L, accept, idx, t_old):
    """the helper with guard bytes behind every output; returns (enough, used, sel_part, sel_idx, dup)"""
    P = len(idx)
    used = ctypes.create_string_buffer(bytes([GUARD]) * (P + 8), P + 8)
    dup = ctypes.create_string_buffer(bytes([GUARD]) * (P + 8), P + 8)
    sp = (ctypes.c_uint32 * (t_old + 3))(*[0xA5A5A5A5] * (t_old + 3))
    si = (ctypes.c_uint64 * (t_old + 3))(*[0xA5A5A5A5A5A5A5A5] * (t_old + 3))
    ia = (ctypes.c_uint64 * max(P, 1))(*idx)
    enough = L.dr_select(None if accept is None else bytes(accept), ia, t_old, P, used, sp, si, dup)
    assert used.raw[P:] == bytes([GUARD]) * 8 and dup.raw[P:] == bytes([GUARD]) * 8
    filled = t_old + 1 if enough else 0
    assert list(sp)[filled:] == [0xA5A5A5A5] * (t_old + 3 - filled) and list(si)[filled:] == [0xA5A5A5A5A5A5A5A5] * (t_old + 3 - filled)
    return bool(enough), list(used.raw[:P]), list(sp)[:filled], list(si)[:filled], list(dup.raw[:P])


def model(accept, idx, t_old):
    P = len(idx)
    acc = [accept is None or accept[p] != 0 for p in range(P)]
    dup = [1 if acc[p] and any(acc[q] and idx[q] == idx[p] for q in range(p)) else 0 for p in range(P)]
    taken = [p for p in range(P) if acc[p]]
    enough = len(taken) > t_old
    S = taken[:t_old + 1] if enough else []
    return enough, [1 if p in S else 0 for p in range(P)], S, [idx[p] for p in S], dup


def test_selection_against_the_model(L):
    for P in range(0, 7):
        idx = [3 * p + 1 for p in range(P)]
        for t_old in range(0, 4):
            for accept in itertools.product((0, 1), repeat=P):
                assert select(L, accept, idx, t_old) == model(accept, idx, t_old), (accept, t_old)
            assert select(L, None, idx, t_old) == model(None, idx, t_old)
    # accept bytes other than 1 count as accepted
    assert select(L, [2, 0, 255], [5, 6, 7], 1) == model([2, 0, 255], [5, 6, 7], 1)


def test_selection_duplicates_and_the_largest_index(L):
    for idx in ([4, 4, 4, 9, 4], [U64, 0, U64, 1, 0, 1], [7, 8, 7, 8, U64, U64 - 1]):
        for t_old in (0, 1, 3):
            for accept in itertools.product((0, 1), repeat=len(idx)):
                assert select(L, accept, idx, t_old) == model(accept, idx, t_old), (idx, accept, t_old)
    # a rejected part's index is nobody's duplicate
    assert select(L, [0, 1, 1], [4, 4, 5], 1)[4] == [0, 0, 0]
    assert select(L, [1, 1, 1], [4, 4, 5], 1)[4] == [0, 1, 0]


def test_lagrange_weights_of_the_selection(L, rnd):
    """the abscissae are idx + 1 in Fr (2^64 for the largest index): sum_i lambda_i f(x_i) = f(0)"""
    for idx in ([0], [2, 0, 1], [U64, 5, 0, 17], [9, 3, U64 - 1, U64, 1]):
        t = len(idx) - 1
        out = ctypes.create_string_buffer(32 * (t + 1))
        assert L.dr_lagrange((ctypes.c_uint64 * (t + 1))(*idx), t, out) == OK
        lam = [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(t + 1)]
        f = [rnd.randrange(o.R) for _ in range(t + 1)]
        assert sum(l * o.poly_evaluate(f, i + 1) for l, i in zip(lam, idx)) % o.R == f[0]


def test_constant_check(L, rnd):
    f = [rnd.randrange(o.R) for _ in range(3)]
    old = b"".join(enc(o.E1.mul(o.G1_GEN, c)) for c in f)
    for idx in (0, 1, 6, U64 - 1, U64):
        share = o.poly_evaluate(f, idx + 1)
        assert L.dr_constant_check(old, 2, idx, enc(o.E1.mul(o.G1_GEN, share))) == OK
        assert L.dr_constant_check(old, 2, idx, enc(o.E1.mul(o.G1_GEN, (share + 1) % o.R))) == MISMATCH
        assert L.dr_constant_check(old, 2, idx, IDENT) == MISMATCH
        assert L.dr_constant_check(old, 2, idx, off_curve(rnd)) == INVALID
    # degree 0: every old node holds the key itself
    assert L.dr_constant_check(old[:96], 0, 5, old[:96]) == OK
