"""The two stages of the G1 comb (threshold_crypto_amd/csrc/tc_comb_g1.h: the decryption shares of one ciphertext by many key
holders) on the CPU: the device headers compiled by g++ (tests/comb/comb_g1_host.cpp, a test harness -- not a product path), once
plainly with the fallback counter and once under the interval analysis of the limb arithmetic (-DTC_BOUND_CHECK aborts on a
violated bound).  Stage T is compared entry by entry, stage S share by share, with Oracle A: E1.mul over Python integers."""
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
SRC = os.path.join(ROOT, "tests", "comb", "comb_g1_host.cpp")
IDENT = bytes([0x40]) + bytes(95)
OK, INVALID = 0, 3
X2 = 0xd201000000010000 ** 2                                    # phi' = [x^2] P on G1
ENTRY = [(1, 0), (1, -1), (1, 2), (1, 1), (3, 0), (3, 1), (3, 2), (3, 3)]   # (A, B) of A P + B phi', the ladder's table order


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)) \
        or os.path.getmtime(path) < os.path.getmtime(SRC)


def _load(name, flags):
    lib = os.path.join(ROOT, "tests", "comb", name)
    if _stale(lib):
        subprocess.run(["g++", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC] + flags + [SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, p, v = ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p
    lib.cg_tables.argtypes = [p, p]
    lib.cg_decrypt.argtypes = [p, sz, v, sz, p, sz, p, p]
    lib.cg_decrypt.restype = ctypes.c_long
    lib.cg_gather.argtypes = [p, sz, v, sz, p, p, p]
    lib.cg_gather.restype = None
    return lib


@pytest.fixture(scope="module", params=["counted", "bounds"])
def L(request):
    if request.param == "counted":
        return _load("libcomb_g1_host.so", ["-O2", "-DTC_COMB_G1_COUNT"])
    return _load("libcomb_g1_host_bounds.so", ["-O1", "-DTC_BOUND_CHECK"])


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0xC0B1)


def enc(P):
    return IDENT if P is None else o.g1_uncompressed(P)


def fr(v):
    return int(v).to_bytes(32, "little")


def off_curve(rnd):
    while True:
        x, y = rnd.randrange(o.Q), rnd.randrange(o.Q)
        if (y * y - x * x * x - 4) % o.Q:
            return x.to_bytes(48, "big") + y.to_bytes(48, "big")


def mul(P, k):
    k %= o.R
    return None if P is None or k == 0 else o.E1.mul(P, k)


def tables(L, u):
    n = L.cg_entries()
    out = ctypes.create_string_buffer(n * 96)
    ok = L.cg_tables(u, out)
    return ok, [out.raw[96 * i:96 * i + 96] for i in range(n)]


def decrypt(L, sks, idx, u, share):
    """sks: integers below 2^256; returns (shares, statuses, fallbacks)"""
    n = len(idx)
    out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    cnt = L.cg_decrypt(b"".join(fr(s) for s in sks), len(sks), (ctypes.c_uint64 * n)(*idx), n, u, share, out, st)
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], list(st.raw), cnt


def want_shares(sks, idx, P):
    shares, st = [], []
    for i in idx:
        good = i < len(sks) and sks[i] < o.R
        shares.append(enc(mul(P, sks[i])) if good else IDENT)
        st.append(OK if good else INVALID)
    return shares, st


# ---- stage T ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random", "generator"])
def test_stage_t_entries_are_the_ladder_table_scaled_by_powers_of_four(L, rnd, which):
    P = o.G1_GEN if which == "generator" else o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R))
    ok, ents = tables(L, enc(P))
    assert ok == 1 and len(ents) == 64 * 8 + 2
    for c in (0, 1, 2, 31, 63):
        for m, (a, b) in enumerate(ENTRY):
            assert ents[c * 8 + m] == enc(mul(P, 4 ** c * (a + b * X2))), (c, m)
    assert ents[512] == enc(mul(P, 4 ** 64))                                   # the start entries of the leading column
    assert ents[513] == enc(mul(P, 4 ** 64 * (1 + X2)))


def test_stage_t_identity_and_undecodable_u(L, rnd):
    ok, ents = tables(L, IDENT)
    assert ok == 1 and all(e == IDENT for e in ents)                           # a valid operand: every entry at infinity
    for junk in (off_curve(rnd), bytes([0xE0]) + bytes(95), b"\xff" * 96):
        ok, ents = tables(L, junk)
        assert ok == 0 and all(e == IDENT for e in ents)


# ---- stage S ---------------------------------------------------------------------------------------------------------------
def test_stage_s_special_and_random_scalars(L, rnd):
    P = o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R))
    sks = [0, 1, 2, 3, 4, 5, X2, X2 - 1, X2 + 1, o.R - 1, o.R, 2 ** 256 - 1] + [rnd.randrange(o.R) for _ in range(20)]
    idx = list(range(len(sks)))
    want = want_shares(sks, idx, P)
    assert want[1][10] == INVALID and want[1][11] == INVALID and want[1].count(INVALID) == 2
    S = L.cg_share()
    for share in (1, 3, S):
        got, st, cnt = decrypt(L, sks, idx, enc(P), share)
        assert (got, st) == want, share                                         # the invalid scalars fail only their own output
        if cnt >= 0:
            assert cnt >= 1                                                     # k = 0: the last addition meets acc = -entry
    # the scalar 0 alone is what takes the guarded fallback; 1, 2, 3, 5 and r - 1 do not need it
    if L.cg_decrypt(fr(0), 1, (ctypes.c_uint64 * 1)(0), 1, enc(P), S, ctypes.create_string_buffer(96), ctypes.create_string_buffer(1)) >= 0:
        assert decrypt(L, [0], [0], enc(P), S)[2] == 1
        assert decrypt(L, [1, 2, 3, 5, o.R - 1], [0, 1, 2, 3, 4], enc(P), S)[2] == 0


def test_stage_s_index_cases_and_holder_counts(L, rnd):
    P = o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R))
    S = L.cg_share()
    sks = [rnd.randrange(o.R) for _ in range(S + 3)]
    N = len(sks)
    for n in (1, S, S + 1):
        for idx in (list(range(n)), list(range(N - 1, N - 1 - n, -1)),           # ascending, descending
                    [2] * n,                                                    # repeated
                    [(N if k == n // 2 else k) for k in range(n)],              # one out of range
                    [2 ** 64 - 1] + list(range(1, n))):
            got, st, _ = decrypt(L, sks, idx, enc(P), S)
            assert (got, st) == want_shares(sks, idx, P), (n, idx)


def test_stage_s_identity_and_undecodable_u(L, rnd):
    S = L.cg_share()
    sks = [rnd.randrange(o.R) for _ in range(4)] + [o.R]
    idx = [0, 1, 4, 9, 2]
    got, st, cnt = decrypt(L, sks, idx, IDENT, S)                                 # identity shares, through the fallback
    assert got == [IDENT] * 5 and st == [OK, OK, INVALID, INVALID, OK]
    got, st, _ = decrypt(L, sks, idx, off_curve(rnd), S)                          # table_ok = false fails all n
    assert got == [IDENT] * 5 and st == [INVALID] * 5


def test_gather_ladders_agree_with_the_comb(L, rnd):
    P = o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R))
    sks = [0, 1, o.R - 1, o.R] + [rnd.randrange(o.R) for _ in range(5)]
    idx = [8, 3, 0, 1, 2, 9, 7, 7]
    n = len(idx)
    out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    L.cg_gather(b"".join(fr(s) for s in sks), len(sks), (ctypes.c_uint64 * n)(*idx), n, enc(P), out, st)
    assert ([out.raw[96 * i:96 * i + 96] for i in range(n)], list(st.raw)) == want_shares(sks, idx, P)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined (host code only)"""
    exe = str(tmp_path / "comb_g1_host_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DCG_MAIN", "-DTC_COMB_G1_COUNT", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "comb_g1_host: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
