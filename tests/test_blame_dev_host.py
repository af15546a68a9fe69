"""The job-level routines of the blame-by-bisection kernels on the CPU (tests/blame/blame_dev_host.cpp: tc_blame_jobs.h under
g++ -DTC_BOUND_CHECK, the interval analysis of the limb arithmetic aborts on a violated bound) against oracle/tc_oracle.py big
integers on a 5-slot job: the pass-2 seed and the digits from the oracle's own ChaCha20, every leaf [r] P in G1 and G2 by the
oracle's textbook double-and-add (r up to 208 bits: nothing of the GLS / GLV ladders enters), and the range sums at every legal
width -- with identity leaves (an identity share, a slot that is not live, a share that does not decode), a range of length 1
and a range that is all identities."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tc_oracle as o  # noqa: E402
from manypoint_conformance import BLAME_KEY as KEY, blame_call_seed as call_seed, blame_scalar as scalar  # noqa: E402  (the suite's helpers)

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "blame", "blame_dev_host.cpp")
N = 5
BAD_POINT = {0: bytes([0x1f]) + b"\xff" * 95, 1: bytes([0x1f]) + b"\xff" * 191}     # x >= p: no decoder takes it


def _stale(path):
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h"))
    return not os.path.exists(path) or os.path.getmtime(path) < max(newest, os.path.getmtime(SRC))


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "blame", "libblame_dev_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-shared", "-fPIC", SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, vp, u64 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint64
    lib.bdh_leaf_bytes.argtypes = [ctypes.c_int]
    lib.bdh_leaf_bytes.restype = sz
    lib.bdh_call_seed.argtypes = [ctypes.c_char_p, u64, ctypes.c_char_p]
    lib.bdh_digits.argtypes = [ctypes.c_char_p, u64, ctypes.POINTER(u64)]
    lib.bdh_leaves.argtypes = [ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_char_p, sz, vp, sz, vp]
    lib.bdh_range_sum.argtypes = [ctypes.c_int, vp, sz, sz, sz, ctypes.c_char_p]
    return lib


def test_seed_and_digits_are_the_oracles_chacha20(L):
    seen = set()
    for call in (0, 1, 7, 2 ** 40 + 3):
        seed = ctypes.create_string_buffer(32)
        L.bdh_call_seed(KEY, call, seed)
        assert seed.raw == call_seed(KEY, call)
        seen.add(seed.raw)
        for leaf in (0, 1, 65535, 2 ** 33):
            d4 = (ctypes.c_uint64 * 4)()
            L.bdh_digits(seed.raw, leaf, d4)
            d, r = scalar(seed.raw, leaf)
            assert list(d4) == d and d[0] & 1 and all(x < 2 ** 16 for x in d) and r < 2 ** 208 < o.R
    assert len(seen) == 4                                        # no two calls share a seed


def job(g2, rnd):
    """5 slots: random multiples of the generator; slot 1 the identity's encoding, slot 3 not live, slot 4 (G2: slot 2)
    undecodable"""
    E, G, enc = (o.E2, o.G2_GEN, o.g2_uncompressed) if g2 else (o.E1, o.G1_GEN, o.g1_uncompressed)
    pts = [E.mul(G, rnd.randrange(1, o.R)) for _ in range(N)]
    pts[1] = None
    raw = [enc(p) for p in pts]
    bad_slot = 2 if g2 else 4
    raw[bad_slot] = BAD_POINT[g2]
    live = [1, 1, 1, 0, 1]
    return E, enc, pts, raw, live, bad_slot


@pytest.mark.parametrize("g2", [0, 1])
def test_leaves_and_range_sums_against_big_integers(L, g2):
    rnd = random.Random(0xB1A3E + g2)
    E, enc, pts, raw, live_in, bad_slot = job(g2, rnd)
    seed, leaf0 = call_seed(KEY, 5), 3 * N                       # the job is the fourth of its chunk: leaf numbers 15 .. 19
    pb = 192 if g2 else 96
    live = ctypes.create_string_buffer(bytes(live_in), N)
    leaves = ctypes.create_string_buffer(N * L.bdh_leaf_bytes(g2))
    L.bdh_leaves(g2, seed, leaf0, b"".join(raw), 0, ctypes.addressof(live), N, ctypes.addressof(leaves))
    want_live = list(live_in)
    want_live[bad_slot] = 0                                      # the share that does not decode is not live any more
    assert list(live.raw) == want_live
    want = [E.mul(pts[i], scalar(seed, leaf0 + i)[1]) if want_live[i] else None for i in range(N)]
    assert want[1] is None and want[0] is not None
    out = ctypes.create_string_buffer(pb)

    def total(lo, hi):
        acc = None
        for i in range(lo, hi):
            acc = E.add(acc, want[i])
        return acc

    for lo in range(N):
        for hi in range(lo + 1, N + 1):
            for parts in (1, 2, 4, 8):                            # (more parts than terms: some lanes own nothing)
                L.bdh_range_sum(g2, ctypes.addressof(leaves), lo, hi, parts, out)
                assert out.raw == enc(total(lo, hi)), (g2, lo, hi, parts)
    # what the ranges above include: every single leaf, the identity leaves alone, and all-identity ranges
    L.bdh_range_sum(g2, ctypes.addressof(leaves), 3, 4, 1, out)
    assert out.raw[0] == 0x40
    if not g2:
        L.bdh_range_sum(g2, ctypes.addressof(leaves), 3, 5, 2, out)      # not live + undecodable: all identities
        assert out.raw[0] == 0x40 and not any(out.raw[1:])


def test_key_share_leaves_use_the_period(L):
    """the key shares are one row of N points for every job: leaf i multiplies point i % N by the scalar of leaf leaf0 + i"""
    rnd = random.Random(77)
    pts = [o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R)) for _ in range(N)]
    seed = call_seed(KEY, 9)
    n = 2 * N
    leaves = ctypes.create_string_buffer(n * L.bdh_leaf_bytes(0))
    L.bdh_leaves(0, seed, 0, b"".join(o.g1_uncompressed(p) for p in pts), N, None, n, ctypes.addressof(leaves))
    out = ctypes.create_string_buffer(96)
    for i in (0, 4, 5, 9):
        L.bdh_range_sum(0, ctypes.addressof(leaves), i, i + 1, 1, out)
        assert out.raw == o.g1_uncompressed(o.E1.mul(pts[i % N], scalar(seed, i)[1])), i


def test_stand_alone_program_agrees():
    """the harness's own main, built with the address and undefined-behaviour sanitizers: the same routines, fixed inputs"""
    exe = os.path.join(ROOT, "tests", "blame", "blame_dev_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-DBD_MAIN", "-fsanitize=address,undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "blame_dev_host: ok" in out.stdout, out.stdout + out.stderr
