"""Blame by bisection on the CPU: threshold_crypto_amd/csrc/tc_blame.h compiled by g++ (tests/blame/blame_host.cpp, a test
harness -- not a product path) and driven with a truthful range oracle: a range passes iff it holds no slot that is live and
bad.  For every N in 1 .. 9, every present mask and every bad mask: the bad bits are exactly present AND bad, the number of
checks and rounds equals `model` below -- written from the rule in the header comment, recursively, not from the C++ work
lists --, checks <= min(1 + 2 k d, 2 N - 1) and rounds <= 2 d + 1.  Spot cases at N = 200 and N = 1000."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "blame", "blame_host.cpp")


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, "tc_blame.h")), os.path.getmtime(SRC))


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "blame", "libblame_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    lib.bh_search.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    lib.bh_search.restype = ctypes.c_int
    return lib


def model(N, live, bad):
    """The rule of tc_blame.h, by recursion over ranges with the round each step happens in.  live / bad: lists of bools
    (bad only counts where live).  Returns (set of slots found bad, checks, rounds)."""
    found, state = set(), {"checks": 0, "last": 0}

    def has_live(lo, hi):
        return any(live[lo:hi])

    def fails(lo, hi):
        return any(live[i] and bad[i] for i in range(lo, hi))

    def check(lo, hi, rnd):
        state["checks"] += 1
        state["last"] = max(state["last"], rnd)
        return not fails(lo, hi)

    def unknown(lo, hi, rnd):
        """an unknown range that is pending in round rnd"""
        if not has_live(lo, hi):
            return                                   # passes without a check
        if not check(lo, hi, rnd):
            failing(lo, hi, rnd + 1)

    def failing(lo, hi, rnd):
        """a failing range that is pending in round rnd"""
        if hi - lo == 1:
            found.add(lo)
            return
        mid = lo + ((hi - lo + 1) >> 1)
        if not has_live(lo, mid):
            failing(mid, hi, rnd)                    # by inference, no check, the same round
        elif check(lo, mid, rnd):
            failing(mid, hi, rnd + 1)                # by inference, no check
        else:
            failing(lo, mid, rnd + 1)
            unknown(mid, hi, rnd + 1)

    if N:
        unknown(0, N, 1)
    return found, state["checks"], state["last"]


def ceil_log2(n):
    return (n - 1).bit_length()


def run(L, N, present, live, bad):
    out = ctypes.create_string_buffer(bytes([9] * N), N)
    st = (ctypes.c_uint64 * 2)()
    rc = L.bh_search(N, bytes(present), bytes(live), bytes(bad), out, st)
    assert rc == 0, (N, present, live, bad)
    return list(out.raw), st[0], st[1]


def check_case(L, N, present, live, bad):
    """live[i] only matters where present[i]; bad[i] is the truth about share i"""
    eff_live = [bool(present[i] and live[i]) for i in range(N)]
    got, checks, rounds = run(L, N, present, live, bad)
    want_bits = [1 if present[i] and (not live[i] or bad[i]) else 0 for i in range(N)]
    assert got == want_bits, (N, present, live, bad, got)
    found, m_checks, m_rounds = model(N, eff_live, [bool(b) for b in bad])
    assert found == {i for i in range(N) if eff_live[i] and bad[i]}
    assert (checks, rounds) == (m_checks, m_rounds), (N, present, live, bad)
    k, d = sum(1 for i in range(N) if eff_live[i] and bad[i]), ceil_log2(N)
    assert checks <= min(1 + 2 * k * d, 2 * N - 1), (N, present, bad, checks)
    assert rounds <= 2 * d + 1, (N, present, bad, rounds)
    return checks, rounds


@pytest.mark.parametrize("N", range(1, 10))
def test_every_present_and_bad_mask(L, N):
    for present in itertools.product((0, 1), repeat=N):
        for bad in itertools.product((0, 1), repeat=N):
            check_case(L, N, present, [1] * N, bad)


@pytest.mark.parametrize("N", [1, 2, 5, 8, 9])
def test_a_present_slot_that_is_not_live_is_bad_without_a_check(L, N):
    for live in itertools.product((0, 1), repeat=N):
        # nothing bad among the live ones: one check when a live slot exists, none otherwise
        checks, rounds = check_case(L, N, [1] * N, live, [0] * N)
        assert (checks, rounds) == ((1, 1) if any(live) else (0, 0))
        # the absent slots hold junk that "is bad": ignored
        present = [1 - (i % 2) for i in range(N)]
        check_case(L, N, present, live, [1 - p for p in present])
    # a job whose own operands are invalid: no slot is live, every present share bad, zero checks
    got, checks, rounds = run(L, N, [1] * N, [0] * N, [0] * N)
    assert got == [1] * N and (checks, rounds) == (0, 0)


@pytest.mark.parametrize("N", [200, 1000])
def test_spot_cases_at_large_n(L, N):
    d = ceil_log2(N)
    for bad_slots in ([0], [N - 1], [N // 2], [3, N // 2, N // 2 + 1], [0, N // 3, N - 1]):
        bad = [0] * N
        for b in bad_slots:
            bad[b] = 1
        checks, rounds = check_case(L, N, [1] * N, [1] * N, bad)
        assert checks <= 1 + 2 * len(bad_slots) * d
        if len(bad_slots) == 1:
            assert checks <= 1 + 2 * d                 # 17 instead of 200 at N = 200
    checks, _ = check_case(L, N, [1] * N, [1] * N, [1] * N)     # every share bad: the worst case
    assert checks == 2 * N - 1


def test_stand_alone_program_agrees():
    """the harness's own main, built with the address and undefined-behaviour sanitizers: same engine, fixed inputs"""
    exe = os.path.join(ROOT, "tests", "blame", "blame_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBH_MAIN", "-I" + CSRC,
                        SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "blame_host: ok" in out.stdout, out.stdout + out.stderr
