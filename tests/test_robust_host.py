"""The share selection of the robust combiners on the CPU: threshold_crypto_amd/csrc/tc_robust.h compiled by g++
(tests/robust/robust_host.cpp, a test harness -- not a product path).  select_first -- the routine every lane of
k_select_shares runs -- is compared with a three-line model over every row length at which its word loop changes shape (shorter
than a word, exactly one, one more, N = 10 whose rows start at every offset, more than a wave of bytes, N = 200), every offset
of a row from an 8-byte boundary, and the three values of `need` that matter: 1, N and N + 1 (never reached)."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "robust", "robust_host.cpp")
SIZES = [1, 7, 8, 9, 10, 64, 65, 200]
GUARD64, GUARD32 = 2 ** 64 - 1, 2 ** 32 - 1


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, "tc_robust.h")),
                                                                    os.path.getmtime(os.path.join(CSRC, "tc_common.h")), os.path.getmtime(SRC))


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "robust", "librobust_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, p = ctypes.c_size_t, ctypes.c_char_p
    lib.rh_select_first.argtypes = [p, sz, p, sz, sz, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    lib.rh_select_first.restype = sz
    return lib


def model(present, bad, N, need):
    """the first `need` slots that are present and not bad"""
    elig = [i for i in range(N) if (present is None or present[i]) and not (bad is not None and bad[i])]
    return elig[:need]


def select(L, present, p_off, bad, b_off, N, need):
    cap = need + 2
    idx = (ctypes.c_uint64 * cap)(*[GUARD64] * cap)
    slot = (ctypes.c_uint32 * cap)(*[GUARD32] * cap)
    count = L.rh_select_first(None if present is None else bytes(present), p_off, None if bad is None else bytes(bad), b_off, N, need, idx, slot)
    return count, list(idx), list(slot)


def check(L, present, p_off, bad, b_off, N, need):
    want = model(present, bad, N, need)
    count, idx, slot = select(L, present, p_off, bad, b_off, N, need)
    assert count == len(want), (N, need, p_off, b_off)
    assert slot[:count] == want and idx[:count] == want, (N, need, p_off, b_off)     # the index IS the slot: the + 1 is the kernels'
    assert all(v == GUARD64 for v in idx[count:]) and all(v == GUARD32 for v in slot[count:]), (N, need, p_off, b_off)


def masks(rnd, N, need):
    """all-zero, all-one, random (bytes of any non-zero value count as set), only the last `need`"""
    last = [0] * N
    for i in range(max(0, N - need), N):
        last[i] = 1
    return [[0] * N, [1] * N, [rnd.choice((0, 0, 1, 0x80, 0xff)) for _ in range(N)], last]


@pytest.mark.parametrize("N", SIZES)
def test_select_first_without_a_bad_row(L, N):
    rnd = random.Random(0xB0B + N)
    for need in (1, N, N + 1):
        for off in range(8):
            for present in masks(rnd, N, need):
                check(L, present, off, None, 0, N, need)
        check(L, None, 0, None, 0, N, need)                                      # no mask at all: every slot is present


@pytest.mark.parametrize("N", SIZES)
def test_select_first_with_a_bad_row(L, N):
    rnd = random.Random(0xBAD + N)
    for need in (1, N, N + 1):
        for off in range(8):
            for present in masks(rnd, N, need):
                for bad in masks(rnd, N, need):
                    check(L, present, off, bad, off, N, need)                    # rows of one job: the same offset (the word loop)
            present, bad = masks(rnd, N, need)[2], masks(rnd, N, need)[2]
            check(L, present, off, bad, (off + 3) % 8, N, need)                  # different offsets: the bytewise loop
            check(L, None, 0, bad, off, N, need)                                 # everything present, some bad


def test_consecutive_rows_of_a_batch_start_at_every_offset(L):
    """B x N mask bytes with N = 10: job j's row starts j * 10 bytes in, which walks through the offsets 0, 2, 4, 6"""
    rnd = random.Random(10)
    N, need = 10, 4
    for j in range(8):
        present = [rnd.randrange(2) for _ in range(N)]
        bad = [rnd.randrange(4) == 0 for _ in range(N)]
        check(L, present, (j * N) % 8, bad, (j * N) % 8, N, need)


def test_stand_alone_program_agrees():
    """the harness's own main (what a sanitizer build runs): same routine, fixed inputs"""
    exe = os.path.join(ROOT, "tests", "robust", "robust_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DRH_MAIN", "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "robust_host: ok" in out.stdout, out.stdout + out.stderr
