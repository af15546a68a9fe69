"""The host arithmetic of the combined entries on the CPU: threshold_crypto_amd/csrc/tc_fallback.h compiled by g++
(tests/fallback/fallback_host.cpp, a test harness -- not a product path) and compared with a few-line model: how B jobs are cut
into groups (group 0 = the default of 64, at most 1024, at most B; B = 1 .. 9 and 1025: a B below, at and above every small
group, and one past the cap), which jobs the bad groups send to the per-job checks (no group, every group, each single group),
and the record / job / slot maps of F failed jobs x N slots over a `failed` list that is neither contiguous nor sorted.  Every
output array carries guard values behind its last entry.  The stand-alone build of the harness runs under
-fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "fallback", "fallback_host.cpp")
GUARD = 2 ** 32 - 1
BS = list(range(1, 10)) + [1025]
GROUPS = [0, 1, 2, 3, 64, 1024, 2000]


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, "tc_fallback.h")), os.path.getmtime(SRC))


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "fallback", "libfallback_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, p8, p32, psz = ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t)
    lib.fh_group_cut.argtypes, lib.fh_group_cut.restype = [sz, sz, psz], None
    lib.fh_failed_jobs.argtypes, lib.fh_failed_jobs.restype = [p8, sz, sz, p32], sz
    lib.fh_slot_maps.argtypes, lib.fh_slot_maps.restype = [p32, sz, sz, p32, p32, p32], None
    return lib


def cut_model(B, group):
    group = min(group or 64, 1024, B)
    G, tail = divmod(B, group)
    return [group, G, tail, G + (1 if tail else 0)]


def group_cut(L, B, group):
    out = (ctypes.c_size_t * 6)(*([GUARD] * 6))
    L.fh_group_cut(B, group, out)
    assert list(out)[4:] == [GUARD] * 2
    return list(out)[:4]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("B", BS)
def test_group_cut(L, B, group):
    got = group_cut(L, B, group)
    assert got == cut_model(B, group)
    g, G, tail, NG = got
    assert 1 <= g <= min(1024, B) and G * g + tail == B and tail < g and NG == -(-B // g)


def failed_jobs(L, bad, B, group):
    out = (ctypes.c_uint32 * (B + 3))(*([GUARD] * (B + 3)))
    n = L.fh_failed_jobs((ctypes.c_uint8 * len(bad))(*bad), B, group, out)
    assert list(out)[n:] == [GUARD] * (B + 3 - n)
    return list(out)[:n]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("B", BS)
def test_jobs_of_the_bad_groups(L, B, group):
    g, G, tail, NG = cut_model(B, group)
    jobs_of = lambda k: list(range(k * g, min((k + 1) * g, B)))
    assert failed_jobs(L, [0] * NG, B, group) == []
    assert failed_jobs(L, [1] * NG, B, group) == list(range(B))
    for k in range(NG):
        bad = [0] * NG
        bad[k] = 1
        got = failed_jobs(L, bad, B, group)
        assert got == jobs_of(k) and len(got) == (tail if tail and k == NG - 1 else g)
    if NG >= 3:                                                    # any non-zero byte marks a group; first and last together
        bad = [0] * NG
        bad[0], bad[NG - 1] = 255, 2
        assert failed_jobs(L, bad, B, group) == jobs_of(0) + jobs_of(NG - 1)


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("F", [1, 3])
def test_record_job_slot_maps(L, F, N):
    failed = [7, 2, 40][:F]                                        # not contiguous, not sorted
    R = F * N
    bufs = [(ctypes.c_uint32 * (R + 3))(*([GUARD] * (R + 3))) for _ in range(3)]
    L.fh_slot_maps((ctypes.c_uint32 * F)(*failed), F, N, *bufs)
    record, job, slot = [list(b) for b in bufs]
    for b in (record, job, slot):
        assert b[R:] == [GUARD] * 3
    assert record[:R] == [j * N + i for j in failed for i in range(N)]
    assert job[:R] == [j for j in failed for _ in range(N)]
    assert slot[:R] == [i for _ in failed for i in range(N)]


def test_stand_alone_program_under_sanitizers():
    """the harness's own main under AddressSanitizer and UBSan: the same arithmetic over exactly-sized heap arrays (a program of
    its own on the CPU; nothing sanitised is loaded into this process)"""
    exe = os.path.join(ROOT, "tests", "fallback", "fallback_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFALLBACK_MAIN",
                        "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "fallback_host: ok" in out.stdout, out.stdout + out.stderr
