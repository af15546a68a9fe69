"""The host arithmetic of the combined entries on the CPU: threshold_crypto_amd/csrc/tc_fallback.h compiled by g++
(tests/fallback/fallback_host.cpp, a test harness -- not a product path) and compared with a few-line model: how B jobs are cut
into groups (group 0 = the default of 64, at most 1024, at most B; B = 1 .. 9 and 1025: a B below, at and above every small
group, and one past the cap), which jobs the bad groups send to the per-job checks (no group, every group, each single group),
and the record / job / slot maps of F failed jobs x N slots over a `failed` list that is neither contiguous nor sorted.  The
bad-group rule (BadGroups: one byte per group, bytes over the jobs / records / pieces of the groups in either polarity, a null
array, spans of length 0, the keys the records name) and the records of the failed jobs of a ragged call, against the same kind
of model.  Every output array carries guard values behind its last entry.  The stand-alone build of the harness runs under
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
    p64 = ctypes.POINTER(ctypes.c_uint64)
    lib.fh_bad_per_group.argtypes, lib.fh_bad_per_group.restype = [sz, sz, p8, p8, ctypes.c_int], None
    lib.fh_bad_all.argtypes, lib.fh_bad_all.restype = [sz, sz, p8], None
    lib.fh_bad_spans.argtypes, lib.fh_bad_spans.restype = [sz, sz, p8, p64, p8, ctypes.c_int], None
    lib.fh_bad_jobs.argtypes, lib.fh_bad_jobs.restype = [sz, sz, p8, p8, p8, ctypes.c_int], None
    lib.fh_bad_named_keys.argtypes, lib.fh_bad_named_keys.restype = [sz, sz, p8, p64, p64, sz, p8], None
    lib.fh_bad_failed_jobs.argtypes, lib.fh_bad_failed_jobs.restype = [sz, sz, p8, p32], sz
    lib.fh_records_of_jobs.argtypes, lib.fh_records_of_jobs.restype = [p64, p32, sz, p32, p32], sz
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


# ---- the bad-group rule -----------------------------------------------------------------------------------------------------------
SMALL_BS, SMALL_GROUPS = [1, 2, 3, 5], [1, 2, 3]                  # B below, at and above the group size
GUARD8 = 0xA5


def a8(v):
    return None if v is None else (ctypes.c_uint8 * len(v))(*v)


def a64(v):
    return None if v is None else (ctypes.c_uint64 * len(v))(*v)


def accumulate(L, B, group, start, fn, *args):
    """one kind of evidence ORed into `start` (NG bytes, guard bytes behind them)"""
    NG = cut_model(B, group)[3]
    assert len(start) == NG
    bad = (ctypes.c_uint8 * (NG + 3))(*(list(start) + [GUARD8] * 3))
    fn(B, group, bad, *args)
    assert list(bad)[NG:] == [GUARD8] * 3
    return list(bad)[:NG]


def is_bad(x, zero_bad):
    return (x == 0) == bool(zero_bad)


def spans_model(first, v, zero_bad):
    """group g is bad if a byte of v[first[g] .. first[g + 1]] is; no array: no evidence"""
    return [int(v is not None and any(is_bad(x, zero_bad) for x in v[first[g]:first[g + 1]])) for g in range(len(first) - 1)]


def named_keys_model(rec_first, key_idx, K, key_ok):
    name = (lambda r: r) if key_idx is None else (lambda r: key_idx[r])
    return [int(key_ok is not None and any(name(r) < K and key_ok[name(r)] == 0 for r in range(rec_first[g], rec_first[g + 1])))
            for g in range(len(rec_first) - 1)]


def job_first(B, group):
    g, _, _, NG = cut_model(B, group)
    return [min(k * g, B) for k in range(NG + 1)]


def one_bad(n, zero_bad):
    """no bad byte, every byte bad, each single bad byte (a status byte is bad at any non-zero value)"""
    good, wrong = (1, 0) if zero_bad else (0, 7)
    yield [good] * n
    yield [wrong] * n
    for at in range(n):
        yield [good] * at + [wrong] + [good] * (n - at - 1)


@pytest.mark.parametrize("zero_bad", [1, 0], ids=["zero_is_bad", "nonzero_is_bad"])
@pytest.mark.parametrize("group", SMALL_GROUPS)
@pytest.mark.parametrize("B", SMALL_BS)
def test_bad_groups_from_bytes_per_group_and_per_job(L, B, group, zero_bad):
    NG = cut_model(B, group)[3]
    first = job_first(B, group)
    clean = [0] * NG
    for v in one_bad(NG, zero_bad):
        assert accumulate(L, B, group, clean, L.fh_bad_per_group, a8(v), zero_bad) == [int(is_bad(x, zero_bad)) for x in v]
    assert accumulate(L, B, group, clean, L.fh_bad_per_group, None, zero_bad) == clean
    for v in one_bad(B, zero_bad):
        want = spans_model(first, v, zero_bad)
        assert accumulate(L, B, group, clean, L.fh_bad_jobs, a8(v), None, zero_bad) == want
        assert accumulate(L, B, group, clean, L.fh_bad_jobs, None, a8(v), zero_bad) == want
        assert accumulate(L, B, group, clean, L.fh_bad_spans, a64(first), a8(v), zero_bad) == want
    assert accumulate(L, B, group, clean, L.fh_bad_jobs, None, None, zero_bad) == clean
    # evidence is ORed in: what was bad stays bad, and two arrays mark the groups of both
    marked = [1] + [0] * (NG - 1)
    good = [1 if zero_bad else 0] * B
    assert accumulate(L, B, group, marked, L.fh_bad_jobs, a8(good), None, zero_bad) == marked
    last = list(good)
    last[B - 1] = 0 if zero_bad else 1
    assert accumulate(L, B, group, marked, L.fh_bad_jobs, a8(good), a8(last), zero_bad) == [1] + [0] * (NG - 2) + [1] if NG > 1 else [1]
    assert accumulate(L, B, group, clean, L.fh_bad_all) == [1] * NG
    # ... and the accumulator ends in the jobs of its bad groups
    out = (ctypes.c_uint32 * (B + 3))(*([GUARD] * (B + 3)))
    n = L.fh_bad_failed_jobs(B, group, a8(marked), out)
    assert list(out)[:n] == failed_jobs(L, marked, B, group) and list(out)[n:] == [GUARD] * (B + 3 - n)


# (rec_off of M jobs, group): a job without records in the middle; a GROUP without records; every job its own group
RAGGED = [([0, 2, 2, 3], 2), ([0, 2, 2, 3], 1), ([0, 0, 0, 1], 2), ([0, 0, 0, 1, 4], 2), ([0, 3], 1)]


def rec_first_model(rec_off, group):
    M = len(rec_off) - 1
    return [rec_off[j] for j in job_first(M, group)]


@pytest.mark.parametrize("zero_bad", [1, 0], ids=["zero_is_bad", "nonzero_is_bad"])
@pytest.mark.parametrize("rec_off,group", RAGGED)
def test_bad_groups_from_bytes_per_record(L, rec_off, group, zero_bad):
    M, R = len(rec_off) - 1, rec_off[-1]
    first = rec_first_model(rec_off, group)
    NG = len(first) - 1
    for v in one_bad(R, zero_bad):
        assert accumulate(L, M, group, [0] * NG, L.fh_bad_spans, a64(first), a8(v), zero_bad) == spans_model(first, v, zero_bad)
    assert accumulate(L, M, group, [0] * NG, L.fh_bad_spans, a64(first), None, zero_bad) == [0] * NG


def test_bad_groups_from_named_keys(L):
    rec_off, group, K = [0, 2, 2, 3, 5], 2, 3                      # groups of records 0 .. 2 and 2 .. 5
    first = rec_first_model(rec_off, group)
    assert first == [0, 2, 5]
    run = lambda key_idx, key_ok, k=K: accumulate(L, 4, group, [0, 0], L.fh_bad_named_keys, a64(first), a64(key_idx), k, a8(key_ok))
    cases = [
        ([0, 1, 0, 1, 0], [1, 1, 1]),                              # no bad key
        ([0, 1, 0, 1, 0], [1, 0, 1]),                              # a bad key named from both groups
        ([0, 1, 0, 2, 0], [1, 0, 1]),                              # ... from the first group only
        ([0, 0, 0, 1, 0], [1, 0, 1]),                              # ... from the second group only
        ([0, 2, 0, 2, 0], [1, 0, 1]),                              # ... from no record: no group
        ([0, K, 0, 2 ** 64 - 1, 2], [1, 0, 1]),                    # an index equal to K and 2^64 - 1 beside a bad key: no group
        ([0, K, 1, 2 ** 64 - 1, 2], [1, 0, 1]),                    # ... and the bad key named next to them
        ([0, 1, 2, 0, 1], [0, 0, 0]),                              # every key bad
    ]
    for key_idx, key_ok in cases:
        want = named_keys_model(first, key_idx, K, key_ok)
        assert run(key_idx, key_ok) == want, (key_idx, key_ok)
        assert run(key_idx, None) == [0, 0]                        # no verdicts: no evidence
    assert run([0, 2, 0, 2, 0], [1, 0, 1]) == [0, 0] and run([0, K, 0, 2 ** 64 - 1, 2], [1, 0, 1]) == [0, 0]
    assert run([0, 1, 0, 2, 0], [1, 0, 1]) == [1, 0] and run([0, 0, 0, 1, 0], [1, 0, 1]) == [0, 1]
    # without key_idx record r names key r: K = R = 5
    for key_ok in ([1] * 5, [1, 0, 1, 1, 1], [1, 1, 1, 1, 0], [1, 1, 0, 1, 1]):
        want = named_keys_model(first, None, 5, key_ok)
        assert run(None, key_ok, 5) == want == [int(0 in key_ok[:2]), int(0 in key_ok[2:])]
    # what was bad stays bad
    assert accumulate(L, 4, group, [1, 0], L.fh_bad_named_keys, a64(first), a64([0, 0, 0, 1, 0]), K, a8([1, 0, 1])) == [1, 1]


@pytest.mark.parametrize("jobs", [[], [1], [0, 2], [2, 0]])
def test_records_of_jobs(L, jobs):
    rec_off = [0, 2, 2, 3]
    want = [(r, j) for j in jobs for r in range(rec_off[j], rec_off[j + 1])]
    record, job = [(ctypes.c_uint32 * (len(want) + 3))(*([GUARD] * (len(want) + 3))) for _ in range(2)]
    n = L.fh_records_of_jobs(a64(rec_off), (ctypes.c_uint32 * max(len(jobs), 1))(*jobs), len(jobs), record, job)
    assert n == len(want) == {(): 0, (1,): 0, (0, 2): 3, (2, 0): 3}[tuple(jobs)]
    assert list(zip(list(record)[:n], list(job)[:n])) == want
    assert list(record)[n:] == [GUARD] * 3 and list(job)[n:] == [GUARD] * 3


def test_stand_alone_program_under_sanitizers():
    """the harness's own main under AddressSanitizer and UBSan: the same arithmetic over exactly-sized heap arrays (a program of
    its own on the CPU; nothing sanitised is loaded into this process)"""
    exe = os.path.join(ROOT, "tests", "fallback", "fallback_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFALLBACK_MAIN",
                        "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "fallback_host: ok" in out.stdout, out.stdout + out.stderr
