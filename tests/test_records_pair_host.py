"""The lane arithmetic of the PAIRED ragged G1 sums on the CPU (tc_verify_decryption_share_records_rlc_batch):
the paired part of threshold_crypto_amd/csrc/tc_records.h compiled by g++ (tests/records/records_pair_host.cpp, a test harness --
not a product path) and compared with a few-line model: which (half, chunk, segment) a stage-T lane works on and where its
tables start -- half 1 behind ALL of half 0, no place owned twice --, which (segment, half, part) a stage-L lane is, for every
split from 1 to 64 lanes per sum, and where the leader of a sum writes in the interleaved operand array of the product check.
Segment lengths 130 / 0 / 1 / 3 / 4 / 5 / 33 and runs of empty segments.  Every output array carries guard values behind its last
entry."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "records", "records_pair_host.cpp")
GUARD = 2 ** 64 - 1
CHUNK = 4
CASES = [[130, 0, 1, 3, 4, 5, 33], [1], [0, 0, 2, 0], [4, 4], [5], [0, 0, 0], []]


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, "tc_records.h")),
                                                                    os.path.getmtime(os.path.join(CSRC, "tc_common.h")), os.path.getmtime(SRC))


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "records", "librecords_pair_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, u64, p64 = ctypes.c_size_t, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    lib.rp_point_bytes.argtypes, lib.rp_point_bytes.restype = [], u64
    lib.rp_tables_lanes.argtypes, lib.rp_tables_lanes.restype = [u64], u64
    lib.rp_ladder_lanes.argtypes, lib.rp_ladder_lanes.restype = [sz, sz], u64
    lib.rp_out.argtypes, lib.rp_out.restype = [sz, sz], u64
    lib.rp_tables_map.argtypes, lib.rp_tables_map.restype = [p64, sz, p64], None
    lib.rp_ladder_map.argtypes, lib.rp_ladder_map.restype = [sz, sz, p64], None
    return lib


def arr(values):
    return (ctypes.c_uint64 * len(values))(*values)


def first_chunks(lens):
    fc = [0]
    for n in lens:
        fc.append(fc[-1] + -(-n // CHUNK))
    return fc


def test_constants(L):
    assert L.rp_point_bytes() == 96
    for chunks in (0, 1, 7, 2 ** 31):
        assert L.rp_tables_lanes(chunks) == 2 * chunks
    for J in (0, 1, 7, 65536):
        for parts in (1, 2, 64):
            assert L.rp_ladder_lanes(J, parts) == 2 * J * parts
    for j in (0, 1, 5, 2 ** 24):
        assert L.rp_out(j, 0) == 2 * j * 96 and L.rp_out(j, 1) == (2 * j + 1) * 96


@pytest.mark.parametrize("lens", CASES)
def test_stage_t_lanes_and_their_table_places(L, lens):
    J, fc = len(lens), first_chunks(lens)
    C = fc[-1]
    out = arr([GUARD] * (4 * 2 * C + 3))
    L.rp_tables_map(arr(fc), J, out)
    got = list(out)
    assert got[8 * C:] == [GUARD] * 3
    owned = {}
    for t in range(2 * C):
        half, c, j, place = got[4 * t:4 * t + 4]
        # model: the first C lanes are half 0 in chunk order, the next C lanes half 1; a chunk belongs to the segment whose range holds it
        want_half, want_c = (0, t) if t < C else (1, t - C)
        want_j = max(s for s in range(J) if fc[s] <= want_c)
        assert (half, c, j) == (want_half, want_c, want_j) and lens[j] > 0 and fc[j] <= c < fc[j + 1]
        assert place == (want_half * C + want_c) * CHUNK
        for k in range(CHUNK):
            assert place + k not in owned, "two lanes write one table place"
            owned[place + k] = t
    assert sorted(owned) == list(range(2 * C * CHUNK))                   # the tables of the launch, exactly
    # a segment's places in half 1 are its places in half 0 moved by the chunks of the launch
    for j, n in enumerate(lens):
        if n:
            assert owned[fc[j] * CHUNK] == fc[j] and owned[(C + fc[j]) * CHUNK] == C + fc[j]


@pytest.mark.parametrize("parts", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("J", [0, 1, 7, 33])
def test_stage_l_lanes(L, J, parts):
    lanes = 2 * J * parts
    out = arr([GUARD] * (4 * lanes + 3))
    L.rp_ladder_map(J, parts, out)
    got = list(out)
    assert got[4 * lanes:] == [GUARD] * 3
    seen = set()
    for l in range(lanes):
        j, half, g, off = got[4 * l:4 * l + 4]
        assert (j, half, g) == (l // (2 * parts), (l // parts) % 2, l % parts)
        assert off == (2 * j + half) * 96
        first = l - g                                                      # the sum's leader lane
        assert first % parts == 0 and first // 64 == (first + parts - 1) // 64   # the exchanges of a sum stay inside one wave
        seen.add((j, half, g))
    assert len(seen) == lanes
    # the twin sums of a segment are neighbours: half 1 starts where half 0 ends; within one wave up to 32 lanes per sum
    for j in range(J):
        a, b = 2 * j * parts, (2 * j + 1) * parts
        assert got[4 * a:4 * a + 3] == [j, 0, 0] and got[4 * b:4 * b + 3] == [j, 1, 0]
        assert (a // 64 == b // 64) == (parts <= 32)
    # the result offsets tile the operand array: 2 J points, A_j then -B_j
    assert sorted({got[4 * l + 3] for l in range(lanes)}) == [96 * i for i in range(2 * J)]


def test_stand_alone_program_agrees():
    """the harness's own main (what a sanitizer build runs): the same arithmetic over exactly-sized heap arrays"""
    exe = os.path.join(ROOT, "tests", "records", "records_pair_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DRECORDS_PAIR_MAIN", "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "records_pair_host: ok" in out.stdout, out.stdout + out.stderr
