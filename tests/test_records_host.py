"""The segment arithmetic of the ragged sums on the CPU: threshold_crypto_amd/csrc/tc_records.h compiled by g++
(tests/records/records_host.cpp, a test harness -- not a product path) and compared with a few-line model: the padded chunk
range of a segment (lengths 0, 1, 3, 4, 5, 8, 33, 130: empty, shorter than a chunk, exactly one / two chunks, one more than
a chunk, longer than a wave of lane pairs), the record range of a group of messages (group 1, 2, 3, 64 over M = 1, 2, 7, 65:
an M that is no multiple of the group, groups made of empty messages only), the owner of a chunk, the split rule at the edges
of its powers of two, and the parts of a segment.  Every output array carries guard values behind its last entry."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "records", "records_host.cpp")
GUARD = 2 ** 64 - 1
LENGTHS = [0, 1, 3, 4, 5, 8, 33, 130]
CHUNK = 4


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(CSRC, "tc_records.h")),
                                                                    os.path.getmtime(os.path.join(CSRC, "tc_common.h")), os.path.getmtime(SRC))


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "records", "librecords_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, u64, p64 = ctypes.c_size_t, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    lib.rh_chunk.restype = ctypes.c_int
    lib.rh_chunks.argtypes, lib.rh_chunks.restype = [u64], u64
    lib.rh_chunk_ranges.argtypes, lib.rh_chunk_ranges.restype = [p64, sz, p64], u64
    lib.rh_group_ranges.argtypes, lib.rh_group_ranges.restype = [p64, sz, sz, p64], sz
    lib.rh_segment_of_chunk.argtypes, lib.rh_segment_of_chunk.restype = [p64, sz, u64], sz
    lib.rh_parts.argtypes, lib.rh_parts.restype = [sz, u64, sz, sz, sz], sz
    lib.rh_part.argtypes, lib.rh_part.restype = [u64, sz, sz, p64], None
    lib.rh_part_trips.argtypes, lib.rh_part_trips.restype = [u64, sz], u64
    lib.rh_piece_size.argtypes, lib.rh_piece_size.restype = [u64, sz, sz], u64
    lib.rh_piece_total.argtypes, lib.rh_piece_total.restype = [p64, sz, u64], u64
    lib.rh_piece_ranges.argtypes, lib.rh_piece_ranges.restype = [p64, sz, u64, p64, p64], None
    return lib


def offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def arr(values):
    return (ctypes.c_uint64 * len(values))(*values)


def chunk_ranges(L, seg_first):
    """(total, first_chunk[J + 1]) with the guards behind the array checked"""
    J = len(seg_first) - 1
    out = arr([GUARD] * (J + 1 + 3))
    total = L.rh_chunk_ranges(arr(seg_first), J, out)
    assert list(out)[J + 1:] == [GUARD] * 3, seg_first
    return total, list(out)[:J + 1]


def test_the_chunk_is_the_two_stage_kernels(L):
    assert L.rh_chunk() == CHUNK
    text = open(os.path.join(CSRC, "tc_msm.h")).read()
    assert "constexpr int kMsmChunk = %d;" % CHUNK in text


@pytest.mark.parametrize("n", LENGTHS)
def test_padded_chunks_of_one_segment(L, n):
    want = -(-n // CHUNK)
    assert L.rh_chunks(n) == want
    # the segment alone, and between two neighbours of every other length: its range starts where the one before ends
    assert chunk_ranges(L, [0, n]) == (want, [0, want])
    for before in LENGTHS:
        for after in LENGTHS:
            total, fc = chunk_ranges(L, offsets([before, n, after]))
            b, a = -(-before // CHUNK), -(-after // CHUNK)
            assert fc == [0, b, b + want, b + want + a] and total == fc[-1]


def test_chunk_ranges_of_all_lengths_in_one_launch_and_the_owner_of_every_chunk(L):
    lens = LENGTHS + [0, 0, 2]
    total, fc = chunk_ranges(L, offsets(lens))
    model = offsets([-(-n // CHUNK) for n in lens])
    assert fc == model and total == model[-1]
    cfc = arr(fc)
    for c in range(total):
        j = L.rh_segment_of_chunk(cfc, len(lens), c)
        assert fc[j] <= c < fc[j + 1] and lens[j] > 0, c
    # places: the chunks of a segment hold all its records and fewer than one chunk of padding
    for j, n in enumerate(lens):
        places = (fc[j + 1] - fc[j]) * CHUNK
        assert n <= places < n + CHUNK


def message_lengths(M):
    """ragged, with runs of empty messages long enough to make whole groups of them at group 2 and 3"""
    pattern = [0, 1, 3, 0, 0, 0, 7, 0, 2, 5, 0, 0, 0, 0, 0, 0, 4]
    return [pattern[m % len(pattern)] for m in range(M)]


@pytest.mark.parametrize("group", [1, 2, 3, 64])
@pytest.mark.parametrize("M", [1, 2, 7, 65])
def test_record_ranges_of_the_groups(L, M, group):
    lens = message_lengths(M)
    off = offsets(lens)
    NG = -(-M // group)
    out = arr([GUARD] * (NG + 1 + 3))
    assert L.rh_group_ranges(arr(off), M, group, out) == NG
    got = list(out)
    assert got[NG + 1:] == [GUARD] * 3
    want = [off[min(g * group, M)] for g in range(NG + 1)]
    assert got[:NG + 1] == want
    assert got[0] == 0 and got[NG] == off[M]
    for g in range(NG):
        msgs = range(g * group, min((g + 1) * group, M))
        assert got[g + 1] - got[g] == sum(lens[m] for m in msgs)               # the group's records, contiguous
    if group in (2, 3) and M >= 7:
        assert any(got[g + 1] == got[g] for g in range(NG)), "no group of empty messages in this case"
    # ... and the chunks of the groups as segments
    total, fc = chunk_ranges(L, got[:NG + 1])
    assert fc == offsets([-(-(got[g + 1] - got[g]) // CHUNK) for g in range(NG)])


@pytest.mark.parametrize("piece", [1, 4, 64, 1000])
@pytest.mark.parametrize("group", [1, 2, 3, 64])
def test_pieces_of_the_groups(L, group, piece):
    """a group's records cut into pieces of at most `piece`: every record in one piece, no piece across two groups, a group of
    empty messages without any; M = 65 with the 130-record segment among the messages"""
    lens = message_lengths(65)
    lens[9] = 130
    M, off = len(lens), offsets(lens)
    NG = -(-M // group)
    grp = [off[min(g * group, M)] for g in range(NG + 1)]
    want_first, want_grp = [], [0]
    for g in range(NG):
        want_first += list(range(grp[g], grp[g + 1], piece))
        want_grp.append(len(want_first))
    NP = L.rh_piece_total(arr(grp), NG, piece)
    assert NP == len(want_first)
    pf, gp = arr([GUARD] * (NP + 1 + 3)), arr([GUARD] * (NG + 1 + 3))
    L.rh_piece_ranges(arr(grp), NG, piece, pf, gp)
    assert list(pf)[NP + 1:] == [GUARD] * 3 and list(gp)[NG + 1:] == [GUARD] * 3
    assert list(pf)[:NP + 1] == want_first + [off[M]] and list(gp)[:NG + 1] == want_grp
    pf = list(pf)
    assert all(0 < pf[q + 1] - pf[q] <= piece for q in range(NP))
    # the chunks of the pieces as segments
    total, fc = chunk_ranges(L, pf[:NP + 1])
    assert fc == offsets([-(-(pf[q + 1] - pf[q]) // CHUNK) for q in range(NP)])


def test_piece_size_gives_the_launch_one_wave_per_simd(L):
    """pieces of one wave (`most` lane pairs) each: ceil(R / (want / most)) records, never fewer than two per lane pair"""
    want, most = 32768, 32
    for R in (1, 63, 64, 65, 65530, 65536, 65537, 10 ** 6, 2 ** 32 - 1):
        got = L.rh_piece_size(R, want, most)
        assert got == max(2 * most, -(-R // (want // most))), R
        assert -(-R // got) * most <= max(want, most)                     # the lane pairs of the launch (dense records)
    assert L.rh_piece_size(65536, want, most) == 64 and L.rh_piece_size(65537, want, most) == 65
    assert L.rh_piece_size(1000, 16, 32) == 1000                          # fewer lane pairs wanted than a wave has: one piece


def parts_model(segments, longest, want, most, forced=0):
    if 1 <= forced <= most and forced & (forced - 1) == 0:
        return forced
    parts = 1
    while parts < most and segments * parts < want and parts * 4 <= longest:
        parts *= 2
    return parts


def test_split_rule_at_the_edges_of_its_powers_of_two(L):
    want = 65536
    for most in (32, 64):
        for p in (1, 2, 4, 8, 16, 32, 64):
            # the longest segment allows p parts at 2 p records and not one record earlier
            for longest in (2 * p - 1, 2 * p, 2 * p + 1, 4 * p - 1, 4 * p):
                for segments in (1, 7, want // p - 1, want // p, want // p + 1, want, want + 1):
                    if segments < 1:
                        continue
                    got = L.rh_parts(segments, longest, want, most, 0)
                    assert got == parts_model(segments, longest, want, most), (segments, longest, most)
                    assert got <= most and got & (got - 1) == 0
                    assert got == 1 or (got * 2 <= longest and segments * got // 2 < want)
    assert L.rh_parts(1, 0, want, 64, 0) == 1 and L.rh_parts(1, 1, want, 64, 0) == 1 and L.rh_parts(1, 3, want, 64, 0) == 1
    assert L.rh_parts(1, 4, want, 64, 0) == 2
    assert L.rh_parts(1, 10 ** 6, want, 32, 0) == 32 and L.rh_parts(1, 10 ** 6, want, 64, 0) == 64
    # forced: a power of two within a wave is taken as it is, anything else is the rule's
    for forced in (1, 2, 32, 64):
        assert L.rh_parts(7, 3, want, 64, forced) == forced
    assert L.rh_parts(7, 3, want, 32, 64) == 1 and L.rh_parts(7, 100, want, 64, 3) == parts_model(7, 100, want, 64)


@pytest.mark.parametrize("n", LENGTHS)
def test_parts_tile_the_segment(L, n):
    for parts in (1, 2, 4, 8, 16, 32, 64):
        trips = L.rh_part_trips(n, parts)
        assert trips == -(-n // parts)
        at = 0
        for g in range(parts):
            out = arr([GUARD] * 4)
            L.rh_part(n, g, parts, out)
            s0, s1 = out[0], out[1]
            assert list(out)[2:] == [GUARD] * 2
            assert (s0, s1) == (g * n // parts, (g + 1) * n // parts)
            assert s0 == at and 0 <= s1 - s0 <= trips
            at = s1
        assert at == n


def test_stand_alone_program_agrees():
    """the harness's own main (what a sanitizer build runs): the same arithmetic over exactly-sized heap arrays"""
    exe = os.path.join(ROOT, "tests", "records", "records_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DRECORDS_MAIN", "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "records_host: ok" in out.stdout, out.stdout + out.stderr
