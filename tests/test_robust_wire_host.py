"""What the wire forms of the robust combiners (tc_combine_signatures_robust_wire_batch / tc_decrypt_robust_wire_batch) add to
the device headers, on the CPU: threshold_crypto_amd/csrc compiled by g++ (tests/robust/robust_wire_host.cpp, a test harness --
not a product path).

(a) The curve-level forms of the three compressed decodes (G1, G2, G2 two points per call) against Oracle A's
    g1_from_compressed / g2_from_compressed with check=False, and the checked forms -- which must be what they were -- against
    check=True, byte for byte over ONE table of encodings: members, on-curve non-members (curve-level ok, checked not), an x
    whose cubic is a non-square, x >= q, the compression flag clear, the identity well-formed and with stray bits, both sign
    flags; for the two-point form every ordered pair of table rows and the odd tail.
(b) The record-to-source mapping of the selected decode, run as the kernels walk it, in all three forms: need in {1, 3, 4},
    N in {need, 10}, B in {1, 3}, with a job that lacks enough shares (enough = 0, slots 0xffffffff) first, in the middle and
    last.  Such a job has no source: no offset is formed from its slots (a guard value comes back instead) and nothing is read
    for it."""
import ctypes
import os
import random
import subprocess

import pytest

import tc_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "robust", "robust_wire_host.cpp")
NO_SOURCE = 2 ** 64 - 1
NO_SLOT = 0xFFFFFFFF
IDENT = {48: o.g1_uncompressed(None), 96: o.g2_uncompressed(None)}


def _stale(path):
    newest = max([os.path.getmtime(SRC)] + [os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h")])
    return not os.path.exists(path) or os.path.getmtime(path) < newest


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "robust", "librobust_wire_host.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    sz, p, u32p = ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)
    lib.rw_decode_g1.argtypes = lib.rw_decode_g2.argtypes = [p, ctypes.c_int, p]
    lib.rw_decode_g2_x2.argtypes = [p, p, ctypes.c_int, p, p, p]
    lib.rw_decode_g2_x2.restype = None
    lib.rw_selected_source.argtypes = [sz, sz, sz, u32p, p, sz]
    lib.rw_selected_source.restype = ctypes.c_uint64
    lib.rw_decompress_selected.argtypes = [ctypes.c_int, p, sz, sz, u32p, p, sz, p, p]
    lib.rw_decompress_selected.restype = None
    return lib


# ---- the table of encodings ------------------------------------------------------------------------------------------------
def _flagged(raw, set_bits=0, clear_bits=0):
    b = bytearray(raw)
    b[0] = (b[0] | set_bits) & ~clear_bits & 0xFF
    return bytes(b)


def _non_member_g1(rnd):
    while True:
        x = rnd.randrange(o.Q)
        y2 = (x * x * x + 4) % o.Q
        y = pow(y2, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == y2 and o.E1.mul((x, y), o.R) is not None:
            return (x, y)


def _non_member_g2(rnd):
    while True:
        P = o.g2_get_point_from_x((rnd.randrange(o.Q), rnd.randrange(o.Q)), bool(rnd.randrange(2)))
        if P is not None and o.E2.mul(P, o.R) is not None:
            return P


def _table(g2):
    """(name, encoding) rows; both curves get the same kinds"""
    rnd = random.Random(0xC0DE + g2)
    E, gen, comp, size = (o.E2, o.G2_GEN, o.g2_compressed, 96) if g2 else (o.E1, o.G1_GEN, o.g1_compressed, 48)
    rows = []
    for k in range(2):
        P = E.mul(gen, rnd.randrange(1, o.R))
        rows.append(("member %d" % k, comp(P)))
        rows.append(("member %d negated: the other sign flag" % k, comp(E.neg(P))))
    for k in range(2):
        rows.append(("on the curve, outside the subgroup %d" % k, comp((_non_member_g2 if g2 else _non_member_g1)(rnd))))
    # an x whose cubic x^3 + b is a non-square, with either sign flag
    while True:
        if g2:
            x = (rnd.randrange(o.Q), rnd.randrange(o.Q))
            if o.f2_sqrt(o.f2_add(o.f2_mul(o.f2_sqr(x), x), o._Fq2.b)) is None:
                raw = x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big")
                break
        else:
            x = rnd.randrange(o.Q)
            if pow((x * x * x + 4) % o.Q, (o.Q - 1) // 2, o.Q) != 1:
                raw = x.to_bytes(48, "big")
                break
    rows.append(("no square root", _flagged(raw, 0x80)))
    rows.append(("no square root, sign flag set", _flagged(raw, 0xA0)))
    # x >= q: the first coordinate word equal to q, and (G2) the second
    member = rows[0][1]
    rows.append(("x = q", _flagged(o.Q.to_bytes(48, "big") + bytes(size - 48), 0x80)))
    if g2:
        rows.append(("x0 = q", member[:48] + o.Q.to_bytes(48, "big")))
    rows.append(("the compression flag clear", _flagged(member, 0, 0x80)))
    rows.append(("the identity", comp(None)))
    rows.append(("the identity with the sign flag", _flagged(comp(None), 0x20)))
    rows.append(("the identity with a stray low bit", comp(None)[:-1] + b"\x01"))
    rows.append(("the infinity flag on a finite x", _flagged(member, 0x40)))
    return rows


@pytest.fixture(scope="module")
def tables():
    return {False: _table(False), True: _table(True)}


def oracle_decode(g2, enc, check):
    """(ok, uncompressed bytes): what from_bytes gives, or the identity after a failure"""
    try:
        P = (o.g2_from_compressed if g2 else o.g1_from_compressed)(enc, check=check)
    except o.DecodeError:
        return 0, IDENT[len(enc)]
    return 1, (o.g2_uncompressed if g2 else o.g1_uncompressed)(P)


@pytest.fixture(scope="module")
def expected(tables):
    """(g2, check) -> [(ok, bytes)] per table row: computed once, shared by every test"""
    return {(g2, check): [oracle_decode(g2, enc, check) for _, enc in tables[g2]] for g2 in (False, True) for check in (False, True)}


def test_the_table_holds_what_it_claims(tables, expected):
    for g2 in (False, True):
        names = [n for n, _ in tables[g2]]
        curve, checked = expected[(g2, False)], expected[(g2, True)]
        for i, name in enumerate(names):
            if name.startswith("member") or name == "the identity":
                assert curve[i][0] == 1 and checked[i] == curve[i], name
            elif name.startswith("on the curve, outside"):
                assert curve[i][0] == 1 and checked[i][0] == 0, name         # curve-level ok, checked not
            else:
                assert curve[i][0] == 0 and checked[i][0] == 0, name
        assert (tables[g2][0][1][0] ^ tables[g2][1][1][0]) & 0x20                # both sign flags occur


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("check", [False, True])
def test_single_decodes_against_oracle_a(L, tables, expected, g2, check):
    fn, size = (L.rw_decode_g2, 192) if g2 else (L.rw_decode_g1, 96)
    for (name, enc), (ok, want) in zip(tables[g2], expected[(g2, check)]):
        out = ctypes.create_string_buffer(size)
        assert fn(enc, int(check), out) == ok, name
        assert out.raw == want, name


@pytest.mark.parametrize("check", [False, True])
def test_two_point_decode_every_ordered_pair_and_the_odd_tail(L, tables, expected, check):
    rows, want = tables[True], expected[(True, check)]
    for a, (na, ea) in enumerate(rows):
        for b, (nb, eb) in enumerate(rows):
            oa, ob, ok = ctypes.create_string_buffer(192), ctypes.create_string_buffer(192), ctypes.create_string_buffer(2)
            L.rw_decode_g2_x2(ea, eb, int(check), oa, ob, ok)
            assert (ok.raw[0], oa.raw) == want[a] and (ok.raw[1], ob.raw) == want[b], (na, nb)
        # the odd tail: the second slot repeats the first and has no output
        oa, ok = ctypes.create_string_buffer(192), ctypes.create_string_buffer(2)
        L.rw_decode_g2_x2(ea, ea, int(check), oa, None, ok)
        assert (ok.raw[0], oa.raw) == want[a], na


# ---- the record-to-source mapping ------------------------------------------------------------------------------------------
def _mapping_cases():
    for need in (1, 3, 4):
        for N in sorted({need, 10}):
            for B in (1, 3):
                for lacking in [None] + list(range(B)):                     # nobody, then the first / middle / last job
                    yield need, N, B, lacking


@pytest.mark.parametrize("form", [0, 1, 2])
def test_selected_decode_maps_records_to_sources(L, tables, expected, form):
    """form 0: G1, 1: G2 one record per lane pair, 2: G2 two records per lane pair (odd record counts: the tail; pairs that
    straddle two jobs, one of which may lack enough shares)"""
    g2 = form != 0
    CB, PB = (96, 192) if g2 else (48, 96)
    rows, want = tables[g2], expected[(g2, False)]
    rnd = random.Random(0x5E1 + form)
    for need, N, B, lacking in _mapping_cases():
        pick = [[rnd.randrange(len(rows)) for _ in range(N)] for _ in range(B)]   # which table row sits in slot i of job j
        src = b"".join(rows[pick[j][i]][1] for j in range(B) for i in range(N))
        slot, enough = [], []
        for j in range(B):
            if j == lacking:
                slot += [NO_SLOT] * need
                enough.append(0)
            else:
                slot += sorted(rnd.sample(range(N), need))
                enough.append(1)
        slots = (ctypes.c_uint32 * len(slot))(*slot)
        out = ctypes.create_string_buffer(bytes([0xAA]) * (B * need * PB), B * need * PB)
        ok = ctypes.create_string_buffer(bytes([0xAA]) * (B * need), B * need)
        L.rw_decompress_selected(form, src, N, need, slots, bytes(enough), B, out, ok)
        for i in range(B * need):
            j = i // need
            got = L.rw_selected_source(i, N, need, slots, bytes(enough), CB)
            if j == lacking:
                assert got == NO_SOURCE, (need, N, B, lacking, i)                # the guard: no offset was formed from 0xffffffff
                assert ok.raw[i] == 1 and out.raw[i * PB:(i + 1) * PB] == IDENT[CB], (need, N, B, lacking, i)
            else:
                assert got == (j * N + slot[i]) * CB, (need, N, B, lacking, i)
                w_ok, w_bytes = want[pick[j][slot[i]]]
                assert ok.raw[i] == w_ok and out.raw[i * PB:(i + 1) * PB] == w_bytes, (need, N, B, lacking, i)


def test_stand_alone_program_agrees():
    """the harness's own main (what a sanitizer build runs): the same routines, fixed inputs"""
    exe = os.path.join(ROOT, "tests", "robust", "robust_wire_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-DRW_MAIN", "-I" + CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "robust_wire_host: ok" in out.stdout, out.stdout + out.stderr
