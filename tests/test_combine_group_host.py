"""The G2 grouping kernels' building blocks on the CPU (tests/group, a test harness -- not a product path): the device header
tc_jobs.h compiled by g++.  k_combine_group counts a workgroup's jobs per key in a table of its own and sends ONE lane per
distinct key to the call's table; k_combine_plan takes the group starts from a prefix sum per order.  Checked here: the
starts against combine_group_start, the placement the pieces give when they feed the serial model of the three kernels, and
the workgroup's table under collisions."""
import ctypes
import itertools
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_combine_uniform_host import _check_perm  # noqa: E402

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "group", "combine_group_host.cpp")
EMPTY = 0xffffffff
GOLDEN = 0x9E3779B97F4A7C15


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max([os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)]
                                                                  + [os.path.getmtime(SRC)])


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "group", "libcombine_group.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    for f in ("cg_wg_jobs", "cg_wg_slots", "cg_wg_hash", "cg_table_hash", "cg_probe_step", "cg_group_slots"):
        getattr(lib, f).restype = ctypes.c_uint32
    lib.cg_key.restype = ctypes.c_uint64
    return lib


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0x6209)


def table_hash(key):
    """the entry a key's probe of the call's table starts at"""
    return ((key * GOLDEN % 2**64) >> 40) & 511


def probe_step(key):
    """the odd step of a key's probe: the top nine bits of the same hash"""
    return ((((key * GOLDEN % 2**64) >> 40) >> 15) & 511) | 1


def tuple_key(ids):
    return sum(v << (16 * k) for k, v in enumerate(ids))


def table_model(keys):
    """the entries the call's table gives `keys`, inserted in this order (none of the tests here fills it)"""
    table = {}
    for key in keys:
        h = table_hash(key)
        while table.get(h, key) != key:
            h = (h + probe_step(key)) & 511
        table[h] = key
    return {key: h for h, key in table.items()}


def wrap_tuples(signers=40, want=3):
    """four-subsets (the fast path's: small distinct indices) whose probe starts at the table's LAST entry, so that all but the
    first of them step past the end and wrap round"""
    out = [s for s in itertools.combinations(range(signers), 4) if table_hash(tuple_key(s)) == 511]
    assert len(out) >= want
    return out[:want]


# ---- starts ----------------------------------------------------------------------------------------------------
def _starts(L, count, order, pad):
    n = len(count)
    c = (ctypes.c_uint32 * n)(*count)
    o = (ctypes.c_uint8 * n)(*order)
    a, b = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    L.cg_scan_starts(c, o, n, pad, a)
    L.cg_walk_starts(c, o, n, pad, b)
    return list(a), list(b)


def test_scan_starts_equal_the_walks(L, rnd):
    cases = []
    for n in (512, 3, 1, 5, 64, 100):
        cases.append(([0] * n, [rnd.randrange(4) for _ in range(n)]))                                    # nothing anywhere
        for _ in range(6):
            cases.append(([rnd.choice([0, 0, 1, 31, 32, 33, rnd.randrange(70000)]) for _ in range(n)], [rnd.randrange(4) for _ in range(n)]))
    one = [0] * 512
    one[rnd.randrange(512)] = 65536
    cases.append((one, [3] * 512))                                                                       # one group
    cases.append((one, [rnd.randrange(4) for _ in range(512)]))
    used = set(rnd.sample(range(512), 256))                                                              # 256 groups, the most subset mode has
    cases.append(([rnd.randrange(1, 600) if s in used else 0 for s in range(512)], [rnd.randrange(3) if s in used else 3 for s in range(512)]))
    cases.append(([2**22] * 512, [s % 4 for s in range(512)]))                                           # sums near 2^31
    for count, order in cases:
        for pad in (32, 64):
            a, b = _starts(L, count, order, pad)
            assert a == b, (len(count), pad)


# ---- placement ---------------------------------------------------------------------------------------------------
def _plan(L, t, idx_rows):
    B = len(idx_rows)
    n = t + 1
    flat = (ctypes.c_uint64 * (B * n))(*[v for row in idx_rows for v in row])
    slots = L.cg_group_slots(ctypes.c_size_t(B))
    perm = (ctypes.c_uint32 * slots)()
    starts = (ctypes.c_uint32 * 512)()
    orders = (ctypes.c_uint8 * 512)()
    groups, need = ctypes.c_uint32(), ctypes.c_uint32()
    mode = L.cg_plan(t, flat, ctypes.c_size_t(n), ctypes.c_size_t(B), perm, starts, orders, ctypes.byref(groups), ctypes.byref(need))
    return mode, list(perm), list(starts), list(orders), groups.value, need.value


def _orders_never_decrease(starts, orders):
    seq = [orders[i] for i in sorted((i for i in range(512) if starts[i] != EMPTY), key=lambda i: starts[i])]
    assert seq == sorted(seq)


@pytest.mark.parametrize("B", [4096, 4097, 4127])
def test_placement_is_valid(L, rnd, B):
    subsets = list(itertools.combinations(range(10), 4))
    for G in (1, 2, 16, 17, 210):
        chosen = rnd.sample(subsets, G)
        rows = [list(chosen[i % G]) for i in range(B)]
        rnd.shuffle(rows)
        mode, perm, starts, orders, groups, need = _plan(L, 3, rows)
        assert groups == G and need == 0
        assert mode == (1 if 32 * G <= B // 8 else 0), (B, G)
        _check_perm(3, rows, mode, perm, 32 if mode else 64)
        if mode:
            _orders_never_decrease(starts, orders)
            sizes = {tuple(s): sum(1 for r in rows if tuple(r) == tuple(s)) for s in chosen}
            assert len([p for p in perm if p != EMPTY]) == B
            assert max(i for i, p in enumerate(perm) if p != EMPTY) < sum((v + 31) // 32 * 32 for v in sizes.values())


def test_overflow_and_jobs_the_fast_path_leaves(L, rnd):
    many = rnd.sample(list(itertools.combinations(range(16), 4)), 300)
    rows = [list(many[i % 300]) for i in range(4127)]
    rnd.shuffle(rows)
    mode, perm, _, _, groups, need = _plan(L, 3, rows)
    assert mode == 0 and groups > 256 and need == 0                # more tuples than the table admits: the classes
    _check_perm(3, rows, mode, perm, 64)
    # an index of 65 535 and a repeated index: one group (key "none"), the last; counted for the Lagrange stage
    rows = [[0, 1, 2, 3]] * 100 + [[0, 1, 2, 65535]] * 3 + [[4, 4, 5, 6]] * 2 + [[1, 2, 3, 4]] * 3991
    rnd.shuffle(rows)
    mode, perm, starts, orders, groups, need = _plan(L, 3, rows)
    assert mode == 1 and groups == 3 and need == 5
    _check_perm(3, [r if r[3] != 65535 and r[0] != r[1] else ["none"] for r in rows], mode, perm, 32)
    _orders_never_decrease(starts, orders)
    assert sorted(orders[i] for i in range(512) if starts[i] != EMPTY)[-1] == 3


def test_probe_wraps_round_the_call_table(L, rnd):
    wrap = wrap_tuples()
    for s in wrap:
        key = ctypes.c_uint64(tuple_key(s))
        assert L.cg_table_hash(key) == 511 and L.cg_key(3, (ctypes.c_uint64 * 4)(*s)) == tuple_key(s)
        assert L.cg_probe_step(key) == probe_step(tuple_key(s)) and probe_step(tuple_key(s)) % 2 == 1
    rows = [list(wrap[i % 3]) for i in range(4096)] + [[0, 1, 2, 3]] * 31
    rnd.shuffle(rows)
    mode, perm, starts, orders, groups, need = _plan(L, 3, rows)
    assert mode == 1 and groups == 4
    used = {i for i in range(512) if starts[i] != EMPTY}
    seen = []                                                     # the keys in the order the serial model meets them
    for r in rows:
        if tuple_key(r) not in seen:
            seen.append(tuple_key(r))
    entry = table_model(seen)
    assert used == set(entry.values()) and 511 in used
    assert sum(1 for s in wrap if entry[tuple_key(s)] < 511) == 2  # two of the three left the last entry: past the end and round
    _check_perm(3, rows, mode, perm, 32)


# ---- the workgroup's table -----------------------------------------------------------------------------------------
def _aggregate(L, keys):
    n, slots = len(keys), L.cg_wg_slots()
    slot, lrank = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    made = (ctypes.c_uint8 * n)()
    wkey, wcount = (ctypes.c_uint64 * slots)(), (ctypes.c_uint32 * slots)()
    entries = L.cg_wg_aggregate((ctypes.c_uint64 * n)(*keys), n, slot, lrank, made, wkey, wcount)
    return entries, list(slot), list(lrank), list(made), list(wkey), list(wcount)


def _check_aggregate(L, keys):
    entries, slot, lrank, made, wkey, wcount = _aggregate(L, keys)
    distinct = sorted(set(keys))
    assert entries == len(distinct) == sum(made) == sum(1 for k in wkey if k)
    assert sum(wcount) == len(keys)
    for k in distinct:
        jobs = [i for i, v in enumerate(keys) if v == k]
        s = {slot[i] for i in jobs}
        assert len(s) == 1                                         # one entry per key ...
        s = s.pop()
        assert wkey[s] == k and wcount[s] == len(jobs)             # ... that holds it and counts its jobs
        assert sorted(lrank[i] for i in jobs) == list(range(len(jobs)))   # ranks 0 .. count - 1, each once
        assert sum(made[i] for i in jobs) == 1                     # ONE lane goes to the call's table for the key
    return slot


def test_workgroup_table(L, rnd):
    W = L.cg_wg_jobs()
    assert W == 256 and L.cg_wg_slots() == 2 * W
    pool = [tuple_key(s) for s in itertools.combinations(range(12), 4)]
    none = 2**64 - 1
    for distinct in (1, 2, 256):
        ks = rnd.sample(pool, distinct)
        keys = [ks[i % distinct] for i in range(W)]
        rnd.shuffle(keys)
        _check_aggregate(L, keys)
    _check_aggregate(L, [none] * 7 + rnd.sample(pool, 40) * 3)     # a ragged last workgroup, with jobs the fast path leaves
    _check_aggregate(L, [pool[0]])
    # keys that meet in the workgroup's table: one start entry for all of them
    by_hash = {}
    for s in itertools.combinations(range(24), 4):
        by_hash.setdefault(L.cg_wg_hash(ctypes.c_uint64(tuple_key(s))), []).append(tuple_key(s))
    h, clash = max(by_hash.items(), key=lambda kv: len(kv[1]))
    assert len(clash) >= 8
    keys = [clash[i % 8] for i in range(W)]
    rnd.shuffle(keys)
    slot = _check_aggregate(L, keys)
    assert sorted(set(slot)) == sorted((h + i) % 512 for i in range(8))
    # ... and at the table's end, where the probe wraps
    last = by_hash.get(511, [])
    assert len(last) >= 3
    slot = _check_aggregate(L, [last[i % 3] for i in range(W)])
    assert sorted(set(slot)) == [0, 1, 511]
    # and the wrap-round tuples of the CALL's table, which the workgroup's table must spread (other bits of the hash)
    wrap = [tuple_key(s) for s in wrap_tuples(want=3)]
    _check_aggregate(L, [wrap[i % 3] for i in range(W)])


def test_stand_alone_program_agrees():
    """the harness's own main, built with the address and undefined-behaviour sanitizers: fixed inputs, exactly-sized arrays"""
    exe = os.path.join(ROOT, "tests", "group", "combine_group_host_main")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCG_MAIN", "-I" + CSRC,
                        SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "combine_group_host: ok" in out.stdout, out.stdout + out.stderr
