"""The launch order of the grouped G2 combination on the CPU (tests/order, a test harness -- not a product path): the pieces of
tc_jobs.h that k_combine_plan / k_combine_place run (combine_key_macs, combine_order_start, combine_order_aligned,
combine_fold_wave, combine_order_slot) compiled by g++ and fed by the serial model of the three grouping kernels.

Checked: perm is a permutation of the jobs plus padding; every wave holds one tuple; a group is one run of waves, or two where
the order folds; the first seats / 2 waves never grow in cost and the waves beside them (k + seats / 2) never shrink; the
degenerate inputs; and the predictor -- the 210 four-subsets of ten signers ordered by combine_tuple_macs and by the executed
multiply-adds of profiles/combine_uniform_macs.json end within 0.5 % of each other in tools/sim_launch_order.py."""
import ctypes
import itertools
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sim_launch_order as sim  # noqa: E402

CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "order", "combine_order_host.cpp")
EMPTY = 0xffffffff
PAD = 32
ALL10 = list(itertools.combinations(range(10), 4))


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max([os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC)]
                                                                  + [os.path.getmtime(SRC)])


@pytest.fixture(scope="module")
def L():
    lib = os.path.join(ROOT, "tests", "order", "libcombine_order.so")
    if _stale(lib):
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-I" + CSRC, SRC, "-o", lib], check=True)
    lib = ctypes.CDLL(lib)
    for f in ("co_tuple_macs", "co_key_macs", "co_mixed_generic_macs", "co_group_slots", "co_fold_wave", "co_divide_macs", "co_divide_macs_by_comparison"):
        getattr(lib, f).restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def rnd():
    return random.Random(0x0DE2)


def macs(L, ids):
    return L.co_tuple_macs(len(ids) - 1, (ctypes.c_uint64 * len(ids))(*ids))


def plan(L, t, rows, seats):
    B, n = len(rows), t + 1
    flat = (ctypes.c_uint64 * (B * n))(*[v for row in rows for v in row])
    slots = L.co_group_slots(ctypes.c_size_t(B))
    perm = (ctypes.c_uint32 * slots)()
    cost, start = (ctypes.c_uint32 * 512)(), (ctypes.c_uint32 * 512)()
    fold, waves = ctypes.c_uint32(), ctypes.c_uint32()
    mode = L.co_plan(t, flat, ctypes.c_size_t(n), ctypes.c_size_t(B), seats, perm, cost, start, ctypes.byref(fold), ctypes.byref(waves))
    return mode, list(perm), fold.value, waves.value


def group_of(row):
    """the fast path leaves a job with an index >= 65 535 or a repeated index: they share the group "none" """
    return "none" if max(row) >= 65535 or len(set(row)) < len(row) else tuple(row)


def check_order(L, t, rows, seats, perm, fold, waves):
    """everything the order promises; returns the cost of every wave in launch order"""
    B = len(rows)
    assert sorted(p for p in perm if p != EMPTY) == list(range(B))              # every job once, the rest padding
    used = [w for w in range(len(perm) // PAD) if any(p != EMPTY for p in perm[w * PAD:(w + 1) * PAD])]
    assert used == list(range(waves))                                           # no hole, nothing past the last wave
    wave_group, wave_cost = [], []
    for w in used:
        groups = {group_of(rows[p]) for p in perm[w * PAD:(w + 1) * PAD] if p != EMPTY}
        assert len(groups) == 1, w                                              # one tuple per wave
        g = groups.pop()
        wave_group.append(g)
        wave_cost.append(L.co_mixed_generic_macs() if g == "none" else macs(L, g))
    sizes = {}
    for r in rows:
        sizes[group_of(r)] = sizes.get(group_of(r), 0) + 1
    assert waves == sum((n + PAD - 1) // PAD for n in sizes.values())           # padding: less than a wave per group
    runs = {}
    for w, g in enumerate(wave_group):
        if w == 0 or wave_group[w - 1] != g:
            runs[g] = runs.get(g, 0) + 1
    assert all(n <= (2 if fold else 1) for n in runs.values()), runs             # a group is cut only where the order folds
    half = seats // 2
    if fold:
        assert fold == seats and seats <= waves and 16 * waves <= 19 * seats
        first, beside, last = wave_cost[:half], wave_cost[half:2 * half], wave_cost[2 * half:]
        assert all(a >= b for a, b in zip(first, first[1:]))                     # the heaviest, descending
        assert all(a <= b for a, b in zip(beside, beside[1:]))                   # wave k + seats / 2: never lighter than the one before
        assert all(a >= b for a, b in zip(last, last[1:]))
        assert min(first) >= max(beside) and (not last or min(beside) >= max(last))   # the cheapest surplus last
    else:
        assert not (seats >= 2 and seats <= waves and 16 * waves <= 19 * seats)
        assert all(a >= b for a, b in zip(wave_cost, wave_cost[1:]))             # plain descending cost
    return wave_cost


def rows_over(rnd, subsets, B, sizes=()):
    rows = []
    for s, n in zip(subsets, sizes):
        rows += [list(s)] * n
    rest = subsets[len(sizes):]
    k = 0
    while len(rows) < B:
        rows.append(list(rest[k % len(rest)]))
        k += 1
    rnd.shuffle(rows)
    return rows


SIXTEEN = [(0, 1, 2, 3), (1, 2, 3, 4), (0, 1, 2, 4), (0, 2, 4, 6), (0, 2, 4, 8)] + ALL10[5:16]


@pytest.mark.parametrize("B", [4096, 4127])
@pytest.mark.parametrize("seats", [128, 129, 130])
def test_single_round_is_folded(L, rnd, B, seats):
    rows = rows_over(rnd, SIXTEEN, B, [1, 31, 33])
    mode, perm, fold, waves = plan(L, 3, rows, seats)
    assert mode == 1 and fold == seats
    cost = check_order(L, 3, rows, seats, perm, fold, waves)
    assert len(set(cost)) > 3                                                    # D = 1, 2^a and generic costs all present


def test_fold_cuts_a_group_in_two(L, rnd):
    rows = rows_over(rnd, SIXTEEN, 4096, [100, 300])
    _, perm, fold, waves = plan(L, 3, rows, 128)
    assert fold == 128
    groups = [group_of(rows[perm[w * PAD]]) for w in range(waves)]
    runs = {}
    for w, g in enumerate(groups):
        if w == 0 or groups[w - 1] != g:
            runs[g] = runs.get(g, 0) + 1
    assert max(runs.values()) == 2                                               # groups of 4, 9 and 10 waves: wave 64 falls inside one


@pytest.mark.parametrize("seats", [0, 1, 64, 100, 4096, 1 << 20])
def test_other_regimes_descend(L, rnd, seats):
    """several rounds (waves > 19 / 16 seats), fewer waves than seats, no seats known"""
    rows = rows_over(rnd, SIXTEEN, 4127, [1, 31])
    mode, perm, fold, waves = plan(L, 3, rows, seats)
    assert mode == 1 and fold == 0
    check_order(L, 3, rows, seats, perm, fold, waves)


@pytest.mark.parametrize("name, subsets", [("one group", [(2, 5, 7, 9)]),
                                            ("only D = 1", [(0, 1, 2, 3), (1, 2, 3, 4), (0, 3, 4, 5), (1, 3, 5, 7)]),
                                            ("only generic", [(0, 1, 2, 5), (0, 1, 2, 6), (0, 1, 3, 4), (0, 1, 2, 9)])])
@pytest.mark.parametrize("seats", [128, 64])
def test_degenerate_groups(L, rnd, name, subsets, seats):
    rows = rows_over(rnd, subsets, 4096)
    mode, perm, fold, waves = plan(L, 3, rows, seats)
    assert mode == 1 and fold == (seats if seats == 128 else 0)
    check_order(L, 3, rows, seats, perm, fold, waves)


@pytest.mark.parametrize("seats", [128, 64])
def test_the_group_none(L, rnd, seats):
    rows = rows_over(rnd, SIXTEEN[:8], 4096)
    for j in rnd.sample(range(4096), 40):
        rows[j] = [rows[j][0], rows[j][1], rows[j][2], rnd.choice([65535, 70000])]
    rows[5] = [4, 4, 5, 6]
    mode, perm, fold, waves = plan(L, 3, rows, seats)
    assert mode == 1
    cost = check_order(L, 3, rows, seats, perm, fold, waves)
    assert max(cost) == L.co_mixed_generic_macs()                                # priced as a mixed wave of the generic class


def test_fallback_is_unchanged(L, rnd):
    """more than 256 tuples, or too many for the batch: the classes, placed as before, whatever the seats"""
    many = rnd.sample(list(itertools.combinations(range(16), 4)), 300)
    for subsets, B in ((many, 4127), (ALL10[:17], 4096)):
        rows = rows_over(rnd, subsets, B)
        got = [plan(L, 3, rows, seats) for seats in (0, 64, 128, 4096)]
        assert all(g[0] == 0 and g[2] == 0 for g in got)
        assert all(g[1] == got[0][1] for g in got)
        perm = got[0][1]
        assert sorted(p for p in perm if p != EMPTY) == list(range(B))
        from test_combine_uniform_host import _check_perm
        _check_perm(3, rows, 0, perm, 64)
        # generic, 2^a, 1: the class order along the permutation never decreases
        def cls(row):
            D = sim.cls_of(_denominator(row))
            return D
        seq = [cls(rows[p]) for p in perm if p != EMPTY]
        assert seq == sorted(seq)


def _denominator(ids):
    from math import gcd
    xs = [i + 1 for i in ids]
    den = []
    for i in range(len(xs)):
        d = 1
        for j in range(len(xs)):
            if j != i:
                d *= xs[j] - xs[i]
        den.append(abs(d))
    D = 1
    for d in den:
        D = D * d // gcd(D, d)
    cs = []
    for i, d in enumerate(den):
        v = D // d
        for j in range(len(xs)):
            if j != i:
                v *= xs[j]
        cs.append(v)
    g = D
    for v in cs:
        g = gcd(g, v)
    return D // g


def test_fold_is_a_permutation_of_the_waves(L):
    for seats in (0, 1, 2, 3, 64, 65, 2048):
        for waves in (0, 1, seats, seats + 7, 2 * seats + 3):
            assert sorted(L.co_fold_wave(d, seats) for d in range(waves + 2 * seats)) == list(range(waves + 2 * seats))[:waves + 2 * seats]
    assert [L.co_fold_wave(d, 8) for d in range(10)] == [0, 1, 2, 3, 7, 6, 5, 4, 8, 9]


def test_small_denominators_take_the_planned_form(L, rnd):
    """combine_divide_macs skips the comparison with the 4-dimensional ladder below 2^12: the planned form is the cheaper there"""
    for D in list(range(3, 1 << 12)) + [rnd.randrange(1 << 12, 1 << 40) for _ in range(300)]:
        if D & (D - 1):
            assert L.co_divide_macs(ctypes.c_uint64(D)) == L.co_divide_macs_by_comparison(ctypes.c_uint64(D)), D


def test_predictor_ranks_as_the_executed_counts(L):
    """the criterion: both orders through the model, makespans within 0.5 % at 65 536 jobs"""
    table = json.load(open(os.path.join(ROOT, "profiles", "combine_uniform_macs.json")))["subsets"]
    executed, unit = sim.load_costs()
    predicted = {k: macs(L, [int(x) for x in k.split()]) for k in table}
    counts = sim.draw_counts(executed, 65536, 1)
    R = 2048
    true_waves = sim.waves_of(counts, executed)
    # the order the predictor gives, run at the executed costs
    by_name = {}
    for w in true_waves:
        by_name.setdefault(w[2], []).append(w)
    pred_waves = [(predicted[name] / unit, ws[0][1], name) for name, ws in by_name.items() for _ in ws]
    order = sim.order_aligned(pred_waves, R)
    at_true_cost = [(executed[w[2]]["cost"], w[1], w[2]) for w in order]
    a = sim.makespan(sim.order_aligned(true_waves, R), R)
    b = sim.makespan(at_true_cost, R)
    print("makespan ordered by executed counts %.4f W, by prediction %.4f W" % (a, b))
    assert abs(a - b) / a < 0.005
