"""The planned quotient form of the [1 / D] step of the subset-grouped G2 combination on the GPU (tc_jobs.h
combine_quotient_plan, combine_divide_cheapest).  Every case is a grouped launch of 4096 .. 4127 jobs over at most 16 index
tuples whose denominators plan every NAF width (2, 3, 4) and a shifted ladder scalar (m != 0); the plans themselves are read
from the host build of the same headers.  Checked as tests/test_gpu_combine_uniform.py checks its launches: every job against
Oracle B, and byte-equal to the same jobs in two ungrouped calls of half the size (the forms of a mixed wave)."""
import itertools
import random

import pytest

import test_combine_plan_host as h
import test_gpu_combine_uniform as u

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return h._build("libcombine_plan.so", [])


def _tuples(host, t, limit=16):
    """one (t + 1)-subset of ten signers per denominator: D = 1 and the smallest power of two, then the generic ones -- first one
    for every (width, m != 0) that occurs, then the rest by D -- up to the subset-mode limit of a 4096-job launch"""
    by_d = {}
    for s in itertools.combinations(range(10), t + 1):
        by_d.setdefault(u._denominator(s)[0], s)
    pow2 = min(D for D in by_d if D > 1 and D & (D - 1) == 0)
    plans = {D: h.plan(host, D)[:2] for D in sorted(by_d) if h.generic(D)}
    first = {}
    for D, (m, width) in plans.items():
        first.setdefault((width, m != 0), D)
    ds = [1, pow2] + sorted(first.values())
    ds += [D for D in plans if D not in ds][:limit - len(ds)]
    assert len(ds) <= limit
    return [by_d[D] for D in ds], {plans[D] for D in ds if D in plans}


@pytest.mark.parametrize("t, B", [(3, 4096 + 31), (2, 4096), (1, 4096)])
def test_planned_widths_and_shifts_in_one_launch(engine, host, t, B):
    """groups of 1, 31, 33 and 65 jobs leave padded lanes in their last wave; the rest is dealt over the other tuples"""
    rnd = random.Random(0x91A0 + t)
    tuples, plans = _tuples(host, t)
    assert {w for _, w in plans} == {2, 3, 4} and any(m for m, _ in plans) and (0, 3) in plans, plans
    src = u.Shares(engine, t, list(range(10)), 0x91A + t)
    rows = u._rows(rnd, tuples[::-1], [1, 31, 33, 65], B)
    idx, shares = u._batch(src, rows)
    u._check(engine, t, idx, shares)


# ---- the plan and the planned division themselves, on the device (tests/device/plan_probe.hip) ----------------------------
@pytest.fixture(scope="module")
def probe():
    import ctypes
    import os
    import device_conformance as dc
    from threshold_crypto_amd import build as tcb
    src = os.path.join(dc.DEV, "plan_probe.hip")
    lib = dc._build("libtc_plan_probe", lambda out: [dc.hipcc()] + tcb.FLAGS + ["-w", "-shared", "-I" + dc.CSRC, src, "-o", out], {"plan_probe.hip"})
    return ctypes.CDLL(lib)


def test_device_plan_is_the_host_plan(host, probe):
    """(m, width, multiply-adds) of combine_quotient_plan as a wave computes them, scalar, against the host build: the ten-signer
    denominators, every D up to 600, random D of 10 .. 61 bits, and what has no decomposition"""
    import ctypes
    rnd = random.Random(0x91B)
    ds = list(range(0, 600)) + [rnd.getrandbits(b) | (1 << (b - 1)) for b in range(10, 62) for _ in range(4)]
    ds += [(1 << 62) - 1, (1 << 62) + 1, 1 << 40, (1 << 61) + 1]
    out = (ctypes.c_int64 * (4 * len(ds)))()
    assert probe.tc_plan_probe(len(ds), (ctypes.c_uint64 * len(ds))(*ds), out) == 0
    planned = set()
    for i, D in enumerate(ds):
        want = h.plan(host, D)
        got = tuple(out[4 * i:4 * i + 4])
        assert got == ((1,) + want[:3] if want else (0, 0, 0, 0)), (D, got, want)
        if want:
            planned.add(want[:2])
    assert {w for _, w in planned} == {2, 3, 4} and {m for m, _ in planned} == {0, 1}


def test_device_division_at_every_candidate(probe):
    """[1 / D] by combine_divide_planned on the device at every (m, width) and at the wave's own plan (width 0): the oracle's
    point for all 32 jobs of the wave and NO exception flag -- the planned ladder itself computed it, not the complete form
    behind it"""
    import ctypes
    rnd = random.Random(0x91C)
    P = [u.o.E2.mul(u.o.G2_GEN, rnd.randrange(1, u.o.R)) for _ in range(4)]
    pts = b"".join(u.o.g2_uncompressed(P[j % 4]) for j in range(32))
    Ds = (3, 7, 9, 189, 12345)
    cand = [(D, m, w) for D in Ds for m, w in [(0, 0)] + [(m, w) for m in (0, 1) for w in (2, 3, 4)]]
    flat = [v for c in cand for v in c]
    out = ctypes.create_string_buffer(len(cand) * 32 * 192)
    flags = (ctypes.c_int32 * (len(cand) * 32 * 2))()
    assert probe.tc_plan_divide_probe(len(cand), (ctypes.c_int64 * len(flat))(*flat), pts, out, flags) == 0
    want = {D: [u.o.g2_uncompressed(u.o.E2.mul(p, 6 * pow(D, -1, u.o.R) % u.o.R)) for p in P] for D in Ds}   # (the probe divides [6] P)
    for i, (D, m, w) in enumerate(cand):
        for j in range(32):
            k = i * 32 + j
            assert (flags[2 * k], flags[2 * k + 1]) == (1, 0), (D, m, w, j)
            assert out.raw[k * 192:(k + 1) * 192] == want[D][j % 4], (D, m, w, j)
