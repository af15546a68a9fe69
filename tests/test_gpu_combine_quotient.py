"""The two forms of the [1 / D] step of the subset-grouped G2 combination on the GPU (tc_jobs.h combine_divide_quotient and
combine_divide_uniform, chosen per wave by combine_divide_takes_quotient).  Every case is a grouped launch of 4096 .. 4127
jobs over at most 16 index tuples, checked as tests/test_gpu_combine_uniform.py checks its launches: every job against
Oracle B, and byte-equal to the same jobs in two ungrouped calls of half the size (the forms of a mixed wave)."""
import itertools
import random

import numpy as np
import pytest

import test_gpu_combine_uniform as u

pytestmark = pytest.mark.gpu

SIGNERS = list(range(11)) + [13, 100, 1000]
MID = (0, 1, 2, 13)              # D = 286: between 2^8 and 2^12, the quotient form with 9-bit coefficients
LARGE = (0, 10, 100, 1000)       # D = 81 000 000 > 2^20: the wave keeps the 4-dimensional ladder


def _tuples():
    """one 4-subset of ten signers for each of D = 3, 5, 35, 189, 1 and the smallest power of two, then MID and LARGE"""
    by_d = {}
    for s in itertools.combinations(range(10), 4):
        by_d.setdefault(u._denominator(s)[0], []).append(s)
    pow2 = next(D for D in sorted(by_d) if D > 1 and D & (D - 1) == 0)
    chosen = [by_d[D][0] for D in (3, 5, 35, 189, 1, pow2)] + [MID, LARGE]
    assert u._denominator(MID)[0] == 286 and u._denominator(LARGE)[0] == 81000000
    return chosen


@pytest.fixture(scope="module")
def src(engine):
    return u.Shares(engine, 3, SIGNERS, 0x9D1)


@pytest.mark.parametrize("B", [4096, 4127])
def test_both_divide_forms_in_one_launch(engine, src, B):
    """groups of 1, 31, 33 and 65 jobs leave padded lanes in their last wave; the rest is dealt over the other tuples"""
    rnd = random.Random(B)
    tuples = _tuples()
    order = tuples[:] if B == 4096 else tuples[::-1]
    rows = u._rows(rnd, order, [1, 31, 33, 65], B)
    idx, shares = u._batch(src, rows)
    u._check(engine, 3, idx, shares)


def test_exceptional_shares_inside_uniform_waves(engine, src):
    """a share at infinity and two equal shares in waves of every generic tuple: the lanes' flags send them to the complete
    form, and their wave-mates are unaffected"""
    rnd = random.Random(3)
    tuples = _tuples()
    rows = u._rows(rnd, tuples, [], 4096)
    idx, shares = u._batch(src, rows)
    inf = np.frombuffer(u.INF, dtype=np.uint8)
    for s in tuples:
        jobs = [j for j, r in enumerate(rows) if tuple(r) == s]
        shares[jobs[0], 3] = inf                                 # a share at infinity
        shares[jobs[1], 0] = inf
        shares[jobs[2], 1] = shares[jobs[2], 0]                  # two equal share points under distinct indices
        shares[jobs[3]] = shares[jobs[3], 2]                     # one point throughout
        shares[jobs[40]] = inf                                   # nothing but infinity: Q itself is the identity
    u._check(engine, 3, idx, np.ascontiguousarray(shares))
