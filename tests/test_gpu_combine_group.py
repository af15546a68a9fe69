"""The G2 grouping kernels on the GPU (k_combine.hip k_combine_group / _plan / _place): ranks aggregated per workgroup in LDS,
one lane per distinct key on the call's table, group starts by a prefix sum, the general jobs counted on the side.  Every case
is a launch of 4096 .. 4127 jobs, the smallest that is grouped; every job is compared with Oracle B and with the same jobs
combined in two ungrouped calls of half the size (test_gpu_combine_uniform._check).  A job the grouping placed nowhere would
keep whatever the fresh output buffer held, so all jobs are compared, not a sample."""
import itertools
import random

import numpy as np
import pytest

import test_gpu_combine_uniform as u
from test_combine_group_host import table_hash, tuple_key, wrap_tuples

pytestmark = pytest.mark.gpu

B0 = u.B0


@pytest.fixture(scope="module")
def src3(engine):
    return u.Shares(engine, 3, list(range(16)), 0x6209)


def _run(engine, src, t, rows, special=()):
    idx, shares = u._batch(src, rows)
    return u._check(engine, t, idx, shares, special)


def test_one_tuple_for_every_job(engine, src3):
    """every workgroup adds its count to ONE entry of the call's table"""
    _run(engine, src3, 3, [[2, 5, 7, 9]] * B0)


@pytest.mark.parametrize("distinct, signers", [(16, 10), (17, 10), (300, 16)])
def test_mode_boundary_and_overflow(engine, src3, distinct, signers):
    """16 tuples of 4096 jobs: subset mode (32 G <= B / 8); 17: the classes; 300 over 16 signers: more than the table admits"""
    rnd = random.Random(100 + distinct)
    subsets = rnd.sample(list(itertools.combinations(range(signers), 4)), distinct)
    _run(engine, src3, 3, u._rows(rnd, subsets, [], B0))


def test_probe_wraps_round_the_call_table(engine):
    """tuples whose probe starts at the last entry of the call's table (found on the host: test_combine_group_host)"""
    rnd = random.Random(7)
    wrap = wrap_tuples()
    assert all(table_hash(tuple_key(s)) == 511 for s in wrap)
    signers = sorted({i for s in wrap for i in s} | {0, 1, 2, 3})
    src = u.Shares(engine, 3, signers, 0x511)
    _run(engine, src, 3, u._rows(rnd, list(wrap) + [(0, 1, 2, 3)], [33, 1], B0))


def test_jobs_the_fast_path_leaves(engine):
    """an index of 65 535 and above, and a repeated index, inside groups of ordinary jobs: the grouping counts them, the
    Lagrange stage behind it and the two-stage kernels take them, statuses as the ungrouped calls give them"""
    rnd = random.Random(9)
    signers = list(range(10)) + [65535, 70000]
    src = u.Shares(engine, 3, signers, 0x3F2)
    subsets = [(0, 1, 2, 3), (1, 3, 4, 8), (2, 5, 7, 9), (0, 4, 6, 9)]
    rows = u._rows(rnd, subsets, [], B0)
    idx, shares = u._batch(src, rows)
    picks = rnd.sample(range(B0), 9)
    for n, j in enumerate(picks):
        ids = [[2, 5, 7, 65535], [1, 70000, 4, 8], [0, 4, 4, 9]][n % 3]
        idx[j] = ids
        shares[j] = src.job(j, ids)
    u._check(engine, 3, idx, np.ascontiguousarray(shares))


def test_workspace_is_fresh_for_every_call(engine, src3):
    """two calls on one context with different tuple sets, a third with a ragged tail, then the first again"""
    rnd = random.Random(78)
    all10 = list(itertools.combinations(range(10), 4))
    first_rows = u._rows(rnd, all10[:12], [], B0)
    first = _run(engine, src3, 3, first_rows)
    _run(engine, src3, 3, u._rows(rnd, list(itertools.combinations(range(4, 14), 4))[60:76], [], B0))
    _run(engine, src3, 3, u._rows(rnd, all10[100:109], [1, 31], 4127))
    idx, shares = u._batch(src3, first_rows)
    again, st = engine.combine_g2(3, idx, shares)
    assert not np.asarray(st).any() and (np.asarray(again) == first).all()


@pytest.mark.parametrize("t", [1, 2])
def test_other_thresholds(engine, t):
    rnd = random.Random(20 + t)
    src = u.Shares(engine, t, list(range(10)), 0x2E4 + t)
    subsets = rnd.sample(list(itertools.combinations(range(10), t + 1)), 8)
    _run(engine, src, t, u._rows(rnd, subsets, [1, 33], B0))
