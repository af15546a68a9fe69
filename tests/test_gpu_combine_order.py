"""The launch order of the grouped G2 combination on the GPU (k_combine.hip k_combine_plan / k_combine_place, tc_jobs.h
combine_order_start / combine_fold_wave): groups in descending order of their predicted cost, the second half of a single
resident round turned round.  The order only moves jobs between waves, so every case compares all signatures and statuses
byte for byte with Oracle B and with the same jobs in two ungrouped calls (test_gpu_combine_uniform._check).

Launches of 4096 and 4127 jobs over 16 tuples that span the generic, 2^a and D = 1 classes, a few indices >= 65 535 (the
group "none"), t = 1, 2, 3, on contexts created under TC_COMBINE_SEATS:
  64    128-160 waves are two resident rounds and more of 64 seats: descending cost, no fold
  128   the same launches are ONE round with a surplus (128 <= waves <= 152): the fold, and groups cut in two by it
  4096  fewer waves than seats: descending cost"""
import itertools
import random

import numpy as np
import pytest

import test_gpu_combine_uniform as u

pytestmark = pytest.mark.gpu


def _sixteen(t):
    """16 tuples of t + 1 of ten signers: D = 1, powers of two and generic denominators all among them"""
    by_cls = {"one": [], "pow2": [], "generic": []}
    for s in itertools.combinations(range(10), t + 1):
        D, _ = u._denominator(s)
        by_cls["one" if D == 1 else "pow2" if D & (D - 1) == 0 else "generic"].append(s)
    assert all(by_cls.values())
    chosen = by_cls["one"][:3] + by_cls["pow2"][:4]
    chosen += by_cls["generic"][:16 - len(chosen)]
    assert len(set(chosen)) == 16
    return chosen


@pytest.fixture(scope="module")
def sources(engine):
    signers = list(range(10)) + [65535, 70000]
    return {t: u.Shares(engine, t, signers, 0x0DE0 + t) for t in (1, 2, 3)}


def _launch(eng, src, t, B, seed):
    rnd = random.Random(seed)
    rows = u._rows(rnd, _sixteen(t), [1, 31, 33], B)
    idx, shares = u._batch(src, rows)
    for n, j in enumerate(rnd.sample(range(B), 5)):       # the group "none": the fast path leaves these jobs
        ids = list(rows[j])
        ids[-1] = (65535, 70000)[n % 2]
        idx[j] = ids
        shares[j] = src.job(j, ids)
    u._check(eng, t, idx, np.ascontiguousarray(shares))


@pytest.fixture(scope="module", params=[64, 128])
def seated(request):
    from conftest import engine_with_env
    with engine_with_env(TC_COMBINE_SEATS=request.param) as eng:
        yield eng


@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("B", [4096, 4127])
def test_ordered_launch(seated, sources, t, B):
    _launch(seated, sources[t], t, B, 31 * t + B)


def test_fewer_waves_than_seats(sources):
    from conftest import engine_with_env
    with engine_with_env(TC_COMBINE_SEATS=4096) as eng:
        _launch(eng, sources[3], 3, 4127, 7)
