"""The subset-grouped G2 combination on the GPU (k_combine.hip k_combine_keys / _plan / _place, tc_jobs.h
combine_uniform_wave).  Every case is a launch of 4096 .. 4127 jobs, the smallest that is grouped: shares from
engine.g2_mul, every job against Oracle B (plain C), and byte-equal to the same jobs combined in two calls of half the
size, which are not grouped and therefore take the forms of a mixed wave."""
import itertools
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o

pytestmark = pytest.mark.gpu

B0 = 4096
INF = bytes([0x40]) + bytes(191)
TC_JOB_INVALID_ENCODING = 3


def _denominator(ids):
    """the common denominator D of the small-index fast path (tc_threshold.h lagrange_small_coeffs) and the longest |c_i|"""
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
    return D // g, max(v // g for v in cs).bit_length()


class Shares:
    """the shares of `signers` signers over a few message points, from the device's own g2_mul"""

    def __init__(self, engine, t, signers, seed, points=4):
        rnd = random.Random(seed)
        self.t = t
        self.poly = [rnd.randrange(o.R) for _ in range(t + 1)]
        fr = np.stack([np.frombuffer(o.fr_to_bytes(o.secret_key_share(self.poly, i)), dtype=np.uint8) for i in signers])
        pts = np.stack([np.frombuffer(o.g2_uncompressed(o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))), dtype=np.uint8) for _ in range(points)])
        sh, st = engine.g2_mul(np.ascontiguousarray(fr), np.ascontiguousarray(pts))      # (points, S, 192)
        assert not np.asarray(st).any()
        self.sh = np.asarray(sh)
        self.col = {s: k for k, s in enumerate(signers)}
        self.points = points

    def job(self, j, ids):
        return self.sh[j % self.points, [self.col[i] for i in ids]]


def _batch(src, rows):
    idx = np.array(rows, dtype=np.uint64)
    shares = np.stack([src.job(j, ids) for j, ids in enumerate(rows)])
    return idx, np.ascontiguousarray(shares)


def _check(engine, t, idx, shares, special=()):
    """the grouped launch against the oracle and against two ungrouped calls; special: jobs whose status is not 0"""
    B = len(idx)
    out, st = engine.combine_g2(t, idx, shares)
    out, st = np.asarray(out), np.asarray(st)
    # (the oracle once per distinct job: the batch repeats a few message points over a few tuples)
    rows = np.concatenate([idx.view(np.uint8).reshape(B, -1), shares.reshape(B, -1)], axis=1)
    _, pick, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    want_u, rc_u = c.combine_g2_batch(t, np.ascontiguousarray(idx[pick]), np.ascontiguousarray(shares[pick]), c.host_threads())
    want, rc = want_u[inv.reshape(-1)], rc_u[inv.reshape(-1)]
    for j in range(B):
        if j in special:
            assert rc[j] != 0 and st[j] == TC_JOB_INVALID_ENCODING and bytes(out[j]) == INF, j
        else:
            assert rc[j] == 0 and st[j] == 0, j
    plain = np.ones(B, dtype=bool)
    plain[list(special)] = False
    bad = np.nonzero((out != want).any(axis=1) & plain)[0]
    assert bad.size == 0, (bad[:8], [tuple(idx[j]) for j in bad[:8]])
    half = B // 2
    lo, st_lo = engine.combine_g2(t, np.ascontiguousarray(idx[:half]), np.ascontiguousarray(shares[:half]))
    hi, st_hi = engine.combine_g2(t, np.ascontiguousarray(idx[half:]), np.ascontiguousarray(shares[half:]))
    assert half < B0 and B - half < B0                      # below the grouping threshold: the jobs' own order
    assert (np.concatenate([np.asarray(lo), np.asarray(hi)]) == out).all()
    assert (np.concatenate([np.asarray(st_lo), np.asarray(st_hi)]) == st).all()
    return out


def _rows(rnd, subsets, sizes, B):
    """sizes[i] jobs of subsets[i], the rest dealt round-robin over the remaining subsets; shuffled"""
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


@pytest.fixture(scope="module")
def src3(engine):
    return Shares(engine, 3, list(range(16)), 0x1D3)


def _twelve_subsets():
    """12 four-subsets of ten signers that cover D = 1, a power of two, D = 3 (the lightest [1 / D] ladder), D = 10 or 40 (the
    heaviest), D = 189, and a 9-bit c_i"""
    by_d = {}
    nine_bit = None
    for s in itertools.combinations(range(10), 4):
        D, bits = _denominator(s)
        by_d.setdefault(D, []).append(s)
        if bits == 9 and nine_bit is None and D & (D - 1):
            nine_bit = s
    assert nine_bit is not None
    pow2 = next(D for D in sorted(by_d) if D > 1 and D & (D - 1) == 0)
    heavy = 10 if 10 in by_d else 40
    chosen = [by_d[1][0], by_d[pow2][0], by_d[3][0], by_d[heavy][0], by_d[189][0], nine_bit]
    for s in itertools.combinations(range(10), 4):
        if len(chosen) == 12:
            break
        if s not in chosen:
            chosen.append(s)
    return chosen


def test_mixed_subsets_with_ragged_groups(engine, src3):
    rnd = random.Random(11)
    subsets = _twelve_subsets()
    assert len(set(subsets)) == 12
    rows = _rows(rnd, subsets, [1, 31, 32, 33, 65], B0)
    idx, shares = _batch(src3, rows)
    _check(engine, 3, idx, shares)


@pytest.mark.parametrize("distinct, signers", [(16, 10), (17, 10), (300, 16)])
def test_mode_boundary(engine, src3, distinct, signers):
    """16 subsets of 4096 jobs: subset mode (32 G <= B / 8); 17: the classes; 300 tuples: more than the table admits"""
    rnd = random.Random(distinct)
    subsets = rnd.sample(list(itertools.combinations(range(signers), 4)), distinct)
    rows = _rows(rnd, subsets, [], B0)
    idx, shares = _batch(src3, rows)
    _check(engine, 3, idx, shares)


@pytest.mark.parametrize("t", [1, 2])
def test_other_thresholds(engine, t):
    rnd = random.Random(t)
    src = Shares(engine, t, list(range(10)), 0x2E0 + t)
    subsets = rnd.sample(list(itertools.combinations(range(10), t + 1)), 8)
    rows = _rows(rnd, subsets, [1, 33], B0)
    idx, shares = _batch(src, rows)
    _check(engine, t, idx, shares)


def test_special_jobs_inside_uniform_groups(engine):
    """an undecodable share, an index of 65 535, a duplicate index, two identical share points and a share at infinity, each
    inside a group of ordinary jobs over the same indices: each matches the oracle and its wave-mates are unaffected"""
    rnd = random.Random(5)
    signers = list(range(10)) + [65535]
    src = Shares(engine, 3, signers, 0x3F1)
    subsets = [(0, 1, 2, 3), (1, 3, 4, 8), (2, 5, 7, 9), (0, 4, 6, 9), (3, 5, 6, 8), (1, 2, 6, 7)]
    rows = _rows(rnd, subsets, [], B0)
    idx, shares = _batch(src, rows)

    def first(s, skip=0):
        return [j for j, r in enumerate(rows) if tuple(r) == s][skip]

    bad = first(subsets[1])
    shares[bad, 2, 0] ^= 0x20                                   # sets a flag bit no uncompressed encoding has: undecodable
    big = first(subsets[2])
    idx[big] = [2, 5, 7, 65535]                                 # leaves the fast path for the general one
    shares[big] = src.job(big, [2, 5, 7, 65535])
    dup = first(subsets[3])
    idx[dup] = [0, 4, 4, 9]                                     # the reference filters equal abscissae by value
    same = first(subsets[4])
    shares[same, 1] = shares[same, 0]                           # two identical share points under distinct indices
    inf = first(subsets[5])
    shares[inf, 3] = np.frombuffer(INF, dtype=np.uint8)
    inf0 = first(subsets[5], 1)
    shares[inf0, 0] = np.frombuffer(INF, dtype=np.uint8)
    _check(engine, 3, idx, np.ascontiguousarray(shares), special=(bad,))


@pytest.mark.parametrize("B", [4097, 4127])
def test_ragged_tails(engine, src3, B):
    rnd = random.Random(B)
    subsets = rnd.sample(list(itertools.combinations(range(10), 4)), 9)
    rows = _rows(rnd, subsets, [1, 31], B)
    idx, shares = _batch(src3, rows)
    _check(engine, 3, idx, shares)


def test_workspace_reuse(engine, src3):
    """two grouped calls on one context with different index sets: the key table and the counters start empty each time"""
    rnd = random.Random(77)
    outs = []
    for subsets in (list(itertools.combinations(range(10), 4))[:10], list(itertools.combinations(range(4, 14), 4))[100:116]):
        rows = _rows(rnd, subsets, [], B0)
        idx, shares = _batch(src3, rows)
        outs.append((idx, shares, _check(engine, 3, idx, shares)))
    idx, shares, first = outs[0]
    again, st = engine.combine_g2(3, idx, shares)               # and the first set once more after the second
    assert not np.asarray(st).any() and (np.asarray(again) == first).all()
