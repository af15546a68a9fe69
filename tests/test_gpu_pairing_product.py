"""The n-pair product check (tc_pairing_product_check_batch: k_miller_pairs + k_fq12_product + k_final_exp) and Ciphertext::verify
by random linear combination (tc_ciphertext_verify_rlc_batch) on a real MI355X.

Expected values of the product check are built BY CONSTRUCTION: pairs (a_k g1, b_k g2) made with engine.g1_mul / g2_mul, whose
product of pairings is e(g1, g2)^(sum a_k b_k) -- 1 iff the sum is 0 mod r.  The truth of the ciphertext entry is the per-job
entry (engine.ciphertext_verify) on the same arrays, anchored at a few ciphertexts in the Python oracle."""
import random

import numpy as np
import pytest

import tc_oracle as o

pytestmark = pytest.mark.gpu


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


G1_GEN = u8(o.g1_uncompressed(o.G1_GEN))
G2_GEN = u8(o.g2_uncompressed(o.G2_GEN))
G1_INF = np.zeros(96, np.uint8)
G1_INF[0] = 0x40
G2_INF = np.zeros(192, np.uint8)
G2_INF[0] = 0x40


def _fr(xs):
    return np.stack([u8(o.fr_to_bytes(int(x) % o.R)) for x in xs])


def g1_points(engine, scalars):
    out, st = engine.g1_mul(_fr(scalars), G1_GEN[None].copy())
    assert not st.any()
    return np.ascontiguousarray(out[0])


def g2_points(engine, scalars):
    out, st = engine.g2_mul(_fr(scalars), G2_GEN[None].copy())
    assert not st.any()
    return np.ascontiguousarray(out[0])


def point_outside_g1(rnd):
    """a point of E(Fq) whose order is not r (as tests/test_gpu_fullsize.py builds it)"""
    while True:
        x = rnd.randrange(o.Q)
        y = pow((x * x * x + 4) % o.Q, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == (x * x * x + 4) % o.Q and o.E1.mul((x, y), o.R) is not None:
            return u8(o.g1_uncompressed((x, y)))


NS = (1, 2, 3, 5, 33, 64, 65, 130)
BS = (1, 7, 70)
POOL = max(NS) * max(BS)


@pytest.fixture(scope="module")
def pool(engine):
    """POOL random scalar pairs and their points, computed once: every shape takes its first n * B pairs and only replaces the
    last G2 point of each job (the one that closes the exponent sum) and the one point of an off-by-one job."""
    rnd = random.Random(20260117)
    a = [rnd.randrange(1, o.R) for _ in range(POOL)]
    b = [rnd.randrange(1, o.R) for _ in range(POOL)]
    return {"a": a, "b": b, "A": g1_points(engine, a), "B": g2_points(engine, b)}


def build_batch(engine, pool, n, B, shift=0):
    """(a points (B * n, 96), b points (B * n, 192), truth (B,)): job j is of kind (j + shift) % 3 --
    0: sum a_k b_k = 0;  1: the same with ONE scalar (a_k of a pair chosen per job; b_k where that pair's b_k is 0, which is the
    one pair of n = 1) off by one;  2: only the LAST pair wrong."""
    a, b = pool["a"], pool["b"]
    A = pool["A"][: n * B].copy()
    Bp = pool["B"][: n * B].copy()
    truth = np.zeros(B, np.uint8)
    last, bumped, where = [], [], []
    for j in range(B):
        lo, kind = j * n, (j + shift) % 3
        s = sum(a[lo + k] * b[lo + k] for k in range(n - 1)) % o.R
        closing = (-s * pow(a[lo + n - 1], o.R - 2, o.R)) % o.R      # a_{n-1} * closing = -s; n = 1: closing = 0, the identity
        if kind == 2:
            closing = (closing + 1) % o.R
        k = (7 * j + 3) % n
        if kind == 1 and k == n - 1 and closing == 0:
            closing = 1      # (n = 1: a_k meets the identity, whatever its value -- the scalar that is off by one is b_k)
        elif kind == 1:
            bumped.append(a[lo + k] + 1)
            where.append(lo + k)
        last.append(closing)
        truth[j] = 1 if kind == 0 else 0
    Bp[np.arange(B) * n + n - 1] = g2_points(engine, last)
    if where:
        A[where] = g1_points(engine, bumped)
    return np.ascontiguousarray(A), np.ascontiguousarray(Bp), truth


@pytest.mark.parametrize("n", NS)
def test_product_check_shapes(engine, pool, n):
    """n in {1, 2, 3, 5, 33, 64, 65, 130} x B in {1, 7, 70}: an odd last pair, exactly one wave of lane pairs per job (64 pairs), one
    wave plus one pair, a job that spans three waves, a partial last block; true jobs, jobs off by one in a single scalar and
    jobs where only the last pair is wrong, mixed in every batch (a batch of ONE job takes a different kind per shape)."""
    for bi, B in enumerate(BS):
        for shift in ((0, 1, 2) if B == 1 else (NS.index(n) + bi,)):
            a, b, truth = build_batch(engine, pool, n, B, shift)
            ok = engine.pairing_product_check(a, b, n)
            assert ok.shape == (B,) and (ok == truth).all(), (n, B, shift, ok.tolist(), truth.tolist())


def test_product_check_edge_operands(engine, pool):
    rnd = random.Random(5)
    n, B = 5, 7
    a, b, truth = build_batch(engine, pool, n, B, shift=0)
    a, b = a.reshape(B, n, 96), b.reshape(B, n, 192)
    flat = lambda x: np.ascontiguousarray(x.reshape(B * n, x.shape[-1]))
    # an identity operand in the middle of a true job: the four other pairs must close the sum among themselves
    for j, g2_side in ((0, False), (3, True)):
        assert truth[j] == 1
        sc_a = [rnd.randrange(1, o.R) for _ in range(n)]
        sc_b = [rnd.randrange(1, o.R) for _ in range(n)]
        s = sum(sc_a[k] * sc_b[k] for k in (0, 1, 3)) % o.R
        sc_b[4] = (-s * pow(sc_a[4], o.R - 2, o.R)) % o.R
        a[j], b[j] = g1_points(engine, sc_a), g2_points(engine, sc_b)
        if g2_side:
            b[j, 2] = G2_INF
        else:
            a[j, 2] = G1_INF
    # an all-identity job (kind 1 before: false -> true)
    assert truth[1] == 0
    a[1], b[1] = G1_INF, G2_INF
    want = truth.copy()
    want[1] = 1
    ok = engine.pairing_product_check(flat(a), flat(b), n)
    assert (ok == want).all(), (ok.tolist(), want.tolist())
    # an undecodable byte fails its own job only
    for arr, j, k in ((a, 6, 4), (b, 3, 0)):
        saved = arr[j, k].copy()
        arr[j, k, 9] ^= 0x55
        bad = want.copy()
        bad[j] = 0
        ok = engine.pairing_product_check(flat(a), flat(b), n)
        assert (ok == bad).all(), (j, k, ok.tolist())
        arr[j, k] = saved
    # an on-curve point outside G1 (checked-input mode is the context's default): its job fails, the others keep their result
    assert engine.input_checks()
    saved = a[0, 1].copy()
    a[0, 1] = point_outside_g1(rnd)
    bad = want.copy()
    bad[0] = 0
    ok = engine.pairing_product_check(flat(a), flat(b), n)
    assert (ok == bad).all(), ok.tolist()
    a[0, 1] = saved


def test_product_check_of_two_pairs_agrees_with_pairing_check(engine, pool):
    """prod of (a, b), (c, d) == 1  <=>  e(a, b) == e(-c, d): 70 mixed jobs against engine.pairing_check, c negated on the host"""
    n, B = 2, 70
    a, b, truth = build_batch(engine, pool, n, B, shift=1)
    assert 0 < truth.sum() < B
    pa, pb = a.reshape(B, 2, 96), b.reshape(B, 2, 192)
    neg_c = np.stack([u8(o.g1_uncompressed(o.E1.neg(o.g1_from_uncompressed(bytes(pa[j, 1]))))) for j in range(B)])
    want = engine.pairing_check(np.ascontiguousarray(pa[:, 0]), np.ascontiguousarray(pb[:, 0]), neg_c, np.ascontiguousarray(pb[:, 1]))
    assert (want == truth).all()
    assert (engine.pairing_product_check(a, b, n) == want).all()


def test_product_check_device_io_equals_host_io(engine, pool):
    import torch
    n, B = 65, 7
    a, b, truth = build_batch(engine, pool, n, B, shift=2)
    host = engine.pairing_product_check(a, b, n)
    dev = engine.pairing_product_check(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), n)
    engine.sync()
    assert bytes(dev.cpu().numpy()) == bytes(host) and (host == truth).all()


# ---- Ciphertext::verify by random linear combination ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc(engine):
    from threshold_crypto_amd.workload import ThresholdEncWorkload
    return ThresholdEncWorkload(engine, 3, 10, 300)


def _g2_add(p192, D, sign):
    P = o.g2_from_uncompressed(bytes(p192))
    return u8(o.g2_uncompressed(o.E2.add(P, D if sign > 0 else o.E2.neg(D))))


def _fallback(faults, group, B):
    return sum(min(group, B - g * group) for g in {j // group for j in faults})


def test_ciphertext_rlc_equals_per_job_entry(engine, enc):
    """B = 300, group = 64: four full groups and a tail of 44, one planted fault per group -- a swapped w, a flipped byte of v, an
    undecodable u, an on-curve u outside G1 and a CANCELLING pair (w[a] += D, w[b] -= D inside one group: it passes any
    combination with equal scalars, so it tests the randomisation itself).  ok[] must equal the per-job entry's, and n_fallback
    the summed sizes of exactly the groups that hold a fault: a run that fell back everywhere would also give the right ok[]."""
    B, group = enc.B, 64
    rnd = random.Random(77)
    u, v, w = enc.u.copy(), enc.v.copy(), enc.w.copy()
    D = o.E2.mul(o.G2_GEN, 0xD1FF)
    w[10] = enc.w[11]                                  # group 0
    v[int(enc.off[70]) + 3] ^= 0x01                    # group 1
    u[130, 7] ^= 0x55                                  # group 2: undecodable
    u[200] = point_outside_g1(rnd)                     # group 3
    w[260], w[270] = _g2_add(enc.w[260], D, +1), _g2_add(enc.w[270], D, -1)   # the tail group
    faults = [10, 70, 130, 200, 260, 270]
    truth = engine.ciphertext_verify(u, v, enc.off, w)
    assert truth.sum() == B - len(faults) and not truth[faults].any()
    # the truth anchored outside the library: 8 ciphertexts, valid and invalid, in the Python oracle
    for j in (0, 11, 71, 299, 10, 70, 260, 270):
        ct = (o.g1_from_uncompressed(bytes(u[j])), bytes(v[int(enc.off[j]): int(enc.off[j + 1])]), o.g2_from_uncompressed(bytes(w[j])))
        assert o.ciphertext_verify(ct) == bool(truth[j]), j
    ok, nfb = engine.ciphertext_verify_rlc(u, v, enc.off, w, group=group, seed=bytes(range(32)))
    assert (ok == truth).all(), np.flatnonzero(ok != truth).tolist()
    assert nfb == _fallback(faults, group, B) == B
    # fewer faults: only their groups fall back (the cancelling pair alone, then with the swapped w)
    w2 = enc.w.copy()
    w2[260], w2[270] = w[260], w[270]
    for extra, hit in (((), [260, 270]), ((10,), [10, 260, 270])):
        for j in extra:
            w2[j] = w[j]
        want = engine.ciphertext_verify(enc.u, enc.v, enc.off, w2)
        assert not want[hit].any() and want.sum() == B - len(hit)
        ok, nfb = engine.ciphertext_verify_rlc(enc.u, enc.v, enc.off, w2, group=group, seed=bytes(range(1, 33)))
        assert (ok == want).all() and nfb == _fallback(hit, group, B), (hit, nfb)
    # the untouched batch: every group passes on the fast path, whatever the seed
    for seed in (bytes(range(32)), bytes(range(100, 132))):
        ok, nfb = engine.ciphertext_verify_rlc(enc.u, enc.v, enc.off, enc.w, group=group, seed=seed)
        assert ok.all() and nfb == 0, (nfb, np.flatnonzero(ok == 0).tolist())


def _head(enc, B):
    return (np.ascontiguousarray(enc.u[:B]), np.ascontiguousarray(enc.v[: int(enc.off[B])]), np.ascontiguousarray(enc.off[: B + 1]),
            np.ascontiguousarray(enc.w[:B]))


@pytest.mark.parametrize("B,group,fault", [(70, 1, 5), (70, 2, 5), (70, 3, 68), (70, 0, 5), (70, 64, 66), (70, 1024, 5), (65, 64, 64), (65, 64, 5),
                                           (1, 0, 0), (1, 64, 0)])
def test_ciphertext_rlc_group_shapes(engine, enc, B, group, fault):
    """group in {1, 2, 3, 0 (the default, 64), 64, 1024 > B}, a tail of one (B = 65, group = 64) and B = 1: all valid, then with one
    planted fault -- the per-job result and the exact number of ciphertexts that fell back"""
    u, v, off, w = _head(enc, B)
    ok, nfb = engine.ciphertext_verify_rlc(u, v, off, w, group=group, seed=bytes(range(32)))
    assert ok.all() and nfb == 0
    bad = w.copy()
    bad[fault] = enc.w[fault + 1]
    want = engine.ciphertext_verify(u, v, off, bad)
    assert want.sum() == B - 1 and not want[fault]
    ok, nfb = engine.ciphertext_verify_rlc(u, v, off, bad, group=group, seed=bytes(range(32)))
    eff = min(group if group else 64, 1024, B)
    assert (ok == want).all() and nfb == _fallback([fault], eff, B), (nfb, eff)


def test_ciphertext_rlc_without_input_checks(engine, enc):
    """after the explicit opt-out (tc_ctx_set_input_checks(ctx, 0)), members only: the same comparison with and without a wrong w"""
    u, v, off, w = _head(enc, 150)
    bad = w.copy()
    bad[100] = w[3]
    engine.set_input_checks(False)
    try:
        ok, nfb = engine.ciphertext_verify_rlc(u, v, off, w, group=64, seed=bytes(range(32)))
        assert ok.all() and nfb == 0
        want = engine.ciphertext_verify(u, v, off, bad)
        assert want.sum() == 149 and not want[100]
        ok, nfb = engine.ciphertext_verify_rlc(u, v, off, bad, group=64, seed=bytes(range(32)))
        assert (ok == want).all() and nfb == 64
    finally:
        engine.set_input_checks(True)


def test_ciphertext_verify_batch_rlc_switch(engine, enc):
    """api.Ciphertext.verify_batch(rlc=True) equals rlc=False on 40 ciphertexts with two bad ones"""
    from threshold_crypto_amd import api
    cts = [api.Ciphertext(enc.u[j], enc.v[int(enc.off[j]): int(enc.off[j + 1])], enc.w[j], _trusted=True) for j in range(40)]
    cts[7] = api.Ciphertext(enc.u[7], enc.v[int(enc.off[7]): int(enc.off[8])], enc.w[8], _trusted=True)
    v = bytearray(cts[31].v)
    v[0] ^= 0x80
    cts[31] = api.Ciphertext(cts[31].u, bytes(v), cts[31].w, _trusted=True)
    plain = api.Ciphertext.verify_batch(cts, engine=engine)
    assert plain.sum() == 38 and not plain[7] and not plain[31]
    assert (api.Ciphertext.verify_batch(cts, engine=engine, rlc=True, seed=bytes(range(32))) == plain).all()
    assert (api.Ciphertext.verify_batch(cts, engine=engine, rlc=True) == plain).all()
