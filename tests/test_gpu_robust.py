"""GPU tests of the robust combiners (tc_combine_signatures_robust_batch / tc_decrypt_robust_batch, include/tc_amd.h): of up to
N shares per job, some absent and some forged, combine the first t+1 valid ones and name the senders of bad ones --
optimistically: the first t+1 PRESENT shares are combined and the combination checked under the master key; only a job whose
combination does not stand is examined share by share.

Key sets, shares and ciphertexts are made with the library's own (separately tested) entries from a polynomial drawn with a
seeded random.Random.  The expected signature is the master key's sign_g2 of the same hash point, the expected plaintext the
message; a handful of jobs are cross-checked against Oracle B (combine + verify).  used / bad / status / n_fallback come from a
pure-Python model of the four rules of the header, in which the validity of every share is known by construction."""
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o
from threshold_crypto_amd import api
from threshold_crypto_amd.engine import pack_messages

pytestmark = pytest.mark.gpu
OK, NOT_ENOUGH, INVALID = 0, 1, 3
IDENT2 = bytes([0x40]) + bytes(191)
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def fr_rows(vals):
    return np.stack([u8(int(v % o.R).to_bytes(32, "little")) for v in vals])


def non_member_g2(rnd):
    """an on-curve point of E'(Fq2) outside the order-r subgroup (as tests/test_gpu_wire.py makes them)"""
    while True:
        P = o.g2_get_point_from_x((rnd.randrange(o.Q), rnd.randrange(o.Q)), True)
        if P is not None and o.E2.mul(P, o.R) is not None:
            return P


def non_member_g1(rnd):
    while True:
        x = rnd.randrange(o.Q)
        y2 = (x * x * x + 4) % o.Q
        y = pow(y2, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == y2 and o.E1.mul((x, y), o.R) is not None:
            return (x, y)


def lagrange_at_zero(slots):
    """lambda_i of the abscissae x = slot + 1 (src/lib.rs:719-767)"""
    lam = {}
    for i in slots:
        num = den = 1
        for k in slots:
            if k != i:
                num = num * (k + 1) % o.R
                den = den * ((k + 1) - (i + 1)) % o.R
        lam[i] = num * pow(den, o.R - 2, o.R) % o.R
    return lam


def model(present, valid, cancels, need):
    """The four rules of include/tc_amd.h for one job: (status, used, bad, examined share by share).  valid[i]: whether slot i's
    share passes its own check; cancels: the shares of S0 are wrong in a way that cancels in the combination."""
    N = len(present)
    P = [i for i in range(N) if present[i]]
    if len(P) < need:
        return NOT_ENOUGH, [], [], False                                   # rule 1
    S0 = P[:need]
    if cancels or all(valid[i] for i in S0):
        return OK, S0, [], False                                           # rule 2: clean, no claim about individual shares
    bad = [i for i in P if not valid[i]]
    good = [i for i in P if valid[i]]
    if len(good) < need:
        return NOT_ENOUGH, [], bad, True                                   # rule 3, too few valid shares
    return OK, good[:need], bad, True                                      # rule 3


class Plan:
    """One batch: the honest share array plus planted faults, and what the model says about it."""

    def __init__(self, B, N, t, shares):
        self.B, self.N, self.t = B, N, t
        self.shares = shares.copy()
        self.honest = shares
        self.present = np.ones((B, N), dtype=np.uint8)
        self.valid = np.ones((B, N), dtype=bool)
        self.cancels = [False] * B

    def absent(self, j, slots, junk=None):
        for i in slots:
            self.present[j, i] = 0
            if junk is not None:
                self.shares[j, i] = junk

    def only(self, j, slots):
        self.present[j] = 0
        self.present[j, list(slots)] = 1

    def wrong(self, j, i, other):
        """a well-formed share of ANOTHER job in slot i"""
        self.shares[j, i] = self.honest[other, i]
        self.valid[j, i] = False

    def spoil(self, j, i, raw):
        self.shares[j, i] = raw
        self.valid[j, i] = False

    def off_curve(self, j, i):
        self.shares[j, i, -1] ^= 1                                          # y changed: not on the curve
        self.valid[j, i] = False

    def expect(self):
        return [model(self.present[j], self.valid[j], self.cancels[j], self.t + 1) for j in range(self.B)]


def plant_main_cases(plan, checked, rnd, non_member_raw, cancel_pair):
    """The cases of the issue spread over a 70-job, N = 10, t = 3 batch (jobs 0..63: first group of 64, 64..69: second)."""
    plan.absent(1, [0, 2])                                                  # holes: S0 = 1, 3, 4, 5
    plan.only(2, range(6, 10))                                              # S0 = the last t+1 slots
    plan.only(3, [1, 4, 8])                                                 # exactly t present
    plan.only(4, [])                                                        # none present
    plan.wrong(5, 1, other=20)                                              # wrong but well-formed, inside S0
    plan.wrong(6, 7, other=21)                                              # wrong, outside S0: never examined, not reported
    plan.off_curve(7, 2)                                                    # undecodable, inside S0
    if checked:
        plan.spoil(8, 0, non_member_raw)                                    # on the curve, outside the subgroup, inside S0
    plan.absent(9, [1], junk=0xFF)                                          # absent slots filled with garbage
    plan.absent(9, [3], junk=u8(bytes(rnd.randrange(256) for _ in range(plan.shares.shape[2]))))
    plan.only(10, range(6))                                                 # six present, three of them bad: too few valid
    plan.wrong(10, 0, other=22)
    plan.off_curve(10, 1)
    plan.wrong(10, 2, other=23)
    a, b = 1, 2                                                             # the cancelling pair, S0 = 0..3
    plan.shares[11, a], plan.shares[11, b] = cancel_pair(11, [0, 1, 2, 3], a, b)
    plan.valid[11, a] = plan.valid[11, b] = False
    plan.cancels[11] = True
    plan.wrong(12, 0, other=24)                                             # examined: the bad share past S0 is reported too
    plan.wrong(12, 8, other=24)
    plan.absent(12, [5], junk=0xAB)
    plan.wrong(65, 3, other=25)                                             # second group, second wave
    plan.absent(69, [0, 1, 2, 9])                                           # the last job: S0 = 3, 4, 5, 6


def as_lists(used, bad, st, B):
    return [(int(st[j]), [int(i) for i in np.nonzero(used[j])[0]], [int(i) for i in np.nonzero(bad[j])[0]]) for j in range(B)]


# ---- signatures ------------------------------------------------------------------------------------------------------------
class SigWorld:
    def __init__(self, engine, t, N, B, seed):
        rnd = random.Random(seed)
        self.rnd, self.t, self.N, self.B = rnd, t, N, B
        self.poly = [rnd.randrange(1, o.R) for _ in range(t + 1)]
        self.sk = [o.poly_evaluate(self.poly, i + 1) for i in range(N)]
        gen = u8(o.g1_uncompressed(o.G1_GEN))[None]
        self.commit = np.ascontiguousarray(engine.g1_mul(fr_rows(self.poly), gen)[0][0])             # (t+1, 96)
        self.msgs = [b"robust message %d" % j for j in range(B)]
        self.flat, self.off = pack_messages(self.msgs)
        self.hashes = engine.hash_g2(self.flat, self.off)
        self.shares = np.ascontiguousarray(engine.g2_mul(fr_rows(self.sk), self.hashes)[0])         # (B, N, 192): slot i = node i
        self.want = np.ascontiguousarray(engine.g2_mul(fr_rows(self.poly[:1]), self.hashes)[0][:, 0])  # master sign_g2
        self.engine = engine

    def cancel_pair(self, j, S0, a, b):
        """s_a + [lambda_b] D and s_b - [lambda_a] D with D = [d] H_j: the errors cancel in the combination over S0"""
        lam = lagrange_at_zero(S0)
        d = self.rnd.randrange(1, o.R)
        out = self.engine.g2_mul(fr_rows([self.sk[a] + lam[b] * d, self.sk[b] - lam[a] * d]), self.hashes[j:j + 1])[0][0]
        return out[0], out[1]

    def check(self, plan, out, used, bad, st, nfb):
        want = plan.expect()
        got = as_lists(used, bad, st, plan.B)
        for j in range(plan.B):
            assert got[j] == want[j][:3], (j, got[j], want[j])
            assert bytes(out[j]) == (bytes(self.want[j]) if want[j][0] == OK else IDENT2), j
        assert nfb == sum(1 for w in want if w[3])


@pytest.fixture(scope="module")
def world(engine):
    return SigWorld(engine, 3, 10, 70, 0x0B57)


@pytest.fixture(scope="module")
def sig_plans(world):
    """checked -> the planted main batch; made once, never modified by a test"""
    plans = {}
    for checked in (True, False):
        plan = Plan(world.B, world.N, world.t, world.shares)
        plant_main_cases(plan, checked, random.Random(77), u8(o.g2_uncompressed(non_member_g2(random.Random(78)))), world.cancel_pair)
        plans[checked] = plan
    return plans


@pytest.fixture
def unchecked(engine):
    engine.set_input_checks(False)
    yield engine
    engine.set_input_checks(True)


def test_all_clean_with_present_null(engine, world):
    out, used, bad, st, nfb = engine.combine_signatures_robust(world.commit, world.shares, hashes=world.hashes, seed=SEED_A)
    assert not st.any() and not bad.any() and nfb == 0
    assert (used[:, :4] == 1).all() and not used[:, 4:].any()
    assert (out == world.want).all()
    # the messages hashed on the device instead
    out2, used2, bad2, st2, nfb2 = engine.combine_signatures_robust(world.commit, world.shares, msgs=world.flat, off=world.off, seed=SEED_A)
    assert (out2 == out).all() and (used2 == used).all() and not bad2.any() and not st2.any() and nfb2 == 0


def test_main_cases_checked(engine, world, sig_plans):
    plan = sig_plans[True]
    res = engine.combine_signatures_robust(world.commit, plan.shares, hashes=world.hashes, present=plan.present, seed=SEED_A)
    world.check(plan, *res)
    want = plan.expect()
    assert [want[j][0] for j in (3, 4, 10)] == [NOT_ENOUGH] * 3 and want[10][2] == [0, 1, 2]        # the model itself
    assert want[6] == (OK, [0, 1, 2, 3], [], False) and want[11] == (OK, [0, 1, 2, 3], [], False)
    assert want[12] == (OK, [1, 2, 3, 4], [0, 8], True) and want[8] == (OK, [1, 2, 3, 4], [0], True)
    # a different seed: the same answer
    res_b = engine.combine_signatures_robust(world.commit, plan.shares, hashes=world.hashes, present=plan.present, seed=SEED_B)
    for x, y in zip(res[:4], res_b[:4]):
        assert (x == y).all()
    assert res[4] == res_b[4]
    # Oracle B on a handful of jobs: the shares the call says it used combine to its output, which verifies under the master key
    out, used = res[0], res[1]
    for j in (0, 1, 2, 5, 12, 65, 69):
        ids = [int(i) for i in np.nonzero(used[j])[0]]
        rc, sig = c.combine_g2(world.t, ids, [bytes(plan.shares[j, i]) for i in ids])
        assert rc == 0 and sig == bytes(out[j]), j
        assert c.verify_g2(bytes(world.commit[0]), bytes(out[j]), bytes(world.hashes[j])), j


def test_main_cases_unchecked_and_hashed_on_the_device(unchecked, world, sig_plans):
    plan = sig_plans[False]
    res = unchecked.combine_signatures_robust(world.commit, plan.shares, msgs=world.flat, off=world.off, present=plan.present, seed=SEED_B)
    world.check(plan, *res)


def test_device_io_gives_identical_bytes(engine, world, sig_plans):
    import torch
    plan = sig_plans[True]
    host = engine.combine_signatures_robust(world.commit, plan.shares, hashes=world.hashes, present=plan.present, seed=SEED_A)
    dev = [torch.from_numpy(x).cuda() for x in (world.commit, plan.shares, world.hashes, plan.present)]
    got = engine.combine_signatures_robust(dev[0], dev[1], hashes=dev[2], present=dev[3], seed=SEED_A)
    engine.sync()
    for h, d in zip(host[:4], got[:4]):
        assert (h == d.cpu().numpy()).all()
    assert host[4] == got[4]
    flat, off = torch.from_numpy(world.flat).cuda(), torch.from_numpy(world.off.view(np.int64)).cuda()
    got = engine.combine_signatures_robust(dev[0], dev[1], msgs=flat, off=off, present=dev[3], seed=SEED_A)
    engine.sync()
    for h, d in zip(host[:4], got[:4]):
        assert (h == d.cpu().numpy()).all()


def test_one_bad_job_in_the_first_group_none_in_the_second(engine, world):
    plan = Plan(world.B, world.N, world.t, world.shares)
    plan.wrong(17, 0, other=3)
    res = engine.combine_signatures_robust(world.commit, plan.shares, hashes=world.hashes, present=plan.present, group=64, seed=SEED_A)
    world.check(plan, *res)
    assert res[4] == 1 and [int(i) for i in np.nonzero(res[2])[1]] == [0]


def test_undecodable_commit_fails_every_job(engine, world, sig_plans):
    plan = sig_plans[True]
    spoiled = world.commit.copy()
    spoiled[1, -1] ^= 1                                                     # off the curve
    outsider = world.commit.copy()
    outsider[2] = u8(o.g1_uncompressed(non_member_g1(random.Random(5))))    # checked-input mode: on the curve, outside G1
    for commit in (spoiled, outsider):
        out, used, bad, st, nfb = engine.combine_signatures_robust(commit, plan.shares, hashes=world.hashes, present=plan.present, seed=SEED_A)
        assert (st == INVALID).all() and not used.any() and not bad.any() and nfb == 0
        assert all(bytes(out[j]) == IDENT2 for j in range(plan.B))


def test_long_rows_and_the_large_threshold_path(engine):
    """B = 6, N = 70, t = 21: mask rows longer than 64 bytes that start at every other offset, the two-stage combine path"""
    w = SigWorld(engine, 21, 70, 6, 0x70)
    plan = Plan(w.B, w.N, w.t, w.shares)
    holes = sorted(random.Random(1).sample(range(70), 30))
    plan.absent(1, holes)
    plan.only(2, range(48, 70))                                             # the last t+1 slots
    plan.wrong(3, 9, other=0)                                               # inside S0
    plan.off_curve(3, 40)                                                   # examined: reported although past S0
    plan.only(4, range(3, 24))                                              # exactly t present
    plan.wrong(5, 65, other=0)                                              # past S0: not reported
    res = engine.combine_signatures_robust(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A)
    w.check(plan, *res)
    assert as_lists(res[1], res[2], res[3], 6)[3] == (OK, [i for i in range(23) if i != 9], [9, 40])


def test_threshold_zero(engine):
    w = SigWorld(engine, 0, 3, 3, 0x03)
    plan = Plan(w.B, w.N, w.t, w.shares)
    plan.absent(1, [0])
    plan.wrong(2, 0, other=0)
    res = engine.combine_signatures_robust(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A)
    w.check(plan, *res)
    assert as_lists(res[1], res[2], res[3], 3) == [(OK, [0], []), (OK, [1], []), (OK, [1], [0])]


def test_argument_checks(engine, world):
    from threshold_crypto_amd.engine import TcError
    with pytest.raises(ValueError):
        engine.combine_signatures_robust(world.commit, world.shares, seed=SEED_A)                           # neither hashes nor messages
    with pytest.raises(ValueError):
        engine.combine_signatures_robust(world.commit, world.shares[:, :3].copy(), hashes=world.hashes)     # t + 1 > N
    import ctypes
    st = np.zeros(1, np.uint8)
    rc = engine._lib.tc_combine_signatures_robust_batch(engine._ctx, None, 3, 10, None, None, None, None, None, 1, 0, SEED_A, None, None, None,
                                                        ctypes.c_void_p(st.ctypes.data), None)
    assert rc == -1                                                         # NULL data pointers with a non-zero size
    assert engine._lib.tc_combine_signatures_robust_batch(engine._ctx, None, 3, 10, None, None, None, None, None, 0, 0, None, None, None, None,
                                                          None, None) == 0  # an empty batch is a no-op
    assert TcError is not None


def test_api_combine_signatures_robust_batch(engine, world, sig_plans):
    plan = sig_plans[True]
    pk_set = api.PublicKeySet([bytes(x) for x in world.commit], _trusted=True)
    picks = [0, 1, 3, 5, 10, 12]
    jobs = [{i: bytes(plan.shares[j, i]) for i in range(world.N) if plan.present[j, i]} for j in picks]
    res = pk_set.combine_signatures_robust_batch(jobs, [world.msgs[j] for j in picks], n_nodes=world.N, engine=engine, seed=SEED_A)
    want = plan.expect()
    for (val, used, bad), j in zip(res, picks):
        assert (used, bad) == (want[j][1], want[j][2]), j
        if want[j][0] == OK:
            assert isinstance(val, api.Signature) and val.raw == bytes(world.want[j]), j
        else:
            assert isinstance(val, api.NotEnoughShares), j


# ---- decryption ------------------------------------------------------------------------------------------------------------
class EncWorld:
    def __init__(self, engine, t, N, B, seed, poly=None):
        rnd = random.Random(seed)
        self.rnd, self.t, self.N, self.B, self.engine = rnd, t, N, B, engine
        self.poly = list(poly) if poly is not None else [rnd.randrange(1, o.R) for _ in range(t + 1)]
        self.sk = [o.poly_evaluate(self.poly, i + 1) for i in range(N)]
        gen = u8(o.g1_uncompressed(o.G1_GEN))[None]
        self.commit = np.ascontiguousarray(engine.g1_mul(fr_rows(self.poly), gen)[0][0])
        self.plain = [bytes(rnd.randrange(256) for _ in range((0, 1, 33)[j % 3])) for j in range(B)]     # lengths 0, 1 and 33
        flat, self.off = pack_messages(self.plain)
        r = fr_rows([rnd.randrange(1, o.R) for _ in range(B)])
        self.u, self.v, self.w, st = engine.encrypt(self.commit[0].copy(), r, flat, self.off)
        assert not st.any()
        self.shares = np.ascontiguousarray(engine.g1_mul(fr_rows(self.sk), self.u)[0])                # (B, N, 96)

    def cancel_pair(self, j, S0, a, b):
        lam = lagrange_at_zero(S0)
        d = self.rnd.randrange(1, o.R)
        out = self.engine.g1_mul(fr_rows([self.sk[a] + lam[b] * d, self.sk[b] - lam[a] * d]), self.u[j:j + 1])[0][0]
        return out[0], out[1]

    def check(self, plan, want, out, used, bad, st, nfb):
        got = as_lists(used, bad, st, plan.B)
        for j in range(plan.B):
            assert got[j] == want[j][:3], (j, got[j], want[j])
            lo, hi = int(self.off[j]), int(self.off[j + 1])
            assert bytes(out[lo:hi]) == (self.plain[j] if want[j][0] == OK else bytes(hi - lo)), j
        assert nfb == sum(1 for w in want if w[3])


@pytest.fixture(scope="module")
def enc_world(engine):
    return EncWorld(engine, 3, 10, 70, 0xDEC)


@pytest.mark.parametrize("checked", [True, False])
def test_decrypt_main_cases(engine, enc_world, checked):
    w = enc_world
    plan = Plan(w.B, w.N, w.t, w.shares)
    plant_main_cases(plan, checked, random.Random(79), u8(o.g1_uncompressed(non_member_g1(random.Random(80)))), w.cancel_pair)
    # an invalid ciphertext (job 30: the w of another one): every honest share fails its check
    ww = w.w.copy()
    ww[30] = w.w[31]
    plan.absent(30, [4])
    want = plan.expect()
    want[30] = (NOT_ENOUGH, [], [i for i in range(w.N) if i != 4], True)
    engine.set_input_checks(checked)
    try:
        res = engine.decrypt_robust(w.commit, plan.shares, w.u, w.v, w.off, ww, present=plan.present)
        w.check(plan, want, *res)
        if checked:
            import torch
            dev = [torch.from_numpy(x).cuda() for x in (w.commit, plan.shares, w.u, w.v, w.off.view(np.int64), ww, plan.present)]
            got = engine.decrypt_robust(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], present=dev[6])
            engine.sync()
            for h, d in zip(res[:4], got[:4]):
                assert (h == d.cpu().numpy()).all()
            assert res[4] == got[4]
            # Oracle B on two jobs: the shares used decrypt the ciphertext
            for j in (1, 5):
                ids = [int(i) for i in np.nonzero(res[1][j])[0]]
                rc, plain = c.threshold_decrypt(w.t, ids, [bytes(plan.shares[j, i]) for i in ids], bytes(w.v[int(w.off[j]):int(w.off[j + 1])]))
                assert rc == 0 and plain == w.plain[j], j
    finally:
        engine.set_input_checks(True)


def test_decrypt_all_clean_present_null_and_api(engine, enc_world):
    w = enc_world
    out, used, bad, st, nfb = engine.decrypt_robust(w.commit, w.shares, w.u, w.v, w.off, w.w)
    assert not st.any() and not bad.any() and nfb == 0 and (used[:, :4] == 1).all() and not used[:, 4:].any()
    assert all(bytes(out[int(w.off[j]):int(w.off[j + 1])]) == w.plain[j] for j in range(w.B))
    pk_set = api.PublicKeySet([bytes(x) for x in w.commit], _trusted=True)
    cts = [api.Ciphertext(bytes(w.u[j]), bytes(w.v[int(w.off[j]):int(w.off[j + 1])]), bytes(w.w[j]), _trusted=True) for j in (1, 2)]
    jobs = [{i: bytes(w.shares[1, i]) for i in (2, 3, 5, 7, 9)}, {i: bytes(w.shares[2 if i != 4 else 3, i]) for i in range(3, 9)}]
    res = pk_set.decrypt_robust_batch(jobs, cts, n_nodes=w.N, engine=engine)
    assert res[0] == (w.plain[1], [2, 3, 5, 7], []) and res[1] == (w.plain[2], [3, 5, 6, 7], [4])
