"""GPU tests of blame by bisection (tc_ctx_set_blame_bisect, include/tc_amd.h): pass 2 of the four robust combiners finds the
bad shares of a failed job with range checks over shares multiplied by secret scalars instead of one pairing check per share.

Every case runs the SAME inputs with the mode off and on and asserts
  * out / used / bad / status / n_fallback byte-identical between the modes and equal to the model of the four rules
    (tests/test_gpu_robust.py, in which the validity of every share is known by construction);
  * tc_ctx_last_blame_stats equal to the Python model of the bisection rule (tests/test_blame_host.py `model`, written from the
    rule of csrc/tc_blame.h) fed with that validity: checks summed over the examined jobs, rounds = the longest search of a chunk;
  * mode off: F * N checks and one round for F examined jobs.
Shapes: t = 3, N = 10, B = 70 (the planted cases of plant_main_cases); t = 2, N = 13, B = 6 (not a power of two: bad at slot 0,
at slot 12, two adjacent, junk in an absent slot, every present share bad, an invalid hash point / ciphertext); t = 2, N = 70,
B = 3 (a range longer than a wave; bad slots {0}, {69}, {31, 32} across the 32-point boundary of the lane-pair layout)."""
import random

import numpy as np
import pytest

import tc_oracle as o
from test_blame_host import model as blame_model
from test_gpu_robust import (EncWorld, IDENT2, NOT_ENOUGH, OK, SEED_A, Plan, SigWorld, as_lists, non_member_g1, non_member_g2, plant_main_cases, u8)
from test_gpu_robust_wire import IDENT_W, WirePlan, WireSig, no_square_root

pytestmark = pytest.mark.gpu
KEY = bytes(range(200, 232))


class _Tracks:
    """a Plan that also knows which bad shares are bad WITHOUT a check: the ones that do not decode and the non-members (planted
    only where membership is tested)"""

    def __init__(self, *a):
        super().__init__(*a)
        self.nonlive = np.zeros((self.B, self.N), dtype=bool)
        self.jvalid = [True] * self.B

    def off_curve(self, j, i):
        super().off_curve(j, i)
        self.nonlive[j, i] = True

    def spoil(self, j, i, raw):
        super().spoil(j, i, raw)
        self.nonlive[j, i] = True

    def invalid_operands(self, j):
        """the job's own hash point / ciphertext is invalid: every present share is bad, none is checked"""
        self.jvalid[j] = False
        self.valid[j] = False


class BPlan(_Tracks, Plan):
    pass


class BWirePlan(_Tracks, WirePlan):
    pass


def expected_stats(plan, want, chunk=None):
    """(checks, rounds) of the bisection over the examined jobs, in chunks of `chunk` jobs (None: one chunk)"""
    per_job = []
    for j in range(plan.B):
        if not want[j][3]:
            continue
        live = [bool(plan.present[j, i]) and not plan.nonlive[j, i] and plan.jvalid[j] for i in range(plan.N)]
        bad = [not plan.valid[j, i] for i in range(plan.N)]
        found, checks, rounds = blame_model(plan.N, live, bad)
        assert sorted(found) == [i for i in range(plan.N) if live[i] and bad[i]]
        per_job.append((checks, rounds))
    chunk = chunk or max(1, len(per_job))
    rounds = sum(max(r for _, r in per_job[k:k + chunk]) for k in range(0, len(per_job), chunk))
    return sum(c for c, _ in per_job), rounds, per_job


def both_modes(eng, call, plan, want, chunk=None):
    """runs `call` with the mode off, on, and on again; returns the results of the first bisection run"""
    assert not eng.blame_bisect()
    off = call()
    off = [np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in off]
    F = sum(1 for w in want if w[3])
    assert off[4] == F and eng.last_blame_stats() == ((F * plan.N, 1) if F else (0, 0))
    eng.set_blame_bisect(KEY)
    try:
        assert eng.blame_bisect()
        on = call()
        stats = eng.last_blame_stats()
        again = call()
        assert eng.last_blame_stats() == stats
    finally:
        eng.set_blame_bisect(None)
    assert not eng.blame_bisect()
    on = [np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in on]
    again = [np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in again]
    for a, b, c in zip(off[:4], on[:4], again[:4]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert off[4] == on[4] == again[4]
    checks, rounds, per_job = expected_stats(plan, want, chunk)
    print("blame stats: per-share %d checks, bisection %s, model %s" % (F * plan.N, stats, (checks, rounds)))
    assert stats == (checks, rounds)
    d = (plan.N - 1).bit_length()
    assert all(c <= 2 * plan.N - 1 and r <= 2 * d + 1 for c, r in per_job)
    return on, per_job


def check_sig(world, plan, want, res, ident=IDENT2, want_out=None):
    out, used, bad, st, nfb = res
    want_out = world.want if want_out is None else want_out
    got = as_lists(used, bad, st, plan.B)
    for j in range(plan.B):
        assert got[j] == want[j][:3], (j, got[j], want[j])
        assert bytes(out[j]) == (bytes(want_out[j]) if want[j][0] == OK else ident), j
    assert nfb == sum(1 for w in want if w[3])


# ---- t = 3, N = 10, B = 70: the planted main cases -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(engine):
    return SigWorld(engine, 3, 10, 70, 0x0B57)


@pytest.mark.parametrize("checked", [True, False])
def test_signatures_main_cases(engine, world, checked):
    plan = BPlan(world.B, world.N, world.t, world.shares)
    plant_main_cases(plan, checked, random.Random(77), u8(o.g2_uncompressed(non_member_g2(random.Random(78)))), world.cancel_pair)
    want = plan.expect()
    engine.set_input_checks(checked)
    try:
        if checked:
            call = lambda: engine.combine_signatures_robust(world.commit, plan.shares, hashes=world.hashes, present=plan.present, seed=SEED_A)
        else:                                                                 # the messages hashed on the device
            call = lambda: engine.combine_signatures_robust(world.commit, plan.shares, msgs=world.flat, off=world.off, present=plan.present, seed=SEED_A)
        on, _ = both_modes(engine, call, plan, want)
        check_sig(world, plan, want, on)
    finally:
        engine.set_input_checks(True)


def test_signatures_device_io(engine, world):
    import torch
    plan = BPlan(world.B, world.N, world.t, world.shares)
    plant_main_cases(plan, True, random.Random(77), u8(o.g2_uncompressed(non_member_g2(random.Random(78)))), world.cancel_pair)
    want = plan.expect()
    dev = [torch.from_numpy(x).cuda() for x in (world.commit, plan.shares, world.hashes, plan.present)]

    def call():
        res = engine.combine_signatures_robust(dev[0], dev[1], hashes=dev[2], present=dev[3], seed=SEED_A)
        engine.sync()
        return res
    on, _ = both_modes(engine, call, plan, want)
    check_sig(world, plan, want, on)


def test_no_job_reaches_pass_two(engine, world):
    engine.set_blame_bisect(KEY)
    try:
        out, used, bad, st, nfb = engine.combine_signatures_robust(world.commit, world.shares, hashes=world.hashes, seed=SEED_A)
        assert nfb == 0 and not bad.any() and not st.any() and (out == world.want).all()
        assert engine.last_blame_stats() == (0, 0)
    finally:
        engine.set_blame_bisect(None)


@pytest.mark.parametrize("checked", [True, False])
def test_decryption_main_cases(engine, checked):
    w = EncWorld(engine, 3, 10, 70, 0xDEC)
    plan = BPlan(w.B, w.N, w.t, w.shares)
    plant_main_cases(plan, checked, random.Random(79), u8(o.g1_uncompressed(non_member_g1(random.Random(80)))), w.cancel_pair)
    # the w of another ciphertext: decodable, a member, and every honest share fails its check -- 2 k - 1 checks for k = 9 live shares
    ww = w.w.copy()
    ww[30] = w.w[31]
    plan.absent(30, [4])
    plan.valid[30] = False
    # a ciphertext whose u is off the curve: the job's operands are invalid, zero checks
    uu = w.u.copy()
    uu[40, -1] ^= 1
    plan.invalid_operands(40)
    want = plan.expect()
    assert want[30] == (NOT_ENOUGH, [], [i for i in range(w.N) if i != 4], True) and want[40] == (NOT_ENOUGH, [], list(range(w.N)), True)
    engine.set_input_checks(checked)
    try:
        on, _ = both_modes(engine, lambda: engine.decrypt_robust(w.commit, plan.shares, uu, w.v, w.off, ww, present=plan.present), plan, want)
        w.check(plan, want, *on)
    finally:
        engine.set_input_checks(True)


# ---- t = 2, N = 13, B = 6: not a power of two ---------------------------------------------------------------------------------------
def plant_n13(plan):
    plan.wrong(0, 0, other=1)                                               # bad at slot 0
    plan.only(1, [2, 9, 12])                                                # bad at slot 12 (the last slot, inside S0)
    plan.wrong(1, 12, other=0)
    plan.only(2, range(5, 13))                                              # two adjacent bad slots
    plan.wrong(2, 5, other=0)
    plan.wrong(2, 6, other=0)
    plan.wrong(3, 1, other=0)                                               # junk in an absent slot of an examined job
    plan.absent(3, [4], junk=0xFF)
    for i in range(13):                                                     # every present share bad
        plan.wrong(4, i, other=3)
    plan.absent(4, [7])
    plan.invalid_operands(5)                                                # an invalid hash point / ciphertext


def test_signatures_n13_checked(engine):
    w = SigWorld(engine, 2, 13, 6, 0x13)
    plan = BPlan(w.B, w.N, w.t, w.shares)
    plant_n13(plan)
    hashes = w.hashes.copy()
    hashes[5] = u8(o.g2_uncompressed(non_member_g2(random.Random(513))))   # checked-input mode: the hash point is no group member
    want = plan.expect()
    assert want[5] == (NOT_ENOUGH, [], list(range(13)), True) and want[4][0] == NOT_ENOUGH and want[2] == (OK, [7, 8, 9], [5, 6], True)
    on, per_job = both_modes(engine, lambda: engine.combine_signatures_robust(w.commit, plan.shares, hashes=hashes, present=plan.present, seed=SEED_A),
                             plan, want)
    check_sig(w, plan, want, on)
    assert per_job[5] == (0, 0) and per_job[4][0] == 2 * 12 - 1             # invalid operands: no check; all 12 bad: the worst case


def test_signatures_n13_two_chunks():
    """six examined jobs through a leaf buffer that holds three: the budget of the two-stage tables (TC_MSM_BUDGET), which
    prices the leaves, forces two chunks -- the rounds of the two searches add up"""
    from conftest import engine_with_env
    with engine_with_env(TC_MSM_BUDGET=3 * 13 * 576) as eng:
        w = SigWorld(eng, 2, 13, 6, 0x13)
        plan = BPlan(w.B, w.N, w.t, w.shares)
        plant_n13(plan)
        hashes = w.hashes.copy()
        hashes[5] = u8(o.g2_uncompressed(non_member_g2(random.Random(513))))
        want = plan.expect()
        assert sum(1 for x in want if x[3]) == 6
        on, _ = both_modes(eng, lambda: eng.combine_signatures_robust(w.commit, plan.shares, hashes=hashes, present=plan.present, seed=SEED_A),
                           plan, want, chunk=3)
        check_sig(w, plan, want, on)


def test_decryption_n13_unchecked(engine):
    w = EncWorld(engine, 2, 13, 6, 0x1313)
    plan = BPlan(w.B, w.N, w.t, w.shares)
    plant_n13(plan)
    uu = w.u.copy()
    uu[5, -1] ^= 1                                                          # u off the curve
    want = plan.expect()
    engine.set_input_checks(False)
    try:
        on, _ = both_modes(engine, lambda: engine.decrypt_robust(w.commit, plan.shares, uu, w.v, w.off, w.w, present=plan.present), plan, want)
        w.check(plan, want, *on)
    finally:
        engine.set_input_checks(True)


# ---- t = 2, N = 70, B = 3: a range longer than a wave ---------------------------------------------------------------------------
def test_signatures_n70(engine):
    w = SigWorld(engine, 2, 70, 3, 0x70B)
    plan = BPlan(w.B, w.N, w.t, w.shares)
    plan.wrong(0, 0, other=1)                                               # {0}
    plan.only(1, [3, 36, 69])                                               # {69}: the last slot, inside S0
    plan.wrong(1, 69, other=0)
    plan.only(2, range(30, 70))                                             # {31, 32}: across the 32-point boundary
    plan.wrong(2, 31, other=0)
    plan.wrong(2, 32, other=0)
    want = plan.expect()
    assert want[0] == (OK, [1, 2, 3], [0], True) and want[1] == (NOT_ENOUGH, [], [69], True) and want[2] == (OK, [30, 33, 34], [31, 32], True)
    on, per_job = both_modes(engine, lambda: engine.combine_signatures_robust(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A),
                             plan, want)
    check_sig(w, plan, want, on)
    assert per_job[0][0] <= 15 and per_job[1][0] <= 15                      # one bad share among 70: at most 1 + 2 * 7 (per share: 70)


# ---- the wire entries ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wire_world(engine):
    return WireSig(engine, 3, 10, 70, 0x0B57)


def test_wire_signatures_main_cases(engine, wire_world):
    ww, w = wire_world, wire_world.w
    plan = BWirePlan(ww.B, ww.N, ww.t, ww.shares, ww.no_root)
    plant_main_cases(plan, True, random.Random(77), u8(o.g2_compressed(non_member_g2(random.Random(78)))), ww.cancel_pair)
    want = plan.expect()
    on, _ = both_modes(engine, lambda: engine.combine_signatures_robust_wire(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A),
                       plan, want)
    check_sig(ww, plan, want, on, ident=IDENT_W)


def test_wire_an_undecodable_and_a_non_member_share_cost_one_check_each(engine, wire_world):
    """the only fault of job 3 is a share that does not decode, of job 9 one outside the subgroup: both are bad without a check and
    the root range passes -- exactly one check per job"""
    ww, w = wire_world, wire_world.w
    plan = BWirePlan(ww.B, ww.N, ww.t, ww.shares, ww.no_root)
    plan.off_curve(3, 1)
    plan.spoil(9, 2, u8(o.g2_compressed(non_member_g2(random.Random(99)))))
    want = plan.expect()
    assert want[3] == (OK, [0, 2, 3, 4], [1], True) and want[9] == (OK, [0, 1, 3, 4], [2], True)
    engine.set_input_checks(False)                                          # (wire shares are checked whatever the switch says)
    try:
        on, per_job = both_modes(engine, lambda: engine.combine_signatures_robust_wire(w.commit, plan.shares, hashes=w.hashes, present=plan.present,
                                                                                        seed=SEED_A), plan, want)
    finally:
        engine.set_input_checks(True)
    check_sig(ww, plan, want, on, ident=IDENT_W)
    assert per_job == [(1, 1), (1, 1)]


def test_wire_decryption_n13(engine):
    w = EncWorld(engine, 2, 13, 6, 0x1314)
    comp, st = engine.g1_compress(w.shares.reshape(-1, 96))
    assert not st.any()
    plan = BWirePlan(w.B, w.N, w.t, np.ascontiguousarray(comp.reshape(w.B, w.N, 48)), no_square_root(False, random.Random(5)))
    plant_n13(plan)
    plan.off_curve(0, 7)                                                    # past S0, found bad without a check once the job is examined
    plan.spoil(3, 9, u8(o.g1_compressed(non_member_g1(random.Random(6)))))
    uu = w.u.copy()
    uu[5, -1] ^= 1
    want = plan.expect()
    on, _ = both_modes(engine, lambda: engine.decrypt_robust_wire(w.commit, plan.shares, uu, w.v, w.off, w.w, present=plan.present), plan, want)
    w.check(plan, want, *on)


def test_setter_getter_and_argument_checks(engine):
    assert not engine.blame_bisect()
    with pytest.raises(ValueError):
        engine.set_blame_bisect(b"short")
    engine.set_blame_bisect(KEY)
    assert engine.blame_bisect()
    engine.set_blame_bisect(None)
    assert not engine.blame_bisect()
    lib = engine._lib
    assert lib.tc_ctx_set_blame_bisect(None, KEY) == -1 and lib.tc_ctx_get_blame_bisect(None) == 0 and lib.tc_ctx_last_blame_stats(None, None, None) == -1
    assert lib.tc_ctx_last_blame_stats(engine._ctx, None, None) == 0        # either pointer may be NULL
