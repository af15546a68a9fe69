"""GPU tests of the robust combiners on wire bytes (tc_combine_signatures_robust_wire_batch / tc_decrypt_robust_wire_batch,
include/tc_amd.h): the shares arrive as SignatureShare::to_bytes (96 B) / compressed decryption shares (48 B), only the t+1
selected ones are decoded -- as far as the curve -- and membership is tested once per job, on the combination.

The worlds, the Plan and the model of the rules are those of tests/test_gpu_robust.py; the planted faults are expressed on the
compressed forms (off the curve = an x whose cubic has no square root, or the compression flag cleared; the non-member = a
compressed on-curve point outside the subgroup, planted in BOTH input-check modes because wire shares are always checked).
Three checkers: the model (status / used / bad / n_fallback) with the master key's signature / the message as the only
accepted output of an OK job -- the invariant status OK => the true result, asserted in every test through check(); the
uncompressed robust entry on the decompressed shares (differential); Oracle B on a handful of jobs."""
import ctypes
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o
from threshold_crypto_amd import api
from test_gpu_robust import (EncWorld, INVALID, NOT_ENOUGH, OK, SEED_A, SEED_B, Plan, SigWorld, as_lists, non_member_g1, non_member_g2,
                             plant_main_cases, u8)

pytestmark = pytest.mark.gpu
IDENT_W = bytes([0xC0]) + bytes(95)


def no_square_root(g2, rnd):
    """a compressed encoding whose x is in range but x^3 + b is a non-square: fails the curve-level decode"""
    while True:
        if g2:
            x = (rnd.randrange(o.Q), rnd.randrange(o.Q))
            if o.f2_sqrt(o.f2_add(o.f2_mul(o.f2_sqr(x), x), o._Fq2.b)) is None:
                raw = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
                break
        else:
            x = rnd.randrange(o.Q)
            if pow((x * x * x + 4) % o.Q, (o.Q - 1) // 2, o.Q) != 1:
                raw = bytearray(x.to_bytes(48, "big"))
                break
    raw[0] |= 0x80
    return u8(raw)


class WirePlan(Plan):
    """A Plan over COMPRESSED shares: "off the curve" alternates between an x without a square root and a cleared compression
    flag (a compressed share has no y to spoil)."""

    def __init__(self, B, N, t, wire_shares, no_root):
        super().__init__(B, N, t, wire_shares)
        self.no_root, self.n_off = no_root, 0

    def off_curve(self, j, i):
        if self.n_off % 2 == 0:
            self.shares[j, i] = self.no_root
        else:
            self.shares[j, i, 0] &= 0x7F
        self.n_off += 1
        self.valid[j, i] = False


class WireSig:
    """a SigWorld plus the wire forms of its shares and of the expected signatures"""

    def __init__(self, engine, t, N, B, seed):
        w = self.w = SigWorld(engine, t, N, B, seed)
        self.t, self.N, self.B, self.engine = t, N, B, engine
        comp, st = engine.g2_compress(w.shares.reshape(B * N, 192))
        assert not st.any()
        self.shares = np.ascontiguousarray(comp.reshape(B, N, 96))
        self.want, st = engine.g2_compress(w.want)
        assert not st.any()
        self.no_root = no_square_root(True, random.Random(seed + 1))

    def plan(self):
        return WirePlan(self.B, self.N, self.t, self.shares, self.no_root)

    def cancel_pair(self, j, S0, a, b):
        pa, pb = self.w.cancel_pair(j, S0, a, b)
        comp, st = self.engine.g2_compress(np.stack([pa, pb]))
        assert not st.any()
        return comp[0], comp[1]

    def check(self, plan, out, used, bad, st, nfb, want=None):
        want = want or plan.expect()
        got = as_lists(used, bad, st, plan.B)
        for j in range(plan.B):
            # the invariant first: whatever the model says, an OK job holds the master key's signature
            assert int(st[j]) != OK or bytes(out[j]) == bytes(self.want[j]), j
            assert got[j] == want[j][:3], (j, got[j], want[j])
            assert bytes(out[j]) == (bytes(self.want[j]) if want[j][0] == OK else IDENT_W), j
        assert nfb == sum(1 for w in want if w[3])


@pytest.fixture(scope="module")
def world(engine):
    return WireSig(engine, 3, 10, 70, 0x0B57)


@pytest.fixture(scope="module")
def main_plan(world):
    """the planted main batch, made once and never modified by a test.  The non-member of job 8 sits inside S0: with the fixed
    seed its cofactor component does not vanish in the combination, so the job MUST reach pass 2 and end with slot 0 bad."""
    plan = world.plan()
    plant_main_cases(plan, True, random.Random(77), u8(o.g2_compressed(non_member_g2(random.Random(78)))), world.cancel_pair)
    return plan


@pytest.fixture(scope="module")
def main_reference(engine, world, main_plan):
    """the uncompressed robust entry on the checked decode of the same shares (an undecodable or non-member share decodes to
    the identity, which fails its own check there): computed once"""
    flat, st = engine.g2_decompress(main_plan.shares.reshape(-1, 96))
    shares = np.ascontiguousarray(flat.reshape(world.B, world.N, 192))
    out, used, bad, status, nfb = engine.combine_signatures_robust(world.w.commit, shares, hashes=world.w.hashes, present=main_plan.present, seed=SEED_A)
    comp, _ = engine.g2_compress(out)
    return comp, used, bad, status, nfb


@pytest.fixture
def unchecked(engine):
    engine.set_input_checks(False)
    yield engine
    engine.set_input_checks(True)


def test_all_clean_with_present_null(engine, world):
    w = world.w
    out, used, bad, st, nfb = engine.combine_signatures_robust_wire(w.commit, world.shares, hashes=w.hashes, seed=SEED_A)
    assert not st.any() and not bad.any() and nfb == 0
    assert (used[:, :4] == 1).all() and not used[:, 4:].any()
    assert out.shape == (world.B, 96) and (out == world.want).all()
    # the messages hashed on the device instead
    out2, used2, bad2, st2, nfb2 = engine.combine_signatures_robust_wire(w.commit, world.shares, msgs=w.flat, off=w.off, seed=SEED_A)
    assert (out2 == out).all() and (used2 == used).all() and not bad2.any() and not st2.any() and nfb2 == 0


def test_main_cases_model_differential_and_oracle_b(engine, world, main_plan, main_reference):
    plan, w = main_plan, world.w
    res = engine.combine_signatures_robust_wire(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A)
    world.check(plan, *res)
    want = plan.expect()
    assert [want[j][0] for j in (3, 4, 10)] == [NOT_ENOUGH] * 3 and want[10][2] == [0, 1, 2]        # the model itself
    assert want[6] == (OK, [0, 1, 2, 3], [], False) and want[11] == (OK, [0, 1, 2, 3], [], False)
    assert want[7] == (OK, [0, 1, 3, 4], [2], True) and want[8] == (OK, [1, 2, 3, 4], [0], True)    # undecodable / non-member in S0
    # differential: the uncompressed entry on the decompressed shares, its signatures compressed
    for got, ref in zip(res[:4], main_reference[:4]):
        assert (got == ref).all()
    assert res[4] == main_reference[4]
    # a second seed: identical bytes
    res_b = engine.combine_signatures_robust_wire(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_B)
    for x, y in zip(res[:4], res_b[:4]):
        assert (x == y).all()
    assert res[4] == res_b[4]
    # Oracle B on a handful of jobs: the shares the call says it used combine (checked decode, combine, to_bytes) to its
    # output, which verifies under the master key
    out, used = res[0], res[1]
    for j in (0, 1, 2, 5, 7, 8, 12, 65, 69):
        ids = [int(i) for i in np.nonzero(used[j])[0]]
        rc, sig = c.combine_signatures_wire(world.t, ids, [bytes(plan.shares[j, i]) for i in ids])
        assert rc == 0 and sig == bytes(out[j]), j
        rc, full = c.g2_decompress(bytes(out[j]))
        assert rc == 0 and c.verify_g2(bytes(w.commit[0]), full, bytes(w.hashes[j])), j


def test_main_cases_with_input_checks_off_and_hashed_on_the_device(unchecked, world, main_plan, main_reference):
    """wire shares are always checked: the same plan, non-member included, gives the same answer with the switch off"""
    w = world.w
    res = unchecked.combine_signatures_robust_wire(w.commit, main_plan.shares, msgs=w.flat, off=w.off, present=main_plan.present, seed=SEED_B)
    world.check(main_plan, *res)
    for got, ref in zip(res[:4], main_reference[:4]):
        assert (got == ref).all()


def test_a_share_with_a_component_of_order_13(engine, world):
    """An honest share plus a point T of order 13 is on the curve and outside the subgroup.  T is made with Oracle A from a
    random point of E'(Fq2): times r, which clears its part in G2, and times h2 / 169 -- NOT h2 / 13: 13^2 divides h2 and the
    13-part of E'(Fq2) is Z13 x Z13, so h2 / 13 still kills it and would leave a point of G2; the order is asserted below.  The
    job either comes out clean -- the Lagrange coefficient may be a multiple of 13, then the combination IS the signature -- or
    goes to pass 2 with the slot marked bad.  Never a wrong output."""
    w, rnd = world.w, random.Random(13)
    T = None
    while T is None:
        P = o.g2_get_point_from_x((rnd.randrange(o.Q), rnd.randrange(o.Q)), True)
        if P is not None:
            T = o.E2.mul(o.E2.mul(P, o.H2 // 169), o.R)
    assert o.E2.on_curve(T) and o.E2.mul(T, 13) is None
    plan = world.plan()
    for j, slot in ((20, 0), (21, 1), (22, 2), (23, 3)):                      # four Lagrange coefficients: four chances
        S = o.g2_from_uncompressed(bytes(w.shares[j, slot]), check=False)
        plan.shares[j, slot] = u8(o.g2_compressed(o.E2.add(S, T)))
    out, used, bad, st, nfb = engine.combine_signatures_robust_wire(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A)
    got = as_lists(used, bad, st, plan.B)
    examined = 0
    for j in range(plan.B):
        assert int(st[j]) == OK and bytes(out[j]) == bytes(world.want[j]), j     # the invariant: every job has t+1 honest shares
        slot = {20: 0, 21: 1, 22: 2, 23: 3}.get(j)
        if slot is None or got[j][2] == []:
            assert got[j] == (OK, [0, 1, 2, 3], []), j                           # clean
        else:
            assert got[j] == (OK, [i for i in range(5) if i != slot], [slot]), j  # pass 2: the slot is bad
            examined += 1
    assert nfb == examined


def test_both_decode_forms(engine):
    """B in {1, 3} x t in {0, 2}: odd record counts (the tail repeats a record) and lane pairs that straddle two jobs, one of
    which lacks enough shares -- through the one-record and the two-record kernel, forced by TC_DUO_MIN"""
    from conftest import engine_with_env
    cases = []
    for t in (0, 2):
        for B in (1, 3):
            ws = WireSig(engine, t, t + 2, B, 0xF0 + 4 * t + B)
            plan = ws.plan()
            if B == 3:
                plan.only(1, range(t))                                        # job 1: one share short
                plan.off_curve(2, 0)                                          # job 2: an undecodable share inside S0
            cases.append((ws, plan))
    results = {}
    for minimum in (1, 10 ** 12):
        with engine_with_env(TC_DUO_MIN=minimum) as eng:
            results[minimum] = [eng.combine_signatures_robust_wire(ws.w.commit, plan.shares, hashes=ws.w.hashes, present=plan.present, seed=SEED_A)
                                for ws, plan in cases]
    for k, (ws, plan) in enumerate(cases):
        one, two = results[10 ** 12][k], results[1][k]
        ws.check(plan, *one)
        ws.check(plan, *two)
        for x, y in zip(one[:4], two[:4]):
            assert (x == y).all()
        if ws.B == 3:
            assert as_lists(one[1], one[2], one[3], 3)[1:] == [(NOT_ENOUGH, [], []), (OK, list(range(1, ws.t + 2)), [0])]


def test_long_rows_and_the_large_threshold_path(engine):
    """B = 6, N = 70, t = 21: mask rows longer than 64 bytes, the two-stage combine path"""
    ws = WireSig(engine, 21, 70, 6, 0x70)
    plan = ws.plan()
    plan.absent(1, sorted(random.Random(1).sample(range(70), 30)))
    plan.only(2, range(48, 70))                                             # the last t+1 slots
    plan.wrong(3, 9, other=0)                                               # inside S0
    plan.off_curve(3, 40)                                                   # examined: reported although past S0
    plan.only(4, range(3, 24))                                              # exactly t present
    plan.wrong(5, 65, other=0)                                              # past S0: not reported
    res = engine.combine_signatures_robust_wire(ws.w.commit, plan.shares, hashes=ws.w.hashes, present=plan.present, seed=SEED_A)
    ws.check(plan, *res)
    assert as_lists(res[1], res[2], res[3], 6)[3] == (OK, [i for i in range(23) if i != 9], [9, 40])


def test_device_io_gives_identical_bytes(engine, world, main_plan):
    import torch
    plan, w = main_plan, world.w
    host = engine.combine_signatures_robust_wire(w.commit, plan.shares, hashes=w.hashes, present=plan.present, seed=SEED_A)
    dev = [torch.from_numpy(x).cuda() for x in (w.commit, plan.shares, w.hashes, plan.present)]
    got = engine.combine_signatures_robust_wire(dev[0], dev[1], hashes=dev[2], present=dev[3], seed=SEED_A)
    engine.sync()
    for h, d in zip(host[:4], got[:4]):
        assert (h == d.cpu().numpy()).all()
    assert host[4] == got[4]
    flat, off = torch.from_numpy(w.flat).cuda(), torch.from_numpy(w.off.view(np.int64)).cuda()
    got = engine.combine_signatures_robust_wire(dev[0], dev[1], msgs=flat, off=off, present=dev[3], seed=SEED_A)
    engine.sync()
    for h, d in zip(host[:4], got[:4]):
        assert (h == d.cpu().numpy()).all()


def test_undecodable_commit_fails_every_job(engine, world, main_plan):
    w = world.w
    spoiled = w.commit.copy()
    spoiled[1, -1] ^= 1                                                     # off the curve
    outsider = w.commit.copy()
    outsider[2] = u8(o.g1_uncompressed(non_member_g1(random.Random(5))))    # checked-input mode: on the curve, outside G1
    for commit in (spoiled, outsider):
        out, used, bad, st, nfb = engine.combine_signatures_robust_wire(commit, main_plan.shares, hashes=w.hashes, present=main_plan.present, seed=SEED_A)
        assert (st == INVALID).all() and not used.any() and not bad.any() and nfb == 0
        assert all(bytes(out[j]) == IDENT_W for j in range(world.B))


def test_argument_checks(engine, world):
    w = world.w
    with pytest.raises(ValueError):
        engine.combine_signatures_robust_wire(w.commit, world.shares, seed=SEED_A)                          # neither hashes nor messages
    with pytest.raises(ValueError):
        engine.combine_signatures_robust_wire(w.commit, world.shares[:, :3].copy(), hashes=w.hashes)        # t + 1 > N
    with pytest.raises(ValueError):
        engine.combine_signatures_robust_wire(w.commit, w.shares, hashes=w.hashes)                          # uncompressed shares
    lib, ctx = engine._lib, engine._ctx
    st = np.zeros(1, np.uint8)
    rc = lib.tc_combine_signatures_robust_wire_batch(ctx, None, 3, 10, None, None, None, None, None, 1, 0, SEED_A, None, None, None,
                                                     ctypes.c_void_p(st.ctypes.data), None)
    assert rc == -1                                                         # NULL data pointers with a non-zero size
    assert lib.tc_combine_signatures_robust_wire_batch(ctx, None, 3, 10, None, None, None, None, None, 0, 0, None, None, None, None, None,
                                                       None) == 0           # an empty batch is a no-op
    # t + 1 > N at the C boundary, with every pointer valid
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    sh, out1 = np.ascontiguousarray(world.shares[:1, :3]), np.zeros((1, 96), np.uint8)
    rc = lib.tc_combine_signatures_robust_wire_batch(ctx, p(w.commit), 3, 3, None, p(sh), p(w.hashes), None, None, 1, 0, SEED_A, p(out1), None, None,
                                                     p(st), None)
    assert rc == -1
    assert lib.tc_decrypt_robust_wire_batch(ctx, None, 3, 10, None, None, None, None, None, None, 1, None, None, None, p(st), None) == -1
    assert lib.tc_decrypt_robust_wire_batch(ctx, None, 3, 10, None, None, None, None, None, None, 0, None, None, None, None, None) == 0


def test_api_combine_signatures_robust_wire_batch(engine, world, main_plan):
    plan, w = main_plan, world.w
    pk_set = api.PublicKeySet([bytes(x) for x in w.commit], _trusted=True)
    picks = [0, 1, 3, 5, 8, 10, 12]
    jobs = [{i: bytes(plan.shares[j, i]) for i in range(world.N) if plan.present[j, i]} for j in picks]
    res = pk_set.combine_signatures_robust_wire_batch(jobs, [w.msgs[j] for j in picks], n_nodes=world.N, engine=engine, seed=SEED_A)
    want = plan.expect()
    for (val, used, bad), j in zip(res, picks):
        assert (used, bad) == (want[j][1], want[j][2]), j
        if want[j][0] == OK:
            assert isinstance(val, api.Signature) and val.raw == bytes(w.want[j]), j
        else:
            assert isinstance(val, api.NotEnoughShares), j


# ---- decryption ------------------------------------------------------------------------------------------------------------
class WireEnc:
    def __init__(self, engine, t, N, B, seed, poly=None):
        w = self.w = EncWorld(engine, t, N, B, seed, poly=poly)
        self.t, self.N, self.B, self.engine = t, N, B, engine
        comp, st = engine.g1_compress(w.shares.reshape(B * N, 96))
        assert not st.any()
        self.shares = np.ascontiguousarray(comp.reshape(B, N, 48))
        self.no_root = no_square_root(False, random.Random(seed + 1))

    def plan(self):
        return WirePlan(self.B, self.N, self.t, self.shares, self.no_root)

    def cancel_pair(self, j, S0, a, b):
        pa, pb = self.w.cancel_pair(j, S0, a, b)
        comp, st = self.engine.g1_compress(np.stack([pa, pb]))
        assert not st.any()
        return comp[0], comp[1]

    def check(self, plan, want, out, used, bad, st, nfb):
        w = self.w
        for j in range(plan.B):                                               # the invariant: an OK job holds the message
            lo, hi = int(w.off[j]), int(w.off[j + 1])
            assert int(st[j]) != OK or bytes(out[lo:hi]) == w.plain[j], j
        w.check(plan, want, out, used, bad, st, nfb)


@pytest.fixture(scope="module")
def enc_world(engine):
    return WireEnc(engine, 3, 10, 70, 0xDEC)


@pytest.mark.parametrize("checked", [True, False])
def test_decrypt_main_cases(engine, enc_world, checked):
    ew, w = enc_world, enc_world.w
    plan = ew.plan()
    # (the non-member G1 share of job 8 is planted in both modes: wire shares are always checked.  Fixed seed: it lands in pass 2)
    plant_main_cases(plan, True, random.Random(79), u8(o.g1_compressed(non_member_g1(random.Random(80)))), ew.cancel_pair)
    # an invalid ciphertext (job 30: the w of another one): every honest share fails its check
    ww = w.w.copy()
    ww[30] = w.w[31]
    plan.absent(30, [4])
    want = plan.expect()
    want[30] = (NOT_ENOUGH, [], [i for i in range(ew.N) if i != 4], True)
    assert want[8] == (OK, [1, 2, 3, 4], [0], True) and want[7] == (OK, [0, 1, 3, 4], [2], True)
    engine.set_input_checks(checked)
    try:
        res = engine.decrypt_robust_wire(w.commit, plan.shares, w.u, w.v, w.off, ww, present=plan.present)
        ew.check(plan, want, *res)
        # differential: the uncompressed entry on the checked decode of the same shares
        flat, _ = engine.g1_decompress(plan.shares.reshape(-1, 48))
        ref = engine.decrypt_robust(w.commit, np.ascontiguousarray(flat.reshape(ew.B, ew.N, 96)), w.u, w.v, w.off, ww, present=plan.present)
        for got, r in zip(res[:4], ref[:4]):
            assert (got == r).all()
        assert res[4] == ref[4]
        if checked:
            import torch
            dev = [torch.from_numpy(x).cuda() for x in (w.commit, plan.shares, w.u, w.v, w.off.view(np.int64), ww, plan.present)]
            got = engine.decrypt_robust_wire(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], present=dev[6])
            engine.sync()
            for h, d in zip(res[:4], got[:4]):
                assert (h == d.cpu().numpy()).all()
            assert res[4] == got[4]
            # Oracle B on three jobs: the shares used decrypt the ciphertext
            for j in (1, 5, 8):
                ids = [int(i) for i in np.nonzero(res[1][j])[0]]
                rc, plain = c.decrypt_wire(ew.t, ids, [bytes(plan.shares[j, i]) for i in ids], bytes(w.v[int(w.off[j]):int(w.off[j + 1])]))
                assert rc == 0 and plain == w.plain[j], j
    finally:
        engine.set_input_checks(True)


def test_decrypt_all_clean_present_null_and_api(engine, enc_world):
    ew, w = enc_world, enc_world.w
    out, used, bad, st, nfb = engine.decrypt_robust_wire(w.commit, ew.shares, w.u, w.v, w.off, w.w)
    assert not st.any() and not bad.any() and nfb == 0 and (used[:, :4] == 1).all() and not used[:, 4:].any()
    assert all(bytes(out[int(w.off[j]):int(w.off[j + 1])]) == w.plain[j] for j in range(ew.B))
    pk_set = api.PublicKeySet([bytes(x) for x in w.commit], _trusted=True)
    cts = [api.Ciphertext(bytes(w.u[j]), bytes(w.v[int(w.off[j]):int(w.off[j + 1])]), bytes(w.w[j]), _trusted=True) for j in (1, 2)]
    jobs = [{i: bytes(ew.shares[1, i]) for i in (2, 3, 5, 7, 9)}, {i: bytes(ew.shares[2 if i != 4 else 3, i]) for i in range(3, 9)}]
    res = pk_set.decrypt_robust_wire_batch(jobs, cts, n_nodes=ew.N, engine=engine)
    assert res[0] == (w.plain[1], [2, 3, 5, 7], []) and res[1] == (w.plain[2], [3, 5, 6, 7], [4])


def test_decrypt_large_threshold_and_undecodable_commit(engine):
    ew = WireEnc(engine, 21, 70, 6, 0x71)
    w = ew.w
    plan = ew.plan()
    plan.only(2, range(48, 70))
    plan.wrong(3, 9, other=0)
    plan.off_curve(3, 40)
    plan.only(4, range(3, 24))
    res = engine.decrypt_robust_wire(w.commit, plan.shares, w.u, w.v, w.off, w.w, present=plan.present)
    ew.check(plan, plan.expect(), *res)
    assert as_lists(res[1], res[2], res[3], 6)[3] == (OK, [i for i in range(23) if i != 9], [9, 40])
    spoiled = w.commit.copy()
    spoiled[1, -1] ^= 1
    out, used, bad, st, nfb = engine.decrypt_robust_wire(spoiled, plan.shares, w.u, w.v, w.off, w.w, present=plan.present)
    assert (st == INVALID).all() and not used.any() and not bad.any() and nfb == 0 and not out.any()
