"""GPU tests of decryption-share verification over ragged input (tc_verify_decryption_share_records_rlc_batch and its pre-hashed
form, include/tc_amd.h): M ciphertexts, ciphertext c owning the records rec_off[c] .. rec_off[c + 1], record r = a
decryption share and the index of its key in a table of K keys.

Keys, ciphertexts and shares come from the library's own tc_g1_commitment_batch / tc_encrypt_batch / tc_g1_mul_batch over fixed
scalars (K = 7 keys, 12 ciphertexts, EVERY share sk_i u_c made once per module); what a record must answer is computed by the C
oracle's verify_decryption_share (once per distinct tuple, cached for the module), and every case is also compared with
tc_verify_decryption_share_batch at pk_stride = 96 on the expanded arrays.  A record whose index is outside the table has no key
to expand: it stands in the expanded arrays with 96 bytes that do not decode, and its expected answer is 0 by construction --
like every record with a malformed operand."""
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o
from threshold_crypto_amd.engine import pack_messages

pytestmark = pytest.mark.gpu
K, CTS = 7, 12
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))
NO_KEY = np.full(96, 0xFF, dtype=np.uint8)


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def fr_rows(vals):
    return np.stack([u8(int(v % o.R).to_bytes(32, "little")) for v in vals])


def non_member_g1(rnd):
    """an on-curve point of E(Fq) outside the order-r subgroup (as tests/test_gpu_robust.py makes them)"""
    while True:
        x = rnd.randrange(o.Q)
        y2 = (x * x * x + 4) % o.Q
        y = pow(y2, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == y2 and o.E1.mul((x, y), o.R) is not None:
            return u8(o.g1_uncompressed((x, y)))


class World:
    def __init__(self, engine):
        rnd = random.Random(0xD5EC)
        self.engine, self.rnd = engine, rnd
        self.sk = [rnd.randrange(1, o.R) for _ in range(K)]
        self.pks, st = engine.g1_commitment(fr_rows(self.sk))                                   # (K, 96)
        assert not np.asarray(st).any()
        master, st = engine.g1_commitment(fr_rows([rnd.randrange(1, o.R)]))
        self.plain = [b"ragged plaintext %d" % i + b"." * (i % 5) for i in range(CTS)]         # lengths differ
        flat, off = pack_messages(self.plain)
        u, v, w, st = engine.encrypt(np.ascontiguousarray(master[0]), fr_rows([rnd.randrange(1, o.R) for _ in range(CTS)]), flat, off)
        assert not np.asarray(st).any()
        self.u, self.w = np.ascontiguousarray(u), np.ascontiguousarray(w)
        v, off = np.asarray(v), np.asarray(off)
        self.v = [bytes(v[int(off[i]):int(off[i + 1])]) for i in range(CTS)]
        out, st = engine.g1_mul(fr_rows(self.sk), self.u)                                       # [c, i] = sk_i u_c
        assert not np.asarray(st).any()
        self.share = np.ascontiguousarray(out)
        self._oracle = {}

    def oracle(self, pk, share, u, v, w):
        key = (bytes(pk), bytes(share), bytes(u), bytes(v), bytes(w))
        if key not in self._oracle:
            self._oracle[key] = int(c.verify_decryption_share(*key))
        return self._oracle[key]


@pytest.fixture(scope="module")
def world(engine):
    return World(engine)


class Case:
    """records of the first len(lens) ciphertexts: ciphertext m's k-th record is the share of key (m + k) % K unless `keys` says otherwise"""

    def __init__(self, world, lens, keys=None, ct_ids=None):
        self.wd, self.lens, self.M = world, list(lens), len(lens)
        self.ct_ids = list(ct_ids) if ct_ids is not None else list(range(self.M))
        self.rec_off = np.zeros(self.M + 1, dtype=np.uint64)
        self.rec_off[1:] = np.cumsum(self.lens, dtype=np.uint64)
        self.R = int(self.rec_off[-1])
        self.ct_of = [m for m in range(self.M) for _ in range(self.lens[m])]
        self.key_idx = np.array([(m + k) % K if keys is None else keys(m, k) for m in range(self.M) for k in range(self.lens[m])], dtype=np.uint64)
        self.pks = world.pks.copy()
        self.u = np.ascontiguousarray(world.u[self.ct_ids])
        self.w = np.ascontiguousarray(world.w[self.ct_ids])
        self.v = [world.v[i] for i in self.ct_ids]
        self.flat, self.off = pack_messages(self.v)
        self.shares = np.zeros((self.R, 96), dtype=np.uint8)
        for r in range(self.R):
            self.shares[r] = world.share[self.ct_ids[self.ct_of[r]], int(self.key_idx[r])]
        self.forced = {}                                   # record -> 0: malformed by construction (no oracle answer)

    def rec(self, m, k=0):
        return int(self.rec_off[m]) + k

    def records_of(self, m):
        return list(range(self.rec(m), self.rec(m + 1)))

    def group_records(self, group, recs):
        """records of the groups that hold any of `recs`"""
        group = group or 64
        groups = {self.ct_of[r] // group for r in recs}
        return [r for r in range(self.R) if self.ct_of[r] // group in groups]

    def expanded(self):
        """(pk, u, flat v, off, w), one row per record"""
        pk = np.stack([self.pks[int(i)] if int(i) < K else NO_KEY for i in self.key_idx]) if self.R else np.zeros((0, 96), np.uint8)
        flat, off = pack_messages([self.v[m] for m in self.ct_of])
        return np.ascontiguousarray(pk), np.ascontiguousarray(self.u[self.ct_of]), flat, off, np.ascontiguousarray(self.w[self.ct_of])

    def expect(self):
        pk = self.expanded()[0]
        return np.array([self.forced[r] if r in self.forced else
                         self.wd.oracle(pk[r], self.shares[r], self.u[self.ct_of[r]], self.v[self.ct_of[r]], self.w[self.ct_of[r]])
                         for r in range(self.R)], dtype=np.uint8)

    def run(self, engine=None, group=0, seed=SEED_A, key_idx="own"):
        eng = engine or self.wd.engine
        kidx = self.key_idx if isinstance(key_idx, str) else key_idx
        ok, nfb = eng.verify_decryption_share_records_rlc(self.pks, kidx, self.shares, self.rec_off, self.u, self.flat, self.off, self.w, group=group,
                                                          seed=seed)
        return np.asarray(ok), nfb

    def check(self, engine=None, group=0, bad=(), seed=SEED_A):
        """the entry against the oracle, against the per-record path, and n_fallback against the records of the groups of `bad`"""
        eng = engine or self.wd.engine
        want = self.expect()
        assert sorted(np.flatnonzero(want == 0).tolist()) == sorted(bad), "the case is not what the test meant to build"
        pk, u, flat, off, w = self.expanded()
        per_record = np.asarray(eng.verify_decryption_share(pk, self.shares, u, flat, off, w)) if self.R else np.zeros(0, np.uint8)
        ok, nfb = self.run(eng, group, seed)
        print("records %d, group %d: rejected %s, n_fallback %d" % (self.R, group, np.flatnonzero(ok == 0).tolist(), nfb))
        assert ok.tolist() == want.tolist()
        assert ok.tolist() == per_record.tolist()
        assert nfb == len(self.group_records(group, bad))
        return ok, nfb


RAGGED = [0, 1, 3, 1, 7, 0, 2]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [3, 1, 64])
def test_ragged_all_valid(world, group):
    """two full groups of three and a tail of one ciphertext at group = 3, an empty ciphertext in the first group and in the second"""
    case = Case(world, RAGGED)
    ok, nfb = case.check(group=group)
    assert ok.all() and nfb == 0


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("kind", ["other_node", "other_ciphertext", "plus_generator", "wrong_index"])
def test_one_forged_record(world, kind, where):
    """groups of three ciphertexts: {3, 4, 5} holds the records 4 .. 11; the forged record is its first or its last"""
    case = Case(world, RAGGED)
    r = case.rec(3, 0) if where == "first" else case.rec(4, 6)
    assert case.group_records(3, [r])[0 if where == "first" else -1] == r
    m, k = case.ct_of[r], int(case.key_idx[r])
    if kind == "other_node":
        case.shares[r] = world.share[m, (k + 1) % K]
    elif kind == "other_ciphertext":
        case.shares[r] = world.share[m + 2, k]
    elif kind == "plus_generator":
        pts = np.stack([case.shares[r], u8(o.g1_uncompressed(o.G1_GEN))])[None]
        out, st = world.engine.lincomb_g1(np.broadcast_to(fr_rows([1])[0], (1, 2, 32)).copy(), np.ascontiguousarray(pts))
        assert not np.asarray(st).any()
        case.shares[r] = np.asarray(out)[0]
    else:
        case.key_idx[r] = (k + 3) % K
    ok, nfb = case.check(group=3, bad=[r])
    assert nfb == 8
    assert [i for i in range(case.R) if not ok[i]] == [r]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_cancelling_pair_is_rejected(world):
    """share_a + delta and share_b - delta on one ciphertext (delta = [d] u_c, a member of G1): the unweighted sum of the
    ciphertext's shares is what it was, so an aggregate check would pass -- the weighted one rejects both records, whatever the seed"""
    case = Case(world, RAGGED)
    m, a, b = 4, case.rec(4, 1), case.rec(4, 4)
    ka, kb = int(case.key_idx[a]), int(case.key_idx[b])
    d = world.rnd.randrange(1, o.R)
    out, st = world.engine.g1_mul(fr_rows([world.sk[ka] + d, world.sk[kb] - d]), world.u[m:m + 1])
    assert not np.asarray(st).any()
    lo, hi = case.rec(m), case.rec(m + 1)
    ones = np.broadcast_to(fr_rows([1])[0], (1, hi - lo, 32)).copy()
    before, st0 = world.engine.lincomb_g1(ones, np.ascontiguousarray(case.shares[lo:hi][None]))
    case.shares[a], case.shares[b] = out[0, 0], out[0, 1]
    after, st1 = world.engine.lincomb_g1(ones, np.ascontiguousarray(case.shares[lo:hi][None]))
    assert not np.asarray(st0).any() and not np.asarray(st1).any()
    assert bytes(np.asarray(before)[0]) == bytes(np.asarray(after)[0]) != bytes(o.g1_uncompressed(None))
    assert world.engine.g1_subgroup_check(np.ascontiguousarray(case.shares[[a, b]])).all()
    for seed in (SEED_A, SEED_B):
        ok, nfb = case.check(group=3, bad=[a, b], seed=seed)
        assert nfb == 8


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
# (a point outside G1 is only told apart in checked-input mode: no case with the checks off)
MALFORMED = [(kind, checked) for kind in ("share_undecodable", "key_undecodable", "index_K", "index_max", "u_undecodable", "w_undecodable",
                                          "share_non_member", "key_non_member", "u_non_member") for checked in (True, False)
             if checked or not kind.endswith("non_member")]


@pytest.mark.parametrize("kind,checked", MALFORMED)
def test_one_malformed_operand(world, kind, checked):
    eng = world.engine
    case = Case(world, RAGGED)
    if kind == "share_undecodable":
        bad = [case.rec(4, 2)]
        case.shares[bad[0], 60] ^= 1                             # not on the curve
    elif kind == "share_non_member":
        bad = [case.rec(2, 0)]
        case.shares[bad[0]] = non_member_g1(random.Random(5))
    elif kind in ("key_undecodable", "key_non_member"):          # every record that names key 3, and only those
        if kind == "key_undecodable":
            case.pks[3, 50] ^= 1
        else:
            case.pks[3] = non_member_g1(random.Random(7))
        bad = [r for r in range(case.R) if int(case.key_idx[r]) == 3]
        assert len(bad) >= 2 and len({case.ct_of[r] for r in bad}) >= 2
    elif kind in ("index_K", "index_max"):
        bad = [case.rec(4, 3)]
        case.key_idx[bad[0]] = K if kind == "index_K" else 2 ** 64 - 1
    elif kind == "u_undecodable":                                # every record of ciphertext 4; ciphertext 3 of its group stays valid
        case.u[4, 60] ^= 1
        bad = case.records_of(4)
    elif kind == "u_non_member":
        case.u[4] = non_member_g1(random.Random(6))
        bad = case.records_of(4)
    else:
        case.w[4, 100] ^= 1
        bad = case.records_of(4)
    for r in bad:
        case.forced[r] = 0
    eng.set_input_checks(checked)
    try:
        ok, nfb = case.check(group=3, bad=bad)
    finally:
        eng.set_input_checks(True)
    assert [r for r in range(case.R) if not ok[r]] == bad


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_an_invalid_ciphertext_fails_its_honest_shares(world):
    """w taken from another ciphertext: Ciphertext::verify fails and so does every share of it, as the oracle says -- the entry
    does not call Ciphertext::verify, the equation does the work"""
    case = Case(world, RAGGED)
    case.w[2] = world.w[7]
    assert not c.ciphertext_verify(bytes(case.u[2]), case.v[2], bytes(case.w[2]))
    bad = case.records_of(2)
    ok, nfb = case.check(group=3, bad=bad)
    assert nfb == 4 and [r for r in range(case.R) if not ok[r]] == bad


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_without_an_index_array_record_r_uses_key_r(world):
    """K = R = 9 records over ciphertexts of 2, 0, 3, 4 records, the key of record r at pks[r]"""
    eng = world.engine
    case = Case(world, [2, 0, 3, 4])
    table = np.ascontiguousarray(world.pks[case.key_idx.astype(np.int64)])                     # K = R = 9
    for forged in ([], [1, 7]):
        cs = Case(world, [2, 0, 3, 4])
        for r in forged:
            cs.shares[r] = world.share[cs.ct_of[r], (int(cs.key_idx[r]) + 1) % K]
        want = cs.expect()
        assert [r for r in range(cs.R) if not want[r]] == forged
        ok, nfb = eng.verify_decryption_share_records_rlc(table, None, cs.shares, cs.rec_off, cs.u, cs.flat, cs.off, cs.w, group=2, seed=SEED_A)
        assert np.asarray(ok).tolist() == want.tolist() and nfb == (9 if forged else 0)        # groups {0, 1}: 2 records, {2, 3}: 7
        pk, u, flat, off, w = cs.expanded()
        assert np.asarray(eng.verify_decryption_share(table, cs.shares, u, flat, off, w)).tolist() == want.tolist()
    with pytest.raises(ValueError):
        eng.verify_decryption_share_records_rlc(table[:8], None, case.shares, case.rec_off, case.u, case.flat, case.off, case.w)   # K < R


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_dense_input_equals_the_share_matrix_entry(world):
    """N = 5 keys x B = 6 ciphertexts, every record present, one forged share: the ok matrix of tc_verify_decryption_shares_rlc_batch"""
    eng = world.engine
    N, B = 5, 6
    case = Case(world, [N] * B, keys=lambda m, k: k)
    case.pks = np.ascontiguousarray(world.pks[:N])
    r = case.rec(3, 2)
    case.shares[r] = world.share[3, 4]
    shares = np.ascontiguousarray(case.shares.reshape(B, N, 96))
    matrix, nfb_m = eng.verify_decryption_shares_rlc(case.pks, shares, case.u, case.flat, case.off, case.w, seed=SEED_A)
    matrix = np.asarray(matrix)
    assert nfb_m == 1 and [tuple(x) for x in np.argwhere(matrix == 0)] == [(3, 2)]
    want = case.expect()
    assert want.reshape(B, N).tolist() == matrix.tolist()
    for group in (1, 4):
        ok, nfb = case.run(group=group)
        assert ok.reshape(B, N).tolist() == matrix.tolist() and nfb == N * group        # the forged share's group: ciphertext 3 alone, or 0 .. 3
    pk, u, flat, off, w = case.expanded()
    assert np.asarray(eng.verify_decryption_share(pk, case.shares, u, flat, off, w)).reshape(B, N).tolist() == matrix.tolist()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
LONG = [130, 0, 1, 3, 4, 5, 33]


@pytest.fixture(scope="module")
def long_cases(world):
    """segment lengths that make a sum span a whole wave, leave padded chunk places, parts without records and put sums of very
    different length in one wave, over 5 repeated keys: all valid, the LAST record of the 130-segment forged (its last chunk
    holds two records and two padded places), and the one record of the one-record segment forged"""
    keys = lambda m, k: (m + k) % 5
    good, last, single = Case(world, LONG, keys=keys), Case(world, LONG, keys=keys), Case(world, LONG, keys=keys)
    r_last, r_single = last.rec(0, 129), single.rec(2, 0)
    last.shares[r_last] = world.share[0, (int(last.key_idx[r_last]) + 1) % 5]
    single.shares[r_single] = world.share[2, (int(single.key_idx[r_single]) + 1) % 5]
    assert good.expect().all()                                                               # the oracle's answers, once for the module
    assert np.flatnonzero(last.expect() == 0).tolist() == [r_last] and np.flatnonzero(single.expect() == 0).tolist() == [r_single]
    return good, last, r_last, single, r_single


def _long(eng, long_cases):
    good, last, r_last, single, r_single = long_cases
    ok, nfb = good.check(eng, group=2)
    assert ok.all() and nfb == 0
    ok, nfb = last.check(eng, group=2, bad=[r_last])
    assert nfb == 130 and [i for i in range(last.R) if not ok[i]] == [r_last]               # the group {0, 1}: 130 + 0 records
    ok, nfb = single.check(eng, group=2, bad=[r_single])
    assert nfb == 4 and [i for i in range(single.R) if not ok[i]] == [r_single]             # the group {2, 3}: 1 + 3 records


def test_long_and_odd_segments_in_one_launch(world, long_cases):
    _long(world.engine, long_cases)


@pytest.mark.parametrize("parts", [1, 2, 64])
def test_long_and_odd_segments_with_the_split_forced(long_cases, parts):
    """TC_RECORDS_PARTS: one lane per sum, both sums of a ciphertext in four lanes of one wave, and 64 lanes per sum -- the two
    sums of a ciphertext in two waves, most parts of the short segments without records"""
    from conftest import engine_with_env
    with engine_with_env(TC_RECORDS_PARTS=parts) as eng:
        _long(eng, long_cases)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_forms_agree(world):
    import torch
    eng = world.engine
    case = Case(world, RAGGED)
    r = case.rec(3, 0)
    case.shares[r] = world.share[2, int(case.key_idx[r])]
    want, _ = case.check(group=3, bad=[r])
    other_seed, nfb = case.run(group=3, seed=SEED_B)
    assert other_seed.tolist() == want.tolist() and nfb == 8
    hashes, st = eng.hash_g1_g2(case.u, case.flat, case.off)
    assert not np.asarray(st).any()
    hashes = np.ascontiguousarray(hashes)
    for seed in (SEED_A, SEED_B):
        ok, nfb = eng.verify_decryption_share_records_prehashed_rlc(case.pks, case.key_idx, case.shares, case.rec_off, hashes, case.w, group=3, seed=seed)
        assert np.asarray(ok).tolist() == want.tolist() and nfb == 8
    dev = torch.device("cuda:0")
    t8 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
    try:
        ok, nfb = eng.verify_decryption_share_records_rlc(t8(case.pks), t64(case.key_idx), t8(case.shares), t64(case.rec_off), t8(case.u), t8(case.flat),
                                                          t64(case.off), t8(case.w), group=3, seed=SEED_A)
        eng.sync()
        assert ok.cpu().numpy().tolist() == want.tolist() and nfb == 8
        ok, nfb = eng.verify_decryption_share_records_prehashed_rlc(t8(case.pks), t64(case.key_idx), t8(case.shares), t64(case.rec_off), t8(hashes),
                                                                    t8(case.w), group=3, seed=SEED_B)
        eng.sync()
        assert ok.cpu().numpy().tolist() == want.tolist() and nfb == 8
    finally:
        eng.sync()


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
def test_empty_inputs(world):
    eng = world.engine
    none8 = lambda n: np.zeros((0, n), dtype=np.uint8)
    ok, nfb = eng.verify_decryption_share_records_rlc(world.pks, np.zeros(0, np.uint64), none8(96), np.zeros(1, np.uint64), none8(96), np.zeros(0, np.uint8),
                                                      np.zeros(1, np.uint64), none8(192), seed=SEED_A)
    assert np.asarray(ok).shape == (0,) and nfb == 0
    # every ciphertext empty: nothing is written, through the C ABI with a guarded ok buffer
    import ctypes
    from threshold_crypto_amd import _native
    lib = _native.load()
    M = 5
    rec_off = np.zeros(M + 1, dtype=np.uint64)
    case = Case(world, [1, 2, 0, 1, 1])
    hashes = np.ascontiguousarray(np.asarray(eng.hash_g1_g2(case.u, case.flat, case.off)[0]))
    guard = np.full(8, 0xA5, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    nfb = ctypes.c_uint64(77)
    rc = lib.tc_verify_decryption_share_records_rlc_batch(eng._ctx, p(world.pks), K, None, None, p(rec_off), p(case.u), p(case.flat), p(case.off),
                                                          p(case.w), M, 2, SEED_A, p(guard), ctypes.byref(nfb))
    assert rc == _native.TC_OK and nfb.value == 0 and (guard == 0xA5).all()
    nfb = ctypes.c_uint64(77)
    rc = lib.tc_verify_decryption_share_records_prehashed_rlc_batch(eng._ctx, p(world.pks), K, None, None, p(rec_off), p(hashes), p(case.w), M, 2, SEED_A,
                                                                    p(guard), ctypes.byref(nfb))
    assert rc == _native.TC_OK and nfb.value == 0 and (guard == 0xA5).all()
    for name, n_none in (("tc_verify_decryption_share_records_rlc_batch", 12), ("tc_verify_decryption_share_records_prehashed_rlc_batch", 10)):
        nfb = ctypes.c_uint64(77)
        rc = getattr(lib, name)(eng._ctx, None, 0, *([None] * 4), *([None] * (n_none - 9)), 0, 0, None, None, ctypes.byref(nfb))   # M = 0
        assert rc == _native.TC_OK and nfb.value == 0
    # NULL pointers: the context, and each data pointer of a call that has records
    full = [p(case.pks), K, p(case.key_idx), p(case.shares), p(case.rec_off), p(case.u), p(case.flat), p(case.off), p(case.w), M, 2, SEED_A]
    fn = lib.tc_verify_decryption_share_records_rlc_batch
    assert fn(None, *full, p(guard), None) == _native.TC_ERR_INVALID_ARG
    for hole in (0, 3, 4, 5, 6, 7, 8, 11):                       # pks, shares, rec_off, u, v, off, w, seed32
        args = list(full)
        args[hole] = None
        assert fn(eng._ctx, *args, p(guard), None) == _native.TC_ERR_INVALID_ARG, hole
        assert (guard == 0xA5).all()
    assert fn(eng._ctx, *full, None, None) == _native.TC_ERR_INVALID_ARG                       # ok
    pre = [p(case.pks), K, p(case.key_idx), p(case.shares), p(case.rec_off), p(hashes), p(case.w), M, 2, SEED_A]
    fn = lib.tc_verify_decryption_share_records_prehashed_rlc_batch
    assert fn(None, *pre, p(guard), None) == _native.TC_ERR_INVALID_ARG
    for hole in (0, 3, 4, 5, 6, 9):                              # pks, shares, rec_off, hashes, w, seed32
        args = list(pre)
        args[hole] = None
        assert fn(eng._ctx, *args, p(guard), None) == _native.TC_ERR_INVALID_ARG, hole
        assert (guard == 0xA5).all()
    # ... and the full calls themselves are good (the guard is large enough: 5 records)
    nfb = ctypes.c_uint64(77)
    assert lib.tc_verify_decryption_share_records_rlc_batch(eng._ctx, *full, p(guard), ctypes.byref(nfb)) == _native.TC_OK
    assert guard[:5].tolist() == [1] * 5 and (guard[5:] == 0xA5).all() and nfb.value == 0
    guard[:] = 0xA5
    # a malformed offset array gets the answer a malformed `off` gets
    for broken in ([1, 2, 4, 5, 5, 5], [0, 2, 1, 3, 4, 5]):
        args = list(full)
        args[4] = p(np.array(broken, dtype=np.uint64))
        assert lib.tc_verify_decryption_share_records_rlc_batch(eng._ctx, *args, p(guard), None) == _native.TC_ERR_INVALID_ARG
        args = list(pre)
        args[4] = p(np.array(broken, dtype=np.uint64))
        assert lib.tc_verify_decryption_share_records_prehashed_rlc_batch(eng._ctx, *args, p(guard), None) == _native.TC_ERR_INVALID_ARG
        assert (guard == 0xA5).all()


# ---- 11: the typed interface -------------------------------------------------------------------------------------------------------
def test_public_key_share_verify_decryption_share_records_batch(world):
    """PublicKeyShare.verify_decryption_share_records_batch: per-ciphertext lists of (key share, decryption share) pairs, equal
    keys deduplicated into the table"""
    from threshold_crypto_amd import api
    case = Case(world, RAGGED)
    forged = case.rec(6, 1)
    case.shares[forged] = world.share[6, (int(case.key_idx[forged]) + 2) % K]
    want = case.expect()
    assert np.flatnonzero(want == 0).tolist() == [forged]
    keys = [api.PublicKeyShare(world.pks[i], _trusted=True) for i in range(K)]
    records = [[(keys[int(case.key_idx[r])] if r % 2 else api.PublicKeyShare(world.pks[int(case.key_idx[r])], _trusted=True),
                 api.DecryptionShare(case.shares[r], _trusted=True)) for r in case.records_of(m)] for m in range(case.M)]
    cts = [api.Ciphertext(case.u[m], case.v[m], case.w[m], _trusted=True) for m in range(case.M)]
    got = api.PublicKeyShare.verify_decryption_share_records_batch(records, cts, engine=world.engine, seed=SEED_A, group=3)
    assert [len(row) for row in got] == RAGGED
    assert [x for row in got for x in row] == [bool(x) for x in want]
    assert api.PublicKeyShare.verify_decryption_share_records_batch([[] for _ in cts], cts, engine=world.engine) == [[] for _ in cts]
    with pytest.raises(ValueError):
        api.PublicKeyShare.verify_decryption_share_records_batch(records[:-1], cts, engine=world.engine)
