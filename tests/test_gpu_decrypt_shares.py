"""Decryption shares of many key holders per ciphertext (tc_decrypt_shares_g1_batch, tc_decrypt_shares_batch) on the GPU, in both
forms: the per-ciphertext comb (csrc/tc_comb_g1.h, k_comb_tables_g1 + k_comb_decrypt; a context created with TC_COMB_G1_MIN="1,1"
and a table budget of three combs, so that a batch runs through many tiles with a short last one) and one arena ladder per share
(k_g1_mul_gather; a context whose thresholds nothing reaches).  Every share is compared byte for byte with tc_g1_mul_batch over ALL
holders, gathered -- a reference made once, itself checked against Oracle B -- and a sample of every case with Oracle B directly.
"""
import random

import numpy as np
import pytest

import c_oracle as c
import tc_oracle as o
from conftest import engine_with_env
from threshold_crypto_amd import _native, api
from threshold_crypto_amd.engine import pack_messages

pytestmark = pytest.mark.gpu

IDENT = bytes([0x40]) + bytes(95)
COMB_TABLE_BYTES = (64 * 8 + 2) * 128            # csrc/tc_comb_g1.h kCombG1TableWords * 4
BS = [1, 63, 64, 65, 130]
NS = [1, 7, 8, 9, 17, 68]
HUGE = 2 ** 63


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


@pytest.fixture(scope="module")
def rnd():
    return random.Random(20261020)


@pytest.fixture(scope="module")
def comb():
    with engine_with_env(TC_COMB_G1_MIN="1,1", TC_MSM_BUDGET=3 * COMB_TABLE_BYTES) as eng:
        yield eng


@pytest.fixture(scope="module")
def ladders():
    with engine_with_env(TC_COMB_G1_MIN="%d,%d" % (HUGE, HUGE)) as eng:
        yield eng


@pytest.fixture(scope="module", autouse=True)
def tidy_device_memory():
    """the device-resident cases leave tensors in torch's cache and in uncollected garbage: given back when the module ends, so
    that the modules after this one (some fill the HBM on purpose) find the memory where they expect it"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def forms(comb, ladders):
    return {"comb": comb, "ladders": ladders}


@pytest.fixture(scope="module")
def world(engine, rnd):
    """200 key shares (small scalars and r - 1 among the first ten), 130 points u of G1, and every product sk[i] * u[j] by
    tc_g1_mul_batch; four products per point checked against Oracle B here, more by the cases"""
    c.load()
    sk = [0, 1, 2, 3, 5, o.R - 1] + [rnd.randrange(o.R) for _ in range(194)]
    table = np.stack([u8(k.to_bytes(32, "little")) for k in sk])
    r = np.stack([u8(rnd.randrange(1, o.R).to_bytes(32, "little")) for _ in range(130)])
    u, st = engine.g1_mul(r, u8(o.g1_uncompressed(o.G1_GEN))[None])
    assert not st.any()
    u = np.ascontiguousarray(u.reshape(130, 96))
    full, st = engine.g1_mul(table, u)
    assert not st.any() and full.shape == (130, 200, 96)
    seen = {}

    def oracle(j, i):
        if (j, i) not in seen:
            rc, out = c.g1_mul(bytes(table[i]), bytes(u[j]))
            assert rc == 0
            seen[(j, i)] = out
        return seen[(j, i)]

    for j in range(130):
        for i in (j % 10, 10 + (7 * j) % 190, 199 - j, (3 * j) % 200):
            assert bytes(full[j, i]) == oracle(j, i), (j, i)
    return {"sk": sk, "table": table, "u": u, "full": full, "oracle": oracle}


def gathered(world, idx):
    B, n = idx.shape
    return world["full"][np.arange(B)[:, None], idx.astype(np.int64)]


def run_both_modes(eng, fn, *arrays):
    """fn(*arrays) with host buffers, then with device-resident ones: the same bytes"""
    import torch
    host = getattr(eng, fn)(*arrays)
    dev = getattr(eng, fn)(*[torch.from_numpy(a).cuda() for a in arrays])
    eng.sync()
    for h, d in zip(host, dev):
        assert (d.cpu().numpy() == h).all(), fn
    return host


# ---- 1. both forms against the full product and Oracle B ------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("form", ["comb", "ladders"])
def test_shares_equal_g1_mul_gathered_and_oracle_b(forms, world, form, B, n):
    eng = forms[form]
    rng = random.Random(1000 * B + n)
    for N in (10, 200):
        idx = np.array([[rng.randrange(N) for _ in range(n)] for _ in range(B)], dtype=np.uint64)      # repeats, any order
        idx[0] = np.array(sorted((int(i) for i in idx[0]), reverse=True), dtype=np.uint64)             # a descending row
        table = np.ascontiguousarray(world["table"][:N])
        u = np.ascontiguousarray(world["u"][:B])
        out, st = run_both_modes(eng, "decrypt_shares_g1", table, idx, u)
        assert out.shape == (B, n, 96) and st.shape == (B, n) and not st.any()
        assert (out == gathered(world, idx)).all(), (form, B, n, N)
        for j, k in {(0, 0), (B - 1, n - 1), (rng.randrange(B), rng.randrange(n))}:
            assert bytes(out[j, k]) == world["oracle"](j, int(idx[j, k])), (j, k)


# ---- 2. statuses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["comb", "ladders"])
def test_undecodable_u_fails_exactly_its_n_outputs(forms, world, form):
    eng, B, n, N = forms[form], 130, 9, 200
    rng = random.Random(5)
    idx = np.array([[rng.randrange(N) for _ in range(n)] for _ in range(B)], dtype=np.uint64)
    want = gathered(world, idx)
    for j_bad in (64, 90, 127, 0, 63):                           # first, middle and last lane of a wave of stage T
        u = world["u"][:B].copy()
        u[j_bad, 50] ^= 4                                        # not on the curve any more
        out, st = eng.decrypt_shares_g1(world["table"], idx, u)
        bad = np.zeros((B, n), bool)
        bad[j_bad] = True
        assert ((st == 3) == bad).all() and not st[~bad].any(), j_bad
        assert all(bytes(out[j_bad, k]) == IDENT for k in range(n))
        assert (out[~bad] == want[~bad]).all()


@pytest.mark.parametrize("form", ["comb", "ladders"])
def test_bad_index_and_bad_scalar_fail_one_output_each(forms, world, form):
    eng, B, n, N = forms[form], 65, 17, 200
    rng = random.Random(6)
    table = world["table"].copy()
    table[77] = u8(o.R.to_bytes(32, "little"))                    # a scalar >= r
    idx = np.array([[rng.choice([i for i in range(N) if i != 77]) for _ in range(n)] for _ in range(B)], dtype=np.uint64)
    idx[3, 5] = N                                                # just out of range
    idx[64, 16] = 2 ** 64 - 1
    idx[40, 0] = 77
    out, st = run_both_modes(eng, "decrypt_shares_g1", table, idx, np.ascontiguousarray(world["u"][:B]))
    bad = np.zeros((B, n), bool)
    bad[3, 5] = bad[64, 16] = bad[40, 0] = True
    assert ((st == 3) == bad).all() and not st[~bad].any()
    assert all(bytes(x) == IDENT for x in out[bad])
    safe = idx.copy()
    safe[bad] = 0
    assert (out[~bad] == gathered(world, safe)[~bad]).all()
    # the identity as u is a valid operand: identity shares
    u = world["u"][:B].copy()
    u[9] = u8(IDENT)
    out, st = eng.decrypt_shares_g1(world["table"], safe, u)
    assert not st.any() and all(bytes(out[9, k]) == IDENT for k in range(n))


def non_member_g1(rnd):
    while True:
        x = rnd.randrange(o.Q)
        y2 = (x * x * x + 4) % o.Q
        y = pow(y2, (o.Q + 1) // 4, o.Q)
        if y * y % o.Q == y2 and o.E1.mul((x, y), o.R) is not None:
            return (x, y)


@pytest.mark.parametrize("form", ["comb", "ladders"])
def test_u_outside_g1_is_rejected(forms, world, rnd, form):
    """u' = u1 + T with T of small order: rejected by tc_decrypt_shares_g1_batch in checked-input mode, and by
    tc_decrypt_shares_batch ALWAYS (the pairing check alone accepts it: e(T, H) = 1)"""
    eng = forms[form]
    sk = rnd.randrange(1, o.R)
    r_enc = rnd.randrange(1, o.R)
    v = bytes(rnd.randrange(256) for _ in range(24))
    T = o.E1.mul(non_member_g1(rnd), o.R)                        # the cofactor component of a random curve point
    assert T is not None
    u_bad = o.E1.add(o.E1.mul(o.G1_GEN, r_enc), T)
    u_good = o.E1.mul(o.G1_GEN, r_enc)
    u = np.stack([u8(o.g1_uncompressed(u_bad)), u8(o.g1_uncompressed(u_good))])
    w = np.stack([u8(o.g2_uncompressed(o.E2.mul(o.hash_g1_g2(p, v), r_enc))) for p in (u_bad, u_good)])
    flat, off = pack_messages([v, v])
    table = np.stack([u8(sk.to_bytes(32, "little")), u8((sk + 1).to_bytes(32, "little"))])
    idx = np.array([[1, 0, 1], [0, 1, 1]], dtype=np.uint64)
    good_row = [o.g1_uncompressed(o.E1.mul(u_good, (sk + int(i)) % o.R)) for i in idx[1]]
    was = eng.input_checks()
    try:
        eng.set_input_checks(True)
        out, st = eng.decrypt_shares_g1(table, idx, u)
        assert st.tolist() == [[3, 3, 3], [0, 0, 0]] and all(bytes(x) == IDENT for x in out[0])
        assert [bytes(x) for x in out[1]] == good_row
        for checks in (False, True):
            eng.set_input_checks(checks)
            out, ok, st = eng.decrypt_shares(table, idx, u, flat, off, w)
            assert ok.tolist() == [0, 1] and all(bytes(x) == IDENT for x in out[0]) and st[0].tolist() == [3, 3, 3]
            assert [bytes(x) for x in out[1]] == good_row and not st[1].any()
    finally:
        eng.set_input_checks(was)


# ---- 3. tc_decrypt_shares_batch --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ciphertexts(engine, rnd):
    """10 key shares of a degree-3 key set, 16 ciphertexts of ragged length under its public key, and the shares of every
    holder by tc_decrypt_share_batch (one call per holder); ciphertext 5 has a tampered w, 11 a flipped byte of v"""
    t, N, B = 3, 10, 16
    sks = api.SecretKeySet([rnd.randrange(o.R) for _ in range(t + 1)])
    pks = sks.public_keys(engine=engine)
    msgs = [bytes(rnd.randrange(256) for _ in range(1 + j % 9)) for j in range(B)]
    cts = pks.public_key().encrypt_with_r_batch([rnd.randrange(1, o.R) for _ in range(B)], msgs, engine=engine)
    shares = [sks.secret_key_share(i) for i in range(N)]
    table = np.stack([u8(s._bytes()) for s in shares])
    u = np.stack([u8(ct.u) for ct in cts])
    w = np.stack([u8(ct.w) for ct in cts])
    flat, off = pack_messages([ct.v for ct in cts])
    w[5] = w[6]
    flat[int(off[11])] ^= 1
    per_holder = [engine.decrypt_share(table[i], u, flat, off, w) for i in range(N)]
    return {"t": t, "N": N, "B": B, "sks": sks, "pks": pks, "msgs": msgs, "cts": cts, "shares": shares, "table": table, "u": u, "w": w,
            "flat": flat, "off": off, "per_holder": per_holder}


@pytest.mark.parametrize("n", [1, 4, 9])
@pytest.mark.parametrize("form", ["comb", "ladders"])
def test_verified_shares_equal_n_calls_of_decrypt_share(forms, ciphertexts, form, n):
    eng, cw = forms[form], ciphertexts
    rng = random.Random(n)
    idx = np.array([rng.sample(range(cw["N"]), n) for _ in range(cw["B"])], dtype=np.uint64)
    out, ok, st = run_both_modes(eng, "decrypt_shares", cw["table"], idx, cw["u"], cw["flat"], cw["off"], cw["w"])
    assert ok.tolist() == [0 if j in (5, 11) else 1 for j in range(cw["B"])]
    for j in range(cw["B"]):
        for k in range(n):
            ref_share, ref_ok = cw["per_holder"][int(idx[j, k])]
            assert ref_ok[j] == ok[j] and bytes(out[j, k]) == bytes(ref_share[j]), (j, k)
            assert st[j, k] == (0 if ok[j] else 3)
    assert all(bytes(out[5, k]) == IDENT and bytes(out[11, k]) == IDENT for k in range(n))


@pytest.mark.parametrize("comb_min", ["1,1", "%d,%d" % (HUGE, HUGE)], ids=["comb", "ladders"])
def test_threshold_enc_example_through_the_python_api(engine, comb_min):
    """examples/threshold_enc.rs with t = 3, N = 10 and 16 ciphertexts: encrypt, the decryption shares of t + 1 of the N holders
    (decrypt_shares_batch), every share verified against its holder's public key share, the plaintext recovered by
    PublicKeySet::decrypt; a ciphertext with a tampered w gets no shares"""
    rnd = random.Random(3)
    t, N, B = 3, 10, 16
    sks = api.SecretKeySet([rnd.randrange(o.R) for _ in range(t + 1)])
    pks = sks.public_keys(engine=engine)
    msgs = [bytes(rnd.randrange(256) for _ in range(1 + j % 9)) for j in range(B)]
    cts = pks.public_key().encrypt_with_r_batch([rnd.randrange(1, o.R) for _ in range(B)], msgs, engine=engine)
    shares = [sks.secret_key_share(i) for i in range(N)]
    holders = [8, 1, 6, 3]                                        # t + 1 = 4 of N = 10
    with engine_with_env(TC_COMB_G1_MIN=comb_min) as eng:
        rows = api.decrypt_shares_batch([shares[i] for i in holders], cts + [api.Ciphertext(cts[5].u, cts[5].v, cts[6].w, _trusted=True)], engine=eng)
        assert rows[-1] is None and all(r is not None and len(r) == 4 for r in rows[:-1])
        rows = rows[:-1]
        pk_shares = pks.public_key_shares(holders, engine=eng)
        ok = api.PublicKeyShare.verify_decryption_share_batch([pk_shares[k] for _ in cts for k in range(4)], [r[k] for r in rows for k in range(4)],
                                                              [ct for ct in cts for _ in range(4)], engine=eng)
        assert ok.all()
        plain, st = pks.decrypt_batch([{holders[k]: r[k] for k in range(4)} for r in rows], cts, engine=eng)
        assert not np.asarray(st).any() and plain == msgs


# ---- 4. degenerate calls -----------------------------------------------------------------------------------------------------
def test_empty_calls_and_a_null_context(engine, world):
    lib = _native.load()
    assert lib.tc_decrypt_shares_g1_batch(engine._ctx, None, 0, None, None, 0, 5, None, None) == _native.TC_OK
    assert lib.tc_decrypt_shares_g1_batch(engine._ctx, None, 0, None, None, 5, 0, None, None) == _native.TC_OK
    assert lib.tc_decrypt_shares_batch(engine._ctx, None, 0, None, None, None, None, None, 0, 5, None, None, None) == _native.TC_OK
    assert lib.tc_decrypt_shares_batch(engine._ctx, None, 0, None, None, None, None, None, 5, 0, None, None, None) == _native.TC_OK
    assert lib.tc_decrypt_shares_g1_batch(None, None, 0, None, None, 0, 0, None, None) == _native.TC_ERR_INVALID_ARG
    assert lib.tc_decrypt_shares_batch(None, None, 0, None, None, None, None, None, 0, 0, None, None, None) == _native.TC_ERR_INVALID_ARG
    # a non-empty call with a missing operand is refused, not run
    assert lib.tc_decrypt_shares_g1_batch(engine._ctx, None, 10, None, None, 2, 2, None, None) == _native.TC_ERR_INVALID_ARG


def test_the_default_context_takes_the_ladders_below_its_thresholds(engine, world):
    """a context without the hook: a small batch runs (whatever form the constants choose) and gives the same bytes"""
    idx = np.array([[3, 199, 0, 7], [1, 1, 5, 150]], dtype=np.uint64)
    out, st = engine.decrypt_shares_g1(world["table"], idx, np.ascontiguousarray(world["u"][:2]))
    assert not st.any() and (out == gathered(world, idx)).all()
