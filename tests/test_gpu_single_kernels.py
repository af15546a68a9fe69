"""GPU leg of the single-point kernel conformance suite (tests/single_conformance.py): the shipped kernels of k_mul.hip,
k_hash.hip, k_check.hip and k_robust.hip, launched by tests/device/single_kernels.hip and single_kernels_mul.hip through the
product's launchers -- and directly wherever a launcher derives a geometry -- over the case tables the host leg has proven
(tests/test_single_kernels_host.py).

Per run everything a kernel left in memory comes back and is compared exactly: outputs and statuses against the oracle or the
restatement of the header comment, the guard row / byte / entry behind every buffer, the buffer a null pointer leaves alone, and
the host leg's bytes wherever a host entry exists.  Every entry that uses the table arena fails unless all slot flags are clear
afterwards.  After one HIP error nothing more is launched."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import single_conformance as sc  # noqa: E402

pytestmark = pytest.mark.gpu

_state = {"lib": None, "host": None, "hip_error": None}


@pytest.fixture(scope="module")
def lib():
    if _state["lib"] is None:
        _state["lib"] = sc.load(sc.build_device(), "sk_")
    return _state["lib"]


@pytest.fixture(scope="module")
def host():
    if _state["host"] is None:
        _state["host"] = sc.load(sc.build_host(), "skh_")
    return _state["host"]


def _launch(fn, *args, **kw):
    if _state["hip_error"]:
        pytest.fail("not launched after an earlier HIP error: %s" % _state["hip_error"])
    try:
        return fn(*args, **kw)
    except sc.HipError as e:
        _state["hip_error"] = str(e)
        raise


def _ok(bad):
    assert not bad, "\n".join(bad[:12])


# ---- block 1: k_mul.hip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("S,B", sc.MUL_SHAPES)
def test_point_mul(lib, host, w, S, B):
    """k_point_mul<Fq>, k_g1_mul_arena and the launcher's choice (G1), k_point_mul<Fq2> and the launcher's choice (G2; the shared
    form when S > 1), status given and null: the oracle's products, the same bytes from every kernel, the host leg's bytes.  A bad
    scalar fails its column and a bad point its row, each first and last; with S B = 65 and 130 the surplus lanes of the arena
    kernel multiply job 0 again -- the undecodable point or the non-canonical scalar in two of the variants -- and leave the live
    results, the guard row and the slot flags alone."""
    for variant in sc.mul_variants(S, B):
        case = sc.mul_case(w, S, B, variant)
        first = sc.run_mul(host, case, sc.MUL_KERNELS[w][1])
        for kernel in sc.MUL_KERNELS[w]:
            res = _launch(sc.run_mul, lib, case, kernel)
            _ok(sc.check_mul(case, 1, res))
            assert sc.same(res, first), "%s kernel %d: not the host leg's bytes" % (case.tag, kernel)
    for kernel in sc.MUL_KERNELS[w]:
        _ok(sc.check_mul(case, 0, _launch(sc.run_mul, lib, case, kernel, 0)))


@pytest.mark.parametrize("S", sc.SHARED_S)
def test_g2_mul_shared(lib, host, S):
    """B = 1, 7, 33; a scalar 0, a non-canonical and a proper one at each of a chunk's four positions (identities first, last and in
    the middle of the shared inversion); a bad point fails exactly its S outputs; the status bytes are per scalar."""
    for B in sc.SHARED_B:
        for rot in range(3):
            case = sc.shared_case(S, B, rot)
            res = _launch(sc.run_mul, lib, case, 5)
            _ok(sc.check_mul(case, 1, res))
            assert sc.same(res, sc.run_mul(host, case, 5)), "%s: not the host leg's bytes" % case.tag
            assert sc.same(res, _launch(sc.run_mul, lib, case, 3)), "%s: the launcher's kernel leaves other bytes" % case.tag
    _ok(sc.check_mul(case, 0, _launch(sc.run_mul, lib, case, 5, 0)))
    assert sc.same(res, _launch(sc.run_mul, lib, case, 4)), "%s: not the bytes of k_point_mul<Fq2>" % case.tag


@pytest.mark.parametrize("n,B", sc.GATHER_SHAPES)
def test_g2_mul_gather(lib, host, n, B):
    """share = 1 .. 8 by direct launch and 0 through the launcher: the same bytes every time."""
    case = sc.gather_case(n, B)
    first = sc.run_gather(host, case, 1)
    for share in sc.GATHER_SHARES:
        res = _launch(sc.run_gather, lib, case, share)
        _ok(sc.check_gather(case, share, 1, res))
        assert sc.same(res, first), "%s: share = %d does not leave the host leg's bytes" % (case.tag, share)
    _ok(sc.check_gather(case, 3, 0, _launch(sc.run_gather, lib, case, 3, 0)))


@pytest.mark.parametrize("g", [1, 2])
def test_codecs(lib, host, g):
    """k_compress, k_decompress and k_decompress_g2_x2 at B = 1, 2, 63, 65 over the shared table of encodings (x >= q, a missing
    flag, a non-square, a non-member, the identity, the other root), malformed entries in slot a, in slot b and in the odd tail."""
    for B in sc.CODEC_B:
        for shift in (0, 1):
            for tail in (sc.CODEC_TAILS if B % 2 else [None]):
                ins = sc.codec_inputs(g, "comp", B, shift, tail)
                want = sc.codec_want(g, "comp", ins)
                ref = sc.run_decompress(host, g, 1, ins)
                for form in ((0, 1, 2) if g == 2 else (0, 1)):
                    res = _launch(sc.run_decompress, lib, g, form, ins)
                    _ok(sc.check_points("decompress G%d form %d B=%d shift=%d tail=%s" % (g, form, B, shift, tail), g, want, 1, res))
                    assert sc.same(res, ref), "decompress G%d form %d B=%d shift=%d tail=%s: not the host leg's bytes" % (g, form, B, shift, tail)
            ins_u = sc.codec_inputs(g, "unc", B, shift)
            want_u = sc.codec_want(g, "unc", ins_u)
            res = _launch(sc.run_compress, lib, g, ins_u)
            _ok(sc.check_points("compress G%d B=%d shift=%d" % (g, B, shift), g, want_u, 1, res))
            assert sc.same(res, sc.run_compress(host, g, ins_u))
    _ok(sc.check_points("compress, null status", g, want_u, 0, _launch(sc.run_compress, lib, g, ins_u, 0)))
    for form in ((1, 2) if g == 2 else (1,)):
        _ok(sc.check_points("decompress, null status", g, want, 0, _launch(sc.run_decompress, lib, g, form, ins, 0)))


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("npj,take", sc.TAKE_SHAPES)
def test_decompress_take(lib, host, g, npj, take):
    """B = 1, 7, 43: n is odd and pairs straddle jobs; the samples behind `take` hold garbage and change nothing; k_take_u64 over
    the same shapes."""
    for B in sc.TAKE_B:
        ref = sc.run_take(host, g, 1, npj, take, B)
        for form in ((0, 1, 2) if g == 2 else (0, 1)):
            res = _launch(sc.run_take, lib, g, form, npj, take, B)
            _ok(sc.check_take(g, npj, take, B, res))
            assert sc.same(res, ref), "take G%d form %d (%d, %d) B=%d: not the host leg's bytes" % (g, form, npj, take, B)
        if g == 1:
            _ok(_launch(sc.run_take_u64, lib, npj, take, B))


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("jobs", sorted(sc.SELECTED_JOBS))
def test_decompress_selected(lib, host, g, jobs):
    """N = 7, need = 3; jobs without enough shares first, last and in the middle, so that a pair has no source in a, in b or in both;
    an on-curve non-member decodes (the decode is curve-level); the malformed table."""
    for lacking in ([sc.SELECTED_JOBS[jobs]] + ([[0]] if jobs == 1 else [])):
        case = sc.SelectedCase(g, jobs, lacking)
        ref = sc.run_selected(host, case, 1)
        for form in ((0, 1, 2) if g == 2 else (0, 1)):
            res = _launch(sc.run_selected, lib, case, form)
            _ok(sc.check_selected(case, res))
            assert sc.same(res, ref), "%s form %d: not the host leg's bytes" % (case.tag, form)


def test_small_kernels(lib, host):
    """k_fr_scale_cofactor_fix (a non-canonical input gives all ones), k_g1_scale_cofactor_fix (strides 96 and 0, an undecodable
    input passed through, the identity), k_fill_g1_generator (both outputs against the oracle)."""
    for what, data, stride, n, want in sc.small_cases():
        out = _launch(sc.run_small, lib, what, data, stride, n)
        _ok(sc.check_small(what, n, want, out))
        assert (out == sc.run_small(host, what, data, stride, n)).all()
    out = _launch(sc.run_small, lib, 2, b"", 0, 0)
    g, unfix = sc.generator_want()
    assert bytes(out[:96]) == g and bytes(out[192:288]) == unfix and sc.is_poison(out[96:192]) and sc.is_poison(out[288:])


# ---- block 2: k_check.hip and k_robust.hip --------------------------------------------------------------------------------
@pytest.mark.parametrize("g1", [0, 1])
@pytest.mark.parametrize("seed", [0, 1])
def test_rlc_scalars(lib, g1, seed):
    """n = 1, 64, 65, 130: every row against the restatement over the oracle's ChaCha20 (key = seed, block counter = i, the first
    two words), the low digit odd, the value below 2^208 / below r, all n values distinct, the guard row as filled."""
    for n in sc.RLC_NS:
        _ok(sc.check_rlc(g1, sc.RLC_SEEDS[seed], n, _launch(sc.run_rlc, lib, g1, sc.RLC_SEEDS[seed], n)))


@pytest.mark.parametrize("g", [1, 2])
def test_subgroup_check(lib, host, g):
    for npj, take in sc.SUBGROUP_SHAPES:
        for n in sc.SUBGROUP_NS:
            res = _launch(sc.run_subgroup, lib, g, npj, take, n, 8 * (n % 2))
            _ok(sc.check_subgroup("subgroup G%d (%d, %d) n=%d" % (g, npj, take, n), res))
            assert (res[0] == sc.run_subgroup(host, g, npj, take, n, 8 * (n % 2))[0]).all()


def test_invalidate_jobs(lib):
    """per_job = 1 and 3, group = 0 (the launcher makes it 1), 1, 4 and (size_t)-1, B = 1, 65, 130; a status that is already not OK
    keeps its value; status, ok and out null in turn; out_bytes = 96, 192, 48 and 0.

    The callers in tc_api.hip pass today: out_bytes = 96 or 192 together with `out` -- the uncompressed width of the call's point
    output, written as a literal or as PB: G1 products, shares and evaluations, G2 products, shares and hash points, the
    combinations -- and 0 together with a null `out` (the boolean entries, which pass `ok`, and the status-only pass in front of
    the keystream kernel).  96 and 192 give the uncompressed identity (0x40, then zeros), pinned here; any other width is zeroed and
    nothing else, pinned at 48 and 0.  So 96 is ALWAYS read as uncompressed G1: a compressed G2 identity, 96 bytes too, would be
    0xC0 and zeros, and a compressed G1 one (48 bytes) 0xC0 as well; no caller passes a compressed output."""
    for case in sc.invalidate_cases():
        got, want = _launch(sc.run_invalidate, lib, *case)
        _ok(sc.check_invalidate("invalidate %s" % (case,), case[2], case[3], got, want))
    got, want = _launch(sc.run_invalidate, lib, 1, 1, 65, 96, None)
    assert any(want[1][j * 96] == 0x40 and not any(want[1][j * 96 + 1:(j + 1) * 96]) for j in range(65))
    got, want = _launch(sc.run_invalidate, lib, 1, 1, 65, 48, None)
    assert any(not any(want[1][j * 48:(j + 1) * 48]) for j in range(65)) and bytes(got[1][:65 * 48]) == bytes(want[1])


def test_byte_movers(lib):
    """k_ok_and_status; k_gather_rows with rows of 8, 96 and 192 bytes and repeated map entries; k_scatter_bytes; k_gather_bytes."""
    _ok(_launch(sc.run_movers, lib))


@pytest.mark.parametrize("N", sc.SELECT_NS)
def test_select_shares(lib, host, N):
    """need = 1, 3 and N; jobs = 1, 65, 130; present and bad each null or given, at the same and at different offsets from an
    8-byte boundary (select_first's word path and its bytewise path on the device); map null and a permutation; used null and
    given.  Per job: the selected slots, the fill N + k / 0xffffffff behind count, enough, used untouched without enough, the guards;
    and the host leg's bytes."""
    for need in sorted({1, min(3, N), N}):
        for jobs in sc.SELECT_JOBS:
            for modes in sc.select_modes(need, jobs):
                res, inputs = _launch(sc.run_select, lib, N, need, jobs, *modes)
                _ok(sc.check_select("select N=%d need=%d jobs=%d modes %s" % (N, need, jobs, modes), N, need, jobs, res, inputs)[0])
                ref, _ = sc.run_select(host, N, need, jobs, *modes)
                assert all(a is None or (a == b).all() for a, b in zip(res, ref))


@pytest.mark.parametrize("point_bytes", [96, 192])
def test_gather_selected(lib, point_bytes):
    """The uint4 form and the uint2 form, each by direct launch and through the launcher: shares or dst 8 bytes behind a 16-byte
    boundary makes the launcher take the 8-byte words.  Jobs without enough shares get identities.  The same rows every time."""
    for jobs in (1, 22):
        for form, off_s, off_d in sc.GATHER_SELECTED_FORMS:
            bad, dst = _launch(sc.run_gather_selected, lib, point_bytes, jobs, form, off_s, off_d)
            _ok(bad)


def test_robust_mark(lib):
    for rows_ in (1, 70, 130):
        for modes in sc.MARK_MODES:
            _ok(_launch(sc.run_mark, lib, rows_, *modes))


@pytest.mark.parametrize("N,point_bytes", [(5, 96), (200, 192), (5, 192), (200, 96)])
def test_robust_finish(lib, N, point_bytes):
    """The whole truth table (enough, st, ok, member with a zero first or last) over 72 jobs, ok / member / map / used / verdict each
    null in turn; N = 5 is below row_words and N = 200 above it, so the strided clear of `used` covers every byte once: the status
    codes, the verdicts, the identity for failed jobs, rows of the caller that no job maps to untouched."""
    for modes in sc.finish_modes():
        _ok(_launch(sc.run_finish, lib, N, point_bytes, *modes))


# ---- block 3: k_hash.hip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_g1", [0, 1])
def test_hashes(lib, host, with_g1):
    """k_hash_g2 / _x2 and k_hash_g1_g2 / _x2 at B = 1, 2, 63, 65, message lengths 0 .. 300 dealt so that the two messages of a pair
    differ widely, fix = 0 and 1, an undecodable G1 operand in slot a, in slot b and in the odd tail: the _x2 bytes equal the
    one-job bytes, which equal the oracle's."""
    for B in sc.HASH_B:
        for fix in (1, 0):
            for bad_at in sc.hash_bad_ats(B, with_g1):
                g1, msgs = sc.hash_case(B, with_g1, bad_at)
                ref = sc.run_hash(host, g1, msgs, fix, 1)
                for form in (0, 1, 2):
                    res = _launch(sc.run_hash, lib, g1, msgs, fix, form)
                    _ok(sc.check_hash("hash g1=%d form %d B=%d fix=%d bad_at=%s" % (with_g1, form, B, fix, bad_at), g1, msgs, fix, 1, res))
                    assert sc.same(res, ref), "hash g1=%d form %d B=%d fix=%d bad_at=%s: not the host leg's bytes" % (with_g1, form, B, fix, bad_at)
    for form in (1, 2):
        _ok(sc.check_hash("null status", g1, msgs, fix, 0, _launch(sc.run_hash, lib, g1, msgs, fix, form, 0)))


def test_xor_with_hash_and_encrypt(lib):
    """k_xor_with_hash: lengths 0, 1, 63, 64, 65 and 200 side by side in one wave, pre-flagged jobs keep their status and leave
    their output bytes as filled, a null status.  k_encrypt: pk_stride 0 and 96, ragged lengths, a non-canonical r and a bad pk give
    an identity u, an identity w and exactly len zero bytes of v."""
    for with_status in (1, 0):
        _ok(_launch(sc.run_xor, lib, 70, with_status))
    _ok(_launch(sc.run_xor, lib, 1, 1))
    for pk_stride in (0, 96):
        _ok(_launch(sc.run_encrypt, lib, 9, pk_stride))
    _ok(_launch(sc.run_encrypt, lib, 70, 96))
    _ok(_launch(sc.run_encrypt, lib, 1, 96, 0))


@pytest.mark.parametrize("t", sc.EVAL_TS)
def test_commitment_evaluate(lib, host, t):
    """t = 0, 1, 2, 7; idx = 0, 1, 2^63, 2^64 - 2 and 2^64 - 1 (x = 0: INVALID); identity coefficients; an off-curve coefficient at
    the top and further down; a Horner step whose acc equals the next coefficient and one whose acc equals its negative; M = 1 and
    70, against the oracle's Commitment::evaluate."""
    for m, tag in sc.eval_commits(t):
        for M in ((1, 70) if tag == "random" else (10,)):
            idxs = sc.eval_idxs(M)
            want = [sc.eval_want(m, i) for i in idxs]
            res = _launch(sc.run_eval, lib, m, t, idxs)
            _ok(sc.check_points("evaluate t=%d %s M=%d" % (t, tag, M), 1, want, 1, res))
            assert sc.same(res, sc.run_eval(host, m, t, idxs)), "evaluate t=%d %s: not the host leg's bytes" % (t, tag)
    _ok(sc.check_points("evaluate, null status", 1, want, 0, _launch(sc.run_eval, lib, m, t, idxs, 0)))
