"""Host leg of the single-point kernel conformance suite (tests/single_conformance.py): proves the case tables, the models and the
checkers on tests/device/single_kernels_host.cpp (the header routines of tc_jobs.h / tc_robust.h under g++ -DTC_BOUND_CHECK, each
kernel's index map as a plain loop) before any GPU time is spent.  The GPU leg (tests/test_gpu_single_kernels.py) runs the same
tables through the shipped kernels.

(a) the stand-alone program of the host leg passes, and runs clean under ASan and UBSan; (b) the models state what they claim;
(c) the host leg passes every checker over the case tables; (d) every checker notices a spoiled buffer.  The kernels whose body
lives in the __global__ function have no host entry: their restatements are checked against a transcription of the kernel text
lane by lane (single_conformance.KernelText), which also shows that the checkers notice the faults the issue names."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import single_conformance as sc  # noqa: E402

o, R = sc.o, sc.R


@pytest.fixture(scope="module")
def host():
    return sc.load(sc.build_host(), "skh_")


@pytest.fixture(scope="module")
def text():
    return sc.KernelText()


def _ok(bad):
    assert not bad, "\n".join(bad[:12])


def _spoiled(check, res, index, *args, at=3):
    """The checker must notice one flipped byte in buffer `index` of a passing result."""
    res = list(res)
    buf = res[index].copy()
    flat = buf.view(np.uint8).reshape(-1)
    flat[min(len(flat) - 1, at)] ^= 0x10
    res[index] = buf
    assert check(*args, tuple(res)), "a spoiled buffer %d went unnoticed" % index


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_of_the_host_leg_passes():
    r = subprocess.run([sc.build_host_main()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_stand_alone_program_runs_clean_under_asan_and_ubsan():
    exe = sc.build_host_main(["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- (b) the models -------------------------------------------------------------------------------------------------------
def test_rlc_restatement_has_the_properties_the_soundness_argument_uses():
    """Odd low digit, below 2^208 / below r, pairwise distinct, the digits recoverable in base |x| (G2 form) and in base x^2 (G1
    form); two seeds and two counters never give the same row."""
    for seed in sc.RLC_SEEDS:
        g2 = [sc.rlc_model(0, seed, i) for i in range(130)]
        g1 = [sc.rlc_model(1, seed, i) for i in range(130)]
        assert all(v & 1 and v < 1 << 208 for v in g2) and all(v & 1 and v < R for v in g1)
        assert len(set(g2)) == 130 and len(set(g1)) == 130
        for v in g2:
            d = [(v // sc.X ** k) % sc.X for k in range(4)]
            assert all(x < 1 << 16 for x in d) and d[0] & 1
        assert all(v % sc.X2 < 1 << 32 and v // sc.X2 < 1 << 32 for v in g1)
    assert sc.rlc_model(0, sc.RLC_SEEDS[0], 5) != sc.rlc_model(0, sc.RLC_SEEDS[1], 5)
    assert sc.X == 0xd201000000010000 and sc.X2 == sc.X * sc.X


def test_case_tables_hold_what_the_issue_names():
    assert sc.MUL_SHAPES == [(1, 1), (1, 70), (3, 33), (5, 13), (2, 65)] and sc.EDGE_SCALARS == [0, 1, R - 1, R, (1 << 256) - 1]
    # the shared form: every position of a chunk sees a zero, a non-canonical and a proper scalar over the three rotations
    for S in sc.SHARED_S:
        kinds = [{(0 if k == 0 else 1 if k >= R else 2) for k in (sc.shared_case(S, 7, rot).scalars[s] for rot in range(3))} for s in range(S)]
        assert all(k == {0, 1, 2} for k in kinds)
    assert sc.shared_case(5, 7, 1).mults[6] is None and sc.shared_case(5, 7, 0).mults.count(None) == 0
    # the gather: an index >= N first, in the middle and last in a row; a zero and a non-canonical key that the rows reach
    c = sc.gather_case(9, 70)
    assert {next((p for p, i in enumerate(row) if i >= c.N), None) for row in c.idx} == {0, 4, 8, None}
    reached = {i for row in c.idx for i in row if i < c.N}
    assert c.keys.index(0) in reached and c.keys.index(R) in reached and None in c.msgs and 0 in c.msgs
    # the selected decode: pairs without a source in a, in b and in both, and the tail
    for jobs, lacking in sc.SELECTED_JOBS.items():
        case = sc.SelectedCase(2, jobs, lacking)
        n = jobs * sc.SEL_NEED
        src = [bool(case.enough[i // sc.SEL_NEED]) for i in range(n)]
        pairs = {(src[i], src[i + 1]) for i in range(0, n - 1, 2)}
        if jobs > 1:
            assert pairs == {(True, True), (True, False), (False, True), (False, False)}, (jobs, pairs)
        assert case.nonmember_record is not None and case.want()[case.nonmember_record][1] == 1
        assert sc.codec_ref(2, "comp", case.shares[min(jobs - 1, 1) * sc.SEL_N + 2])[0] is False  # the checked decode rejects it
    assert 22 * 3 == 66 and (66 + 1) // 2 * 2 > 64  # 33 pairs: one of them in a second wave
    # the take shapes: n = B take is odd somewhere, and a pair straddles two jobs
    assert any((B * take) % 2 for _, take in sc.TAKE_SHAPES for B in sc.TAKE_B) and any(take % 2 for _, take in sc.TAKE_SHAPES)
    # hash: the two messages of a pair differ widely
    assert set(sc.HASH_DEAL) == set(sc.HASH_LENS) and abs(sc.HASH_DEAL[0] - sc.HASH_DEAL[1]) == 300
    # Horner events of the directed commitments at x = 2
    for t in (1, 2, 7):
        ev = {tag: sc.dk.horner(m, 2)[1] for m, tag in sc.eval_commits(t) if None not in m}
        assert "double" in ev["acc == c at x = 2"] and "cancel" in ev["acc == -c at x = 2"]
        if t >= 2:
            assert "double" in ev["acc == c at the second step, x = 2"]
    assert sc.eval_want([5, 7], (1 << 64) - 1) == (sc.IDENT[1], sc.INVALID)
    # the multiples model of the evaluation is the oracle's Commitment::evaluate
    m = sc.eval_commits(2)[0][0]
    for idx in (0, 1, 1 << 63, (1 << 64) - 2):
        assert sc.eval_want(m, idx)[0] == sc.enc(1, o.commitment_evaluate([sc.gmul(1, c) for c in m], idx + 1))


# ---- (c), (d): the host leg over the case tables --------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("S,B", sc.MUL_SHAPES)
def test_point_mul(host, w, S, B):
    """The register form, the arena form and the launcher's choice leave the same bytes, and those are the oracle's."""
    for variant in sc.mul_variants(S, B):
        case = sc.mul_case(w, S, B, variant)
        first = None
        for kernel in sc.MUL_KERNELS[w]:
            res = sc.run_mul(host, case, kernel)
            _ok(sc.check_mul(case, 1, res))
            first = first or res
            assert sc.same(res, first), case.tag
        _ok(sc.check_mul(case, 0, sc.run_mul(host, case, sc.MUL_KERNELS[w][1], 0)))
    _spoiled(sc.check_mul, first, 0, case, 1)
    _spoiled(sc.check_mul, first, 1, case, 1)
    _spoiled(sc.check_mul, first, 0, case, 1, at=S * B * sc.PB[w] + 5)  # the guard row


@pytest.mark.parametrize("S", sc.SHARED_S)
def test_g2_mul_shared(host, S):
    for B in sc.SHARED_B:
        for rot in range(3):
            case = sc.shared_case(S, B, rot)
            res = sc.run_mul(host, case, 5)
            _ok(sc.check_mul(case, 1, res))
            assert sc.same(res, sc.run_mul(host, case, 4)), "%s: not the bytes of k_point_mul<Fq2>" % case.tag
    _ok(sc.check_mul(case, 0, sc.run_mul(host, case, 5, 0)))


@pytest.mark.parametrize("n,B", sc.GATHER_SHAPES)
def test_g2_mul_gather(host, n, B):
    case = sc.gather_case(n, B)
    first = None
    for share in (sc.GATHER_SHARES[:-1] if B <= 8 else (1, 3, 8)):
        res = sc.run_gather(host, case, share)
        _ok(sc.check_gather(case, share, 1, res))
        first = first or res
        assert sc.same(res, first), "%s: share = %d leaves other bytes" % (case.tag, share)
    _ok(sc.check_gather(case, 3, 0, sc.run_gather(host, case, 3, 0)))
    _spoiled(sc.check_gather, first, 0, case, 1, 1, at=200)


@pytest.mark.parametrize("g", [1, 2])
def test_codecs(host, g):
    """k_compress and k_decompress over the shared table of encodings, malformed entries in slot a, in slot b and in the odd
    tail; the two-jobs form leaves the one-job bytes."""
    for B in sc.CODEC_B:
        for shift in (0, 1):
            for tail in (sc.CODEC_TAILS if B % 2 else [None]):
                ins = sc.codec_inputs(g, "comp", B, shift, tail)
                want = sc.codec_want(g, "comp", ins)
                res = sc.run_decompress(host, g, 1, ins)
                _ok(sc.check_points("decompress G%d B=%d shift=%d tail=%s" % (g, B, shift, tail), g, want, 1, res))
                if g == 2:
                    assert sc.same(res, sc.run_decompress(host, g, 2, ins)), "the _x2 bytes differ (B=%d shift=%d tail=%s)" % (B, shift, tail)
            ins = sc.codec_inputs(g, "unc", B, shift)
            want = sc.codec_want(g, "unc", ins)
            _ok(sc.check_points("compress G%d B=%d" % (g, B), g, want, 1, sc.run_compress(host, g, ins)))
    _ok(sc.check_points("compress, null status", g, want, 0, sc.run_compress(host, g, ins, 0)))
    ins = sc.codec_inputs(g, "comp", 65, 0)
    _ok(sc.check_points("decompress, null status", g, sc.codec_want(g, "comp", ins), 0, sc.run_decompress(host, g, g, ins, 0)))


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("npj,take", sc.TAKE_SHAPES)
def test_decompress_take(host, g, npj, take):
    for B in sc.TAKE_B:
        res = sc.run_take(host, g, 1, npj, take, B)
        _ok(sc.check_take(g, npj, take, B, res))
        if g == 2:
            assert sc.same(res, sc.run_take(host, g, 2, npj, take, B)), "the _x2 bytes differ"
    _spoiled(lambda r: sc.check_take(g, npj, take, B, r), res, 1, at=B * take - 1)


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("jobs", sorted(sc.SELECTED_JOBS))
def test_decompress_selected(host, g, jobs):
    for lacking in ([sc.SELECTED_JOBS[jobs]] + ([[0]] if jobs == 1 else [])):
        case = sc.SelectedCase(g, jobs, lacking)
        res = sc.run_selected(host, case, 1)
        _ok(sc.check_selected(case, res))
        if g == 2:
            assert sc.same(res, sc.run_selected(host, case, 2)), "%s: the _x2 bytes differ" % case.tag
    _spoiled(sc.check_selected, res, 1, case, at=0)


def test_small_kernels(host):
    for what, data, stride, n, want in sc.small_cases():
        _ok(sc.check_small(what, n, want, sc.run_small(host, what, data, stride, n)))


@pytest.mark.parametrize("g", [1, 2])
def test_subgroup_check(host, g):
    for npj, take in sc.SUBGROUP_SHAPES:
        for n in sc.SUBGROUP_NS:
            _ok(sc.check_subgroup("subgroup G%d (%d, %d) n=%d" % (g, npj, take, n), sc.run_subgroup(host, g, npj, take, n, slack=8 * (n % 2))))
    valid, want = sc.run_subgroup(host, g, 5, 3, 33)
    assert set(want) == {0, 1}
    valid[7] ^= 1
    assert sc.check_subgroup("spoiled", (valid, want))


@pytest.mark.parametrize("N", sc.SELECT_NS)
def test_select_shares(host, N):
    lacking = 0
    for need in sorted({1, min(3, N), N}):
        for jobs in sc.SELECT_JOBS:
            for with_present, with_bad, off_p, off_b, with_map, with_used in sc.select_modes(need, jobs):
                res, inputs = sc.run_select(host, N, need, jobs, with_present, with_bad, off_p, off_b, with_map, with_used)
                bad, lack = sc.check_select("select N=%d need=%d jobs=%d modes %s" % (N, need, jobs, (with_present, with_bad, off_p, off_b, with_map, with_used)),
                                            N, need, jobs, res, inputs)
                _ok(bad)
                lacking += lack if with_present else 0
    assert lacking or N == 1
    res = list(res)
    res[1] = res[1].copy()
    res[1][0] ^= 1
    assert sc.check_select("spoiled", N, need, jobs, tuple(res), inputs)[0]


@pytest.mark.parametrize("t", sc.EVAL_TS)
def test_commitment_evaluate(host, t):
    for m, tag in sc.eval_commits(t):
        for M in ((1, 70) if tag == "random" else (10,)):
            idxs = sc.eval_idxs(M)
            want = [sc.eval_want(m, i) for i in idxs]
            res = sc.run_eval(host, m, t, idxs)
            _ok(sc.check_points("evaluate t=%d %s M=%d" % (t, tag, M), 1, want, 1, res))
    _ok(sc.check_points("evaluate, null status", 1, want, 0, sc.run_eval(host, m, t, idxs, 0)))


@pytest.mark.parametrize("with_g1", [0, 1])
def test_hashes(host, with_g1):
    for B in sc.HASH_B:
        for fix in (1, 0):
            for bad_at in sc.hash_bad_ats(B, with_g1):
                g1, msgs = sc.hash_case(B, with_g1, bad_at)
                res = sc.run_hash(host, g1, msgs, fix, 1)
                _ok(sc.check_hash("hash g1=%d B=%d fix=%d bad_at=%s" % (with_g1, B, fix, bad_at), g1, msgs, fix, 1, res))
                assert sc.same(res, sc.run_hash(host, g1, msgs, fix, 2)), "the _x2 bytes differ (B=%d fix=%d bad_at=%s)" % (B, fix, bad_at)
    _ok(sc.check_hash("null status", g1, msgs, fix, 0, sc.run_hash(host, g1, msgs, fix, 1, 0)))


def test_xor_and_encrypt(host):
    for with_status in (1, 0):
        _ok(sc.run_xor(host, 70, with_status))
    _ok(sc.run_xor(host, 1, 1))
    for pk_stride in (0, 96):
        _ok(sc.run_encrypt(host, 9, pk_stride))
    _ok(sc.run_encrypt(host, 1, 96, 0))


# ---- the kernels without a host routine: the restatements against a transcription of the kernel text ------------------------
def test_restatements_agree_with_the_kernel_text(text):
    for g1 in (0, 1):
        for n in sc.RLC_NS:
            _ok(sc.check_rlc(g1, sc.RLC_SEEDS[1], n, sc.run_rlc(text, g1, sc.RLC_SEEDS[1], n)))
    for case in sc.invalidate_cases():
        got, want = sc.run_invalidate(text, *case)
        _ok(sc.check_invalidate("invalidate %s" % (case,), case[2], case[3], got, want))
    _ok(sc.run_movers(text))
    for npj, take in sc.TAKE_SHAPES:
        _ok(sc.run_take_u64(text, npj, take, 43))
    for pb in (96, 192):
        for form, off_s, off_d in sc.GATHER_SELECTED_FORMS:
            _ok(sc.run_gather_selected(text, pb, 22, form, off_s, off_d)[0])
    for modes in sc.MARK_MODES:
        _ok(sc.run_mark(text, 70, *modes))
    for N in (5, 200):
        for modes in sc.finish_modes():
            _ok(sc.run_finish(text, N, 96 if N == 5 else 192, *modes))


@pytest.mark.parametrize("fault", ["counter & 63", "no | 1", "used from w + row_words"])
def test_checkers_notice_the_device_faults_the_issue_names(fault):
    text = sc.KernelText(fault)
    if fault == "used from w + row_words":
        assert sc.run_finish(text, 200, 192, 1, 1, 1, 1, 1) or sc.run_finish(text, 5, 96, 1, 1, 1, 1, 1)
    else:
        assert sc.check_rlc(0, sc.RLC_SEEDS[0], 130, sc.run_rlc(text, 0, sc.RLC_SEEDS[0], 130))
        assert sc.check_rlc(1, sc.RLC_SEEDS[0], 130, sc.run_rlc(text, 1, sc.RLC_SEEDS[0], 130))


def test_stride_one_clear_of_used_leaves_the_same_bytes():
    """`used` cleared with stride 1 from w instead of stride row_words: every lane of the job then clears the row's tail, each byte
    more than once but always to zero, inside the row.  No comparison of bytes can tell it from the shipped loop; what the suite does
    see is a clear that skips bytes (above)."""
    text = sc.KernelText("used stride 1")
    assert not sc.run_finish(text, 200, 192, 1, 1, 1, 1, 1) and not sc.run_finish(text, 5, 96, 1, 1, 1, 1, 1)
