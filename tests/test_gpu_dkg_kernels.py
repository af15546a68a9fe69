"""GPU leg of the DKG kernel conformance suite (tests/dkg_conformance.py): the shipped kernels of k_dkg.hip, launched by
tests/device/dkg_kernels.hip through the product's launchers with `cus`, `parts` and `slices` chosen by the test, over the case
tables the host leg has proven (tests/test_dkg_kernels_host.py).

Per run everything a kernel left in memory comes back and is compared exactly: outputs and statuses against the oracle, the guard
row / byte / entry behind every buffer, the buffer a null pointer or the other mode leaves alone (status, part_ok, term_bad), the
512 entries of the fixed-base table, the interpolation workspaces and the recoded weights against the host leg's bytes, the
Montgomery matrices, every intermediate array of the resharing verdict.  k_g1_sum and k_g1_wsum run at parts = 0 (the launcher's
rule), every power of two up to 64, and 3 and 128 (run as 1), the weighted sums over the whole slices x parts grid, and must leave
the same bytes every time.  After one HIP error nothing more is launched."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dkg_conformance as dk  # noqa: E402

pytestmark = pytest.mark.gpu

_state = {"lib": None, "host": None, "hip_error": None}


@pytest.fixture(scope="module")
def lib():
    if _state["lib"] is None:
        _state["lib"] = dk.load(dk.build_device(), "dk_")
    return _state["lib"]


@pytest.fixture(scope="module")
def host():
    if _state["host"] is None:
        _state["host"] = dk.load(dk.build_host(), "dkh_")
    return _state["host"]


def _launch(fn, *args, **kw):
    if _state["hip_error"]:
        pytest.fail("not launched after an earlier HIP error: %s" % _state["hip_error"])
    try:
        return fn(*args, **kw)
    except dk.HipError as e:
        _state["hip_error"] = str(e)
        raise


def _ok(bad):
    assert not bad, "\n".join(bad[:12])


# ---- 1. the fixed-base table and multiplication ---------------------------------------------------------------------------
def test_fixed_base_table(lib, host):
    """All 512 entries against the oracle's [m 16^w] g1 -- (63, 8), which no scalar below r reaches, included --, the limb form the
    multiplication relies on, the guard entry, and the host leg's words."""
    tbl = _launch(dk.run_fb_table, lib)
    _ok(dk.check_fb_table(tbl))
    assert (tbl[:512] == dk.run_fb_table(host)[:512]).all()


def test_fixed_base_directed_and_random_products(lib, host):
    """Every directed scalar (each digit at windows 0, 31 and 62, the carry chains, 0, 1, r - 1, r - 2, r, 2^256 - 1) and 32 random
    ones against the oracle, and against the host leg's bytes."""
    case = dk.fb_case()
    res = _launch(dk.run_fb, lib, case, dk.FB_ALL, 1, 1)
    _ok(dk.check_fb(case, dk.FB_ALL, 1, res))
    ref = dk.run_fb(host, case, dk.FB_ALL, 1, 1)
    assert dk.same(res, ref)


@pytest.mark.parametrize("M,cus", dk.FB_SHAPES)
def test_fixed_base_grid_stride(lib, M, cus):
    """cus = 1: two workgroups walk M = 1 .. 1061 (three trips, the last one ragged); cus = 0: the default of 256.  status given
    and null."""
    case = dk.fb_case()
    for with_status in (1, 0):
        _ok(dk.check_fb(case, M, with_status, _launch(dk.run_fb, lib, case, M, cus, with_status)))


# ---- 2. rows and evaluations in G1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dk.ROWS_SHAPES)
def test_commitment_rows(lib, shape):
    case = dk.rows_case(*shape)
    for with_status in (1, 0):
        _ok(dk.check_rows(case, with_status, _launch(dk.run_rows, lib, case, with_status)))


def test_commitment_rows_directed(lib):
    """Identity coefficients, a Horner step that meets c = [x] res (must double) and c = -[x] res (the identity, and on), an
    off-curve coefficient, a stride larger than the commitment: the three kernels."""
    for case in dk.rows_directed_cases():
        _ok(dk.check_rows(case, 1, _launch(dk.run_rows, lib, case)))


# ---- 3. the Fr kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_interpolation(lib, host, n):
    """k_fr_interpolate over 70 jobs: coefficients, statuses, and every word of every workspace block as the host leg leaves it (so
    job j's block holds nothing of job j - 1 or j + 1), the guard block behind the last; then k_fr_interpolate_at_zero over the same
    samples, with and without `accept` (a rejected part holds garbage and is not read)."""
    case = dk.interp_case(n)
    for with_status in (1, 0):
        res = _launch(dk.run_interp, lib, case, with_status)
        _ok(dk.check_interp(case, with_status, res))
        assert dk.same(res, dk.run_interp(host, case, with_status)), "%s: not the host leg's bytes (out, ws or status)" % case.tag
    for with_accept in (0, 1):
        _ok(dk.check_interp0(case, with_accept, _launch(dk.run_interp0, lib, case, with_accept)))


def test_montgomery_matrices(lib):
    vals = dk.mont_values()
    _ok(dk.check_to_mont(vals, -1, _launch(dk.run_to_mont, lib, vals)))
    for degree, variant in [(0, 0), (2, 0), (2, 1), (7, 0)]:
        c = dk.bivar_coeffs(degree, variant)
        _ok(dk.check_to_mont(c, degree, _launch(dk.run_to_mont, lib, c, degree)))


def test_fr_evaluations(lib):
    for n in (0, 1, 4):
        polys, xs, want = dk.poly_evaluate_case(n)
        for with_status in (1, 0):
            _ok(dk.check_fr_rows("poly evaluate n = %d" % n, want, _launch(dk.run_poly_evaluate, lib, polys, xs, with_status), with_status))
    for degree, M, variant in dk.BIVAR_ROW_SHAPES:
        c = dk.bivar_coeffs(degree, variant)
        xs = [dk.XS[m % len(dk.XS)] for m in range(M)]
        want = dk.bivar_row_want(degree, c, xs)
        for with_status in (1, 0):
            _ok(dk.check_fr_rows("bivar row degree %d" % degree, want, _launch(dk.run_bivar_row, lib, degree, c, xs, with_status), with_status))


def test_fr_sums(lib):
    """k_fr_sum and k_fr_wsum at n = 0 .. 67 over 70 outputs: masks that exclude the non-canonical terms, included non-canonical
    values (their outputs: zero, status 3) and weights (every output), term_stride = 32 B and larger."""
    for n in range(68):
        for weighted in (0, 1):
            case = dk.FrSumCase(n, weighted, n % 3)
            with_status = int(n != 7)
            _ok(dk.check_fr_rows(case.tag, case.want(), _launch(dk.run_fr_sum, lib, case, with_status), with_status))


# ---- 4. k_g1_sum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dk.SUM_NS)
@pytest.mark.parametrize("variant", ["masked", "included"])
def test_g1_sum(lib, n, variant):
    """parts = 0, 1 .. 64, 3 and 128: out, status and term_bad equal the oracle's and are the same bytes at every value."""
    case = dk.sum_case(n, variant)
    first = None
    for parts in dk.PARTS:
        res = _launch(dk.run_sum, lib, case, parts)
        _ok(dk.check_sum(case, parts, res))
        first = first or res
        assert dk.same(dk.sum_head(res), dk.sum_head(first)), "%s: parts = %d and parts = %d leave different bytes" % (case.tag, parts, dk.PARTS[0])
    _ok(dk.check_sum(case, 8, _launch(dk.run_sum, lib, case, 8, 1, 0, 0), 0, 0))  # status and term_bad null
    _ok(dk.check_sum(case, 0, _launch(dk.run_sum, lib, case, 0, 0)))               # the rule at the default cus


@pytest.mark.parametrize("degree", [2, 7])
def test_g1_sum_over_first_columns(lib, degree):
    case = dk.Column0Case(degree)
    for parts in (0, 1, 2, 4, 3):
        _ok(dk.check_column0_sum(case, parts, _launch(dk.run_column0_sum, lib, case, parts)))


# ---- 5. k_wsum_recode and k_g1_wsum ---------------------------------------------------------------------------------------
def test_weight_recoding(lib, host):
    weights = dk.rec_weights()
    rec = _launch(dk.recode_only, lib, weights)
    _ok(dk.check_rec(weights, rec))
    assert (rec == dk.recode_only(host, weights)).all()


@pytest.mark.parametrize("n,variant,with_sel", [(n, v, False) for n in dk.WSUM_NS for v in ("masked", "failing")] +
                         [(5, "masked", True), (5, "failing", True)])
def test_g1_weighted_sum(lib, n, variant, with_sel):
    """The whole slices x parts grid, chained with k_g1_sum as tc_api.hip does: the final bytes are the same everywhere and equal
    the one-slice run; with slices > 1 every (slice, output) partial sum and part_ok byte is checked and status stays as filled,
    with one slice the converse; the recoded weights are the same words in every run."""
    case = dk.wsum_case(n, variant, with_sel)
    first, by_slices = None, {}
    for slices in dk.wsum_slices(n):
        for parts in dk.PARTS:
            res = _launch(dk.run_wsum, lib, case, parts, slices)
            S = res[6]
            if S not in by_slices:
                _ok(dk.check_wsum(case, parts, slices, res))
                by_slices[S] = res
            assert dk.same(res[:6], by_slices[S][:6]), "%s: parts = %d, slices = %d: not the bytes of the first run with %d slices" % (case.tag, parts, slices, S)
            first = first or res
            assert dk.same(res[:3], first[:3]), "%s: parts = %d, slices = %d: other final bytes" % (case.tag, parts, slices)
    assert 1 in by_slices and len(by_slices) >= min(n, 3)
    if n == 130:  # the slices rule itself: three slices at the default cus
        res = _launch(dk.run_wsum, lib, case, 0, 0, 0)
        assert res[6] == 3
        _ok(dk.check_wsum(case, 0, 0, res))
        assert dk.same(res[:3], first[:3])


# ---- 6. the pieces of the combined values check -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dk.RLC_SHAPES)
def test_rlc_scalars(lib, shape):
    case = dk.RlcCase(*shape)
    _ok(dk.check_rlc(case, _launch(dk.run_rlc, lib, case)))


@pytest.mark.parametrize("column0,degree,B", dk.COPY_SHAPES)
def test_copy_kernels(lib, column0, degree, B):
    """k_dkg_rlc_points / k_bivar_column0 word for word, and the 96 bytes behind the last row."""
    out, want = _launch(dk.run_copy_points, lib, column0, degree, B)
    assert bytes(out[:len(want)]) == want and dk.is_poison(out[len(want):])


@pytest.mark.parametrize("per_job", [1, 3])
def test_g1_equal(lib, per_job):
    a, sa, b, sb, want = dk.compare_case(per_job)
    ok = _launch(dk.run_compare, lib, a, sa, b, sb, per_job, 70)
    assert [int(x) for x in ok[:70]] == want and ok[70] == dk.POISON


def test_g1_is_identity(lib):
    pts, st, valid, want = dk.identity_case()
    ok = _launch(dk.run_compare, lib, pts, st, None, valid, 1, 70)
    assert [int(x) for x in ok[:70]] == want and ok[70] == dk.POISON


# ---- 7. the verdict chains ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dk.RESHARE_SHAPES)
def test_reshare_verdict_chain(lib, host, shape):
    """k_reshare_check -> k_reshare_part_status -> k_reshare_plan -> k_reshare_guard: every intermediate array against the rules of
    the header comments, the weights against the oracle's Lagrange coefficients, the guards; null out_commit / out_share."""
    case = dk.reshare_case(*shape)
    res = _launch(dk.run_reshare, lib, case)
    _ok(dk.check_reshare(case, res))
    ref = dk.run_reshare(host, case)
    assert (res["ws"][:(case.t_old + 1) * 8] == ref["ws"][:(case.t_old + 1) * 8]).all()
    _ok(dk.check_reshare(case, _launch(dk.run_reshare, lib, case, (False, True))))
    _ok(dk.check_reshare(case, _launch(dk.run_reshare, lib, case, (True, False))))


@pytest.mark.parametrize("P,kind", dk.GENERATE_SHAPES)
def test_generate_verdict(lib, P, kind):
    for with_outputs in ((True, True), (False, True), (True, False)):
        _ok(_launch(dk.run_generate_verdict, lib, P, kind, 2, with_outputs))
