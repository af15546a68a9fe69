// DKG kernel conformance harness (test code only: never linked into libtc_amd.so, never run by bench.py).
// Includes the product's kernel unit k_dkg.hip as it is (every unit of the product is self-contained: -fno-gpu-rdc), so the
// __global__ kernels launched here are the product's own text, compiled with the product's flags.  Every entry allocates, fills
// each written buffer with 0x5A, copies in, launches THROUGH THE PRODUCT'S LAUNCHER, synchronises once, copies out, frees and
// returns the first HIP error.  Every output buffer carries one guard row / byte / entry behind it, which comes back as it was
// filled.  Where a launcher takes `cus`, `parts` or `slices` they go in by value; parts / slices = 0: g1_sum_parts /
// g1_wsum_parts / g1_wsum_slices with the `cus` given.  The host leg with the same entries: dkg_kernels_host.cpp.
//   build: tests/dkg_conformance.py (hipcc, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "../../threshold_crypto_amd/csrc/k_dkg.hip"

#include "manypoint_dev.h"  // Dev, kMpPoison

using namespace tc;

namespace {
const uint8_t* up(Dev& d, const void* p, size_t bytes) { return p ? (const uint8_t*)d.upload(p, bytes) : nullptr; }
uint8_t* fresh(Dev& d, size_t bytes) { return (uint8_t*)d.alloc(bytes, kMpPoison); }
}  // namespace

// tbl: the 512 entries of 28 words and one guard entry
extern "C" int dk_fixed_base_table(int32_t* tbl) {
  Dev d;
  const size_t bytes = fixed_base_table_bytes() + kFbPointWords * sizeof(int32_t);
  int32_t* dt = (int32_t*)fresh(d, bytes);
  if (d.e == hipSuccess) {
    launch_fixed_base_table(0, dt);
    d.after_launch();
  }
  d.sync();
  d.download(tbl, dt, bytes);
  return (int)d.e;
}

// out: (M + 1) x 96, status: M + 1 (all of it stays as filled when with_status == 0)
extern "C" int dk_g1_fixed_base(const uint8_t* fr, size_t M, int cus, int with_status, uint8_t* out, uint8_t* status) {
  Dev d;
  int32_t* dt = (int32_t*)fresh(d, fixed_base_table_bytes());
  const uint8_t* dfr = up(d, fr, M * 32);
  uint8_t* dout = fresh(d, (M + 1) * 96);
  uint8_t* dst = fresh(d, M + 1);
  if (d.e == hipSuccess) {
    launch_fixed_base_table(0, dt);
    launch_g1_fixed_base(0, dt, dfr, M, dout, with_status ? dst : nullptr, cus);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (M + 1) * 96);
  d.download(status, dst, M + 1);
  return (int)d.e;
}

// form 0: k_bivar_commitment_row (one commitment, B abscissae), 1: k_bivar_commitment_row_jobs (B commitments `stride` bytes apart, one
// abscissa each), 2: k_commitment_evaluate_jobs (B rows of degree + 1 points, n abscissae each).  lanes = B (degree + 1) or B n;
// out: (lanes + 1) x 96, status: lanes + 1.
extern "C" int dk_commitment_rows(int form, const uint8_t* commits, size_t commit_bytes, size_t stride, size_t degree, const uint64_t* xs, size_t B,
                                  size_t n, int with_status, uint8_t* out, uint8_t* status) {
  if (form < 0 || form > 2 || (form && !with_status)) return (int)hipErrorInvalidValue;
  const size_t lanes = form == 2 ? B * n : B * (degree + 1);
  Dev d;
  const uint8_t* dc = up(d, commits, commit_bytes);
  const uint64_t* dxs = (const uint64_t*)up(d, xs, (form == 2 ? B * n : B) * 8);
  uint8_t* dout = fresh(d, (lanes + 1) * 96);
  uint8_t* dst = fresh(d, lanes + 1);
  if (d.e == hipSuccess) {
    if (form == 0) launch_bivar_commitment_row(0, dc, degree, dxs, B, dout, with_status ? dst : nullptr);
    else if (form == 1) launch_bivar_commitment_row_jobs(0, dc, stride, degree, dxs, B, dout, dst);
    else launch_commitment_evaluate_jobs(0, dc, degree, dxs, n, B, dout, dst);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (lanes + 1) * 96);
  d.download(status, dst, lanes + 1);
  return (int)d.e;
}

// out: (B n + 1) x 8 words, ws: (B + 1) blocks of 2 (n + 1) x 8 words, status: B + 1
extern "C" int dk_fr_interpolate(size_t n, const uint32_t* xs, const uint32_t* ys, size_t B, int with_status, uint32_t* out, uint32_t* ws,
                                 uint8_t* status) {
  Dev d;
  const size_t ob = (B * n + 1) * 32, wb = (B + 1) * 2 * (n + 1) * 32;
  const uint32_t* dxs = (const uint32_t*)up(d, xs, B * n * 32);
  const uint32_t* dys = (const uint32_t*)up(d, ys, B * n * 32);
  uint32_t* dout = (uint32_t*)fresh(d, ob);
  uint32_t* dws = (uint32_t*)fresh(d, wb);
  uint8_t* dst = fresh(d, B + 1);
  if (d.e == hipSuccess) {
    launch_fr_interpolate(0, n, dxs, dys, B, dout, dws, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, ob);
  d.download(ws, dws, wb);
  d.download(status, dst, B + 1);
  return (int)d.e;
}

// out: (P + 1) x 32, status: P + 1
extern "C" int dk_fr_interpolate_at_zero(size_t n, const uint64_t* xs, const uint8_t* vals, const uint8_t* accept, size_t P, uint8_t* out,
                                         uint8_t* status) {
  Dev d;
  const uint64_t* dxs = (const uint64_t*)up(d, xs, P * n * 8);
  const uint8_t* dv = up(d, vals, P * n * 32);
  const uint8_t* da = up(d, accept, P);
  uint8_t* dout = fresh(d, (P + 1) * 32);
  uint8_t* dst = fresh(d, P + 1);
  if (d.e == hipSuccess) {
    launch_fr_interpolate_at_zero(0, n, dxs, dv, da, P, dout, dst);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (P + 1) * 32);
  d.download(status, dst, P + 1);
  return (int)d.e;
}

// degree < 0: k_fr_to_mont over `count` values; else k_bivar_to_mont (count = (degree + 1)^2 outputs from the triangle `fr`).
// mont: (count + 1) x 8 words, valid: count + 1
extern "C" int dk_to_mont(const uint8_t* fr, size_t fr_bytes, size_t count, int degree, uint32_t* mont, uint8_t* valid) {
  if (degree >= 0 && count != (size_t)(degree + 1) * (degree + 1)) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dfr = up(d, fr, fr_bytes);
  uint32_t* dm = (uint32_t*)fresh(d, (count + 1) * 32);
  uint8_t* dv = fresh(d, count + 1);
  if (d.e == hipSuccess) {
    if (degree < 0) launch_fr_to_mont(0, dfr, count, dm, dv);
    else launch_bivar_to_mont(0, dfr, (size_t)degree, dm, dv);
    d.after_launch();
  }
  d.sync();
  d.download(mont, dm, (count + 1) * 32);
  d.download(valid, dv, count + 1);
  return (int)d.e;
}

// k_fr_to_mont, then k_fr_poly_evaluate over what it left: coeff B x n x 32 B, xs M x 32 B; out: (B M + 1) x 32, status: B M + 1
extern "C" int dk_fr_poly_evaluate(const uint8_t* coeff, size_t n, const uint8_t* xs, size_t M, size_t B, int with_status, uint8_t* out,
                                   uint8_t* status) {
  Dev d;
  const uint8_t* dc = up(d, coeff, B * n * 32);
  const uint8_t* dxs = up(d, xs, M * 32);
  uint32_t* dm = (uint32_t*)fresh(d, B * n * 32);
  uint8_t* dv = fresh(d, B * n);
  uint8_t* dout = fresh(d, (B * M + 1) * 32);
  uint8_t* dst = fresh(d, B * M + 1);
  if (d.e == hipSuccess) {
    launch_fr_to_mont(0, dc, B * n, dm, dv);
    launch_fr_poly_evaluate(0, dm, dv, n, dxs, M, B, dout, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B * M + 1) * 32);
  d.download(status, dst, B * M + 1);
  return (int)d.e;
}

// k_bivar_to_mont, then k_bivar_poly_row: out: (M (degree + 1) + 1) x 32, status: M (degree + 1) + 1
extern "C" int dk_bivar_poly_row(const uint8_t* coeff, size_t degree, const uint64_t* xs, size_t M, int with_status, uint8_t* out, uint8_t* status) {
  Dev d;
  const size_t n = degree + 1, lanes = M * n;
  const uint8_t* dc = up(d, coeff, n * (n + 1) / 2 * 32);
  const uint64_t* dxs = (const uint64_t*)up(d, xs, M * 8);
  uint32_t* dm = (uint32_t*)fresh(d, n * n * 32);
  uint8_t* dv = fresh(d, n * n);
  uint8_t* dout = fresh(d, (lanes + 1) * 32);
  uint8_t* dst = fresh(d, lanes + 1);
  if (d.e == hipSuccess) {
    launch_bivar_to_mont(0, dc, degree, dm, dv);
    launch_bivar_poly_row(0, dm, dv, degree, dxs, M, dout, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (lanes + 1) * 32);
  d.download(status, dst, lanes + 1);
  return (int)d.e;
}

// k_fr_sum (weights == null) / k_fr_wsum: out: (B + 1) x 32, status: B + 1
extern "C" int dk_fr_sum(const uint8_t* vals, size_t vals_bytes, size_t term_stride, size_t n, const uint8_t* weights, const uint8_t* mask, size_t B,
                         int with_status, uint8_t* out, uint8_t* status) {
  Dev d;
  const uint8_t* dv = up(d, vals, vals_bytes);
  const uint8_t* dw = up(d, weights, n * 32);
  const uint8_t* dm = up(d, mask, n);
  uint8_t* dout = fresh(d, (B + 1) * 32);
  uint8_t* dst = fresh(d, B + 1);
  if (d.e == hipSuccess) {
    if (weights) launch_fr_wsum(0, dv, term_stride, n, dw, dm, B, dout, with_status ? dst : nullptr);
    else launch_fr_sum(0, dv, term_stride, n, dm, B, dout, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B + 1) * 32);
  d.download(status, dst, B + 1);
  return (int)d.e;
}

// k_g1_sum: mask n bytes or null, member n x B bytes or null; out: (B + 1) x 96, status: B + 1, term_bad: n zeroed bytes and a
// guard byte (as filled when with_term_bad == 0); used[0] = the parts handed to the launcher
extern "C" int dk_g1_sum(int column0, const uint8_t* pts, size_t pts_bytes, size_t term_stride, size_t n, const uint8_t* mask, const uint8_t* member,
                         size_t B, size_t parts, int cus, int with_status, int with_term_bad, uint8_t* out, uint8_t* status, uint8_t* term_bad,
                         size_t* used) {
  Dev d;
  const uint8_t* dp = up(d, pts, pts_bytes);
  const uint8_t* dm = up(d, mask, n);
  const uint8_t* dmem = up(d, member, n * B);
  uint8_t* dout = fresh(d, (B + 1) * 96);
  uint8_t* dst = fresh(d, B + 1);
  uint8_t* dbad = fresh(d, n + 1);
  if (d.e == hipSuccess && with_term_bad && n) d.e = hipMemset(dbad, 0, n);
  used[0] = g1_sum_parts(B, n, cus, parts);
  if (d.e == hipSuccess) {
    launch_g1_sum(0, column0 != 0, dp, term_stride, n, dm, dmem, B, used[0], dout, with_status ? dst : nullptr, with_term_bad ? dbad : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B + 1) * 96);
  d.download(status, dst, B + 1);
  d.download(term_bad, dbad, n + 1);
  return (int)d.e;
}

// k_wsum_recode over the n_terms weights, then k_g1_wsum over n terms (sel == null: n == n_terms; else the n positions of sel), as
// tc_api.hip chains them: parts = g1_wsum_parts(.., parts), slices = g1_wsum_slices(.., slices); BOTH status and part_ok go to the
// launcher.  rec: (n_terms + 1) x 9 words; out: (rows + 1) x 96, status / part_ok: rows + 1 with rows >= B slices (else an error, nothing
// launched).  chain != 0 and slices > 1: k_g1_sum over the partial sums where they lie (n = slices, member = part_ok) into final_out
// ((B + 1) x 96) / final_status (B + 1).  used: parts, slices as handed to the launcher.
extern "C" int dk_g1_wsum(int column0, const uint8_t* pts, size_t pts_bytes, size_t term_stride, size_t n_terms, const uint8_t* weights, size_t n,
                          const uint8_t* mask, const uint8_t* member, size_t B, size_t parts, size_t slices, int cus, const uint32_t* sel, int chain,
                          size_t rows, uint32_t* rec, uint8_t* out, uint8_t* status, uint8_t* part_ok, uint8_t* final_out, uint8_t* final_status,
                          size_t* used) {
  used[0] = g1_wsum_parts(B, n, cus, parts);
  used[1] = g1_wsum_slices(B, n, used[0], cus, slices);
  if (B * used[1] > rows || (!sel && n != n_terms)) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t rw = wsum_rec_words();
  const uint8_t* dp = up(d, pts, pts_bytes);
  const uint8_t* dw = up(d, weights, n_terms * 32);
  const uint8_t* dm = up(d, mask, n_terms);
  const uint8_t* dmem = up(d, member, n_terms * B);
  const uint32_t* dsel = (const uint32_t*)up(d, sel, n * 4);
  uint32_t* drec = (uint32_t*)fresh(d, (n_terms + 1) * rw * 4);
  uint8_t* dout = fresh(d, (rows + 1) * 96);
  uint8_t* dst = fresh(d, rows + 1);
  uint8_t* dpok = fresh(d, rows + 1);
  uint8_t* dfo = fresh(d, (B + 1) * 96);
  uint8_t* dfs = fresh(d, B + 1);
  if (d.e == hipSuccess) {
    launch_wsum_recode(0, dw, n_terms, drec);
    launch_g1_wsum(0, column0 != 0, dp, term_stride, n, drec, dm, dmem, B, used[0], used[1], dout, dst, dpok, dsel);
    if (chain && used[1] > 1)
      launch_g1_sum(0, false, dout, B * 96, used[1], nullptr, dpok, B, g1_sum_parts(B, used[1], cus, 0), dfo, dfs, nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(rec, drec, (n_terms + 1) * rw * 4);
  d.download(out, dout, (rows + 1) * 96);
  d.download(status, dst, rows + 1);
  d.download(part_ok, dpok, rows + 1);
  d.download(final_out, dfo, (B + 1) * 96);
  d.download(final_status, dfs, B + 1);
  return (int)d.e;
}

// scalars: (B (degree + 2) + 1) x 8 words, valid: B + 1
extern "C" int dk_rlc_scalars(const uint8_t* seed32, const uint64_t* xs, const uint8_t* vals, size_t n, size_t degree, size_t B, uint32_t* scalars,
                              uint8_t* valid) {
  Dev d;
  const size_t sb = (B * (degree + 2) + 1) * 32;
  const uint8_t* ds = up(d, seed32, 32);
  const uint64_t* dxs = (const uint64_t*)up(d, xs, B * n * 8);
  const uint8_t* dv = up(d, vals, B * n * 32);
  uint32_t* dsc = (uint32_t*)fresh(d, sb);
  uint8_t* dva = fresh(d, B + 1);
  if (d.e == hipSuccess) {
    launch_dkg_rlc_scalars(0, ds, dxs, dv, n, degree, B, dsc, dva);
    d.after_launch();
  }
  d.sync();
  d.download(scalars, dsc, sb);
  d.download(valid, dva, B + 1);
  return (int)d.e;
}

// column0 == 0: k_dkg_rlc_points (src: B rows of degree + 1 points, `extra`: the 96 bytes appended to each), out: (B (degree + 2) + 1) x 96;
// else k_bivar_column0 (src: B commitments `stride` bytes apart), out: (B (degree + 1) + 1) x 96
extern "C" int dk_copy_points(int column0, const uint8_t* src, size_t src_bytes, size_t stride, size_t degree, const uint8_t* extra, size_t B,
                              uint8_t* out) {
  Dev d;
  const size_t ob = (B * (degree + (column0 ? 1 : 2)) + 1) * 96;
  const uint8_t* dsrc = up(d, src, src_bytes);
  const uint8_t* dex = up(d, extra, 96);
  uint8_t* dout = fresh(d, ob);
  if (d.e == hipSuccess) {
    if (column0) launch_bivar_column0(0, dsrc, stride, degree, B, dout);
    else launch_dkg_rlc_points(0, dsrc, degree, dex, B, dout);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, ob);
  return (int)d.e;
}

// b != null: k_g1_equal over B jobs of per_job points; else k_g1_is_identity (per_job = 1, st_b = the `valid` bytes).  ok: B + 1
extern "C" int dk_g1_compare(const uint8_t* a, const uint8_t* st_a, const uint8_t* b, const uint8_t* st_b, size_t per_job, size_t B, uint8_t* ok) {
  Dev d;
  const uint8_t* da = up(d, a, B * per_job * 96);
  const uint8_t* dsa = up(d, st_a, B * per_job);
  const uint8_t* db = up(d, b, B * per_job * 96);
  const uint8_t* dsb = up(d, st_b, B * per_job);
  uint8_t* dok = fresh(d, B + 1);
  if (d.e == hipSuccess) {
    if (b) launch_g1_equal(0, da, dsa, db, dsb, per_job, B, dok);
    else launch_g1_is_identity(0, da, dsa, dsb, B, dok);
    d.after_launch();
  }
  d.sync();
  d.download(ok, dok, B + 1);
  return (int)d.e;
}

// The resharing verdict chain: k_reshare_check -> k_reshare_part_status -> k_reshare_plan -> k_reshare_guard.  const_st, point_bad, dup,
// part_status, used: P + 1; old_bad, status: 2; sel_part (uint32), sel_idx (uint64): t_old + 2; ws: reshare_plan_ws_words(t_old) + 8 words;
// weights: P x 32 zeroed and 32 guard bytes.  out_commit ((degree + 2) x 96) and out_share (64 bytes) come in from the caller, so that
// the guard kernel's "only on failure" shows; either may be null.
extern "C" int dk_reshare_chain(const uint8_t* old_commit, const uint8_t* old_member, size_t t_old, const uint64_t* dealer_idx, const uint8_t* commits,
                                size_t commit_bytes, size_t stride, size_t degree, const uint8_t* accept, const uint8_t* member,
                                const uint8_t* share_st, size_t P, uint8_t* const_st, uint8_t* point_bad, uint8_t* dup, uint8_t* old_bad,
                                uint8_t* part_status, uint8_t* used, uint32_t* sel_part, uint64_t* sel_idx, uint32_t* ws, uint8_t* weights,
                                uint8_t* status, uint8_t* out_commit, uint8_t* out_share) {
  if (!P) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t wsb = (reshare_plan_ws_words(t_old) + 8) * 4;
  const uint8_t* doc = up(d, old_commit, (t_old + 1) * 96);
  const uint8_t* dom = up(d, old_member, t_old + 1);
  const uint64_t* didx = (const uint64_t*)up(d, dealer_idx, P * 8);
  const uint8_t* dc = up(d, commits, commit_bytes);
  const uint8_t* dacc = up(d, accept, P);
  const uint8_t* dmem = up(d, member, P * (degree + 1));
  const uint8_t* dss = up(d, share_st, P);
  uint8_t* dcs = fresh(d, P + 1);
  uint8_t* dpb = fresh(d, P + 1);
  uint8_t* ddu = fresh(d, P + 1);
  uint8_t* dob = fresh(d, 2);
  uint8_t* dps = fresh(d, P + 1);
  uint8_t* dus = fresh(d, P + 1);
  uint32_t* dsp = (uint32_t*)fresh(d, (t_old + 2) * 4);
  uint64_t* dsi = (uint64_t*)fresh(d, (t_old + 2) * 8);
  uint32_t* dws = (uint32_t*)fresh(d, wsb);
  uint8_t* dwt = fresh(d, (P + 1) * 32);
  uint8_t* dst = fresh(d, 2);
  uint8_t* dco = (uint8_t*)up(d, out_commit, (degree + 2) * 96);
  uint8_t* dsh = (uint8_t*)up(d, out_share, 64);
  if (d.e == hipSuccess) d.e = hipMemset(dwt, 0, P * 32);
  if (d.e == hipSuccess) {
    launch_reshare_check(0, doc, dom, t_old, didx, dc, stride, degree, dacc, dmem, P, dcs, dpb, ddu, dob);
    launch_reshare_verdict(0, dacc, didx, t_old, P, dcs, dpb, ddu, dss, dob, dps, dus, dsp, dsi, dws, dwt, dst);
    launch_reshare_guard(0, dst, degree, dco, dsh);
    d.after_launch();
  }
  d.sync();
  d.download(const_st, dcs, P + 1);
  d.download(point_bad, dpb, P + 1);
  d.download(dup, ddu, P + 1);
  d.download(old_bad, dob, 2);
  d.download(part_status, dps, P + 1);
  d.download(used, dus, P + 1);
  d.download(sel_part, dsp, (t_old + 2) * 4);
  d.download(sel_idx, dsi, (t_old + 2) * 8);
  d.download(ws, dws, wsb);
  d.download(weights, dwt, (P + 1) * 32);
  d.download(status, dst, 2);
  if (out_commit) d.download(out_commit, dco, (degree + 2) * 96);
  if (out_share) d.download(out_share, dsh, 64);
  return (int)d.e;
}

// k_dkg_part_status -> k_dkg_generate_guard: part_status: P + 1; out_commit / out_share as in dk_reshare_chain
extern "C" int dk_generate_verdict(const uint8_t* accept, const uint8_t* point_bad, const uint8_t* share_st, size_t P, size_t degree,
                                   uint8_t* part_status, uint8_t* out_commit, uint8_t* out_share) {
  if (!P) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dacc = up(d, accept, P);
  const uint8_t* dpb = up(d, point_bad, P);
  const uint8_t* dss = up(d, share_st, P);
  uint8_t* dps = fresh(d, P + 1);
  uint8_t* dco = (uint8_t*)up(d, out_commit, (degree + 2) * 96);
  uint8_t* dsh = (uint8_t*)up(d, out_share, 64);
  if (d.e == hipSuccess) {
    launch_dkg_generate_verdict(0, dacc, dpb, dss, P, degree, dps, dco, dsh);
    d.after_launch();
  }
  d.sync();
  d.download(part_status, dps, P + 1);
  if (out_commit) d.download(out_commit, dco, (degree + 2) * 96);
  if (out_share) d.download(out_share, dsh, 64);
  return (int)d.e;
}
